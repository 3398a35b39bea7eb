#!/usr/bin/env python3
"""Golden vectors of KRCNN.NMS_OKS: the REAL reference's `utils.keypoints.nms_oks` and `compute_oks`, run under the py3 shims of
make_golden.py (same directory) on seeded float32 poses and boxes -> tests/golden/reference_oks_nms.json (inputs, keep lists and OKS
matrices, a few KB).

Run in the build container only (needs the reference checkout):
    python tests/golden/make_golden_oks_nms.py

The sets (threshold 0.3, the value the reference hard-codes at lib/core/test.py:886):
  near_duplicates   two pairs of shifted copies, one with an OKS above the threshold (the copy goes), one below (both stay)
  asymmetric_area   a small high-scoring box beside a large one: OKS(small -> large) < 0.3 < OKS(large -> small); the small row is
                    visited first and its area counts, so the large row stays
  asymmetric_area_reversed   the same pair with the large box scoring higher: the small row goes
  chain             A removes B; B alone would have removed C; A does not remove C, so C is kept
  removes_all       the best row removes all the others
  none_removed      poses far apart: every row is kept, in score order
The maker fails unless every OKS the reference evaluates is further than 1e-6 from the threshold and neighbouring scores differ by
more than 1e-4 relative (the reference's argsort leaves ties undefined), and unless each set shows what its name says.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_shims  # noqa: E402

THRESH = 0.3
K = 17


def base_pose(rs, box):
    """17 keypoints inside `box` (x1, y1, x2, y2), arbitrary float32 positions."""
    x1, y1, x2, y2 = box
    p = np.zeros((4, K), dtype=np.float32)
    p[0] = rs.uniform(x1, x2, K)
    p[1] = rs.uniform(y1, y2, K)
    return p


def shifted(p, dx, dy):
    q = p.copy()
    q[0] += np.float32(dx)
    q[1] += np.float32(dy)
    return q


def with_score(p, rs, score):
    """The logit row: mean close to `score`."""
    q = p.copy()
    q[2] = (score + rs.uniform(-0.5, 0.5, K)).astype(np.float32)
    return q


def side(box):
    return float(np.sqrt((box[2] - box[0] + 1) * (box[3] - box[1] + 1)))


def make_sets():
    rs = np.random.RandomState(1907)
    sets = {}

    # near duplicates: a uniform shift of f * sqrt(area) gives OKS ~ 0.37 at f = 0.18 and ~ 0.24 at f = 0.24
    b1, b2 = (100.3, 80.7, 220.9, 330.2), (600.1, 90.4, 700.6, 300.8)
    a, c = base_pose(rs, b1), base_pose(rs, b2)
    rows = [with_score(a, rs, 9.0), with_score(shifted(a, 0.18 * side(b1), 0.0), rs, 7.0),
            with_score(c, rs, 8.0), with_score(shifted(c, 0.0, 0.24 * side(b2)), rs, 6.0)]
    sets['near_duplicates'] = (rows, [b1, b1, b2, b2], [0, 2, 3])

    # asymmetric area: the large box has 4 x the area; the shift is 0.12 of its side and 0.24 of the small one's
    small, large = (300.2, 200.6, 360.4, 320.1), (270.5, 140.3, 391.2, 379.9)
    a = base_pose(rs, small)
    d = 0.12 * side(large)
    rows = [with_score(a, rs, 8.0), with_score(shifted(a, d, 0.0), rs, 5.0)]
    sets['asymmetric_area'] = (rows, [small, large], [0, 1])
    rows = [with_score(a, rs, 5.0), with_score(shifted(a, d, 0.0), rs, 8.0)]
    sets['asymmetric_area_reversed'] = (rows, [small, large], [1])

    # chain: steps of 0.15 side (OKS ~ 0.47), two steps 0.30 (OKS ~ 0.15)
    b = (50.9, 60.2, 190.3, 280.8)
    a = base_pose(rs, b)
    s = 0.15 * side(b)
    rows = [with_score(shifted(a, s, 0.0), rs, 6.0), with_score(shifted(a, 2 * s, 0.0), rs, 4.0), with_score(a, rs, 8.0)]
    sets['chain'] = (rows, [b, b, b], [2, 1])

    # the best row (the third) removes all the others: jitter of at most 0.04 side per coordinate
    b = (400.7, 100.1, 520.3, 340.6)
    a = base_pose(rs, b)
    rows, scores = [], [3.0, 5.0, 9.0, 4.0]
    for sc in scores:
        q = a.copy()
        if sc != 9.0:
            q[:2] += rs.uniform(-0.04, 0.04, (2, K)).astype(np.float32) * np.float32(side(b))
        rows.append(with_score(q, rs, sc))
    sets['removes_all'] = (rows, [b] * 4, [2])

    # nothing removed
    boxes = [(10.2 + 200 * i, 20.4, 110.8 + 200 * i, 260.3) for i in range(3)]
    rows = [with_score(base_pose(rs, bx), rs, sc) for bx, sc in zip(boxes, [2.0, 7.0, 5.0])]
    sets['none_removed'] = (rows, boxes, [1, 2, 0])
    return sets


def short(a):
    """float32 array -> nested lists of the shortest decimals that round back to the same float32 values."""
    a = np.asarray(a, dtype=np.float32)
    return np.vectorize(float, otypes=[object])(a.astype(str)).tolist()


def main():
    _install_shims()
    import utils.keypoints as ref
    evaluated = []
    real_compute_oks = ref.compute_oks

    def recording(*args):
        out = real_compute_oks(*args)
        evaluated.extend(np.asarray(out, dtype=np.float64).tolist())
        return out

    out = {'thresh': THRESH, 'sets': {}}
    for name, (rows, boxes, want) in sorted(make_sets().items()):
        # two decimals keep the file small; the float32 values of such decimals are still arbitrary bit patterns
        kps, rois = np.round(np.stack(rows).astype(np.float64), 2).astype(np.float32), np.asarray(boxes, dtype=np.float32)
        assert np.array_equal(kps, np.asarray(json.loads(json.dumps(short(kps))), dtype=np.float32))        # what a reader of the file gets
        assert np.array_equal(rois, np.asarray(json.loads(json.dumps(short(rois))), dtype=np.float32))
        del evaluated[:]
        ref.compute_oks = recording
        try:
            keep = [int(i) for i in ref.nms_oks(kps, rois, THRESH)]
        finally:
            ref.compute_oks = real_compute_oks
        margin = min([abs(v - THRESH) for v in evaluated] + [1.0])
        assert margin > 1e-6, (name, margin)
        scores = np.sort(np.mean(kps[:, 2, :], axis=1).astype(np.float64))
        gaps = np.abs(np.diff(scores)) / np.maximum(np.abs(scores[1:]), np.abs(scores[:-1]))
        assert gaps.size == 0 or gaps.min() > 1e-4, (name, gaps)
        assert keep == want, (name, keep, want)
        oks = np.stack([np.asarray(real_compute_oks(kps[i], rois[i], kps, rois), dtype=np.float64) for i in range(len(rows))])
        out['sets'][name] = {'kps': short(kps), 'rois': short(rois), 'keep': keep, 'oks': oks.tolist()}
        print('%-26s keep %s   evaluated OKS %s' % (name, keep, ['%.4f' % v for v in evaluated]))
    s = out['sets']
    o = np.asarray(s['asymmetric_area']['oks'])
    assert o[0, 1] < THRESH < o[1, 0], o                   # the result depends on whose area is used
    o = np.asarray(s['chain']['oks'])
    assert o[2, 0] > THRESH and o[0, 1] > THRESH and o[2, 1] < THRESH, o
    o = np.asarray(s['near_duplicates']['oks'])
    assert o[0, 1] > THRESH > o[2, 3], o
    assert np.asarray(s['none_removed']['oks'])[~np.eye(3, dtype=bool)].max() < THRESH
    path = os.path.join(HERE, 'reference_oks_nms.json')
    with open(path, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
    print('wrote reference_oks_nms.json: %d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
