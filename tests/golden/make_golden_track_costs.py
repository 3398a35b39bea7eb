#!/usr/bin/env python3
"""Golden vectors of the tracker's pose cost: the REAL reference's `utils.keypoints.pck_distance` and
`core.tracking_engine._compute_distance_matrix` with ('bbox-overlap', 'pose-pck') at weights (1.0, 0.5), run under the py3 shims of
make_golden.py (same directory) on seeded poses -> tests/golden/reference_track_costs.json (inputs + expected outputs, a few KB).

Run in the build container only (needs the reference checkout):
    python tests/golden/make_golden_track_costs.py

The seeded poses include a head of length zero (head size 1), keypoints at a normalised distance of EXACTLY the threshold 0.5 (not a
match: the comparison is strict) and just inside it.  `cnn-cosdist` cannot be generated here: the reference computes it with torchvision,
cv2 and CUDA, none of which exist in this environment.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_shims, _Stub  # noqa: E402

# the person keypoints of the PoseTrack annotation files (`person_cat_info['keypoints']`)
POSETRACK_KEYPOINTS = ['nose', 'head_bottom', 'head_top', 'left_ear', 'right_ear', 'left_shoulder', 'right_shoulder', 'left_elbow',
                       'right_elbow', 'left_wrist', 'right_wrist', 'left_hip', 'right_hip', 'left_knee', 'right_knee', 'left_ankle',
                       'right_ankle']


class _Dataset(object):
    person_cat_info = {'keypoints': POSETRACK_KEYPOINTS}


def seeded_poses(seed=31, n_prev=5, n_cur=6):
    """(prev, cur): lists of 4 x 17 float32 poses on a half-pixel grid, so that distances and head sizes are exact in float64."""
    rs = np.random.RandomState(seed)
    K = len(POSETRACK_KEYPOINTS)
    top, bottom = POSETRACK_KEYPOINTS.index('head_top'), POSETRACK_KEYPOINTS.index('head_bottom')
    prev = []
    for i in range(n_prev):
        p = np.zeros((4, K), dtype=np.float32)
        p[:2] = rs.randint(100, 600, (2, K))
        p[2:] = rs.uniform(0, 1, (2, K))
        p[:2, top] = (200 + 10 * i, 100)
        p[:2, bottom] = (203 + 10 * i, 104)            # a 3-4-5 triangle: head size 6
        prev.append(p)
    prev[0][:2, bottom] = prev[0][:2, top]             # zero head length: head size 1
    cur = []
    for j in range(n_cur):
        src = prev[j % n_prev]
        p = src.copy()
        p[:2] += rs.choice([0.0, 1.0, 2.0, 30.0], size=(2, K)).astype(np.float32)
        p[2:] = rs.uniform(0, 1, (2, K))
        cur.append(p)
    # exactly at the threshold: distance 3 of head size 6 (prev 1 / cur 1), distance 0.5 of head size 1 (prev 0 / cur 0); just inside: 2.5
    cur[1][:2, 5] = prev[1][:2, 5] + np.float32([3.0, 0.0])
    cur[1][:2, 6] = prev[1][:2, 6] + np.float32([0.0, 2.5])
    cur[0][:2, 7] = prev[0][:2, 7] + np.float32([0.5, 0.0])
    cur[0][:2, 8] = prev[0][:2, 8] + np.float32([0.0, 0.0])
    return prev, cur


def seeded_boxes(seed, n):
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 400, (n, 2))
    wh = rs.uniform(40, 200, (n, 2))
    return np.hstack([xy, xy + wh, rs.uniform(0.9, 1.0, (n, 1))]).astype(np.float32)


def main():
    _install_shims()
    sys.modules['utils.vis'] = _Stub('utils.vis')       # matplotlib drawing only
    import core.tracking_engine as ref
    import utils.keypoints as ref_kps
    prev, cur = seeded_poses()
    prev_boxes, cur_boxes = seeded_boxes(41, len(prev)), seeded_boxes(42, len(cur))
    pck = [[float(ref_kps.pck_distance(a, b, POSETRACK_KEYPOINTS)) for b in cur] for a in prev]
    entry = {'dataset': _Dataset(), 'image': '/data/vid00/00000.jpg'}
    types, wts = ('bbox-overlap', 'pose-pck'), (1.0, 0.5)
    combined = ref._compute_distance_matrix(entry, prev_boxes, prev, entry, cur_boxes, cur, types, wts)
    out = {'keypoints': POSETRACK_KEYPOINTS, 'cost_types': list(types), 'cost_weights': list(wts),
           'prev_poses': [p.astype(np.float64).tolist() for p in prev], 'cur_poses': [p.astype(np.float64).tolist() for p in cur],
           'prev_boxes': prev_boxes.astype(np.float64).tolist(), 'cur_boxes': cur_boxes.astype(np.float64).tolist(),
           'pck': pck, 'combined': np.asarray(combined, dtype=np.float64).tolist()}
    with open(os.path.join(HERE, 'reference_track_costs.json'), 'w') as f:
        json.dump(out, f)
    print('wrote reference_track_costs.json: pck %dx%d, distinct values %s' % (len(prev), len(cur), sorted(set(sum(pck, [])))))


if __name__ == '__main__':
    main()
