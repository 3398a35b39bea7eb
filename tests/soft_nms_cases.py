"""Inputs and the NumPy restatement shared by tests/test_soft_nms_cpu.py and tests/test_gpu_soft_nms.py."""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ('hard', 'linear', 'gaussian')
SIGMA, NT, THRESH = 0.5, 0.3, 0.001          # the arguments of the golden file (tests/golden/make_golden.py)
TIE_SIZES = (0, 1, 2, 63, 64, 65, 1000)
CAPACITY = 2048                              # DAT_SOFT_NMS_MAX_BOXES
ULP = 2.0 ** -23                             # one float32 ulp, relative (test 3's unit for the gaussian scores)


def golden_dets():
    return np.load(os.path.join(REPO, 'tests', 'golden', 'reference_postproc.npz'))['soft_dets']


def tie_dets(n, seed):
    """n random boxes in a 300 x 300 window (plenty of overlap) with scores drawn from 8 distinct values: ties everywhere."""
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 300, (n, 2))
    wh = rs.uniform(10, 160, (n, 2))
    levels = np.linspace(0.15, 0.95, 8).astype(np.float32)
    return np.hstack((xy, xy + wh, levels[rs.randint(0, 8, n)][:, None])).astype(np.float32)


def smooth_dets(n, seed):
    """n random boxes with continuous scores: the gaussian inputs of the device comparison (qualified on the CPU)."""
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 400, (n, 2))
    wh = rs.uniform(10, 200, (n, 2))
    return np.hstack((xy, xy + wh, rs.uniform(0.05, 1.0, (n, 1)))).astype(np.float32)


# (n, seed) of the gaussian cases; test_soft_nms_cpu.py asserts that every one of them qualifies
GAUSSIAN_CASES = ((1, 11), (2, 12), (63, 13), (64, 14), (65, 15), (300, 16), (1000, 17), (CAPACITY, 18))


def host_soft_nms(dets, method, sigma=SIGMA, nt=NT, thresh=THRESH):
    from detectandtrack_amd.core import nms_wrapper
    return nms_wrapper.soft_nms(dets, sigma=sigma, overlap_thresh=nt, score_thresh=thresh, method=method)


def _rescore(box, rows, method, sigma, nt):
    """New scores of `rows` [m, 5] against `box` in the C float order of lib/utils/cython_nms.pyx:139-181 (see dat_soft_nms_host),
    and the mask of the rows the loop re-scored (iw > 0 and ih > 0: only those are tested against the threshold)."""
    f32, f64 = np.float32, np.float64
    tx1, ty1, tx2, ty2 = (f32(v) for v in box[:4])
    x1, y1, x2, y2, s = (rows[:, c] for c in range(5))
    area = (((x2 - x1).astype(f64) + 1.0) * ((y2 - y1).astype(f64) + 1.0)).astype(f32)
    iw = ((np.minimum(tx2, x2) - np.maximum(tx1, x1)).astype(f64) + 1.0).astype(f32)
    ih = ((np.minimum(ty2, y2) - np.maximum(ty1, y1)).astype(f64) + 1.0).astype(f32)
    hit = (iw > 0) & (ih > 0)
    tarea = (f64(tx2 - tx1) + 1.0) * (f64(ty2 - ty1) + 1.0)
    inter = iw * ih
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        ua = ((tarea + area.astype(f64)) - inter.astype(f64)).astype(f32)
        ov = inter / ua
        if method == 'linear':
            w = np.where(ov > f32(nt), (1.0 - ov.astype(f64)).astype(f32), f32(1))
        elif method == 'gaussian':
            w = np.exp((-(ov * ov) / f32(sigma)).astype(f64)).astype(f32)
        else:
            w = np.where(ov > f32(nt), f32(0), f32(1))
        new = (w * s).astype(f32)
    return np.where(hit, new, s), hit


def parallel_soft_nms(dets, method, sigma=SIGMA, nt=NT, thresh=THRESH, count_rescorings=False, audit=None):
    """The specification soft_nms_kernel is written from: per iteration, arg-max with the earliest position winning ties, swap,
    re-score ALL later positions at once, then survivors below the new N stay and the holes below it, ascending, receive the
    surviving tail rows, descending.  Returns (rows, original indices[, re-scorings each output row received]).
    audit (a dict): receives `slack`, the smallest margin of any decision of the run minus the tolerance of the device comparison at
    that decision, in units of ULP * score -- a winner over the best other candidate (tolerance: the re-scorings both rows have
    received so far), and a re-scored score against the threshold (tolerance: its re-scorings)."""
    b = np.array(dets, dtype=np.float32, copy=True)
    idx = np.arange(len(b))
    hits = np.zeros(len(b), np.int64)
    N, i = len(b), 0
    while i < N:
        m = i + int(np.argmax(b[i:N, 4]))                 # np.argmax returns the first maximum
        if audit is not None and N > i + 1:
            rest = np.delete(np.arange(i, N), m - i)
            gap = (np.float64(b[m, 4]) - b[rest, 4].astype(np.float64)) / (ULP * np.float64(abs(b[m, 4])))
            audit['slack'] = min(audit.get('slack', np.inf), float(np.min(gap - (hits[m] + hits[rest]))))
        for a in (b, idx, hits):
            a[[i, m]] = a[[m, i]]
        if N > i + 1:
            new, hit = _rescore(b[i], b[i + 1:N], method, sigma, nt)
            b[i + 1:N, 4] = new
            hits[i + 1:N] += hit
            if audit is not None and hit.any():
                d = np.abs(new[hit].astype(np.float64) - np.float32(thresh)) / (ULP * np.float64(np.float32(thresh)))
                audit['slack'] = min(audit.get('slack', np.inf), float(np.min(d - hits[i + 1:N][hit])))
            dead = np.zeros(N, bool)
            dead[i + 1:N] = hit & (new < np.float32(thresh))
            N2 = N - int(dead.sum())
            holes = np.where(dead[:N2])[0]
            fill = (N2 + np.where(~dead[N2:N])[0])[::-1]
            assert len(holes) == len(fill)
            for a in (b, idx, hits):
                a[holes] = a[fill]
            N = N2
        i += 1
    return (b[:N], idx[:N], hits[:N]) if count_rescorings else (b[:N], idx[:N])
