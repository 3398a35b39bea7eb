"""Inputs and NumPy restatements shared by tests/test_tube_soft_nms_cpu.py and tests/test_gpu_tube_soft_nms.py: Soft-NMS and box voting
for tubes (rows of 4T coordinates + score) as DESIGN.md section 3.13 defines them.

The overlap of two tubes: per frame the IoU in the C float arithmetic of dat_soft_nms_host (the current maximum row `a` keeps its
area in double, `b`'s area and the union are rounded to float32, 0 when iw <= 0 or ih <= 0); the T values are added in float32 in
frame order starting from 0 and divided by float32(T)."""
import ctypes as C

import numpy as np

METHODS = ('hard', 'linear', 'gaussian')
SIGMA, NT, THRESH = 0.5, 0.3, 0.001
ULP = 2.0 ** -23                             # one float32 ulp, relative
F32, F64 = np.float32, np.float64


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def grid_tubes(n, T, seed):
    """Integer-grid tubes: corners randint(20, 200), sizes randint(10, 60), every frame moved by randint(-4, 5) in x and y; the scores
    are a permutation of n distinct values in [0.05, 0.95]."""
    rs = np.random.RandomState(seed)
    c = rs.randint(20, 200, (n, 1, 2))
    s = rs.randint(10, 60, (n, 1, 2))
    xy = c + rs.randint(-4, 5, (n, T, 2))
    coords = np.concatenate((xy, xy + s), axis=2).reshape(n, 4 * T)
    scores = np.linspace(0.05, 0.95, n).astype(F32)[rs.permutation(n)] if n else np.zeros((0,), F32)
    return np.hstack((coords.astype(F32), scores[:, None])).astype(F32)


def smooth_tubes(n, T, seed):
    """Continuous coordinates and scores, dense enough (corners in a 150 x 150 window, sizes 40 .. 120, frames moved by up to 4) that
    64 rows already re-score one another below the threshold."""
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 150, (n, 1, 2)) + rs.uniform(-4, 4, (n, T, 2))
    wh = rs.uniform(40, 120, (n, 1, 2)) + rs.uniform(-4, 4, (n, T, 2))
    coords = np.concatenate((xy, xy + wh), axis=2).reshape(n, 4 * T)
    return np.hstack((coords, rs.uniform(0.05, 1.0, (n, 1)))).astype(F32)


def tie_tubes(n, T, seed):
    """The tube form of soft_nms_cases.tie_dets: scores drawn from 8 values and a quarter of the rows duplicates of other rows, so
    positions decide nearly every arg-max and overlaps of exactly 1 occur."""
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 300, (n, 1, 2)) + rs.uniform(-4, 4, (n, T, 2))
    wh = rs.uniform(10, 160, (n, 1, 2))
    coords = np.concatenate((xy, xy + wh), axis=2).reshape(n, 4 * T)
    levels = np.linspace(0.15, 0.95, 8).astype(F32)
    rows = np.hstack((coords, levels[rs.randint(0, 8, n)][:, None])).astype(F32)
    if n >= 4:
        dst = rs.permutation(n)[:n // 4]
        rows[dst, :4 * T] = rows[rs.randint(0, n, n // 4), :4 * T]
    return rows


# ---- the definition --------------------------------------------------------------------------------------------------------------
def tube_ov(a, rows, T):
    """float32 overlaps of the row `a` [4T] (the current maximum / the kept row) with `rows` [m, >= 4T]."""
    a = np.asarray(a, F32)
    rows = np.asarray(rows, F32)
    total = np.zeros(len(rows), F32)
    for t in range(T):
        tx1, ty1, tx2, ty2 = (a[4 * t + k] for k in range(4))
        x1, y1, x2, y2 = (rows[:, 4 * t + k] for k in range(4))
        area = (((x2 - x1).astype(F64) + 1.0) * ((y2 - y1).astype(F64) + 1.0)).astype(F32)
        iw = ((np.minimum(tx2, x2) - np.maximum(tx1, x1)).astype(F64) + 1.0).astype(F32)
        ih = ((np.minimum(ty2, y2) - np.maximum(ty1, y1)).astype(F64) + 1.0).astype(F32)
        tarea = (F64(tx2 - tx1) + 1.0) * (F64(ty2 - ty1) + 1.0)
        inter = iw * ih
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            ua = ((tarea + area.astype(F64)) - inter.astype(F64)).astype(F32)
            iou = np.where((iw > 0) & (ih > 0), inter / ua, F32(0)).astype(F32)
        total = (total + iou).astype(F32)
    return (total / F32(T)).astype(F32)


def _weights(ov, method, sigma, nt):
    with np.errstate(over='ignore'):
        if method == 'linear':
            return np.where(ov > F32(nt), (1.0 - ov.astype(F64)).astype(F32), F32(1))
        if method == 'gaussian':
            return np.exp((-(ov * ov) / F32(sigma)).astype(F64)).astype(F32)
        return np.where(ov > F32(nt), F32(0), F32(1))


def serial_soft_nms(dets, T, method, sigma=SIGMA, nt=NT, thresh=THRESH, count_rescorings=False, audit=None):
    """The loop of lib/utils/cython_nms.pyx:98-203 for rows [n, 4T+1]: arg-max with strict `<` (the earliest position wins), swap,
    re-score the positions (i, N) -- a pair iff its overlap is > 0 -- and remove a row re-scored below `thresh` by the swap-with-last
    walk, which visits the slot again.  (Every re-score depends on row i and the row itself only, so the new scores are formed at
    once; the walk below is the serial one, row by row.)  Returns (rows, original indices[, re-scorings each output row received]).
    audit (a dict) receives: `slack`, as soft_nms_cases.parallel_soft_nms defines it (the smallest margin of any decision of the run
    minus the allowance of the device comparison at that decision, in units of ULP * score); `nt_gap`, the smallest |ov - nt| over
    all compared pairs; `rescored`, the number of re-scorings."""
    cols = 4 * T + 1
    b = np.array(dets, dtype=F32, copy=True).reshape(-1, cols)
    idx = np.arange(len(b))
    hits = np.zeros(len(b), np.int64)
    N, i = len(b), 0
    while i < N:
        m = i + int(np.argmax(b[i:N, -1]))                # np.argmax returns the first maximum
        if audit is not None and N > i + 1:
            rest = np.delete(np.arange(i, N), m - i)
            gap = (F64(b[m, -1]) - b[rest, -1].astype(F64)) / (ULP * F64(abs(b[m, -1])))
            audit['slack'] = min(audit.get('slack', np.inf), float(np.min(gap - (hits[m] + hits[rest]))))
        for a in (b, idx, hits):
            a[[i, m]] = a[[m, i]]
        if N > i + 1:
            ov = tube_ov(b[i], b[i + 1:N], T)
            hit = ov > 0
            new = np.where(hit, (_weights(ov, method, sigma, nt) * b[i + 1:N, -1]).astype(F32), b[i + 1:N, -1])
            b[i + 1:N, -1] = new
            hits[i + 1:N] += hit
            if audit is not None:
                audit['nt_gap'] = min(audit.get('nt_gap', np.inf), float(np.min(np.abs(ov.astype(F64) - F64(F32(nt))))))
                audit['rescored'] = audit.get('rescored', 0) + int(hit.sum())
                if hit.any():
                    d = np.abs(new[hit].astype(F64) - F32(thresh)) / (ULP * F64(F32(thresh)))
                    audit['slack'] = min(audit.get('slack', np.inf), float(np.min(d - hits[i + 1:N][hit])))
            dead = np.zeros(N, bool)
            dead[i + 1:N] = hit & (new < F32(thresh))
            if dead.any():
                pos = i + 1
                while pos < N:
                    if dead[pos]:                        # discard: the last row comes here, N shrinks, the slot is visited again
                        for a in (b, idx, hits, dead):
                            a[pos] = a[N - 1]
                        N -= 1
                    else:
                        pos += 1
        i += 1
    return (b[:N], idx[:N], hits[:N]) if count_rescorings else (b[:N], idx[:N])


def vote_f64(top, all_dets, T, thresh):
    """Tube voting: for every row of `top` the float64 score-weighted mean of ALL 4T coordinates over the rows of `all_dets` whose
    float32 tube_ov with it (the kept row in a's role) is >= thresh; the score stays.  Returns (rows float64, voters per row, and per
    row the float32 accumulation bound (m + 2) * 2^-24 * max|coordinate of its m voters| of tests/test_gpu_soft_nms.py)."""
    c4 = 4 * T
    out = np.asarray(top, F32).astype(F64)
    voters = np.zeros(len(top), np.int64)
    bound = np.zeros((len(top), 1))
    for k in range(len(top)):
        v = np.where(tube_ov(top[k, :c4], all_dets[:, :c4], T) >= F32(thresh))[0]
        w = all_dets[v, c4].astype(F64)
        out[k, :c4] = (all_dets[v, :c4].astype(F64) * w[:, None]).sum(axis=0) / w.sum()
        voters[k] = len(v)
        bound[k] = (len(v) + 2) * 2.0 ** -24 * np.abs(all_dets[v, :c4]).max()
    return out, voters, bound


def one_ulp(ref):
    """One float32 ulp at every value of `ref` (float64): the bound of a float64 mean rounded to float32 once."""
    return np.spacing(np.abs(ref).astype(F32)).astype(F64)


# ---- the host twin ---------------------------------------------------------------------------------------------------------------
def host_soft_nms_tubes(dets, T, method, sigma=SIGMA, nt=NT, thresh=THRESH):
    """dat_soft_nms_tubes_host through the C ABI (no config switch involved): (rows, original indices)."""
    from detectandtrack_amd import libdat as L
    src = np.ascontiguousarray(dets, dtype=F32).reshape(-1, 4 * T + 1)
    n = src.shape[0]
    out = np.empty((max(n, 1), 4 * T + 1), F32)
    inds = np.empty((max(n, 1),), np.int32)
    m = C.c_int(0)
    rc = L.lib().dat_soft_nms_tubes_host(src.ctypes.data_as(C.POINTER(C.c_float)), n, T, F32(sigma), F32(nt), F32(thresh),
                                         METHODS.index(method), out.ctypes.data_as(C.POINTER(C.c_float)),
                                         inds.ctypes.data_as(C.POINTER(C.c_int)), C.byref(m))
    assert rc == L.DAT_OK, rc
    return out[:m.value], inds[:m.value].astype(np.int64)


# (T, n, seed) of the gaussian cases of the device comparison; tests/test_tube_soft_nms_cpu.py asserts that every one qualifies
GPU_SIZES = (0, 1, 2, 63, 64, 65, 257, 1000, 2048)
CAPACITY_T5 = 1792                           # dat_soft_nms_tubes_max_boxes(5): (160 KB - 512) / (16 * 5 + 11) bytes, down to a multiple of 64
_SEEDS = {(2, 257): 1206, (3, 2048): 1308}   # (the seeds 100 T + k of these two leave a decision inside the allowance: they do not qualify)
GAUSSIAN_CASES = tuple((T, n, _SEEDS.get((T, n), 100 * T + k)) for T in (2, 3) for k, n in enumerate(GPU_SIZES)) + ((5, CAPACITY_T5, 555),)
