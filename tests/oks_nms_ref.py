"""Seeded inputs for the OKS-NMS tests (tests/test_gpu_oks_nms.py) and the margin check that makes a comparison of keep lists
meaningful: clusters of jittered poses whose similarities fall on both sides of the threshold."""
import numpy as np

K = 17
THRESH = 0.3
OKS_MARGIN = 1e-6          # every evaluated OKS is further than this from the threshold ...
SCORE_MARGIN = 1e-4        # ... and neighbouring scores differ by more than this, relative (tests/golden/make_golden_oks_nms.py)


def seed_for(n, T):
    """The seed of case (n rows, T frames).  Checked on the CPU with the host twin (dat_oks_nms_host): every case of the GPU test passes
    `margins` with these seeds, so no case is ever skipped."""
    return 1000 + 17 * n + T


def clustered_poses(n, T, seed):
    """n rows in clusters of about four: kps fp32 [n, 4, 17 T], dets fp32 [n, 4 T + 2] = [boxes | score | class 1].  A cluster's rows are
    one pose plus per-keypoint noise of 0.02 ... 0.25 of the box side (OKS from about 0.9 down to 0.1), in boxes that differ a little, so
    that the kept row's area matters.  Scores (mean logits) are 1 + 0.01 * a permutation of 0 .. n-1: 2.5e-3 apart, relative, at worst."""
    rs = np.random.RandomState(seed)
    kps = np.zeros((n, 4, K * T), dtype=np.float32)
    dets = np.zeros((n, 4 * T + 2), dtype=np.float32)
    pattern = rs.uniform(-0.5, 0.5, K * T)
    pattern -= pattern.mean()
    score = 1.0 + 0.01 * rs.permutation(n)
    r = 0
    while r < n:
        m = min(n - r, int(rs.randint(2, 7)))
        wh = rs.uniform(30, 200, (T, 2))
        xy = rs.uniform(0, 1000, (T, 2))
        pose = rs.uniform(0, 1, (T, 2, K))
        for i in range(r, r + m):
            f = rs.uniform(0.02, 0.25)
            for t in range(T):
                box_xy = xy[t] + rs.uniform(-2, 2, 2)
                box_wh = wh[t] * rs.uniform(0.9, 1.1, 2)
                dets[i, 4 * t:4 * t + 4] = (box_xy[0], box_xy[1], box_xy[0] + box_wh[0], box_xy[1] + box_wh[1])
                side = np.sqrt(wh[t, 0] * wh[t, 1])
                kps[i, 0, t * K:(t + 1) * K] = xy[t, 0] + pose[t, 0] * wh[t, 0] + rs.normal(0, f, K) * side
                kps[i, 1, t * K:(t + 1) * K] = xy[t, 1] + pose[t, 1] * wh[t, 1] + rs.normal(0, f, K) * side
            kps[i, 2] = score[i] + pattern
            kps[i, 3] = rs.uniform(0, 1, K * T)
            dets[i, 4 * T] = rs.uniform(0.1, 1.0)
            dets[i, 4 * T + 1] = 1.0
        r += m
    return kps, dets


def margins(scores, oks, thresh=THRESH):
    """(smallest |OKS - thresh| over the evaluated pairs, smallest relative gap of neighbouring scores) of a dat_oks_nms_host run."""
    seen = oks[~np.isnan(oks)]
    m_oks = float(np.abs(seen - thresh).min()) if seen.size else 1.0
    s = np.sort(np.asarray(scores, dtype=np.float64))
    m_score = float((np.diff(s) / np.maximum(np.abs(s[1:]), np.abs(s[:-1]))).min()) if s.size > 1 else 1.0
    return m_oks, m_score
