"""The exact host statement of the device proposal path (csrc/proposals.hip): NumPy only, float32 in the kernels' operation order.

keys -> select -> decode -> filter -> NMS -> emit, and the FPN collect, follow rpn_keys_hist_kernel (K0), the K1-K3 selection,
decode_tube, rpn_emit_kernel and collect_rois_kernel line by line.  Every intermediate is np.float32, no product is fused into a
sum (the kernels are compiled with -ffp-contract=off) and `ws / 2` stays a division, as written there.  The one operation NumPy's
float32 cannot state is the device's exp, a double exp rounded once: it is np.exp(float64) rounded to float32 here, and
`exp_is_safe` tells for which arguments a double exp that is an ulp off still rounds to the same float32 -- a condition on a
test's inputs, not a tolerance on its outputs.

The order rule is the one of oracle/proposals.py: higher score first, then lower flat (h, w, a) index.
"""
import numpy as np

from oracle.nms import nms as oracle_nms

F32 = np.float32
XFORM_CLIP = F32(np.log(1000. / 16.))          # float32(log(1000 / 16)) = 4.135166556742356f, decode_tube's `clip`


class Level(object):
    """Host twin of hip_ops.RpnLevelSpec: the geometry of one RPN level inside a head array [frames, H, W, cstride]."""

    def __init__(self, H, W, A, T, feat_stride, cstride, logit_off, delta_off, frame, anchors, apply_sigmoid=False, per_frame=False):
        self.H, self.W, self.A, self.T = int(H), int(W), int(A), int(T)
        self.feat_stride, self.cstride = float(feat_stride), int(cstride)
        self.logit_off, self.delta_off, self.frame = int(logit_off), int(delta_off), int(frame)
        self.anchors = np.ascontiguousarray(anchors, dtype=F32).reshape(self.A, 4 * self.T)
        self.apply_sigmoid, self.per_frame = bool(apply_sigmoid), bool(per_frame)

    @property
    def N(self):
        return self.H * self.W * self.A

    def at_frame(self, frame):
        return Level(self.H, self.W, self.A, self.T, self.feat_stride, self.cstride, self.logit_off, self.delta_off, frame, self.anchors,
                     self.apply_sigmoid, self.per_frame)


def _head(head, spec):
    head = np.asarray(head)
    assert head.dtype == F32 and head.ndim == 4 and head.shape[1:] == (spec.H, spec.W, spec.cstride), (head.dtype, head.shape)
    return head


def keys(head, spec):
    """The probability of every anchor in flat (h, w, a) order, float32 [N] (K0).  per_frame: the T frames' logits added one after
    the other in float32 and divided by float32(T).  apply_sigmoid: the kernel's 1 / (1 + exp(-l)) in float32 with a correctly
    rounded exp in place of expf -- exact where exp(-l) overflows (0) or vanishes against 1 (1.0), within a few ulps elsewhere;
    tests of that path keep distinct probabilities 2^-16 apart and compare mid-range values to 1e-6."""
    head = _head(head, spec)
    sl = slice(spec.logit_off, spec.logit_off + spec.A)
    logit = head[spec.frame, :, :, sl].reshape(-1).copy()
    if spec.per_frame:
        for t in range(1, spec.T):
            logit = logit + head[spec.frame + t, :, :, sl].reshape(-1)
        logit = logit / F32(spec.T)
    assert logit.dtype == F32
    if spec.apply_sigmoid:
        with np.errstate(over='ignore'):
            e = np.exp(-logit.astype(np.float64)).astype(F32)       # (inf beyond the float32 range, as expf: the probability is 0)
        return F32(1) / (F32(1) + e)
    return logit


def select(k, pre_nms):
    """Flat indices of the min(pre_nms, N) best keys: score descending, then flat index ascending (K1-K3's composite order)."""
    k = np.asarray(k, dtype=F32)
    assert not np.signbit(k).any() and not np.isnan(k).any(), 'keys are probabilities: the bit pattern must be monotonic'
    return np.argsort(-k, kind='stable')[:min(int(pre_nms), k.shape[0])]


def exp_f32(x):
    """The device's `(float)exp((double)x)`."""
    return np.exp(np.asarray(x, dtype=F32).astype(np.float64)).astype(F32)


def exp_is_safe(x, margin=16):
    """True where exp(float64(x)) lies at least `margin` double ulps from both float32 rounding midpoints around it: a double exp
    that is an ulp off (any libm's) then rounds to the same float32."""
    x = np.minimum(np.asarray(x, dtype=F32), XFORM_CLIP)
    y = np.exp(x.astype(np.float64))
    f = y.astype(F32)
    up = (f.astype(np.float64) + np.nextafter(f, F32(np.inf)).astype(np.float64)) / 2
    dn = (f.astype(np.float64) + np.nextafter(f, F32(-np.inf)).astype(np.float64)) / 2
    dist = np.minimum(np.abs(up - y), np.abs(y - dn))
    return dist >= margin * np.spacing(y)


def min_size_scaled(min_size, scale):
    """dat_rpn_proposals_batch: float32(float64(min_size) * float64(scale)) of the two float32 arguments."""
    return F32(np.float64(F32(min_size)) * np.float64(F32(scale)))


def decode(idx, head, spec, im_info, min_size):
    """decode_tube for the flat anchor indices `idx`: (boxes float32 [n, 4T], ok bool [n]).  im_info = (im_h, im_w, scale)."""
    head = _head(head, spec)
    idx = np.asarray(idx, dtype=np.int64)
    im_h, im_w, scale = F32(im_info[0]), F32(im_info[1]), F32(im_info[2])
    mss = min_size_scaled(min_size, scale)
    A, T, W = spec.A, spec.T, spec.W
    pos, a = idx // A, idx % A
    h, w = pos // W, pos % W
    fs = F32(spec.feat_stride)
    sx, sy = w.astype(F32) * fs, h.astype(F32) * fs
    half, one, zero = F32(0.5), F32(1), F32(0)
    out = np.zeros((idx.shape[0], 4 * T), F32)
    ok = np.ones(idx.shape[0], bool)
    for t in range(T):
        an = spec.anchors[a, 4 * t:4 * t + 4]
        ax1, ay1, ax2, ay2 = an[:, 0] + sx, an[:, 1] + sy, an[:, 2] + sx, an[:, 3] + sy
        if spec.per_frame:
            d = head[spec.frame + t, h, w]
            c0 = spec.delta_off + a * 4
        else:
            d = head[spec.frame, h, w]
            c0 = spec.delta_off + (a * T + t) * 4
        rows = np.arange(idx.shape[0])
        dx, dy, dw, dh = d[rows, c0], d[rows, c0 + 1], d[rows, c0 + 2], d[rows, c0 + 3]
        width, height = ax2 - ax1 + one, ay2 - ay1 + one
        cx, cy = ax1 + half * width, ay1 + half * height
        dw, dh = np.minimum(dw, XFORM_CLIP), np.minimum(dh, XFORM_CLIP)
        pcx, pcy = dx * width + cx, dy * height + cy
        pw, ph = exp_f32(dw) * width, exp_f32(dh) * height
        x1, y1, x2, y2 = pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph
        x1 = np.maximum(np.minimum(x1, im_w - one), zero)
        y1 = np.maximum(np.minimum(y1, im_h - one), zero)
        x2 = np.maximum(np.minimum(x2, im_w - one), zero)
        y2 = np.maximum(np.minimum(y2, im_h - one), zero)
        for c, v in enumerate((x1, y1, x2, y2)):
            assert v.dtype == F32
            out[:, 4 * t + c] = v
        ws, hs = x2 - x1 + one, y2 - y1 + one
        xc, yc = x1 + ws / F32(2), y1 + hs / F32(2)
        ok &= (ws >= mss) & (hs >= mss) & (xc < im_w) & (yc < im_h)
    return out, ok


def proposals(head, spec, im_info, pre_nms, post_nms, nms_thresh, min_size, batch_idx=0., select_fn=select):
    """One level of one image: (rois float32 [n, 4T+1], probs float32 [n], flat anchor indices int64 [n]), n <= post_nms, in the order
    rpn_emit_kernel writes them.  nms_thresh > 1 disables suppression (IoU <= 1): the result is the sorted, filtered list itself.
    select_fn: the selection rule (tests swap in wrong ones to show that a case tells them apart)."""
    k = keys(head, spec)
    idx = select_fn(k, pre_nms)
    boxes, ok = decode(idx, head, spec, im_info, min_size)
    idx, boxes, scores = idx[ok], boxes[ok], k[idx][ok]
    if nms_thresh <= 1 and idx.shape[0]:
        keep = np.asarray(oracle_nms(np.hstack((boxes, scores[:, None])), nms_thresh), dtype=np.int64)
        idx, boxes, scores = idx[keep], boxes[keep], scores[keep]
    idx, boxes, scores = idx[:post_nms], boxes[:post_nms], scores[:post_nms]
    rois = np.hstack((np.full((idx.shape[0], 1), batch_idx, F32), boxes)).astype(F32)
    return rois, scores.astype(F32), idx


def collect(rois_lvls, probs_lvls, counts, post_nms):
    """collect_rois_kernel for one image: rois_lvls [nl, cap, cols], probs_lvls [nl, cap], counts [nl] -> the min(total, post_nms)
    best rows, score descending, then position in the concatenation of the levels' first counts[l] rows ascending."""
    rois = np.concatenate([np.asarray(rois_lvls[l], F32)[:int(c)] for l, c in enumerate(counts)])
    probs = np.concatenate([np.asarray(probs_lvls[l], F32)[:int(c)] for l, c in enumerate(counts)])
    return rois[np.argsort(-probs, kind='stable')[:int(post_nms)]]
