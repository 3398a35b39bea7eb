"""Float64 CPU restatements of the inference kernels that tests/test_gpu_infer_kernels.py holds to per-element bounds: RoIAlign
forward (csrc/roi_align.hip), the pooling / reduction / copy kernels of csrc/elementwise.hip and the word scatter of csrc/labels.hip.
The keypoint tail's reference is tests/train_refs.py's kps_finalize_ref.  tests/test_infer_refs_cpu.py checks them against the oracle.

As in tests/train_refs.py every function takes the operands as the kernel sees them (quantised to the build's 16-bit format where the
kernel reads 16-bit data) and returns float64: the reference, the same expression on absolute values (`absref`, the scale of the fp32
rounding term of tests/numerics.py), and where a path has an error source that term does not cover, a named per-element `extra`."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.train_refs import U32, _f64, roi_frames


# ---- RoIAlign forward -------------------------------------------------------------------------------------------------------------
def _gather(Ay, Ax, sup_y, sup_x, blk):
    """sum_{h, w} Ay[p, h] Ax[q, w] blk[h, w, c] with the matrices cut to the support rows / columns of the block: -> [p, q, c]."""
    t1 = np.tensordot(Ay[:, sup_y], blk, axes=(1, 0))                       # (p, w, c)
    return np.tensordot(t1, Ax[:, sup_x], axes=(1, 1)).transpose(0, 2, 1)


def roi_align_ref(feats, scales, rois, T, Tr, t0, pooled, sampling, k_min=2, canon_scale=224., canon_level=4, strict=True):
    """dat_roi_align: the legacy RoIAlign (oracle/roi_align.py) over [frames, H, W, C] maps (finest level first) with the FPN level
    picked per roi, the transpose of train_refs.roi_align_bwd_ref:

        out[r*Tr + t, p, q, :] = 1 / (gh*gw) * sum_h sum_w Ay[p, h] Ax[q, w] feat[level][frame, h, w, :]

    Returns (ref, absref, extra, K) for out [R*Tr, P, P, C]: absref is the same on |feat|, extra the taps' weight error from the fp32
    sample coordinates ((Ey Ix + Iy Ex) on |feat|, over gh*gw) and K = 4*gh*gw, the largest number of taps summed into one element.
    Raises where a sample lies within the fp32 coordinate error of a validity cut-off, unless strict=False (train_refs._axis)."""
    fs = [_f64(f).astype(np.float64) for f in feats]
    afs = [np.abs(f) for f in fs]
    shapes = [f.shape[:3] for f in fs]
    C = fs[0].shape[-1]
    P = pooled
    rows = _f64(rois).shape[0] * Tr
    ref, ab, ex = np.zeros((rows, P, P, C)), np.zeros((rows, P, P, C)), np.zeros((rows, P, P, C))
    K = 4
    for row, li, fr, gh, gw, (Ay, Iy, Ey), (Ax, Ix, Ex) in roi_frames(shapes, scales, rois, T, Tr, t0, P, sampling, k_min,
                                                                      canon_scale, canon_level, strict):
        K = max(K, 4 * gh * gw)
        hs, ws = np.nonzero(Iy.any(0))[0], np.nonzero(Ix.any(0))[0]           # only the rows and columns the roi touches
        if len(hs) == 0 or len(ws) == 0:
            continue
        sy, sx = slice(hs[0], hs[-1] + 1), slice(ws[0], ws[-1] + 1)
        inv = 1.0 / (gh * gw)
        blk, ablk = fs[li][fr, sy, sx], afs[li][fr, sy, sx]
        ref[row] = _gather(Ay, Ax, sy, sx, blk) * inv
        ab[row] = _gather(Ay, Ax, sy, sx, ablk) * inv
        ex[row] = (_gather(Ey, Ix, sy, sx, ablk) + _gather(Iy, Ex, sy, sx, ablk)) * inv
    return ref, ab, ex, K


# ---- pooling, reductions ----------------------------------------------------------------------------------------------------------
def time_avg_ref(x, N, T):
    """dat_time_avg: x [N*T, ...] -> the mean over the T frames of each clip [N, ...].  -> (ref, absref)."""
    a = _f64(x).astype(np.float64)
    a = a.reshape((N, T) + a.shape[1:])
    return a.mean(1), np.abs(a).mean(1)


def spatial_mean_ref(x, C):
    """dat_spatial_mean: x [frames, H, W, Cs] (Cs >= C) -> the mean over H, W of the first C channels [frames, C].  -> (ref, absref)."""
    a = _f64(x).astype(np.float64)
    a = a.reshape(a.shape[0], -1, a.shape[-1])[:, :, :C]
    return a.mean(1), np.abs(a).mean(1)


def softmax_rows_ref(x, K):
    """dat_softmax_rows: softmax over the first K columns of x [rows, ld_in] (ld_in >= K).  -> (p, extra): x - max rounds in fp32
    (absolute 2^-24 |x - max|) and exp turns that into a relative error of each term, of p_k directly and of the row sum through
    sum_j p_j |x_j - max| -- the term tests/train_refs.py's softmax_ce_ref names."""
    a = _f64(x).astype(np.float64)[:, :K]
    if a.shape[0] == 0:
        return a.copy(), a.copy()
    m = a.max(1, keepdims=True)
    e = np.exp(a - m)
    p = e / e.sum(1, keepdims=True)
    dxm = np.abs(a - m)
    spread = (p * dxm).sum(1, keepdims=True)
    return p, p * (dxm + spread) * U32


def maxpool_hw_ref(x, k, stride, pad):
    """dat_maxpool_hw: MaxPool [1, k, k] on [frames, H, W, C]; padding cells behave as -inf."""
    a = torch.from_numpy(_f64(x).astype(np.float64)).permute(0, 3, 1, 2)
    return F.max_pool2d(a, k, stride, pad).permute(0, 2, 3, 1).numpy()


def split_bf16x2_ref(x):
    """dat_split_bf16x2: fp32 [npos, C] (C % 64 == 0) -> fp32 values of the bf16 split [npos, 2C]: per 64-channel chunk q the 64
    values bf16(x) (line 2q) and then the 64 values bf16(x - bf16(x)) (line 2q + 1)."""
    from tests.numerics import q16
    a = np.ascontiguousarray(_f64(x), np.float32)
    npos, C = a.shape
    hi = q16(a, 'bf16')
    lo = q16(a - hi, 'bf16')                                                 # the difference is exact in fp32
    return np.stack([hi.reshape(npos, C // 64, 64), lo.reshape(npos, C // 64, 64)], axis=2).reshape(npos, 2 * C)


# ---- copies -----------------------------------------------------------------------------------------------------------------------
def copy_frames_ref(src, src_idx, dst, dst_idx):
    """dat_copy_frames: dst[dst_idx[i]] = src[src_idx[i]] over whole frames; every other frame of dst stays."""
    out = np.array(dst, copy=True)
    for s, d in zip(src_idx, dst_idx):
        out[d] = src[s]
    return out


def scatter_words_ref(dst, offsets, values):
    """dat_scatter_words: dst.view(32-bit words)[offsets[i]] = values[i]; an offset outside [0, words) is ignored."""
    out = np.array(dst, copy=True)
    w = out.reshape(-1).view(np.uint32)
    offsets = np.asarray(offsets, np.int64)
    ok = (offsets >= 0) & (offsets < w.size)
    w[offsets[ok]] = np.ascontiguousarray(values).reshape(-1).view(np.uint32)[ok]
    return out
