"""A float64 reference of the conv weight gradient for tests/test_gpu_wgrad.py, a simulation of the kernels' fp32 accumulation and a
set of seeded defects -- the last two for tests/test_wgrad_refs_cpu.py, which shows on the CPU that the per-element bound of
tests/numerics.py lets a correctly accumulating kernel through and stops a wrong one.

Reference semantics: the ConvGradient of every ConvNd (lib/modeling/model_builder.py:908-951) with the fused AffineChannelNd scale
folded in,

    dW[co][ci][kt][kh][kw] = scale[co] * sum_p g[p][co] * x[in(p, tap)][ci],   in(p, tap) = (t + kt - pt, s oy + kh - ph, s ox + kw - pw),

written as ONE float64 matmul per tap over the zero-padded, strided, shifted slice of x: a second formulation next to
torch.nn.grad.conv3d_weight, which tests/test_wgrad_refs_cpu.py compares it with."""
import numpy as np
import torch

from tests import numerics as nm


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def out_hw(H, W, k, stride, pads):
    return (H + 2 * pads[1] - k[1]) // stride + 1, (W + 2 * pads[2] - k[2]) // stride + 1


def frame_range(N, T, window):
    """The output frames that count: the window (t0, n) of a single clip; every frame when N > 1 (hip_ops.ConvGrad.weight and the
    launcher ignore a window then) or without a window."""
    if window is None or N > 1:
        return 0, T
    t0, n = int(window[0]), int(window[1])
    assert 0 <= t0 and n > 0 and t0 + n <= T
    return t0, t0 + n


def _valid(n_out, off, step, size):
    """The outputs o in [0, n_out) whose input step * o + off lies in [0, size): (first o, one past the last o)."""
    lo = max(0, -(off // step))                 # ceil(-off / step)
    hi = min(n_out, (size - 1 - off) // step + 1)
    return lo, max(lo, hi)


def tap_matrix(x, tap, stride, pads, Ho, Wo, t_lo, t_hi):
    """(Cin, N * (t_hi - t_lo) * Ho * Wo) float64: the input of tap (kt, kh, kw) at every counted output position, zero where the tap
    falls into the padding."""
    N, Cin, T, H, W = x.shape
    kt, kh, kw = tap
    out = np.zeros((Cin, N, t_hi - t_lo, Ho, Wo))
    a_t, b_t = _valid(t_hi - t_lo, t_lo + kt - pads[0], 1, T)
    a_y, b_y = _valid(Ho, kh - pads[1], stride, H)
    a_x, b_x = _valid(Wo, kw - pads[2], stride, W)
    if b_t > a_t and b_y > a_y and b_x > a_x:
        t0 = a_t + t_lo + kt - pads[0]
        y0, x0 = stride * a_y + kh - pads[1], stride * a_x + kw - pads[2]
        sub = x[:, :, t0:t0 + (b_t - a_t), y0:y0 + stride * (b_y - a_y - 1) + 1:stride, x0:x0 + stride * (b_x - a_x - 1) + 1:stride]
        out[:, :, a_t:b_t, a_y:b_y, a_x:b_x] = np.transpose(sub, (1, 0, 2, 3, 4))
    return out.reshape(Cin, -1)


def grad_matrix(g, scale, t_lo, t_hi):
    """(Cout, N * (t_hi - t_lo) * Ho * Wo) float64: g (times the scale of its channel) at every counted output position."""
    g = _np(g)
    gm = np.transpose(g[:, :, t_lo:t_hi], (1, 0, 2, 3, 4)).astype(np.float64)
    if scale is not None:
        gm = gm * _np(scale).astype(np.float64).reshape(-1, 1, 1, 1, 1)
    return gm.reshape(g.shape[1], -1)


def taps_of(k):
    return [(kt, kh, kw) for kt in range(k[0]) for kh in range(k[1]) for kw in range(k[2])]


def wgrad_ref64(x, g, scale, k, stride, pads, window=None):
    """(ref, absref, K): dW (Cout, Cin, KT, KH, KW) in float64 from the given (already quantised) operands, the same sum over |x| and
    |g * scale|, and the number of output positions reduced.  x: (N, Cin, T, H, W); g: (N, Cout, T, Ho, Wo); scale: (Cout,) or None;
    stride: the spatial stride; pads: (pt, ph, pw); window = (t0, n): g counts only in those frames of a single clip."""
    x, g = _np(x), _np(g)
    N, Cin, T, H, W = x.shape
    Cout = g.shape[1]
    Ho, Wo = out_hw(H, W, k, stride, pads)
    assert g.shape == (N, Cout, T, Ho, Wo), (g.shape, (N, Cout, T, Ho, Wo))
    t_lo, t_hi = frame_range(N, T, window)
    gm = grad_matrix(g, scale, t_lo, t_hi)
    gm_abs = np.abs(gm)
    ref = np.zeros((Cout, Cin) + tuple(k))
    absref = np.zeros_like(ref)
    for tap in taps_of(k):
        xm = tap_matrix(x, tap, stride, pads, Ho, Wo, t_lo, t_hi)
        ref[(slice(None), slice(None)) + tap] = gm @ xm.T
        absref[(slice(None), slice(None)) + tap] = gm_abs @ np.abs(xm).T
    return ref, absref, N * (t_hi - t_lo) * Ho * Wo


def worst_ratio(got, ref, absref, K):
    """max over the elements of |got - ref| / bound (the fp32-output bound of tests/numerics.py): <= 1 is what assert_elementwise asks."""
    b = nm.bound(ref, absref, K, 'fp32')
    err = np.abs(nm._np64(got) - ref)
    return float(np.max(np.where(np.isfinite(err), err / b, np.inf)))


# ---- fp32 accumulation the way the kernels do it (tests/test_wgrad_refs_cpu.py) ------------------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def position_chunks(N, tn, Ho, Wo, chunking):
    """The counted positions (flattened (N, tn, Ho, Wo)) in the groups one pipeline step of a kernel accumulates: 'linear64' / 'linear32'
    consecutive positions (wgrad_direct_kernel / wgrad_gemm_kernel; wgrad_pw_kernel and the fp32 re-pack GEMM), 'patch8' the 8 x 8
    patches of a frame (wgrad_dma9_kernel; patches at the right and lower edge are partial)."""
    P = N * tn * Ho * Wo
    if chunking.startswith('linear'):
        n = int(chunking[6:])
        return [np.arange(i, min(i + n, P)) for i in range(0, P, n)]
    assert chunking == 'patch8'
    idx = np.arange(P).reshape(N * tn, Ho, Wo)
    return [idx[f, y:y + 8, x:x + 8].reshape(-1) for f in range(N * tn) for y in range(0, Ho, 8) for x in range(0, Wo, 8)]


def chunk_partials(x, g, k, stride, pads, window, chunking, partial_fmt=None):
    """(ntaps, nchunks, Cout, Cin): the exact sum of every chunk's products (an MFMA chain's own rounding is below the step modelled
    here: one fp32 rounding per chunk), optionally rounded to `partial_fmt` -- the seeded defect of 16-bit partial sums."""
    x, g = _np(x), _np(g)
    N, Cin, T, H, W = x.shape
    Ho, Wo = out_hw(H, W, k, stride, pads)
    t_lo, t_hi = frame_range(N, T, window)
    gm = grad_matrix(g, None, t_lo, t_hi)
    chunks = position_chunks(N, t_hi - t_lo, Ho, Wo, chunking)
    out = np.zeros((int(np.prod(k)), len(chunks), g.shape[1], Cin))
    for ti, tap in enumerate(taps_of(k)):
        xm = tap_matrix(x, tap, stride, pads, Ho, Wo, t_lo, t_hi)
        for c, idx in enumerate(chunks):
            out[ti, c] = gm[:, idx] @ xm[:, idx].T
    if partial_fmt is not None:
        out = nm.q16(out.astype(np.float32), partial_fmt).astype(np.float64)
    return out


def accumulate_fp32(partials, scale, k, nsplit, rs):
    """dW (Cout, Cin, KT, KH, KW) from the chunk sums as a K-split kernel leaves it: the chunks in `nsplit` contiguous ranges (range r =
    chunks [n r / nsplit, n (r + 1) / nsplit), the kernels' own split), each range accumulated chunk by chunk with one fp32 rounding per
    chunk, the ranges added in a shuffled order with one fp32 rounding each (float atomics), then the finish kernel's fp32 multiply by
    the scale."""
    ntaps, nch, Cout, Cin = partials.shape
    nsplit = max(1, min(int(nsplit), nch))
    ranges = []
    for r in range(nsplit):
        acc = np.zeros((ntaps, Cout, Cin))
        for c in range(nch * r // nsplit, nch * (r + 1) // nsplit):
            acc = _f32(acc + partials[:, c])
        ranges.append(acc)
    total = np.zeros((ntaps, Cout, Cin))
    for r in rs.permutation(nsplit):
        total = _f32(total + ranges[r])
    if scale is not None:
        total = _f32(total * _f32(_np(scale)).reshape(1, -1, 1))
    return np.transpose(total, (1, 2, 0)).reshape((Cout, Cin) + tuple(k))


# ---- seeded defects: what a subtly wrong kernel would return, computed exactly ---------------------------------------------------------------
DEFECTS = ['position_dropped', 'position_twice', 'border_tap_reads_the_opposite_neighbour', 'window_off_by_one_frame',
           'partial_sums_in_bf16', 'scale_left_out', 'scale_per_ci', 'one_column_map_addressing']


def defect(name, x, g, scale, k, stride, pads, window):
    """The result of a kernel with the named defect and otherwise exact arithmetic (float64), or None where the defect does not apply to
    the shape (no scale, no window, no padded border with a neighbour, Wo > 1 or Ho == 1)."""
    x, g = _np(x).astype(np.float64), _np(g).astype(np.float64)
    N, Cin, T, H, W = x.shape
    Cout = g.shape[1]
    Ho, Wo = out_hw(H, W, k, stride, pads)
    t_lo, t_hi = frame_range(N, T, window)
    ref = lambda x_, g_, scale_=scale, stride_=stride, pads_=pads, window_=window: wgrad_ref64(x_, g_, scale_, k, stride_, pads_, window_)[0]
    if name in ('position_dropped', 'position_twice'):
        g2 = g.copy()
        g2[N - 1, :, (t_lo + t_hi) // 2, Ho // 2, Wo // 2] *= 0.0 if name == 'position_dropped' else 2.0
        return ref(x, g2)
    if name == 'border_tap_reads_the_opposite_neighbour':
        # the tap left of (above) the first column (row) reads the pixel right of (below) it where it should read the padding
        if pads[2] > 0 and W > 1:
            xp = np.pad(x, ((0, 0),) * 4 + ((pads[2], pads[2]),))
            xp[..., pads[2] - 1] = x[..., 1]
            return ref(xp, g, pads_=(pads[0], pads[1], 0))
        if pads[1] > 0 and H > 1:
            xp = np.pad(x, ((0, 0),) * 3 + ((pads[1], pads[1]), (0, 0)))
            xp[..., pads[1] - 1, :] = x[..., 1, :]
            return ref(xp, g, pads_=(pads[0], 0, pads[2]))
        return None
    if name == 'window_off_by_one_frame':
        if window is None or N > 1:
            return None
        gz = np.zeros_like(g)                   # (the caller's g is zero outside its window: the shifted launch reads those zeros)
        gz[:, :, t_lo:t_hi] = g[:, :, t_lo:t_hi]
        t0 = t_lo + 1 if t_hi + 1 <= T else t_lo - 1
        return ref(x, gz, window_=(t0, t_hi - t_lo))
    if name == 'partial_sums_in_bf16':
        # (the one defect that IS a rounding: the kernel as it would run -- every 64-position chunk sum rounded to bf16, then added in fp32)
        parts = chunk_partials(x, g, k, stride, pads, window, 'linear64', partial_fmt='bf16')
        return accumulate_fp32(parts, scale, k, 1, np.random.RandomState(0))
    if name == 'scale_left_out':
        return None if scale is None else ref(x, g, scale_=None)
    if name == 'scale_per_ci':
        if scale is None:
            return None
        s = _np(scale).astype(np.float64)
        return ref(x, g, scale_=None) * s[np.arange(Cin) % Cout].reshape(1, -1, 1, 1, 1)
    if name == 'one_column_map_addressing':
        # the position of a frame taken as (row 0, column = position) on a map of one column and several rows
        if not (Wo == 1 and Ho > 1):
            return None
        if tuple(k) == (1, 1, 1) and tuple(pads) == (0, 0, 0):
            # pointwise kernel: reads input row (f H) W + s position where (f H + s position) W is meant
            xw = x.reshape(N, Cin, T, H * W)[..., stride * np.arange(Ho)].reshape(N, Cin, T, Ho, 1)
            return wgrad_ref64(xw, g, scale, k, 1, pads, window)[0]
        # direct kernel: column s position + kw - pw fails the bound, every row but the first is dropped
        g2 = g.copy()
        g2[:, :, :, 1:] = 0.0
        return ref(x, g2)
    raise KeyError(name)
