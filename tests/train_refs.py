"""Float64 CPU restatements of the training-step kernels of csrc/losses.hip and csrc/train_ops.hip (the three losses, RoIAlign
backward, keypoint-tail backward), for tests/test_gpu_train_kernels.py; tests/test_train_refs_cpu.py checks them against the forward
operators they are the transposes of.

Every function takes the operands as the kernel sees them (already quantised to the build's 16-bit format where the kernel reads
16-bit data) and returns float64 arrays: the reference value, the same expression on absolute values (`abs`, the scale of the fp32
rounding term of tests/numerics.py), and where a path has an error source that term does not cover, a named per-element `extra`."""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
CE_CLAMP = float(np.float32(1e-20))      # softmax_ce_rows: -log(max(p, 1e-20f))


def _f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu()
        return a.double().numpy() if a.is_floating_point() else a.numpy()
    return np.asarray(a)


def _smooth_l1(x, tg, wi, wo, beta, mult):
    """Elementwise SmoothL1 (Detectron's SmoothL1Loss): value, |value|, gradient and |gradient| scale per element."""
    v = wi * (x - tg)
    av = np.abs(v)
    vabs = np.abs(wi) * (np.abs(x) + np.abs(tg))
    quad = av < beta
    loss = wo * np.where(quad, 0.5 * v * v / beta, av - 0.5 * beta)
    loss_abs = np.abs(wo) * np.where(quad, 0.5 * vabs * vabs / beta, vabs + 0.5 * beta)
    grad = wi * wo * np.where(quad, v / beta, np.sign(v)) * mult
    grad_abs = np.abs(wi * wo) * np.where(quad, vabs / beta, 1.0) * mult
    return loss, loss_abs, grad, grad_abs


def rpn_loss_ref(head, labels, tgt, w_in, w_out, A, logit_off, delta_off, T, per_frame, cls_mult, beta, bbox_mult):
    """dat_rpn_loss.  head [N*Th, H, W, cs] (Th = T if per_frame else 1); labels (N, A, Hw, Ww); tgt / w_in / w_out
    (N, 4*T*A, Hw, Ww), channel (a*T + t)*4 + c.  Returns a dict: dhead / dhead_abs / dhead_extra (head layout, zeros in every
    other channel), loss (2,) = (cls, bbox), loss_abs (2,), loss_extra (2,), n (2,) terms per sum."""
    head = _f64(head).astype(np.float64)
    labels, tgt, w_in, w_out = _f64(labels), _f64(tgt).astype(np.float64), _f64(w_in).astype(np.float64), _f64(w_out).astype(np.float64)
    Fr, H, W, cs = head.shape
    Th = T if per_frame else 1
    N = Fr // Th
    nd = 4 * A if per_frame else 4 * A * T
    h5 = head.reshape(N, Th, H, W, cs)
    out = np.zeros_like(h5)
    out_abs = np.zeros_like(h5)
    out_extra = np.zeros_like(h5)
    # ---- sigmoid cross entropy on the frame mean of the logits, -1 = ignore ----
    lg = h5[..., logit_off:logit_off + A]
    v = lg.mean(1)                                   # (N, H, W, A)
    absx = np.abs(lg).mean(1)
    lab = labels[:, :, :H, :W].transpose(0, 2, 3, 1).astype(np.float64)
    valid = lab >= 0
    lab = np.where(valid, lab, 0.0)
    sig = 1.0 / (1.0 + np.exp(-v))
    g = np.where(valid, (sig - lab) * cls_mult / Th, 0.0)
    g_abs = np.where(valid, (sig + lab) * cls_mult / Th, 0.0)
    # the fp32 frame mean rounds Th - 1 additions and a division (relative to mean |x|); the sigmoid passes that on with slope sig(1 - sig)
    g_extra = np.where(valid, sig * (1.0 - sig) * (Th + 1) * U32 * absx * cls_mult / Th, 0.0)
    # below v = -88.7 expf(-v) overflows and 1 / (1 + inf) is 0: the true sigmoid lies under fp32's normal range there
    g_extra += np.where(valid & (sig < 2.0 ** -126), sig * cls_mult / Th, 0.0)
    out[..., logit_off:logit_off + A] = g[:, None]
    out_abs[..., logit_off:logit_off + A] = g_abs[:, None]
    out_extra[..., logit_off:logit_off + A] = g_extra[:, None]
    sp = np.log1p(np.exp(-np.abs(v)))
    term = np.where(valid, np.maximum(v, 0.0) - v * lab + sp, 0.0)
    term_abs = np.where(valid, absx * (1.0 + lab) + sp, 0.0)
    # per term: the frame mean's rounding (slope <= 1) and a few ulps of expf / log1pf on the softplus part
    term_extra = np.where(valid, (Th + 1) * U32 * absx + 4 * U32 * sp, 0.0)
    # ---- smooth L1 on the deltas (per_frame: frame t holds the deltas of tube slot t) ----
    tg = tgt[:, :, :H, :W]
    wi, wo = w_in[:, :, :H, :W], w_out[:, :, :H, :W]
    if per_frame:
        lay = lambda a: a.reshape(N, A, T, 4, H, W).transpose(0, 2, 4, 5, 1, 3).reshape(N, T, H, W, 4 * A)
    else:
        lay = lambda a: a.transpose(0, 2, 3, 1)[:, None]
    x = h5[..., delta_off:delta_off + nd]
    lb, lb_abs, gb, gb_abs = _smooth_l1(x, lay(tg), lay(wi), lay(wo), beta, bbox_mult)
    out[..., delta_off:delta_off + nd] = gb
    out_abs[..., delta_off:delta_off + nd] = gb_abs
    sh = (Fr, H, W, cs)
    return dict(dhead=out.reshape(sh), dhead_abs=out_abs.reshape(sh), dhead_extra=out_extra.reshape(sh),
                loss=np.array([term.sum() * cls_mult, lb.sum() * bbox_mult]),
                loss_abs=np.array([term_abs.sum() * cls_mult, lb_abs.sum() * bbox_mult]),
                loss_extra=np.array([term_extra.sum() * cls_mult, 0.0]),
                n=(N * H * W * A, N * Th * H * W * nd))


def smooth_l1_rows_ref(pred, tgt, w_in, w_out, D, beta, mult):
    """dat_smooth_l1_rows.  pred [R, ld]; tgt / w_in / w_out [R, D].  -> (dpred, dpred_abs, loss, loss_abs) with zero padding."""
    pred = _f64(pred).astype(np.float64)
    R, ld = pred.shape
    l, l_abs, g, g_abs = _smooth_l1(pred[:, :D], _f64(tgt).astype(np.float64), _f64(w_in).astype(np.float64),
                                    _f64(w_out).astype(np.float64), beta, mult)
    dp, dp_abs = np.zeros((R, ld)), np.zeros((R, ld))
    dp[:, :D], dp_abs[:, :D] = g, g_abs
    return dp, dp_abs, l.sum() * mult, l_abs.sum() * mult


def softmax_ce_ref(logits, labels, weights, D, mult, C=8.0):
    """dat_softmax_ce_rows.  logits [R, ld]; labels [R] in [0, D); weights [R] or None.  Returns a dict: dl / dl_abs / dl_extra
    [R, ld], loss / loss_abs / loss_extra, correct (lowest index wins a tie, like np.argmax)."""
    xs = _f64(logits).astype(np.float64)
    R, ld = xs.shape
    x = xs[:, :D]
    lab = _f64(labels).astype(np.int64)
    w = np.ones(R) if weights is None else _f64(weights).astype(np.float64)
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(1, keepdims=True)
    p = e / s
    onehot = np.zeros_like(p)
    onehot[np.arange(R), lab] = 1.0
    aw = np.abs(w)[:, None]
    dl, dl_abs, dl_extra = np.zeros((R, ld)), np.zeros((R, ld)), np.zeros((R, ld))
    dl[:, :D] = w[:, None] * (p - onehot) * mult
    dl_abs[:, :D] = aw * (p + onehot) * mult
    # x - max rounds in fp32 (relative 2^-24, i.e. absolute 2^-24 |x - max|) and exp turns that into a relative error of each term:
    # of p_c directly and of the row sum through sum_j p_j |x_j - max|
    dxm = np.abs(x - m)
    spread = (p * dxm).sum(1, keepdims=True)
    dl_extra[:, :D] = aw * mult * p * (dxm + spread) * U32
    pl = p[np.arange(R), lab]
    term = -w * np.log(np.maximum(pl, CE_CLAMP)) * mult
    # relative error of the kernel's p_label (fp32 row sum, x - max rounding, expf / division) = absolute error of its logarithm
    dl_lab = dxm[np.arange(R), lab]
    term_extra = np.abs(w) * mult * (C * np.sqrt(D) + 4.0 + dl_lab + spread[:, 0]) * U32
    return dict(dl=dl, dl_abs=dl_abs, dl_extra=dl_extra, loss=term.sum(), loss_abs=np.abs(term).sum(), loss_extra=term_extra.sum(),
                correct=int((x.argmax(1) == lab).sum()), p_label=pl)


# ---- RoIAlign backward ----------------------------------------------------------------------------------------------------------
def roi_levels(rois, Tr, n_levels, k_min, canon_scale, canon_level):
    """The FPN level of every roi (FPN.py map_rois_to_fpn_levels on the tube's mean area), as an index into the level list."""
    if n_levels == 1:
        return np.zeros(rois.shape[0], np.int64)
    r = _f64(rois).astype(np.float64)
    asum = sum((r[:, 3 + 4 * t] - r[:, 1 + 4 * t] + 1) * (r[:, 4 + 4 * t] - r[:, 2 + 4 * t] + 1) for t in range(Tr))
    lv = np.floor(canon_level + np.log2(np.sqrt(asum / Tr) / canon_scale + 1e-6))
    return (np.clip(lv, k_min, k_min + n_levels - 1) - k_min).astype(np.int64)


def _axis(c1, c2, size, P, grid, strict=True):
    """Bilinear weights of one axis of a roi: A[p, i] = sum over the grid samples of bin p of their weight on pixel i (0 for samples
    outside [-1, size]), I = the number of taps on (p, i), E = the taps' weight error from the fp32 sample coordinate (8 ulps of the
    magnitudes it is computed from).  The kernels' per-sample weight is the product of the two axes' weights, its validity the product
    of their indicators, so a bin's scatter is A_y^T G A_x.  A sample within that error of a validity cut-off (-1 or size) raises: the
    kernel may decide it either way.  strict=False decides it in float64 instead (hand-worked cases with samples exactly on a cut-off)."""
    A, I, E = np.zeros((P, size)), np.zeros((P, size)), np.zeros((P, size))
    rw = max(c2 - c1, 1.0)
    b = rw / P
    for p in range(P):
        for i in range(grid):
            y = c1 + p * b + (i + 0.5) * b / grid
            e = 8 * U32 * (abs(c1) + abs(c2) + abs(y) + 1.0)
            if strict and min(abs(y + 1.0), abs(y - size)) < 4 * e:
                raise ValueError('sample %.7f within the fp32 coordinate error of a validity cut-off: the kernel may decide it either '
                                 'way' % y)
            if y < -1.0 or y > size:
                continue
            yy = max(y, 0.0)
            lo = int(yy)
            if lo >= size - 1:
                lo = hi = size - 1
                yy = float(lo)
            else:
                hi = lo + 1
            ly = yy - lo
            for at, wt in ((lo, 1.0 - ly), (hi, ly)):
                A[p, at] += wt
                I[p, at] += 1
                E[p, at] += e
    return A, I, E


def _scatter(Ay, Ax, G):
    """sum_{p, q} Ay[p, h] Ax[q, w] G[p, q, c] over the rows / columns the roi touches: -> (h0, w0, block [h, w, c])."""
    hs, ws = np.nonzero(Ay.any(0))[0], np.nonzero(Ax.any(0))[0]
    if len(hs) == 0 or len(ws) == 0:
        return 0, 0, None
    h0, h1, w0, w1 = hs[0], hs[-1] + 1, ws[0], ws[-1] + 1
    t1 = np.tensordot(Ay[:, h0:h1], G, axes=(0, 0))                 # (h, q, c)
    return h0, w0, np.tensordot(t1, Ax[:, w0:w1], axes=(1, 0)).transpose(0, 2, 1)


def roi_frames(shapes, scales, rois, T, Tr, t0, pooled, sampling, k_min=2, canon_scale=224., canon_level=4, strict=True):
    """What the RoIAlign kernels (forward and backward) decide per roi and frame, for rois [R, 4*Tr + 1] over levels of shapes
    [(frames, H, W)]: yields (row, level, frame, gh, gw, (Ay, Iy, Ey), (Ax, Ix, Ex)) with row = r * Tr + t the roi-frame's row of the
    pooled tensor and the axis matrices of `_axis`."""
    r32 = _f64(rois).astype(np.float32)
    P = pooled
    lv = roi_levels(r32, Tr, len(shapes), k_min, canon_scale, canon_level)
    for r in range(r32.shape[0]):
        li = int(lv[r])
        _, H, W = shapes[li]
        sc32 = np.float32(scales[li])
        n = int(r32[r, 0])
        for t in range(Tr):
            fr = n * T + (t0 if Tr == 1 else t)
            bx = r32[r, 1 + 4 * t:5 + 4 * t]
            # the sampling grid is a discrete choice: decided in fp32 like the oracle and the kernel
            x1, y1, x2, y2 = [np.float32(v * sc32) for v in bx]
            gh = sampling if sampling > 0 else int(np.ceil(np.float32(max(y2 - y1, np.float32(1.))) / np.float32(P)))
            gw = sampling if sampling > 0 else int(np.ceil(np.float32(max(x2 - x1, np.float32(1.))) / np.float32(P)))
            c = [float(v) * float(sc32) for v in bx]          # sample coordinates in float64
            yield r * Tr + t, li, fr, gh, gw, _axis(c[1], c[3], H, P, gh, strict), _axis(c[0], c[2], W, P, gw, strict)


def roi_align_bwd_ref(shapes, scales, rois, dout, T, Tr, t0, pooled, sampling, k_min=2, canon_scale=224., canon_level=4):
    """dat_roi_align_bwd: the transpose of the legacy RoIAlign (oracle/roi_align.py) with the FPN level picked per roi.
    shapes: [(frames, H, W)] per level (finest first); rois [R, 4*Tr + 1]; dout [R*Tr, P, P, C].  Returns (ref, abs, extra) lists of
    float64 [frames, H, W, C] maps and K, the largest number of atomic contributions to one element."""
    G_all = _f64(dout).astype(np.float64)
    C = G_all.shape[-1]
    ref = [np.zeros(s + (C,)) for s in shapes]
    ab = [np.zeros(s + (C,)) for s in shapes]
    ex = [np.zeros(s + (C,)) for s in shapes]
    cnt = [np.zeros(s) for s in shapes]
    for row, li, fr, gh, gw, (Ay, Iy, Ey), (Ax, Ix, Ex) in roi_frames(shapes, scales, rois, T, Tr, t0, pooled, sampling, k_min,
                                                                      canon_scale, canon_level):
        G = G_all[row] / (gh * gw)
        aG = np.abs(G)
        for dst, ay, ax, g in ((ref, Ay, Ax, G), (ab, Ay, Ax, aG), (ex, Ey, Ix, aG), (ex, Iy, Ex, aG)):
            h0, w0, blk = _scatter(ay, ax, g)
            if blk is not None:
                dst[li][fr, h0:h0 + blk.shape[0], w0:w0 + blk.shape[1]] += blk
        cnt[li][fr] += np.outer(Iy.sum(0), Ix.sum(0))
    return ref, ab, ex, int(max(c.max() for c in cnt))


# ---- keypoint tail ----------------------------------------------------------------------------------------------------------------
def _bilinear_up(K, up):
    from oracle.net3d import bilinear_kernel
    return torch.from_numpy(np.ascontiguousarray(bilinear_kernel(K, up), np.float64))


def _bilinear_up_matrix(L, up):
    """The fixed bilinear ConvTranspose (k = 2*up, s = up, p = up/2) of oracle.net3d.bilinear_kernel along one axis, as a matrix
    U [L*up, L]: the kernel is the outer product f f^T of one 1-D factor and acts on every channel alone, so a map's output is
    U low U^T (tests/test_train_refs_cpu.py holds this to the ConvTranspose itself)."""
    from oracle.net3d import bilinear_kernel
    k2 = np.asarray(bilinear_kernel(2, up), np.float64)
    assert np.all(k2[0, 1] == 0) and np.array_equal(k2[0, 0], k2[1, 1]), 'the bilinear kernel is diagonal over the channels'
    f = k2[0, 0].sum(1) / np.sqrt(k2[0, 0].sum())
    assert np.allclose(np.outer(f, f), k2[0, 0], rtol=1e-15, atol=0)
    U = np.zeros((L * up, L))
    for o in range(L * up):
        for y in range(L):
            ky = o + up // 2 - up * y
            if 0 <= ky < 2 * up:
                U[o, y] = f[ky]
    return torch.from_numpy(U)


def kps_finalize_ref(sub, R, Tr, K, up):
    """dat_kps_finalize in float64: the sub-pixel channels (a*2 + b)*K + k of sub [R*Tr, S, S, cs] unfolded into kps_score_lowres
    [R*Tr, K, 2S, 2S], then the fixed bilinear ConvTranspose of oracle.net3d.kps_outputs_2d -> [R, Tr*K, M, M]."""
    s = torch.from_numpy(_f64(sub).astype(np.float64))
    Fr, S = s.shape[0], s.shape[1]
    low = s[..., :4 * K].reshape(Fr, S, S, 2, 2, K).permute(0, 5, 1, 3, 2, 4).reshape(Fr, K, 2 * S, 2 * S)
    U = _bilinear_up_matrix(2 * S, up)
    out = torch.matmul(torch.matmul(U, low), U.t())
    return out.reshape(R, Tr * K, out.shape[-2], out.shape[-1]).numpy()


def kps_finalize_bwd_ref(dout, R, Tr, S, cs, K, up):
    """dat_kps_finalize_bwd in float64: the transpose of kps_finalize_ref, written out -- the adjoint of a ConvTranspose is the conv
    with the same kernel, stride and padding -- and folded back into the sub-pixel channel layout [R*Tr, S, S, cs] (zeros in 4K..cs)."""
    d = torch.from_numpy(_f64(dout).astype(np.float64))
    M = d.shape[-1]
    dlow = F.conv2d(d.reshape(R * Tr, K, M, M), _bilinear_up(K, up), None, stride=up, padding=up // 2)
    out = np.zeros((R * Tr, S, S, cs))
    out[..., :4 * K] = dlow.reshape(R * Tr, K, S, 2, S, 2).permute(0, 2, 4, 3, 5, 1).reshape(R * Tr, S, S, 4 * K).numpy()
    return out
