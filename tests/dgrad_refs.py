"""Float64 reference of the dense data gradient (hip_ops.ConvGrad.data), a restatement of the packed weight layout of
csrc/conv_pack.hip, seeded defects of both, and the case tables of tests/test_gpu_weight_pack.py and tests/test_gpu_dgrad.py.

Semantics.  The forward conv is y[n, :, t, i, j] = sum over taps of w[:, :, kt, kh, kw] * x[n, :, t + kt - pt, i * sh + kh - ph,
j * sw + kw - pw] for EVERY frame t of [0, T) (input outside the clip counts as zero; pt = (kT - 1) / 2 is "same" padding, pt = 0 with
kT = 3 the windowed / (2+1)D form whose last kT - 1 output frames see the zero frames behind the clip), followed by the
AffineChannelNd scale.  Its data gradient is the transpose of that sum -- written here as such (`dgrad_ref64`), without the flip,
the channel swap and the `k - 1 - p` padding through which the device code computes it (`pipeline_dx64` restates THOSE, with the
seeded defects).
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import numerics as nm


def _t64(a):
    if a is None:
        return None
    return a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.float64))


def round_up(v, m):
    return (v + m - 1) // m * m


# ---- the packed layout ---------------------------------------------------------------------------------------------------------------------
def _esize(dtype):
    return 4 if dtype in ('fp32', torch.float32) else 2


def _tdtype(dtype):
    return {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}.get(dtype, dtype)


def cout_pad(rows):
    """Rows of a packed image: the real rows rounded up to 4 (the descriptor's Cout), then to the kernels' channel tile (64 up to 64
    rows, else 128)."""
    c = round_up(rows, 4)
    return round_up(c, 64 if c <= 64 else 128)


def pack_desc(rows, cols, ntap, cin=None):
    """dict(ntap, cout_pad, cin) of a packed image of a [rows x cols] matrix per tap; `cin`: the channel stride (default: cols rounded
    up to 64)."""
    return dict(ntap=int(ntap), cout_pad=cout_pad(rows), cin=int(cin or round_up(cols, 64)))


def _dims(desc, dtype):
    """The nesting of a packed image, outermost first: tap, 128-byte channel chunk, 32-row block, k-slice (4), k-half (2), row of the
    block (32), element of the 16-byte slot.  A lane is (k-half, row): lane = k-half * 32 + row."""
    es = _esize(dtype)
    ck, eps = 128 // es, 16 // es
    assert desc['cin'] % ck == 0 and desc['cout_pad'] % 32 == 0, desc
    return (desc['ntap'], desc['cin'] // ck, desc['cout_pad'] // 32, 4, 2, 32, eps), ck, eps


def pack_index(tap, co, ci, desc, dtype):
    """Element offset of logical (tap, co, ci) in the packed image (numpy arrays or ints)."""
    dims, ck, eps = _dims(desc, dtype)
    tap, co, ci = np.asarray(tap), np.asarray(co), np.asarray(ci)
    within = ci % ck                    # channel inside its 128-byte chunk
    slot = within // eps                # which of the chunk's eight 16-byte slots: slot = 2 * k-slice + k-half
    coords = (tap, ci // ck, co // 32, slot // 2, slot % 2, co % 32, within % eps)
    return np.ravel_multi_index(coords, dims)


def pack(logical, dtype):
    """[ntap][Cout_pad][Cin] tensor -> the flat packed image (a host packer through pack_index: the round trip's other half)."""
    t = logical if isinstance(logical, torch.Tensor) else torch.from_numpy(np.asarray(logical))
    ntap, cp, cin = t.shape
    desc = dict(ntap=ntap, cout_pad=cp, cin=cin)
    tap, co, ci = np.meshgrid(np.arange(ntap), np.arange(cp), np.arange(cin), indexing='ij')
    idx = torch.from_numpy(pack_index(tap, co, ci, desc, dtype).reshape(-1))
    out = torch.empty(t.numel(), dtype=t.dtype)
    out[idx] = t.reshape(-1)
    return out


def unpack(packed_bytes, desc, dtype):
    """uint8 tensor / array of a packed image -> the logical [ntap][Cout_pad][Cin] tensor in `dtype` (bits untouched)."""
    dims, ck, eps = _dims(desc, dtype)
    b = packed_bytes.detach().cpu() if isinstance(packed_bytes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(packed_bytes))
    t = b.contiguous().view(torch.uint8).view(_tdtype(dtype)) if b.dtype == torch.uint8 else b
    assert t.numel() == int(np.prod(dims)), (t.numel(), dims)
    t = t.view(dims)                                   # (tap, chunk, row block, k-slice, k-half, row, e)
    t = t.permute(0, 2, 5, 1, 3, 4, 6)                 # (tap, row block, row, chunk, k-slice, k-half, e)
    return t.reshape(desc['ntap'], desc['cout_pad'], desc['cin']).contiguous()


def bits(t):
    """The raw bits of a tensor as integers: -0 != +0 and every NaN pattern shows."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


PACK_DEFECTS = ('no_flip', 'flip_t_only', 'flip_hw_only', 'no_swap', 'no_scale', 'scale_by_dgrad_row', 'scale_after_rounding')


def _flip(w5, axes):
    return torch.flip(w5, axes) if axes else w5


def dgrad_weights(w, scale, dtype, defect=None):
    """fp32 [Cin][Cout][kT][kH][kW]: the data-gradient conv's weights W'[co'][ci'][tap'] = fl32(w[ci'][co'][ntap - 1 - tap'] *
    scale[ci']) rounded once to `dtype` -- one multiply, one rounding, both in IEEE arithmetic, so the device packer must give these
    bits.  `defect`: one of PACK_DEFECTS seeded."""
    w = w.detach().cpu().float() if isinstance(w, torch.Tensor) else torch.from_numpy(np.asarray(w, dtype=np.float32))
    cout, cin = int(w.shape[0]), int(w.shape[1])
    if scale is None:
        s = torch.ones(cout)
    else:
        s = scale.detach().cpu().float() if isinstance(scale, torch.Tensor) else torch.from_numpy(np.asarray(scale, dtype=np.float32))
    q = (lambda v: v) if _tdtype(dtype) == torch.float32 else (lambda v: v.to(_tdtype(dtype)).float())
    if defect == 'no_swap':           # the master read as if it were stored [Cin][Cout][taps]
        src = w.reshape((cin, cout) + tuple(w.shape[2:]))
    else:
        src = w.transpose(0, 1)
    srow = s.view(1, cout, 1, 1, 1)
    if defect == 'no_scale':
        srow = torch.ones_like(srow)
    elif defect == 'scale_by_dgrad_row':      # scale[co'] (read past the end wraps: whatever lies there)
        srow = s[torch.arange(cin) % cout].view(cin, 1, 1, 1, 1)
    axes = {None: (2, 3, 4), 'no_flip': (), 'flip_t_only': (2,), 'flip_hw_only': (3, 4)}.get(defect, (2, 3, 4))
    if defect == 'scale_after_rounding':
        out = q(q(src) * srow)
    else:
        out = q(src * srow)
    return _flip(out, axes).contiguous()


def packed_expected(w, scale, dgrad, dtype, cin=None, defect=None):
    """The logical [ntap][Cout_pad][Cin] matrix a correct packer leaves, in `dtype`, padding +0.  w: the fp32 master
    [Cout, Cin, kT, kH, kW]; dgrad: the data-gradient twin (scale: the forward layer's, or None)."""
    w = w.detach().cpu().float() if isinstance(w, torch.Tensor) else torch.from_numpy(np.asarray(w, dtype=np.float32))
    ntap = int(np.prod(w.shape[2:]))
    m = dgrad_weights(w, scale, dtype, defect) if dgrad else w
    rows, cols = int(m.shape[0]), int(m.shape[1])
    d = pack_desc(rows, cols, ntap, cin)
    out = torch.zeros((ntap, d['cout_pad'], d['cin']), dtype=torch.float32)
    out[:, :rows, :cols] = m.reshape(rows, cols, ntap).permute(2, 0, 1)
    return out.to(_tdtype(dtype)), d


# ---- the data gradient in float64 --------------------------------------------------------------------------------------------------------
def out_hw(H, W, k, stride, pads):
    return (H + 2 * pads[1] - k[1]) // stride[0] + 1, (W + 2 * pads[2] - k[2]) // stride[1] + 1


def _g_window(g, g_frames):
    if g_frames is None:
        return g
    g = g.clone()
    g[:, :, :g_frames[0]] = 0
    g[:, :, g_frames[0] + g_frames[1]:] = 0
    return g


def dgrad_ref64(g, w, scale, stride, pads, x_shape, base=None, mask=None, g_frames=None, positions=None):
    """(ref64, absref64) of dL/dx = transpose-conv(g, w * scale) + base, then `mask > 0 ? v : 0` (absref: the same sum over absolute
    values, + |base|, no mask).  g (N, Cout, T, Ho, Wo), w (Cout, Cin, kT, kH, kW), scale (Cout,) or None, stride (sh, sw), pads
    (pt, ph, pw), x_shape (N, Cin, T, H, W); g_frames = (t0, n): g counts as zero outside those frames of every clip.
    positions: None -> numpy (N, Cin, T, H, W); an int array (P, 4) of (n, t, h, w) rows -> (P, Cin), each sampled position from
    its own receptive field (no full conv)."""
    if positions is None:
        g = _g_window(_t64(g), g_frames)
    else:       # (rows are gathered first and widened afterwards: a large map is never copied to float64 as a whole)
        g = g.detach().cpu() if isinstance(g, torch.Tensor) else torch.from_numpy(np.asarray(g))
    w = _t64(w)
    f_lo, f_hi = (g_frames[0], g_frames[0] + g_frames[1]) if g_frames is not None else (0, int(g.shape[2]))
    N, Cin, T, H, W = [int(v) for v in x_shape]
    kt, kh, kw = [int(v) for v in w.shape[2:]]
    pt, ph, pw = pads
    sh, sw = stride
    assert g.shape[0] == N and g.shape[2] == T and tuple(g.shape[3:]) == out_hw(H, W, (kt, kh, kw), stride, pads), (g.shape, x_shape)
    ws = w if scale is None else w * _t64(scale).view(-1, 1, 1, 1, 1)
    outs = []
    for absolute in (False, True):
        f = (lambda v: v.abs()) if absolute else (lambda v: v)
        if positions is None:
            # the forward conv is a VALID temporal conv over the clip padded by pt zero frames in front and kT - 1 - pt behind (T output
            # frames from T + kT - 1): its gradient w.r.t. the padded clip, of which frames [pt, pt + T) are the clip
            assert 0 <= pt <= kt - 1
            full = torch.nn.grad.conv3d_input((N, Cin, T + kt - 1, H, W), f(ws), f(g), stride=(1, sh, sw), padding=(0, ph, pw))
            y = full[:, :, pt:pt + T]
        else:
            pos = np.asarray(positions, dtype=np.int64)
            n_i, t_i, h_i, w_i = [torch.from_numpy(pos[:, c].copy()) for c in range(4)]
            y = torch.zeros((pos.shape[0], Cin), dtype=torch.float64)
            for a in range(kt):
                to = t_i + pt - a
                for b in range(kh):
                    hn = h_i + ph - b
                    for c in range(kw):
                        wn = w_i + pw - c
                        ok = (to >= f_lo) & (to < f_hi) & (hn % sh == 0) & (wn % sw == 0)
                        ho, wo = hn // sh, wn // sw
                        ok &= (ho >= 0) & (ho < g.shape[3]) & (wo >= 0) & (wo < g.shape[4])
                        if not bool(ok.any()):
                            continue
                        rows = g[n_i, :, to.clamp(0, T - 1), ho.clamp(0, g.shape[3] - 1), wo.clamp(0, g.shape[4] - 1)]
                        rows = f(rows.double()) * ok.view(-1, 1).double()
                        y += rows @ f(ws)[:, :, a, b, c]
        if base is not None:
            bb = _t64(base)
            if positions is not None and bb.dim() == 5:
                bb = bb[n_i, :, t_i, h_i, w_i]
            y = y + f(bb)
        if mask is not None and not absolute:
            mm = _t64(mask)
            if positions is not None and mm.dim() == 5:
                mm = mm[n_i, :, t_i, h_i, w_i]
            y = torch.where(mm > 0, y, torch.zeros_like(y))
        outs.append(y.numpy())
    return outs[0], outs[1]


def gather(a5, positions):
    """(N, C, T, H, W) -> (P, C) at the (n, t, h, w) rows of `positions`"""
    pos = np.asarray(positions, dtype=np.int64)
    a = a5 if isinstance(a5, np.ndarray) else a5.detach().cpu().numpy()
    return a[pos[:, 0], :, pos[:, 1], pos[:, 2], pos[:, 3]]


def sample_positions(N, T, H, W, n_min=2048, seed=0):
    """(n, t, h, w) rows, unique, at least min(n_min, all): the four corners of the first and the last frame, the whole first and
    last row and column of frame 0, both sides of every 256-position boundary of the flat (frame, h, w) order inside the first and the
    last frame, and a seeded random remainder."""
    hw, frames = H * W, N * T
    flat = set()
    for fr in (0, frames - 1):
        flat.update(fr * hw + h * W + w for h in (0, H - 1) for w in (0, W - 1))
        lo, hi = fr * hw, (fr + 1) * hw
        for b in range((lo + 255) // 256 * 256, hi + 1, 256):
            flat.update(p for p in (b - 1, b) if lo <= p < hi)
    flat.update(h * W + w for h in (0, H - 1) for w in range(W))
    flat.update(h * W + w for h in range(H) for w in (0, W - 1))
    total = frames * hw
    want = min(n_min, total)
    if len(flat) < want:
        rs = np.random.RandomState(seed)
        for p in rs.permutation(total):
            flat.add(int(p))
            if len(flat) >= want:
                break
    p = np.array(sorted(flat), dtype=np.int64)
    fr, r = p // hw, p % hw
    return np.stack([fr // T, fr % T, r // W, r % W], axis=1)


def sample_holds_the_required(positions, N, T, H, W):
    """dict of booleans: what the issue wants every sample to contain"""
    hw = H * W
    s = {int(((n * T + t) * H + h) * W + w) for n, t, h, w in np.asarray(positions)}
    frames = N * T
    corners = all(fr * hw + h * W + w in s for fr in (0, frames - 1) for h in (0, H - 1) for w in (0, W - 1))
    edges = all(h * W + w in s for h in (0, H - 1) for w in range(W)) and all(h * W + w in s for h in range(H) for w in (0, W - 1))
    bounds = True
    for fr in (0, frames - 1):
        lo, hi = fr * hw, (fr + 1) * hw
        for b in range((lo + 255) // 256 * 256, hi + 1, 256):
            bounds &= all(p in s for p in (b - 1, b) if lo <= p < hi)
    return dict(corners=corners, edges=edges, block_boundaries=bounds, count=len(s) >= min(2048, frames * hw))


# ---- the device pipeline, restated, with seeded defects ----------------------------------------------------------------------------------
DX_DEFECTS = ('no_flip', 'flip_t_only', 'flip_hw_only', 'pad_not_mirrored', 'no_swap', 'no_scale', 'scale_by_dgrad_row',
              'zero_insert_offset', 'zero_insert_extent', 'mask_before_sum')
DEFECTS = DX_DEFECTS + ('scale_after_rounding',)
DEFECT_CLASS = {'no_flip': 'flip', 'flip_t_only': 'flip', 'flip_hw_only': 'flip', 'pad_not_mirrored': 'pad', 'no_swap': 'swap',
                'no_scale': 'scale', 'scale_by_dgrad_row': 'scale', 'scale_after_rounding': 'scale', 'zero_insert_offset': 'zero_insert',
                'zero_insert_extent': 'zero_insert', 'mask_before_sum': 'epilogue'}


def _shifted_conv(gz, wp, pads, out_ext):
    """out[.., t, h, w] = sum_j wp[.., j] * gz[.., (t, h, w) + j - pads] over an output of extent `out_ext`, zeros outside gz"""
    k = wp.shape[2:]
    padding = []
    for ax in (2, 1, 0):                  # F.pad: last axis first
        back = out_ext[ax] + k[ax] - 1 - pads[ax] - gz.shape[2 + ax]
        padding += [pads[ax], back]
    return F.conv3d(F.pad(gz, padding), wp)


def pipeline_dx64(g, w, scale, stride, pads, x_shape, fmt, base=None, mask=None, defect=None):
    """dL/dx the way ConvGrad.data computes it, in float64: the packed weights of `dgrad_weights` (rounded to `fmt`), the stride-2
    zero insertion to H - k + 1 + 2p, a stride-1 conv with padding k - 1 - p, then + base and the mask -- with `defect` (one of
    DX_DEFECTS) seeded.  numpy (N, Cin, T, H, W)."""
    g = _t64(g)
    N, Cin, T, H, W = [int(v) for v in x_shape]
    k = tuple(int(v) for v in w.shape[2:])
    wdef = defect if defect in PACK_DEFECTS else None
    wp = dgrad_weights(w, scale, fmt, wdef).double()                    # [Cin][Cout][taps]: (out, in) of the stride-1 conv
    Ho, Wo = int(g.shape[3]), int(g.shape[4])
    Hz, Wz = H - k[1] + 1 + 2 * pads[1], W - k[2] + 1 + 2 * pads[2]
    if stride[0] == 2:
        if defect == 'zero_insert_extent':
            Hz, Wz = 2 * Ho, 2 * Wo
        gz = torch.zeros((N, g.shape[1], T, max(Hz, 2 * Ho), max(Wz, 2 * Wo)), dtype=torch.float64)
        o = 1 if defect == 'zero_insert_offset' else 0
        gz[:, :, :, o:2 * Ho:2, o:2 * Wo:2] = g
        gz = gz[:, :, :, :Hz, :Wz]
    else:
        assert (Hz, Wz) == (Ho, Wo)
        gz = g
    mirrored = [k[i] - 1 - pads[i] for i in range(3)]
    if defect == 'pad_not_mirrored':
        ax = [i for i in range(3) if mirrored[i] != pads[i]][0]
        mirrored[ax] = pads[ax]
    # the extent the stride-1 conv writes: (input extent) + 2 * padding - k + 1; only a wrong zero-inserted extent changes it
    ext = (T, Hz + 2 * (k[1] - 1 - pads[1]) - k[1] + 1, Wz + 2 * (k[2] - 1 - pads[2]) - k[2] + 1)
    y = _shifted_conv(gz, wp, mirrored, ext)
    if ext != (T, H, W):                  # the launch's rows have another pitch than the tensor the caller reads them as
        flat = y.permute(0, 2, 3, 4, 1).reshape(-1, Cin)
        need = N * T * H * W
        flat = torch.cat([flat, torch.zeros((max(0, need - flat.shape[0]), Cin), dtype=torch.float64)])[:need]
        y = flat.reshape(N, T, H, W, Cin).permute(0, 4, 1, 2, 3)
    if defect == 'mask_before_sum':
        y = torch.where(_t64(mask) > 0, y, torch.zeros_like(y)) + _t64(base)
        return y.numpy()
    if base is not None:
        y = y + _t64(base)
    if mask is not None:
        y = torch.where(_t64(mask) > 0, y, torch.zeros_like(y))
    return y.numpy()


def defect_applicable(defect, case, fmt='bf16'):
    """Whether `defect` makes the device pipeline compute ANOTHER function at this case -- decided from the shape alone.  Where it
    does not (nothing to flip in a 1 x 1 x 1 layer, k - 1 - p == p on every axis, no zero insertion at stride 1) the defective code IS
    the correct code."""
    k, pads, st = case['k'], case['pads'], case['stride']
    Ho, Wo = out_hw(case['H'], case['W'], k, st, pads)
    if defect == 'no_flip':
        return max(k) > 1
    if defect == 'flip_t_only':
        return k[1] > 1 or k[2] > 1
    if defect == 'flip_hw_only':
        return k[0] > 1
    if defect == 'pad_not_mirrored':
        return any(k[i] - 1 - pads[i] != pads[i] for i in range(3))
    if defect in ('no_swap', 'no_scale', 'scale_by_dgrad_row', 'mask_before_sum'):
        return True
    if defect == 'zero_insert_offset':
        return st[0] == 2
    if defect == 'zero_insert_extent':
        return st[0] == 2 and (2 * Ho, 2 * Wo) != (case['H'] - k[1] + 1 + 2 * pads[1], case['W'] - k[2] + 1 + 2 * pads[2])
    if defect == 'scale_after_rounding':      # visible in the packed bits of a 16-bit format only (in fp32 it is the same multiply)
        return fmt != 'fp32'
    raise KeyError(defect)


# Defects that DO change the computed function at a case but stay inside the dx bound there, each with its reason; at most one class
# per case.  'scale_after_rounding' is not a dx defect at all: q16(q16(w) * s) differs from q16(w * s) by a second rounding of at
# most u16 * |w * s| per weight -- the very term (`extra`) the dx bound grants the packer's one rounding -- so it is held against
# the packed BITS (packed_expected), where it always shows.
INVISIBLE = {}


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------
def _c(name, cout, cin, k, stride, pads, N, T, H, W, **kw):
    d = dict(name=name, cout=cout, cin=cin, k=tuple(k), stride=(stride, stride), pads=tuple(pads), N=N, T=T, H=H, W=W)
    d.update(kw)
    return d


# the small cases (forward layer cout <- cin): full float64 reference, every seeded defect on the CPU
SMALL_CASES = [
    _c('k333_same', 40, 24, (3, 3, 3), 1, (1, 1, 1), 2, 4, 9, 11),
    _c('k333_pad_t0', 40, 24, (3, 3, 3), 1, (0, 1, 1), 2, 4, 9, 11),
    _c('k333_window', 40, 24, (3, 3, 3), 1, (1, 1, 1), 1, 5, 9, 11, g_frames=(2, 2)),     # g is zero outside frames 2, 3 of the one clip
    _c('k311', 48, 32, (3, 1, 1), 1, (1, 0, 0), 1, 4, 5, 7),
    _c('k133', 128, 64, (1, 3, 3), 1, (0, 1, 1), 1, 4, 14, 18),
    _c('k133_roi', 128, 64, (1, 3, 3), 1, (0, 1, 1), 64, 1, 7, 7),
    _c('k333_s2_13x16', 128, 64, (3, 3, 3), 2, (1, 1, 1), 1, 3, 13, 16),
    _c('k333_s2_12x15', 128, 64, (3, 3, 3), 2, (1, 1, 1), 1, 3, 12, 15),
    _c('k333_s2_12x16', 128, 64, (3, 3, 3), 2, (1, 1, 1), 1, 3, 12, 16),
    _c('k111_s2_13x16', 256, 128, (1, 1, 1), 2, (0, 0, 0), 1, 2, 13, 16),
    _c('k111_s2_12x16', 256, 128, (1, 1, 1), 2, (0, 0, 0), 1, 2, 12, 16),
    _c('k111_200', 256, 200, (1, 1, 1), 1, (0, 0, 0), 1, 4, 14, 18),
    _c('ws64', 64, 64, (1, 3, 3), 1, (0, 1, 1), 1, 2, 20, 33),
    _c('pw256', 64, 256, (1, 1, 1), 1, (0, 0, 0), 1, 1, 5, 7),
    _c('tks', 256, 256, (3, 1, 1), 1, (1, 0, 0), 1, 4, 7, 10),
]
SMALL_BY_NAME = {c['name']: c for c in SMALL_CASES}

# the large-map cases (sampled float64 reference)
LARGE_CASES = [
    _c('pwlw', 128, 512, (1, 1, 1), 1, (0, 0, 0), 1, 4, 127, 130),       # 66 040 positions: >= 2 * 4 * 256 wave tiles of 32, ragged last one
    _c('pwks', 512, 2048, (1, 1, 1), 1, (0, 0, 0), 2, 1, 48, 64),         # 24 position blocks x 8 column blocks = 192 = 3/4 of 256 CUs
    _c('big_tile', 256, 256, (1, 3, 3), 1, (0, 1, 1), 2, 4, 96, 128),     # 48 tiles x 8 frames = 384 blocks = 1.5 per CU
]
LARGE_BY_NAME = {c['name']: c for c in LARGE_CASES}

_OPERANDS = {}


def case_operands(case, fmt, taps_ramp=False):
    """dict(g, w, scale, base, mask) of a case, numpy fp32, made once per (case, format) and left unchanged: g (N, Cout, T, Ho, Wo),
    base and mask (N, Cin, T, H, W) -- g, base and mask rounded to a 16-bit `fmt` (tensors the kernels read as they are); w and scale
    stay fp32 masters (the packer rounds w * scale).  mask is a ReLU output: about half of it zero.  The temporal taps of w carry
    the factors 1, 2, 3 so that no flip of them goes unnoticed."""
    key = (case['name'], fmt)
    if key not in _OPERANDS:
        rs = np.random.RandomState(sum(map(ord, case['name'])))
        k, cout, cin = case['k'], case['cout'], case['cin']
        Ho, Wo = out_hw(case['H'], case['W'], k, case['stride'], case['pads'])
        q = (lambda a: nm.q16(a, fmt)) if fmt in ('bf16', 'fp16') else (lambda a: a)
        g = q(rs.randn(case['N'], cout, case['T'], Ho, Wo).astype(np.float32))
        if case.get('g_frames'):
            t0, n = case['g_frames']
            g[:, :, :t0] = 0
            g[:, :, t0 + n:] = 0
        w = (rs.randn(cout, cin, *k) * np.sqrt(2.0 / (cin * k[0] * k[1] * k[2]))).astype(np.float32)
        w *= np.arange(1, k[0] + 1, dtype=np.float32).reshape(1, 1, -1, 1, 1) * np.float32(2.0 / (k[0] + 1))
        scale = rs.uniform(0.5, 1.5, cout).astype(np.float32)
        xs = (case['N'], cin, case['T'], case['H'], case['W'])
        base = q(rs.randn(*xs).astype(np.float32))
        mask = q(np.maximum(rs.randn(*xs), 0).astype(np.float32))
        _OPERANDS[key] = dict(g=g, w=w, scale=scale, base=base, mask=mask)
    return _OPERANDS[key]


def x_shape(case):
    return (case['N'], case['cin'], case['T'], case['H'], case['W'])


MODES = ('plain', 'accumulate', 'mask', 'mask_accumulate')


def mode_operands(o, mode):
    """(base, mask) of a run mode"""
    return (o['base'] if 'accumulate' in mode else None), (o['mask'] if 'mask' in mode else None)


def dx_bound(ref, absref, case, fmt):
    """The bound of tests/test_gpu_dgrad.py: K = cout * taps fp32 accumulations, one rounding to the stored format, and the packer's
    one rounding of w * scale (unit roundoff of the weight format times the sum of absolute products)."""
    return nm.bound(ref, absref, nm.conv_k(case['cout'], case['k']), fmt, extra=nm.unit_roundoff(fmt) * absref)


# ---- pack cases ------------------------------------------------------------------------------------------------------------------------------
# (forward master shape, data gradient?)  rows / columns of the packed matrix: forward Cout x Cin, data gradient Cin x Cout
PACK_CASES = [
    ((64, 64, 1, 1, 1), False), ((64, 64, 1, 1, 1), True),                # tile boundaries, one tap
    ((256, 128, 3, 1, 1), False), ((128, 256, 3, 1, 1), True),            # 256 x 128, three taps
    ((40, 24, 1, 3, 3), False), ((40, 24, 1, 3, 3), True),                # ragged 40 x 24 / 24 x 40, nine taps
    ((130, 72, 3, 3, 3), False), ((72, 130, 3, 3, 3), True),              # ragged 130 x 72, 27 taps
    ((12, 200, 1, 7, 7), False), ((200, 12, 1, 7, 7), True),              # ragged 12 x 200, 49 taps
    ((10, 7, 1, 3, 3), False), ((10, 7, 1, 3, 3), True),                  # runs of 7 x 9 = 63 floats: no 16-byte loads in either form
    ((130, 200, 1, 1, 1), True), ((40, 72, 3, 1, 1), False),
    ((16, 8, 5, 5, 5), False), ((16, 8, 5, 5, 5), True),                  # 125 taps: the element-wise kernel
]


def pack_case_id(c):
    return '%s-%s' % ('x'.join(str(v) for v in c[0]), 'dgrad' if c[1] else 'fwd')


def pack_master(shape, seed=0):
    """(w, scale): an fp32 master whose taps are all different and its forward-layer scale"""
    rs = np.random.RandomState(seed + sum(shape))
    w = rs.randn(*shape).astype(np.float32)
    scale = rs.uniform(0.5, 1.5, shape[0]).astype(np.float32)
    return w, scale
