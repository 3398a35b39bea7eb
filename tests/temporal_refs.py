"""Float64 reference of a conv with frame windows (the descriptor's out_t / in_t), a restatement of the frame bookkeeping every conv
kernel with temporal taps shares (valid tap range, rotated tap start, split-K patch ranges), seeded indexing defects, and the case
table of tests/test_gpu_temporal_windows.py.

Semantics (dat_conv_desc): out[n, :, t] = sum_kt w[:, :, kt] * x[n, :, t + kt - pad_t]; input frames outside [0, T) and outside
in_t = (t0, n) count as zero; only output frames out_t = [t0, t0 + n) of every clip exist; residual, mask and addend have the shape of
the RETURNED frames (indexed by output frame clip * otn + fc, the input by clip * T + t)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import numerics as nm


def _t64(a):
    if a is None:
        return None
    return a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.float64))


def _windows(T, out_t, in_t):
    ot0, otn = out_t if out_t is not None else (0, T)
    in_lo, in_hi = (in_t[0], in_t[0] + in_t[1]) if in_t is not None else (0, T)
    assert 0 <= ot0 and otn >= 1 and ot0 + otn <= T and 0 <= in_lo < in_hi <= T, (T, out_t, in_t)
    return ot0, otn, in_lo, in_hi


def _epilogue(y, absolute, scale, bias, res, relu, mask, addend):
    """The chain of numerics.conv_ref64 -- affine, + residual, ReLU, `mask > 0 ? v : 0` -- with mode 4's addend (`m > 0 ? v + addend
    : 0`) summed where the residual is; on absolute values: no ReLU, no mask."""
    f = (lambda v: v.abs()) if absolute else (lambda v: v)
    if scale is not None:
        y = y * f(_t64(scale)).view(1, -1, 1, 1, 1)
    if bias is not None:
        y = y + f(_t64(bias)).view(1, -1, 1, 1, 1)
    if res is not None:
        y = y + f(_t64(res))
    if addend is not None:
        y = y + f(_t64(addend))
    if relu and not absolute:
        y = torch.relu(y)
    if mask is not None and not absolute:
        y = torch.where(_t64(mask) > 0, y, torch.zeros_like(y))
    return y


def windowed_conv_ref64(x, w, scale, bias, res, stride, pads, relu, out_t=None, in_t=None, mask=None, addend=None):
    """(ref64, absref64), numpy float64 (N, Cout, otn, Ho, Wo), from the given (already quantised) operands.  x: (N, Cin, T, H, W);
    w: (Cout, Cin, KT, KH, KW); stride (sh, sw); pads (pad_t, pad_h, pad_w), any pad_t.
    F.conv3d over x padded by KT - 1 zero frames on either side yields at index j the sum of w[kt] * x[j + kt - (KT - 1)], so output
    frame t is index t + KT - 1 - pad_t; only the padded frames that the wanted outputs read are convolved."""
    x, w = _t64(x), _t64(w)
    T, KT = x.shape[2], w.shape[2]
    ot0, otn, in_lo, in_hi = _windows(T, out_t, in_t)
    x = x.clone()
    x[:, :, :in_lo] = 0
    x[:, :, in_hi:] = 0
    j0 = ot0 + KT - 1 - pads[0]
    assert 0 <= j0 and j0 + otn + KT - 1 <= T + 2 * (KT - 1), 'pad_t %d out of the range [0, KT - 1]' % pads[0]
    xp = F.pad(x, (0, 0, 0, 0, KT - 1, KT - 1))[:, :, j0:j0 + otn + KT - 1]
    outs = []
    for absolute in (False, True):
        f = (lambda v: v.abs()) if absolute else (lambda v: v)
        y = F.conv3d(f(xp), f(w), None, stride=(1,) + tuple(stride), padding=(0, pads[1], pads[2]))
        assert y.shape[2] == otn
        outs.append(_epilogue(y, absolute, scale, bias, res, relu, mask, addend).numpy())
    return outs[0], outs[1]


def grouped_windowed_conv_ref64(x, w, groups, scale, bias, res, stride, pads, relu, out_t=None, in_t=None, mask=None):
    """The same per group, as tests/grouped_ref.grouped_conv_ref64 states a grouped conv: G dense convs over channel slices, concatenated."""
    x, w = np.asarray(x), np.asarray(w)
    ci, co = x.shape[1] // groups, w.shape[0] // groups
    assert w.shape[1] == ci
    sl = lambda a, s, ax: None if a is None else (np.asarray(a)[s] if ax == 0 else np.asarray(a)[:, s])
    parts = []
    for g in range(groups):
        so = slice(g * co, (g + 1) * co)
        parts.append(windowed_conv_ref64(x[:, g * ci:(g + 1) * ci], w[so], sl(scale, so, 0), sl(bias, so, 0), sl(res, so, 1), stride, pads,
                                         relu, out_t, in_t, sl(mask, so, 1)))
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)


# ---- the kernels' frame bookkeeping, restated ------------------------------------------------------------------------------------------
def tap_range(t, T, KT, pad_t, in_lo, in_hi):
    """(kt_lo, n_kt) of output frame t: the two `while` loops of the kernels' prologue."""
    kt_lo, kt_hi = 0, KT - 1
    while kt_lo < KT and t + kt_lo - pad_t < in_lo:
        kt_lo += 1
    while kt_hi >= 0 and t + kt_hi - pad_t >= in_hi:
        kt_hi -= 1
    return kt_lo, kt_hi - kt_lo + 1


def frame_bookkeeping(T, KT, pad_t, out_t=None, in_t=None, n_cchunks=1, ksplit=1):
    """Per output frame of one clip: dict(t, n_kt, kshift (bool: the rotated tap start is not the first valid tap), empty_split (bool:
    some split-K slice s of `ksplit` gets the empty patch range [npatch * s / ksplit, npatch * (s + 1) / ksplit))).  `ksplit` is what
    the caller forces; the launcher caps it at (KT - 1) * n_cchunks (n_cchunks for KT == 1), restated here."""
    ot0, otn, in_lo, in_hi = _windows(T, out_t, in_t)
    ks = max(1, min(int(ksplit), (KT - 1 if KT > 1 else 1) * n_cchunks))
    out = []
    for fc in range(otn):
        t = ot0 + fc
        kt_lo, n_kt = tap_range(t, T, KT, pad_t, in_lo, in_hi)
        kshift = (KT - (t + kt_lo - pad_t) % KT) % KT if n_kt == KT else 0
        npatch = n_kt * n_cchunks
        empty = any(npatch * s // ks == npatch * (s + 1) // ks for s in range(ks))
        out.append(dict(t=t, n_kt=n_kt, kshift=kshift != 0, empty_split=empty))
    return out


# ---- seeded defects ----------------------------------------------------------------------------------------------------------------------
DEFECTS = ('origin', 'neighbour_clip', 'in_lo_plus_1', 'in_hi_minus_1', 'tap_shift', 'stale_sum', 'res_by_input_frame')


class TapProducts(object):
    """P[kt][n, :, tf] = the spatial conv of input frame tf of clip n with temporal tap kt's weights, float64, for every (kt, tf) of a
    shape row's UNWINDOWED input: every windowed result, right or defective, is a sum of these.  Made once per (row, format)."""

    def __init__(self, x, w, stride, pads, groups=1):
        x, w = _t64(x), _t64(w)
        self.N, self.T, self.KT, self.pads = x.shape[0], x.shape[2], w.shape[2], tuple(pads)
        self.P = [F.conv3d(x, w[:, :, kt:kt + 1], None, stride=(1,) + tuple(stride), padding=(0, pads[1], pads[2]), groups=groups)
                  for kt in range(self.KT)]

    def _frame(self, kt, n, tf, in_lo, in_hi, neighbour):
        """tap kt's product with frame tf of clip n under the input window, or None where that is zero"""
        if 0 <= tf < self.T:
            return self.P[kt][n, :, tf] if in_lo <= tf < in_hi else None
        if neighbour:                     # defect: the flat frame index runs into the next / previous clip
            n2, tf2 = n + (1 if tf >= self.T else -1), tf % self.T
            if 0 <= n2 < self.N and in_lo <= tf2 < in_hi:
                return self.P[kt][n2, :, tf2]
        return None

    def sums(self, out_t, in_t, defect=None):
        """(N, Cout, otn, Ho, Wo): the conv sums before the epilogue, with `defect` (one of DEFECTS, or None) seeded."""
        T, KT, pt = self.T, self.KT, self.pads[0]
        ot0, otn, in_lo, in_hi = _windows(T, out_t, in_t)
        y = torch.zeros((self.N, self.P[0].shape[1], otn) + tuple(self.P[0].shape[3:]), dtype=torch.float64)
        prev = None
        for n in range(self.N):
            for fc in range(otn):
                t = fc if defect == 'origin' else ot0 + fc
                kt_lo, n_kt = tap_range(t, T, KT, pt, in_lo, in_hi)     # (the true window: what the data is zero outside of)
                lo = in_lo + 1 if defect == 'in_lo_plus_1' else in_lo
                hi = in_hi - 1 if defect == 'in_hi_minus_1' else in_hi
                shift = 1 if (defect == 'tap_shift' and 0 < n_kt < KT) else 0
                if defect == 'stale_sum' and n_kt == 0 and prev is not None:
                    y[n, :, fc] = prev
                else:
                    for kt in range(KT):
                        tf = t + kt - pt
                        if shift and not (in_lo <= tf < in_hi):
                            continue          # the loop still runs over the valid taps only; each reads its neighbour's frame
                        v = self._frame(kt, n, tf + shift, lo, hi, defect == 'neighbour_clip')
                        if v is not None:
                            y[n, :, fc] += v
                prev = y[n, :, fc].clone()
        return y

    def applicable(self, defect, out_t, in_t, has_frame_operand):
        """Whether `defect` changes which products a result of this case sums (or which operand frame its epilogue reads): decided
        from the indices alone, never from the values."""
        T, KT, pt, N = self.T, self.KT, self.pads[0], self.N
        ot0, otn, in_lo, in_hi = _windows(T, out_t, in_t)
        frames = [(n, fc, ot0 + fc) for n in range(N) for fc in range(otn)]
        taps = lambda t: [t + kt - pt for kt in range(KT)]
        if defect == 'origin':
            return ot0 > 0
        if defect == 'neighbour_clip':
            return any((tf < 0 and n > 0 or tf >= T and n + 1 < N) and in_lo <= tf % T < in_hi for n, _, t in frames for tf in taps(t))
        if defect == 'in_lo_plus_1':
            return any(tf == in_lo for _, _, t in frames for tf in taps(t))
        if defect == 'in_hi_minus_1':
            return any(tf == in_hi - 1 for _, _, t in frames for tf in taps(t))
        if defect == 'tap_shift':
            return any(0 < tap_range(t, T, KT, pt, in_lo, in_hi)[1] < KT for _, _, t in frames)
        if defect == 'stale_sum':
            nk = [tap_range(t, T, KT, pt, in_lo, in_hi)[1] for _, _, t in frames]
            return any(k == 0 and any(nk[:i]) for i, k in enumerate(nk))
        if defect == 'res_by_input_frame':
            return has_frame_operand and any(n * T + t != n * otn + fc for n, fc, t in frames)
        raise KeyError(defect)


def defective_ref64(tp, defect, scale, bias, res, relu, out_t=None, in_t=None, mask=None, addend=None):
    """The float64 result of a kernel with `defect` seeded: (N, Cout, otn, Ho, Wo) numpy."""
    y = tp.sums(out_t, in_t, None if defect == 'res_by_input_frame' else defect)
    if defect == 'res_by_input_frame':
        ot0, otn = _windows(tp.T, out_t, in_t)[:2]
        N = tp.N

        def by_input_frame(a):
            if a is None:
                return None
            a = _t64(a)
            flat = a.permute(0, 2, 1, 3, 4).reshape((N * otn,) + tuple(a.shape[1:2]) + tuple(a.shape[3:]))
            flat = torch.cat([flat, torch.zeros_like(flat[:1])])             # (a read past the end -- whatever lies there -- counts as zeros)
            idx = [min(n * tp.T + ot0 + fc, N * otn) for n in range(N) for fc in range(otn)]
            return flat[idx].reshape((N, otn) + tuple(flat.shape[1:])).permute(0, 2, 1, 3, 4)
        res, mask, addend = by_input_frame(res), by_input_frame(mask), by_input_frame(addend)
    return _epilogue(y, False, scale, bias, res, relu, mask, addend).numpy()


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
OUT_WINDOWS = [((0, 1), None), ((3, 1), None), ((1, 2), None), ((0, 4), None)]
IN_WINDOWS = [(None, (0, 1)), (None, (3, 1)), (None, (1, 2))]
BOTH = [((2, 2), (1, 1))]
ALL_WINDOWS = OUT_WINDOWS + IN_WINDOWS + BOTH

# row name -> dict(N, Cin, Cout, T, H, W, k, stride, pads, groups); the sizes of the issue's table (the smallest at which each kernel
# variant runs; H * W never a multiple of 128)
ROWS = {
    'dense': dict(N=2, Cin=64, Cout=128, T=4, H=9, W=13, k=(3, 3, 3), stride=(1, 1), pads=(1, 1, 1)),
    'strips': dict(N=2, Cin=64, Cout=64, T=4, H=12, W=21, k=(3, 3, 3), stride=(1, 1), pads=(1, 1, 1)),
    'stride2': dict(N=2, Cin=64, Cout=128, T=3, H=13, W=17, k=(3, 3, 3), stride=(2, 2), pads=(1, 1, 1)),
    'k311': dict(N=2, Cin=128, Cout=256, T=4, H=7, W=9, k=(3, 1, 1), stride=(1, 1), pads=(1, 0, 0)),
    'time_to_channels_3': dict(N=3, Cin=64, Cout=128, T=3, H=5, W=7, k=(3, 1, 1), stride=(1, 1), pads=(0, 0, 0)),
    'time_to_channels_2': dict(N=3, Cin=64, Cout=128, T=2, H=5, W=7, k=(2, 1, 1), stride=(1, 1), pads=(0, 0, 0)),
    'short_t1': dict(N=3, Cin=64, Cout=128, T=1, H=6, W=10, k=(3, 3, 3), stride=(1, 1), pads=(1, 1, 1)),
    'short_t2': dict(N=3, Cin=64, Cout=128, T=2, H=6, W=10, k=(3, 3, 3), stride=(1, 1), pads=(1, 1, 1)),
    # two clips: 48 tiles x 2 channel blocks a frame, so two output frames of two clips are the 384 blocks at which DAT_CONV_BT=2
    # (blocks * 2 >= 3 * 256 CUs) picks the big-tile kernel
    'big_tile': dict(N=2, Cin=64, Cout=512, T=4, H=96, W=128, k=(3, 3, 3), stride=(1, 1), pads=(1, 1, 1)),
    'grouped': dict(N=2, Cin=128, Cout=128, T=4, H=11, W=13, k=(3, 3, 3), stride=(1, 1), pads=(1, 1, 1), groups=4),
    'grouped_s2': dict(N=2, Cin=128, Cout=128, T=4, H=11, W=13, k=(3, 3, 3), stride=(2, 2), pads=(1, 1, 1), groups=4),
}
EPILOGUES = ('none', 'affine_res_relu', 'mask', 'sum_mask')


def _case(row, out_t, in_t, epi='none', ksplits=(1,)):
    return dict(row=row, out_t=out_t, in_t=in_t, epi=epi, ksplits=tuple(ksplits),
                id='%s-out%s-in%s-%s' % (row, 'all' if out_t is None else '%d+%d' % out_t, 'all' if in_t is None else '%d+%d' % in_t, epi))


def _table():
    c = []
    for epi in ('none', 'affine_res_relu'):
        c += [_case('dense', o, i, epi, (1, 2)) for o, i in ALL_WINDOWS]
    for epi in ('mask', 'sum_mask'):        # (the data-gradient epilogues: always with the window of non-zero gradient frames)
        c += [_case('dense', o, i, epi, (1, 2)) for o, i in IN_WINDOWS + BOTH]
    c += [_case('strips', o, i, 'affine_res_relu') for o, i in ALL_WINDOWS]
    c += [_case('stride2', o, i, 'affine_res_relu', (1, 2)) for o, i in (((0, 1), None), ((2, 1), None), (None, (1, 1)))]
    c += [_case('k311', o, i, 'affine_res_relu') for o, i in ALL_WINDOWS]      # (one-tap layers of < 16 chunks never split)
    c += [_case('time_to_channels_3', (0, 1), None, 'affine_res_relu'), _case('time_to_channels_2', (0, 1), None, 'affine_res_relu')]
    c += [_case('short_t1', None, None, 'affine_res_relu', (1, 2, 3)), _case('short_t2', None, None, 'affine_res_relu', (1, 2, 3)),
          _case('short_t2', (1, 1), None, 'affine_res_relu', (1, 2, 3)), _case('short_t2', None, (0, 1), 'mask', (1, 2, 3))]
    c += [_case('big_tile', (1, 2), None, 'affine_res_relu'), _case('big_tile', (2, 2), None, 'affine_res_relu'), _case('big_tile', None, (1, 1), 'none')]
    c += [_case('grouped', o, None, 'affine_res_relu') for o in ((0, 1), (3, 1), (1, 2))]
    c += [_case('grouped', None, (1, 1), 'mask'), _case('grouped_s2', (3, 1), None, 'affine_res_relu')]
    return c


CASES = _table()
CASES_BY_ID = {c['id']: c for c in CASES}
assert len(CASES_BY_ID) == len(CASES)


def n_cchunks(row, fmt):
    """(kt, channel chunk) patches per temporal tap: 64 channels a chunk in the 16-bit formats, 32 in fp32, three 64-channel chunks
    [hi | hi | lo] per 64 channels in bf16x3."""
    cin = ROWS[row]['Cin'] // ROWS[row].get('groups', 1)
    return {'fp32': cin // 32, 'bf16x3': cin // 64 * 3}.get(fmt, max(1, cin // 64))


_ROW_OPERANDS = {}


def row_operands(row, fmt):
    """numpy fp32 operands of a shape row, made once per (row, format) and left unchanged: x (N, Cin, T, H, W) with every clip and
    frame different, w in the Caffe2 filter layout, scale, bias; 16-bit formats ('bf16' / 'fp16'): x and w rounded to the format."""
    key = (row, fmt)
    if key not in _ROW_OPERANDS:
        r = ROWS[row]
        rs = np.random.RandomState(sum(map(ord, row)))
        k, g = r['k'], r.get('groups', 1)
        x = rs.randn(r['N'], r['Cin'], r['T'], r['H'], r['W']).astype(np.float32)
        w = (rs.randn(r['Cout'], r['Cin'] // g, *k) * np.sqrt(2.0 / (r['Cin'] // g * k[0] * k[1] * k[2]))).astype(np.float32)
        scale = rs.uniform(0.5, 1.5, r['Cout']).astype(np.float32)
        bias = (rs.randn(r['Cout']) * 0.1).astype(np.float32)
        if fmt in ('bf16', 'fp16'):
            x, w = nm.q16(x, fmt), nm.q16(w, fmt)
        _ROW_OPERANDS[key] = (x, w, scale, bias)
    return _ROW_OPERANDS[key]


def out_hw(row):
    r = ROWS[row]
    return ((r['H'] + 2 * r['pads'][1] - r['k'][1]) // r['stride'][0] + 1, (r['W'] + 2 * r['pads'][2] - r['k'][2]) // r['stride'][1] + 1)


def case_operands(case, fmt):
    """dict(x, w, scale, bias, res, mask, addend, relu) of a case: x zero outside in_t (the contract of the window: the kernels skip
    those frames' taps, the 1x1 kernels read them), the frame operands in the shape of the returned frames, different in every frame."""
    r = ROWS[case['row']]
    x, w, scale, bias = row_operands(case['row'], fmt)
    ot0, otn, in_lo, in_hi = _windows(r['T'], case['out_t'], case['in_t'])
    if case['in_t'] is not None:
        x = x.copy()
        x[:, :, :in_lo] = 0
        x[:, :, in_hi:] = 0
    rs = np.random.RandomState(sum(map(ord, case['id'])) % (2 ** 31))
    ho, wo = out_hw(case['row'])
    frame_op = lambda: (nm.q16(rs.randn(r['N'], r['Cout'], otn, ho, wo).astype(np.float32), fmt) if fmt in ('bf16', 'fp16')
                        else rs.randn(r['N'], r['Cout'], otn, ho, wo).astype(np.float32))
    epi = case['epi']
    o = dict(x=x, w=w, scale=None, bias=None, res=None, mask=None, addend=None, relu=False)
    if epi == 'affine_res_relu':
        o.update(scale=scale, bias=bias, res=frame_op(), relu=True)
    elif epi == 'mask':
        o.update(mask=frame_op())
    elif epi == 'sum_mask':
        o.update(mask=frame_op(), addend=frame_op())
    else:
        assert epi == 'none'
    return o


def case_ref64(case, fmt, operands=None):
    """(ref64, absref64) of a case from case_operands (or from `operands`, e.g. a slice of their output channels)."""
    r, o = ROWS[case['row']], (operands if operands is not None else case_operands(case, fmt))
    if r.get('groups', 1) > 1:
        assert o['addend'] is None
        return grouped_windowed_conv_ref64(o['x'], o['w'], r['groups'], o['scale'], o['bias'], o['res'], r['stride'], r['pads'], o['relu'],
                                           case['out_t'], case['in_t'], o['mask'])
    return windowed_conv_ref64(o['x'], o['w'], o['scale'], o['bias'], o['res'], r['stride'], r['pads'], o['relu'], case['out_t'],
                               case['in_t'], o['mask'], o['addend'])
