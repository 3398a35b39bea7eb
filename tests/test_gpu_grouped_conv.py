"""The grouped forward conv kernel (conv3d_grouped_kernel) through hip_ops.ConvLayer(groups=G): every output
element against the float64 reference of tests/grouped_ref.py (per-group dense convs, concatenated) under the per-element bound of
tests/numerics.py with K = (Cin / G) * taps, in bf16 (the build's 16-bit format), fp32 and bf16x3; no leakage between groups; and
the default (groups = 1) routing unchanged."""
import numpy as np
import pytest
import torch

from tests import numerics as nm
from tests.grouped_ref import grouped_conv_ref64

pytestmark = pytest.mark.gpu

# name, C, channels per group, kT, stride, N, T, H, W, res_mode, relu.  The block tile is 256 positions (16 x 16 or a neighbour shape):
# H * W is never a multiple of it, so every case has partial tiles; the smallest shapes at which the slab logic can go wrong.
CASES = [
    ('c128_g32x4_1x3x3', 128, 4, 1, 1, 2, 1, 19, 23, 0, True),          # two slabs, 16 groups per slab
    ('c256_g32x8_3x3x3', 256, 8, 3, 1, 2, 3, 17, 21, 0, True),          # temporal taps at clip edges (two clips)
    ('c256_g16x16_1x3x3_s2', 256, 16, 1, 2, 2, 1, 37, 41, 0, False),    # stride-2 parity planes, odd sizes
    ('c128_g4x32_3x3x3_s2', 128, 32, 3, 2, 1, 2, 33, 29, 0, True),      # T = 2: a side tap always reads zeros
    ('c128_g2x64_1x3x3_sum', 128, 64, 1, 1, 3, 1, 15, 13, 1, True),     # one group per slab; Sum + ReLU (res_mode 1)
    ('c192_g3x64_3x3x3', 192, 64, 3, 1, 1, 3, 20, 20, 0, True),         # three slabs: block count not a power of two
]
MODES = ['bf16', 'fp32', 'bf16x3']
U16 = 2.0 ** -8                         # unit roundoff of bfloat16 (the split format of bf16x3)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mode(ops, mode):
    """(ConvLayer dtype, x3, output format of the bound)"""
    if mode == 'bf16x3' and ops.L.H16 == 'fp16':
        pytest.skip('bf16 build only')
    return (ops.BF16, False, nm.h16()) if mode == 'bf16' else (ops.F32, mode == 'bf16x3', 'fp32')


_OPERANDS = {}


def _operands(case, mode16):
    """numpy fp32 operands in NC(T)HW / Caffe2 filter layout; 16-bit mode: rounded to the build's 16-bit format (what the kernel sees).
    Made once per (case, quantised or not) and left unchanged."""
    key = (case[0], mode16)
    if key not in _OPERANDS:
        name, C, cg, kt, s, N, T, H, W, res_mode, relu = case
        rs = np.random.RandomState(sum(map(ord, name)))
        x = rs.randn(N, C, T, H, W).astype(np.float32)
        w = (rs.randn(C, cg, kt, 3, 3) * np.sqrt(2.0 / (cg * kt * 9))).astype(np.float32)
        scale = rs.uniform(0.5, 1.5, C).astype(np.float32)
        bias = (rs.randn(C) * 0.1).astype(np.float32)
        Ho, Wo = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
        res = rs.randn(N, C, T, Ho, Wo).astype(np.float32) if res_mode else None
        if mode16:
            x, w = nm.q16(x), nm.q16(w)
            res = nm.q16(res) if res is not None else None
        ref = grouped_conv_ref64(x, w, C // cg, scale, bias, res, (s, s), (kt // 2, 1, 1), relu)
        absconv = grouped_conv_ref64(x, w, C // cg, scale, None, None, (s, s), (kt // 2, 1, 1), False)[1]
        _OPERANDS[key] = (x, w, scale, bias, res, ref, absconv)
    return _OPERANDS[key]


def _run(ops, case, mode, x, w, scale, bias, res, want_split=False):
    name, C, cg, kt, s, N, T, H, W, res_mode, relu = case
    dtype, x3, fmt = _mode(ops, mode)
    layer = ops.ConvLayer(_dev(w), _dev(scale), _dev(bias), stride=(s, s), pads=(kt // 2, 1, 1), relu=relu, dtype=dtype, x3=x3,
                          groups=C // cg)
    xd = ops.to_ndhwc(_dev(x), dtype)
    rd = ops.to_ndhwc(_dev(res), dtype, layer.cstride) if res is not None else None
    prof = ops.ConvProfiler(capacity=8)
    prof.start()
    y = layer(xd, T=T, residual=rd, res_mode=res_mode, want_split=want_split)
    tags = [t for t, _, _ in prof.stop()]
    assert tags == [642570 + (2 if x3 else dtype)], 'not the grouped kernel: tags %r' % (tags,)
    return layer, y


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_grouped_conv_against_float64(ops, case, mode):
    name, C, cg, kt, s, N, T, H, W, res_mode, relu = case
    dtype, x3, fmt = _mode(ops, mode)
    x, w, scale, bias, res, (ref, absref), absconv = _operands(case, mode == 'bf16')
    layer, y = _run(ops, case, mode, x, w, scale, bias, res, want_split=x3)
    assert y.shape == (N * T,) + ref.shape[3:] + (C,)
    got = ops.to_ncdhw(y, dtype, N, C, T).cpu().numpy()
    # bf16x3 computes each product as x_hi w_hi + x_hi w_lo + x_lo w_hi with x = x_hi + x_lo + e_x, |x_lo| <= u |x|, |e_x| <= u^2 |x|
    # (u = 2^-8, bf16's unit roundoff; the same for w): it drops x_lo w_lo + e_x w + (x_hi + x_lo) e_w, at most (3 + u^2) u^2 |x w| per
    # product -- the arithmetic format's own error, on the conv sum (times |scale|) only, named here as the bound's `extra` term
    extra = (3.0 + U16 ** 2) * U16 ** 2 * absconv if x3 else 0.0
    err = np.abs(got - ref)
    print('grouped %s %s: max-abs err %.3e, worst err / bound %.3f' % (name, mode, err.max(), (err / nm.bound(ref, absref, cg * kt * 9, fmt, extra)).max()))
    nm.assert_elementwise(got, ref, absref, nm.conv_k(cg, (kt, 3, 3)), fmt, 'grouped %s %s' % (name, mode), extra)
    if x3:      # the split of the output written by the same launch is bit for bit dat_split_bf16x2 of the stored output
        assert y._split is not None and y._split.shape[-1] == 2 * C
        assert torch.equal(y._split, ops.split_bf16x2(y)), name


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('idx,channel', [(0, 70), (2, 129), (1, 63)])
def test_no_leakage_between_groups(ops, idx, channel, mode):
    """One perturbed input channel changes the outputs of its own group only, bit for bit -- what a wrong slab offset or a non-zero
    off-diagonal entry of the packed 64 x 64 image would break.  Channels at a slab edge and inside a slab."""
    case = CASES[idx]
    name, C, cg, kt, s, N, T, H, W, res_mode, relu = case
    dtype, x3, fmt = _mode(ops, mode)
    x, w, scale, bias, res = _operands(case, mode == 'bf16')[:5]
    _, y0 = _run(ops, case, mode, x, w, scale, bias, res)
    x1 = x.copy()
    x1[:, channel] += 1.0
    if mode == 'bf16':
        x1 = nm.q16(x1)             # (the other channels hold 16-bit values already: unchanged)
    assert np.array_equal(x1[:, :channel], x[:, :channel]) and np.array_equal(x1[:, channel + 1:], x[:, channel + 1:])
    _, y1 = _run(ops, case, mode, x1, w, scale, bias, res)
    g = channel // cg
    changed = (y0 != y1).reshape(-1, C).any(dim=0).cpu().numpy()
    own = np.zeros(C, dtype=bool)
    own[g * cg:(g + 1) * cg] = True
    assert not changed[~own].any(), 'channels outside group %d changed: %r' % (g, np.where(changed & ~own)[0].tolist())
    assert changed[own].all(), 'group %d did not see its own input channel %d' % (g, channel)


def test_groups_1_is_the_dense_layer_byte_for_byte(ops):
    rs = np.random.RandomState(3)
    x = nm.q16(rs.randn(1, 64, 2, 19, 23).astype(np.float32))
    w = nm.q16((rs.randn(128, 64, 3, 3, 3) * 0.05).astype(np.float32))
    scale, bias = rs.uniform(0.5, 1.5, 128).astype(np.float32), rs.randn(128).astype(np.float32)
    kw = dict(stride=(1, 1), pads=(1, 1, 1), relu=True, dtype=ops.BF16)
    a = ops.ConvLayer(_dev(w), _dev(scale), _dev(bias), **kw)
    b = ops.ConvLayer(_dev(w), _dev(scale), _dev(bias), groups=1, **kw)
    assert torch.equal(a.packed, b.packed)
    xd = ops.to_ndhwc(_dev(x), ops.BF16)
    ya, yb = a(xd, T=2), b(xd, T=2)
    assert torch.equal(ya.view(torch.int16), yb.view(torch.int16))
    assert a.flops(2, 19, 23) == b.flops(2, 19, 23) and a.hbm_bytes(2, 19, 23) == b.hbm_bytes(2, 19, 23)


@pytest.mark.parametrize('shape,match', [((128, 2, 1, 3, 3), 'channels per group'), ((128, 8, 1, 5, 5), 'kernel'),
                                         ((128, 8, 5, 3, 3), 'kernel')])
def test_unsupported_grouped_shapes_are_errors_not_dense_fallbacks(ops, shape, match):
    from detectandtrack_amd.libdat import DatError
    w = torch.zeros(shape, device='cuda')
    with pytest.raises(DatError, match=match) as e:
        ops.ConvLayer(w, stride=(1, 1), pads=(shape[2] // 2, shape[3] // 2, shape[4] // 2), dtype=ops.BF16, groups=128 // shape[1])
    assert '(code -4)' in str(e.value)
