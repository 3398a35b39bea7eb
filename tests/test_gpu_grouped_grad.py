"""Backward of the grouped conv through hip_ops.ConvGrad(groups=G): the data gradient (the grouped forward kernel
over the gradient with dat_conv3d_grouped_pack_weights_dgrad's weights; res_mode 1 and 3) and the weight gradient
(wgrad_grouped_kernel, immediate and deferred form), every element against the float64 references of tests/grouped_grad_ref.py under
the per-element bound of tests/numerics.py, in the build's 16-bit format and in fp32; no leakage between groups; unsupported calls."""
import numpy as np
import pytest
import torch

from tests import numerics as nm
from tests.grouped_grad_ref import grouped_dgrad_ref64, grouped_wgrad_ref64

pytestmark = pytest.mark.gpu

# name, C, channels per group, kT, stride, N, T, H, W (input), extra.  H * W (and Ho * Wo) is never a multiple of the 256-position tile of
# the data-gradient layer nor of the 8 x 8 patches of the weight gradient: every case has partial tiles.
CASES = [
    ('c128_g32x4_1x3x3', 128, 4, 1, 1, 2, 1, 19, 23, None),
    ('c256_g32x8_3x3x3', 256, 8, 3, 1, 2, 3, 17, 21, None),              # temporal taps at clip edges (two clips)
    ('c256_g16x16_1x3x3_s2', 256, 16, 1, 2, 2, 1, 37, 41, None),         # zero-insert, odd sizes
    ('c128_g4x32_3x3x3_s2', 128, 32, 3, 2, 1, 2, 36, 40, None),          # even sizes: the last input row / column has no output
    ('c128_g2x64_1x3x3', 128, 64, 1, 1, 3, 1, 15, 13, 'mask'),           # res_mode 3, then res_mode 1 in place and out of place
    ('c192_g3x64_3x3x3', 192, 64, 3, 1, 1, 3, 20, 20, 'window'),         # g_frames = (1, 1)
]
# the weight gradient: the six geometries with a full g -- the sixth too, so that the cg = 64, KT = 3 layout sees gradient in the frames at
# the clip edges, whose outer temporal taps fall outside the clip -- and the windowed case as the seventh
WGRAD_CASES = CASES[:5] + [('c192_g3x64_3x3x3_full', 192, 64, 3, 1, 1, 3, 20, 20, None), CASES[5]]
MODES = ['bf16', 'fp32']
GROUPED_FWD_TAG, GROUPED_WGRAD_TAG = 642570, 642580


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mode(ops, mode):
    return (ops.BF16, nm.h16()) if mode == 'bf16' else (ops.F32, 'fp32')


def _out_hw(H, W, s):
    return (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1


_OPERANDS = {}


def _operands(case, mode16):
    """numpy fp32 operands in NC(T)HW / Caffe2 filter layout, made once per (case, quantised or not) and left unchanged.  16-bit mode:
    x, g, mask and the addend rounded to the build's 16-bit format; the fp32 master w and the scale stay fp32 (the pack rounds their
    product)."""
    key = (case[0], mode16)
    if key not in _OPERANDS:
        name, C, cg, kt, s, N, T, H, W, extra = case
        rs = np.random.RandomState(sum(map(ord, name)) + 1)
        Ho, Wo = _out_hw(H, W, s)
        x = rs.randn(N, C, T, H, W).astype(np.float32)
        g = rs.randn(N, C, T, Ho, Wo).astype(np.float32)
        if extra == 'window':
            g[:, :, 0] = 0
            g[:, :, 2:] = 0
        w = (rs.randn(C, cg, kt, 3, 3) * np.sqrt(2.0 / (cg * kt * 9))).astype(np.float32)
        scale = rs.uniform(0.5, 1.5, C).astype(np.float32)
        mask = rs.randn(N, C, T, H, W).astype(np.float32)
        add = rs.randn(N, C, T, H, W).astype(np.float32)
        if mode16:
            x, g, mask, add = nm.q16(x), nm.q16(g), nm.q16(mask), nm.q16(add)
        _OPERANDS[key] = dict(x=x, g=g, w=w, scale=scale, mask=mask, add=add)
    return _OPERANDS[key]


def _w_seen(o, mode16, with_scale=True):
    """The filter operand of the data-gradient kernel: fp32(w) * fp32(scale[co]) in fp32, rounded to the 16-bit format in 16-bit mode."""
    ws = (o['w'] * o['scale'].reshape(-1, 1, 1, 1, 1)).astype(np.float32) if with_scale else o['w']
    return nm.q16(ws) if mode16 else ws


def _convgrad(ops, case, mode, o, with_scale=True):
    name, C, cg, kt, s, N, T, H, W, extra = case
    dtype = _mode(ops, mode)[0]
    return ops.ConvGrad(_dev(o['w']), _dev(o['scale']) if with_scale else None, (s, s), (kt // 2, 1, 1), dtype, C, C, groups=C // cg)


def _profiled(ops, fn):
    prof = ops.ConvProfiler(capacity=8)
    prof.start()
    out = fn()
    return out, [t for t, _, _ in prof.stop()]


# ---- data gradient ------------------------------------------------------------------------------------------------------------------------
_DGRAD_REF = {}


def _dgrad_ref(case, mode16, variant):
    key = (case[0], mode16, variant)
    if key not in _DGRAD_REF:
        name, C, cg, kt, s, N, T, H, W, extra = case
        o = _operands(case, mode16)
        _DGRAD_REF[key] = grouped_dgrad_ref64(o['g'], _w_seen(o, mode16), C // cg, s, (kt // 2, 1, 1), H, W,
                                              add=o['add'] if variant.startswith('add') else None,
                                              mask=o['mask'] if variant == 'mask' else None)
    return _DGRAD_REF[key]


def _dgrad_variants(case):
    return ['plain', 'mask', 'add_inplace', 'add_new'] if case[9] == 'mask' else ['plain']


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_grouped_data_gradient_against_float64(ops, case, mode):
    name, C, cg, kt, s, N, T, H, W, extra = case
    dtype, fmt = _mode(ops, mode)
    mode16 = mode == 'bf16'
    o = _operands(case, mode16)
    cgr = _convgrad(ops, case, mode, o)
    gd = ops.to_ndhwc(_dev(o['g']), dtype)
    g_frames = (1, 1) if extra == 'window' else None
    for variant in _dgrad_variants(case):
        ref, absref = _dgrad_ref(case, mode16, variant)
        kw, addd = {}, None
        if variant == 'mask':
            kw = dict(mask=ops.to_ndhwc(_dev(o['mask']), dtype))
        elif variant.startswith('add'):
            addd = ops.to_ndhwc(_dev(o['add']), dtype)
            keep = addd.clone()
            kw = dict(accumulate_into=addd, inplace=variant == 'add_inplace')
        dx, tags = _profiled(ops, lambda: cgr.data(gd, T, H, W, g_frames=g_frames, **kw))
        assert tags == [GROUPED_FWD_TAG + dtype], 'not the grouped kernel: tags %r' % (tags,)
        assert dx.shape == (N * T, H, W, C)
        if variant == 'add_inplace':
            assert dx.data_ptr() == addd.data_ptr()
        elif variant == 'add_new':
            assert dx.data_ptr() != addd.data_ptr() and torch.equal(addd, keep), 'inplace=False must leave the addend untouched'
        got = ops.to_ncdhw(dx, dtype, N, C, T).cpu().numpy()
        K = nm.conv_k(cg, (kt, 3, 3))
        err = np.abs(got - ref)
        print('grouped dgrad %s %s %s: max-abs err %.3e, worst err / bound %.3f'
              % (name, mode, variant, err.max(), (err / nm.bound(ref, absref, K, fmt)).max()))
        nm.assert_elementwise(got, ref, absref, K, fmt, 'grouped dgrad %s %s %s' % (name, mode, variant))


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------------
_WGRAD_REF = {}


def _wgrad_ref(case, mode16, with_scale):
    key = (case[0], mode16, with_scale)
    if key not in _WGRAD_REF:
        name, C, cg, kt, s, N, T, H, W, extra = case
        o = _operands(case, mode16)
        _WGRAD_REF[key] = grouped_wgrad_ref64(o['x'], o['g'], C // cg, o['scale'] if with_scale else None, (kt, 3, 3), s, (kt // 2, 1, 1),
                                              window=(1, 1) if extra == 'window' else None)
    return _WGRAD_REF[key]


@pytest.mark.parametrize('with_scale', [True, False], ids=['scale', 'noscale'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', WGRAD_CASES, ids=[c[0] + ('_window' if c[9] == 'window' else '') for c in WGRAD_CASES])
def test_grouped_weight_gradient_against_float64(ops, case, mode, with_scale):
    """The immediate form, and the deferred form added TWICE into one accumulator and finished by WeightFinishBatch (reference and
    bound doubled).  The 'window' case passes g_frames; its g is zero outside that frame.  Every other case has a full g."""
    name, C, cg, kt, s, N, T, H, W, extra = case
    dtype = _mode(ops, mode)[0]
    mode16 = mode == 'bf16'
    o = _operands(case, mode16)
    ref, absref, K = _wgrad_ref(case, mode16, with_scale)
    Ho, Wo = _out_hw(H, W, s)
    assert K == N * (1 if extra == 'window' else T) * Ho * Wo
    cgr = _convgrad(ops, case, mode, o, with_scale)
    xd, gd = ops.to_ndhwc(_dev(o['x']), dtype), ops.to_ndhwc(_dev(o['g']), dtype)
    g_frames = (1, 1) if extra == 'window' else None
    (dW, _), tags = _profiled(ops, lambda: cgr.weight(xd, gd, T, g_frames=g_frames))
    assert tags == [GROUPED_WGRAD_TAG + dtype], 'not the grouped weight-gradient kernel: tags %r' % (tags,)
    assert tuple(dW.shape) == (C, cg, kt, 3, 3) and dW.dtype == torch.float32
    got = dW.cpu().numpy()
    err = np.abs(got - ref)
    print('grouped wgrad %s %s: max-abs err %.3e, worst err / bound %.3f' % (name, mode, err.max(), (err / nm.bound(ref, absref, K, 'fp32')).max()))
    nm.assert_elementwise(got, ref, absref, K, 'fp32', 'grouped wgrad %s %s' % (name, mode))
    # deferred: the accumulator has the kept elements only
    gt = torch.zeros(C * cg * kt * 9, dtype=torch.float32, device='cuda')
    assert gt.numel() == cgr.w.numel()
    assert cgr.weight_acc(xd, gd, T, gt, g_frames=g_frames) and cgr.weight_acc(xd, gd, T, gt, g_frames=g_frames)
    dW2 = torch.full((C, cg, kt, 3, 3), float('nan'), dtype=torch.float32, device='cuda')
    ops.WeightFinishBatch([(gt, cgr.scale, dW2, False)]).run()
    nm.assert_elementwise(dW2.cpu().numpy(), 2.0 * ref, 2.0 * absref, K, 'fp32', 'grouped wgrad (deferred, twice) %s %s' % (name, mode))


# ---- no leakage between groups ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('idx,channel', [(0, 64), (2, 127), (1, 77)])
def test_no_leakage_between_groups_in_either_gradient(ops, idx, channel, mode):
    """One perturbed channel of g: the data gradient changes in the channels of that channel's group only, bit for bit; the weight
    gradient changes in row `channel` -- a row of its own group -- and stays the float64 reference's everywhere else (its float atomics
    arrive in any order, so the untouched rows are compared under the bound, not bit for bit).  Channels at both edges of a slab and
    inside one."""
    case = CASES[idx]
    name, C, cg, kt, s, N, T, H, W, extra = case
    dtype = _mode(ops, mode)[0]
    mode16 = mode == 'bf16'
    o = _operands(case, mode16)
    g1 = o['g'].copy()
    g1[:, channel] += 1.0
    if mode16:
        g1 = nm.q16(g1)
    assert np.array_equal(np.delete(g1, channel, axis=1), np.delete(o['g'], channel, axis=1))
    cgr = _convgrad(ops, case, mode, o)
    xd = ops.to_ndhwc(_dev(o['x']), dtype)
    gd0, gd1 = ops.to_ndhwc(_dev(o['g']), dtype), ops.to_ndhwc(_dev(g1), dtype)
    grp = channel // cg
    own = np.zeros(C, dtype=bool)
    own[grp * cg:(grp + 1) * cg] = True
    dx0, dx1 = cgr.data(gd0, T, H, W), cgr.data(gd1, T, H, W)
    changed = (dx0 != dx1).reshape(-1, C).any(dim=0).cpu().numpy()
    assert not changed[~own].any(), 'dx channels outside group %d changed: %r' % (grp, np.where(changed & ~own)[0].tolist())
    assert changed[own].all(), 'group %d did not see its own gradient channel %d' % (grp, channel)
    dW0 = cgr.weight(xd, gd0, T)[0].cpu().numpy()
    dW1 = cgr.weight(xd, gd1, T)[0].cpu().numpy()
    ref0, abs0, K = _wgrad_ref(case, mode16, True)
    ref1, abs1, _ = grouped_wgrad_ref64(o['x'], g1, C // cg, o['scale'], (kt, 3, 3), s, (kt // 2, 1, 1))
    rows = np.arange(C) != channel
    assert np.array_equal(ref1[rows], ref0[rows])
    nm.assert_elementwise(dW1, ref1, abs1, K, 'fp32', 'grouped wgrad, perturbed g, %s %s' % (name, mode))
    nm.assert_elementwise(dW1[rows], ref0[rows], abs0[rows], K, 'fp32', 'grouped wgrad rows outside the perturbed one, %s %s' % (name, mode))
    assert (dW1[channel] != dW0[channel]).any()
    # the accumulator is Gt[tap][C][cg]: elements outside the diagonal blocks do not exist, so nothing can land in them.  The kernel fills
    # exactly this tensor: row `channel` of every tap holds its own group's cg products, the finish turns it into dW
    gt = torch.zeros(kt * 9, C, cg, dtype=torch.float32, device='cuda')
    assert gt.numel() == C * cg * kt * 9
    assert cgr.weight_acc(xd, gd1, T, gt)
    dW2 = torch.full((C, cg, kt, 3, 3), float('nan'), dtype=torch.float32, device='cuda')
    ops.WeightFinishBatch([(gt, cgr.scale, dW2, False)]).run()
    nm.assert_elementwise(dW2.cpu().numpy(), ref1, abs1, K, 'fp32', 'grouped wgrad through Gt[tap][C][cg], perturbed g, %s %s' % (name, mode))


# ---- unsupported calls --------------------------------------------------------------------------------------------------------------------
def _refused(ops, fn, match):
    from detectandtrack_amd.libdat import DatError
    prof = ops.ConvProfiler(capacity=8)
    prof.start()
    try:
        with pytest.raises(DatError, match=match) as e:
            fn()
    finally:
        launched = prof.stop()
    assert '(code -4)' in str(e.value), str(e.value)       # DAT_ERR_UNSUPPORTED
    assert launched == [], 'a refused call launched %r' % (launched,)


@pytest.mark.parametrize('what', ['cg2', 'cin_ne_cout', 'k5x5', 'res_mode4'])
def test_unsupported_grouped_gradient_calls_are_errors(ops, what):
    C, cg, k, x_cs, match = {'cg2': (128, 2, 3, 128, 'channels per group'), 'cin_ne_cout': (128, 8, 3, 64, 'Cin 64 == Cout 128'),
                             'k5x5': (128, 8, 5, 128, 'kernel'), 'res_mode4': (128, 8, 3, 128, 'res_mode 4')}[what]
    w = torch.zeros(C, cg, 1, k, k, device='cuda')
    cgr = ops.ConvGrad(w, None, (1, 1), (0, k // 2, k // 2), ops.BF16, x_cs, C, groups=C // cg)
    x = torch.zeros(2, 11, 9, x_cs, dtype=nm.h16(), device='cuda')
    g = torch.zeros(2, 11, 9, C, dtype=nm.h16(), device='cuda')
    if what == 'res_mode4':
        into, mask = torch.zeros_like(g), torch.zeros_like(g)
        _refused(ops, lambda: cgr.data(g, 1, 11, 9, accumulate_into=into, mask=mask), match)
        return
    _refused(ops, lambda: cgr.weight(x, g, 1), match)
    gt = torch.zeros(w.numel(), dtype=torch.float32, device='cuda')
    _refused(ops, lambda: cgr.weight_acc(x, g, 1, gt), match)
    assert not gt.any()
    if what != 'cin_ne_cout':
        _refused(ops, lambda: cgr.data(g, 1, 11, 9), match)
