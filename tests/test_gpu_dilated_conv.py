"""Dilated convs (dat_conv_desc.dil_h / dil_w) on the device, through hip_ops.ConvLayer and hip_ops.ConvGrad: every output element
against float64 under the per-element bound of tests/numerics.py.

Forward: the reference is tests/temporal_refs.windowed_conv_ref64 (numerics.conv_ref64 with frame windows) on the ZERO-INFLATED
kernel (tests/dilated_ref.inflate): a 3 x 3 dilated by d is the dense (2d + 1)^2 conv whose other weights are zero, so the zeros
add nothing to the reduction length K = Cin x taps or to the sum of absolute products.  Gradients: torch.nn.grad in float64 with
`dilation=`; K is the respective reduction length, as in tests/dgrad_refs.py (Cout x taps, plus the packer's one rounding of
w * scale) and tests/wgrad_refs.py (the output positions).

The shapes are the smallest at which each path can go wrong:
  a  64 -> 64, two 7 x 9 frames, d 2           the halo is as large as the map
  b  128 -> 128, kT 3, two clips of T 3, 12 x 20, d 2    temporal taps, clip borders and dilation together; also a key-frame window
  c  64 -> 128, 10 x 6, d 4                    taps entirely outside the map; the patch leaves the unrolled variant's registers
  d  512 -> 512, five 14 x 14 maps, d 2        the linear strips of RoI heads (the dilated-strip variant)
  e  256 -> 256, 48 x 84, d 2                  several 2-D tiles with partial border tiles
  f  64 -> 64, 17 x 23, d 3                    an odd d"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dgrad_refs
from tests import dilated_ref as dr
from tests import numerics as nm
from tests import temporal_refs as tr
from tests.test_gpu_kernels import _in_fresh_context

pytestmark = pytest.mark.gpu

#              N  Cin Cout T   H   W  kT  d
CASES = {'a': (2, 64, 64, 1, 7, 9, 1, 2), 'b': (2, 128, 128, 3, 12, 20, 3, 2), 'c': (1, 64, 128, 1, 10, 6, 1, 4),
         'd': (5, 512, 512, 1, 14, 14, 1, 2), 'e': (1, 256, 256, 1, 48, 84, 1, 2), 'f': (1, 64, 64, 1, 17, 23, 1, 3)}
MODES = ('16', 'fp32', 'bf16x3')


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mode(ops, mode):
    """(ConvLayer dtype, x3, operand format, output format of the bound) of '16' | 'fp32' | 'bf16x3'"""
    if mode == '16':
        fmt = 'fp16' if ops.L.H16 == 'fp16' else 'bf16'
        return ops.BF16, False, fmt, fmt
    if mode == 'bf16x3' and ops.L.H16 == 'fp16':
        pytest.skip('bf16x3 exists in the bf16 build only')
    return ops.F32, mode == 'bf16x3', 'fp32', 'fp32'


_OPERANDS, _REFS = {}, {}


def _operands(name, fmt):
    """numpy fp32 operands of a case, made once per (case, format) and left unchanged: x, w, scale, bias, a residual in the shape of
    ALL output frames (a window takes its frames), every clip and frame different; 16-bit formats: x, w, res rounded to the format."""
    key = (name, fmt)
    if key not in _OPERANDS:
        N, cin, cout, T, H, W, kt, d = CASES[name]
        rs = np.random.RandomState(sum(map(ord, 'dilated' + name)))
        x = rs.randn(N, cin, T, H, W).astype(np.float32)
        w = (rs.randn(cout, cin, kt, 3, 3) * np.sqrt(2.0 / (cin * kt * 9))).astype(np.float32)
        scale = rs.uniform(0.5, 1.5, cout).astype(np.float32)
        bias = (rs.randn(cout) * 0.1).astype(np.float32)
        res = rs.randn(N, cout, T, H, W).astype(np.float32)
        if fmt in ('bf16', 'fp16'):
            x, w, res = nm.q16(x, fmt), nm.q16(w, fmt), nm.q16(res, fmt)
        _OPERANDS[key] = dict(x=x, w=w, scale=scale, bias=bias, res=res)
    return _OPERANDS[key]


def _fwd_ref(name, fmt, epilogue, out_t=None):
    """(ref64, absref64) from the zero-inflated kernel, computed once and left unchanged"""
    key = (name, fmt, epilogue, out_t)
    if key not in _REFS:
        N, cin, cout, T, H, W, kt, d = CASES[name]
        o = _operands(name, fmt)
        res = o['res'] if out_t is None else o['res'][:, :, out_t[0]:out_t[0] + out_t[1]]
        e = dict(scale=o['scale'], bias=o['bias'], res=res, relu=True) if epilogue else dict(scale=None, bias=None, res=None, relu=False)
        _REFS[key] = tr.windowed_conv_ref64(o['x'], dr.inflate(o['w'], d), e['scale'], e['bias'], e['res'], (1, 1), (kt // 2, d, d),
                                            e['relu'], out_t=out_t)
    return _REFS[key]


class _Fwd(object):
    def __init__(self, ops, name, mode, epilogue=False, out_t=None):
        self.ops, self.name, self.mode, self.epilogue, self.out_t = ops, name, mode, epilogue, out_t
        N, cin, cout, T, H, W, kt, d = CASES[name]
        self.dtype, self.x3, self.fmt, self.out_fmt = _mode(ops, mode)
        o = _operands(name, self.fmt)
        self.layer = ops.ConvLayer(_dev(o['w']), _dev(o['scale']) if epilogue else None, _dev(o['bias']) if epilogue else None,
                                   stride=(1, 1), pads=(kt // 2, d, d), relu=epilogue, dtype=self.dtype, x3=self.x3, dilation=d)
        self.x = ops.to_ndhwc(_dev(o['x']), self.dtype)
        self.res = None
        if epilogue:
            res = o['res'] if out_t is None else o['res'][:, :, out_t[0]:out_t[0] + out_t[1]]
            self.res = ops.to_ndhwc(_dev(res), self.dtype, self.layer.cstride)
        self.otn = T if out_t is None else out_t[1]

    def run(self, plan=None):
        ops = self.ops
        T = CASES[self.name][3]
        prof = ops.ConvProfiler(capacity=8)
        try:
            if plan is not None:
                assert ops.tune_plan(*plan) == 0
            prof.start()
            y = self.layer(self.x, T=T, residual=self.res, res_mode=1 if self.res is not None else 0, out_t=self.out_t)
            tags = [t for t, _, _ in prof.stop()]
        finally:
            if plan is not None:
                ops.tune_plan(0, 0)
        return y, tags

    def check(self, y, tags, what):
        N, cin, cout, T, H, W, kt, d = CASES[self.name]
        # the generic kernel, marked dilated: channels per block * 10000 + positions * 10 + dtype + 5
        want = [(64 if cout <= 64 else 128) * 10000 + bp * 10 + (2 if self.x3 else self.dtype) + 5 for bp in (128, 256)]
        assert len(tags) == 1 and tags[0] in want, 'not the generic kernel with the dilated mark: tags %r' % (tags,)
        assert tuple(y.shape) == (N * self.otn, H, W, self.layer.cstride)
        got = self.ops.to_ncdhw(y, self.dtype, N, cout, self.otn).cpu().numpy()
        ref, absref = _fwd_ref(self.name, self.fmt, self.epilogue, self.out_t)
        K = nm.conv_k(cin, (kt, 3, 3))
        err = np.abs(got - ref)
        print('dilated %s %s %s: max-abs err %.3e, worst err / bound %.3f' %
              (self.name, self.mode, what, err.max(), float((err / nm.bound(ref, absref, K, self.out_fmt)).max())))
        nm.assert_elementwise(got, ref, absref, K, self.out_fmt, 'dilated %s %s %s' % (self.name, self.mode, what))


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sorted(CASES))
def test_dilated_forward(ops, name, mode):
    """The planner's plan; the small cases also under both forced tile sizes (128 and 256 positions take different patch shapes)."""
    L = _Fwd(ops, name, mode)
    y, tags = L.run()
    L.check(y, tags, 'planner')
    if name in ('a', 'c', 'f'):
        for plan in ((128, 1), (256, 1)):
            y, tags = L.run(plan)
            L.check(y, tags, 'plan %dx%d' % plan)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['b', 'e'])
def test_dilated_forward_full_epilogue(ops, name, mode):
    """scale, bias, residual and ReLU behind the dilated sums; on `b` also split-K over the (kt, chunk) patches."""
    L = _Fwd(ops, name, mode, epilogue=True)
    y, tags = L.run()
    L.check(y, tags, 'planner')
    if name == 'b':
        y, tags = L.run((128, 2))
        L.check(y, tags, 'plan 128x2')


@pytest.mark.parametrize('mode', MODES)
def test_dilated_key_frame_window(ops, mode):
    """`b` with out_t = (1, 1), what a following SliceKeyFrame keeps: the residual is indexed by OUTPUT frame."""
    L = _Fwd(ops, 'b', mode, epilogue=True, out_t=(1, 1))
    y, tags = L.run()
    L.check(y, tags, 'key frame')


@pytest.mark.parametrize('name', ['a', 'f'])
def test_dilated_table_driven_loop(ops, name):
    """DAT_CONV_NTAP=0 sends every layer to the table-driven loop: the same patch geometry read through the tap table per step."""
    L = _Fwd(ops, name, '16')
    y, tags = _in_fresh_context({'DAT_CONV_NTAP': '0'}, L.run)
    L.check(y, tags, 'table-driven loop')


@pytest.mark.parametrize('mode', ['16', 'fp32'])
def test_dilated_linear_strips_against_2d_tiles(ops, mode):
    """`d`, five 14 x 14 maps: linear strips save the dispatcher more than 10 % of the tiles, so the dilated-strip variant runs; with
    DAT_CONV_LINEAR=0 the same layer runs on 2-D tiles.  Both inside the bound, and bit for bit each other (the same products in the
    same order; a neighbour that left the map reads the zero row in one, the zero halo in the other)."""
    L = _Fwd(ops, 'd', mode)
    y_lin, tags = _in_fresh_context({'DAT_CONV_LINEAR': '1'}, L.run)
    y_2d, tags2 = _in_fresh_context({'DAT_CONV_LINEAR': '0'}, L.run)
    L.check(y_lin, tags, 'linear strips')
    L.check(y_2d, tags2, '2-D tiles')
    assert torch.equal(y_lin, y_2d)


def test_per_frame_strips_with_temporal_taps(ops):
    """kT 3 on 12 x 21 maps, d 2: one strip per frame (a tile must not span frames), against the 2-D tiles."""
    N, cin, cout, T, H, W, kt, d = 2, 64, 64, 3, 12, 21, 3, 2
    rs = np.random.RandomState(7)
    x = nm.q16(rs.randn(N, cin, T, H, W).astype(np.float32))
    w = nm.q16((rs.randn(cout, cin, kt, 3, 3) * np.sqrt(2.0 / (cin * kt * 9))).astype(np.float32))
    layer = ops.ConvLayer(_dev(w), None, None, stride=(1, 1), pads=(1, d, d), dtype=ops.BF16, dilation=d)
    xd = ops.to_ndhwc(_dev(x), ops.BF16)
    run = lambda: layer(xd, T=T)
    y_lin = _in_fresh_context({'DAT_CONV_LINEAR': '1'}, run)
    y_2d = _in_fresh_context({'DAT_CONV_LINEAR': '0'}, run)
    assert torch.equal(y_lin, y_2d)
    ref, absref = tr.windowed_conv_ref64(x, dr.inflate(w, d), None, None, None, (1, 1), (1, d, d), False)
    got = ops.to_ncdhw(y_lin, ops.BF16, N, cout, T).cpu().numpy()
    nm.assert_elementwise(got, ref, absref, nm.conv_k(cin, (kt, 3, 3)), nm.h16(), 'per-frame dilated strips')


# ---- what must not change -----------------------------------------------------------------------------------------------------------------
def _with_desc_dilation(layer, dil_h, dil_w):
    """the layer's descriptor with the dilation fields forced (what a C caller could pass and hip_ops never builds)"""
    real = layer.desc

    def desc(*a, **k):
        d = real(*a, **k)
        d.dil_h, d.dil_w = dil_h, dil_w
        return d
    layer.desc = desc
    return layer


def test_a_1x1_conv_ignores_the_dilation_fields(ops):
    rs = np.random.RandomState(1)
    x = ops.to_ndhwc(_dev(nm.q16(rs.randn(2, 128, 1, 9, 11).astype(np.float32))), ops.BF16)
    w = _dev((rs.randn(256, 128, 1, 1, 1) * 0.1).astype(np.float32))
    y0 = ops.ConvLayer(w, None, None, dtype=ops.BF16)(x)
    y2 = ops.ConvLayer(w, None, None, dtype=ops.BF16, dilation=2)(x)
    d = ops.ConvLayer(w, None, None, dtype=ops.BF16, dilation=2).desc(2, 1, 9, 11)
    assert (d.dil_h, d.dil_w) == (2, 2)
    assert torch.equal(y0, y2)


def test_dil_0_and_dil_1_are_the_same_undilated_conv(ops):
    rs = np.random.RandomState(2)
    x = ops.to_ndhwc(_dev(nm.q16(rs.randn(2, 64, 1, 13, 17).astype(np.float32))), ops.BF16)
    w = _dev((rs.randn(128, 64, 1, 3, 3) * 0.05).astype(np.float32))
    mk = lambda: ops.ConvLayer(w, None, None, pads=(0, 1, 1), dtype=ops.BF16)
    prof = ops.ConvProfiler(capacity=8)
    prof.start()
    y0 = mk()(x)
    y1 = _with_desc_dilation(mk(), 1, 1)(x)
    tags = [t for t, _, _ in prof.stop()]
    assert torch.equal(y0, y1)
    assert tags[0] == tags[1] and tags[0] % 10 == ops.BF16, tags      # (no dilated mark)


# ---- what is refused ----------------------------------------------------------------------------------------------------------------------
def test_refused_combinations_raise_with_their_text(ops):
    from detectandtrack_amd.libdat import DatError
    rs = np.random.RandomState(3)
    x = ops.to_ndhwc(_dev(nm.q16(rs.randn(1, 64, 1, 16, 16).astype(np.float32))), ops.BF16)
    w = _dev((rs.randn(64, 64, 1, 3, 3) * 0.05).astype(np.float32))
    with pytest.raises(DatError, match='dilation with a spatial stride > 1 is unsupported'):
        _with_desc_dilation(ops.ConvLayer(w, None, None, stride=(2, 2), pads=(0, 1, 1), dtype=ops.BF16), 2, 2)(x)
    with pytest.raises(DatError, match='dil_h != dil_w is unsupported'):
        _with_desc_dilation(ops.ConvLayer(w, None, None, pads=(0, 2, 2), dtype=ops.BF16), 2, 3)(x)
    wg = _dev((rs.randn(64, 16, 1, 3, 3) * 0.05).astype(np.float32))
    with pytest.raises(DatError, match='grouped dilated convs are unsupported'):
        _with_desc_dilation(ops.ConvLayer(wg, None, None, pads=(0, 1, 1), dtype=ops.BF16, groups=4), 2, 2)(x)
    # the Python layer says the same before a descriptor exists
    with pytest.raises(ValueError, match='stride'):
        ops.ConvLayer(w, None, None, stride=(2, 2), pads=(0, 2, 2), dtype=ops.BF16, dilation=2)
    with pytest.raises(ValueError, match='grouped'):
        ops.ConvLayer(wg, None, None, pads=(0, 2, 2), dtype=ops.BF16, groups=4, dilation=2)
    with pytest.raises(ValueError, match='stride'):
        ops.ConvGrad(w, None, (2, 2), (0, 2, 2), ops.BF16, 64, 64, dilation=2)
    # a patch beyond 160 KiB of LDS: 8 x 16 positions + a halo of 2 * 24 cells is 56 x 64 rows of 128 bytes
    xl = ops.to_ndhwc(_dev(nm.q16(rs.randn(1, 64, 1, 64, 64).astype(np.float32))), ops.BF16)
    with pytest.raises(DatError, match='dilation 24 is unsupported for this layer'):
        ops.ConvLayer(w, None, None, pads=(0, 24, 24), dtype=ops.BF16, dilation=24)(xl)
    # the weight gradient refuses the same descriptors
    cg = ops.ConvGrad(w, None, (2, 2), (0, 1, 1), ops.BF16, 64, 64)
    real = cg._fwd_desc

    def desc(*a, **k):
        d = real(*a, **k)
        d.dil_h = d.dil_w = 2
        return d
    cg._fwd_desc = desc
    g = torch.zeros((1, 8, 8, 64), dtype=x.dtype, device='cuda')
    with pytest.raises(DatError, match='dilation with a spatial stride > 1 is unsupported'):
        cg.weight(x, g, 1)


# ---- gradients ----------------------------------------------------------------------------------------------------------------------------
GRAD_CASES = ['a', 'b', 'd', 'e']
_GRADS = {}


def _grad_operands(ops, name, mode):
    """x (the forward input after a ReLU: the mask of the data gradient), g, the fp32 master w, scale; made once per (case, format)"""
    dtype, _, fmt, _ = _mode(ops, mode)
    key = (name, fmt)
    if key not in _GRADS:
        N, cin, cout, T, H, W, kt, d = CASES[name]
        rs = np.random.RandomState(sum(map(ord, 'dilated grad' + name)))
        x = np.maximum(rs.randn(N, cin, T, H, W), 0).astype(np.float32)
        g = rs.randn(N, cout, T, H, W).astype(np.float32)
        w = (rs.randn(cout, cin, kt, 3, 3) * np.sqrt(2.0 / (cin * kt * 9))).astype(np.float32)
        scale = rs.uniform(0.5, 1.5, cout).astype(np.float32)
        if fmt in ('bf16', 'fp16'):
            x, g = nm.q16(x, fmt), nm.q16(g, fmt)
        _GRADS[key] = dict(x=x, g=g, w=w, scale=scale)
    return dtype, fmt, _GRADS[key]


def _conv_grad(ops, name, dtype, o):
    N, cin, cout, T, H, W, kt, d = CASES[name]
    cg = ops.ConvGrad(_dev(o['w']), _dev(o['scale']), (1, 1), (kt // 2, d, d), dtype, ops.round_up(cin, 64), ops.round_up(cout, 64), dilation=d)
    return cg, ops.to_ndhwc(_dev(o['x']), dtype), ops.to_ndhwc(_dev(o['g']), dtype)


@pytest.mark.parametrize('mode', ['16', 'fp32'])
@pytest.mark.parametrize('name', GRAD_CASES)
def test_dilated_data_gradient_plain_and_relu_masked(ops, name, mode):
    """dL/dx = the conv of g with the flipped weights, dilation d, pads d (K - 1) - p; then the same launch with the ReLU mask of the
    forward input in its epilogue (res_mode 3)."""
    N, cin, cout, T, H, W, kt, d = CASES[name]
    dtype, fmt, o = _grad_operands(ops, name, mode)
    cg, xd, gd = _conv_grad(ops, name, dtype, o)
    case = dict(cout=cout, k=(kt, 3, 3))
    for mask in (None, o['x']):
        ref, absref = dr.dgrad_ref64(o['g'], o['w'], o['scale'], (kt // 2, d, d), d, (N, cin, T, H, W), mask=mask)
        dx = cg.data(gd, T, H, W, mask=None if mask is None else xd)
        got = ops.to_ncdhw(dx, dtype, N, cin, T).cpu().numpy()
        b = dgrad_refs.dx_bound(ref, absref, case, fmt)
        err = np.abs(got - ref)
        what = 'dilated dgrad %s %s %s' % (name, mode, 'masked' if mask is not None else 'plain')
        print('%s: max-abs err %.3e, worst err / bound %.3f' % (what, err.max(), float((err / b).max())))
        nm.assert_elementwise(got, ref, absref, nm.conv_k(cout, (kt, 3, 3)), fmt, what, extra=nm.unit_roundoff(fmt) * absref)


@pytest.mark.parametrize('mode', ['16', 'fp32'])
@pytest.mark.parametrize('name', GRAD_CASES)
def test_dilated_weight_gradient_direct_and_deferred(ops, name, mode):
    """dW[tap] = scale * sum_q g[q] x[q + (kh d - p, kw d - p)]: dat_conv3d_wgrad (kernel + finish), and the deferred-finish form the
    trainer uses by default -- dat_conv3d_wgrad_acc twice into one accumulator, then hip_ops.WeightFinishBatch: 2 x the reference.
    (fp32 layers have no deferred form: the re-pack kernels, immediate only.)"""
    N, cin, cout, T, H, W, kt, d = CASES[name]
    dtype, fmt, o = _grad_operands(ops, name, mode)
    cg, xd, gd = _conv_grad(ops, name, dtype, o)
    ref, absref, K = dr.wgrad_ref64(o['x'], o['g'], o['scale'], (kt, 3, 3), (kt // 2, d, d), d)
    dW, _ = cg.weight(xd, gd, T)
    nm.assert_elementwise(dW.cpu(), ref, absref, K, 'fp32', 'dilated wgrad %s %s immediate' % (name, mode))
    gt = torch.zeros(o['w'].size, dtype=torch.float32, device='cuda')
    ok = cg.weight_acc(xd, gd, T, gt)
    assert ok == (mode == '16'), 'deferred-finish support changed: %r' % (ok,)
    if ok:
        assert cg.weight_acc(xd, gd, T, gt)
        dW2 = torch.empty(o['w'].shape, dtype=torch.float32, device='cuda')
        ops.WeightFinishBatch([(gt, _dev(o['scale']), dW2, False)]).run()
        torch.cuda.synchronize()
        nm.assert_elementwise(dW2.cpu(), 2 * ref, 2 * absref, K, 'fp32', 'dilated wgrad %s %s deferred x2' % (name, mode))
        job = cg.weight_acc_job(xd, gd, T, torch.zeros_like(gt))
        assert job is not None
        ops.wgrad_acc_batch([job])
        dW3 = torch.empty(o['w'].shape, dtype=torch.float32, device='cuda')
        ops.WeightFinishBatch([(job[6], _dev(o['scale']), dW3, False)]).run()
        torch.cuda.synchronize()
        nm.assert_elementwise(dW3.cpu(), ref, absref, K, 'fp32', 'dilated wgrad %s %s batch' % (name, mode))
