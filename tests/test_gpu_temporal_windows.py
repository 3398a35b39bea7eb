"""Frame windows (out_t / in_t) of the conv kernels with temporal taps -- the generic implicit-GEMM kernel in its variants, the big-tile
kernel, the grouped kernel -- through hip_ops.ConvLayer: every output element against tests/temporal_refs.windowed_conv_ref64 under
the per-element bound of tests/numerics.py.  The cases (tests/temporal_refs.CASES; tests/test_temporal_refs_cpu.py shows that every
seeded frame-indexing defect leaves the bound at each of them) reach output frames with 0, 1, 2 and 3 valid taps, the rotated tap
start, split-K slices with an empty patch range, clip borders, and residual / mask / addend operands indexed by OUTPUT frame.
x is zero outside in_t by construction: that is the window's contract (the kernels skip those frames' taps)."""
import numpy as np
import pytest
import torch

from tests import numerics as nm
from tests import temporal_refs as tr
from tests.test_gpu_kernels import _in_fresh_context

pytestmark = pytest.mark.gpu

BT_TAG, GROUPED_TAG = 2562560, 642570


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bf16_only(ops):
    if ops.L.H16 == 'fp16':
        pytest.skip('bf16 build only')


def _mode(ops, mode):
    """(ConvLayer dtype, x3, operand format, output format of the bound) of '16' | 'fp32' | 'bf16x3'"""
    if mode == '16':
        fmt = 'fp16' if ops.L.H16 == 'fp16' else 'bf16'
        return ops.BF16, False, fmt, fmt
    return ops.F32, mode == 'bf16x3', 'fp32', 'fp32'


def _generic_tag(ops, case, mode, bp):
    return (64 if tr.ROWS[case['row']]['Cout'] <= 64 else 128) * 10000 + bp * 10 + (2 if mode == 'bf16x3' else _mode(ops, mode)[0])


_REFS = {}


def _ref(case, fmt):
    """(ref64, absref64) of a case, computed once and left unchanged"""
    key = (case['id'], fmt)
    if key not in _REFS:
        _REFS[key] = tr.case_ref64(case, fmt)
    return _REFS[key]


class _Launcher(object):
    """The layer and the device operands of a case; run(plan) -> (NDHWC output, dispatcher tags) on the CURRENT context."""

    def __init__(self, ops, case, mode):
        self.ops, self.case, self.r = ops, case, tr.ROWS[case['row']]
        r = self.r
        self.dtype, self.x3, self.fmt, self.out_fmt = _mode(ops, mode)
        o = tr.case_operands(case, self.fmt)
        dv = lambda a: None if a is None else _dev(a)
        self.layer = ops.ConvLayer(_dev(o['w']), dv(o['scale']), dv(o['bias']), stride=r['stride'], pads=r['pads'], relu=o['relu'],
                                   dtype=self.dtype, x3=self.x3, groups=r.get('groups', 1))
        self.x = ops.to_ndhwc(_dev(o['x']), self.dtype)
        fr = lambda a: None if a is None else ops.to_ndhwc(_dev(a), self.dtype, self.layer.cstride)
        self.res, self.mask, self.addend = fr(o['res']), fr(o['mask']), fr(o['addend'])
        self.otn = case['out_t'][1] if case['out_t'] is not None else r['T']

    def run(self, plan=None):
        ops, case = self.ops, self.case
        kw = dict(T=self.r['T'], out_t=case['out_t'], in_t=case['in_t'])
        prof = ops.ConvProfiler(capacity=8)
        try:
            if plan is not None:
                assert ops.tune_plan(*plan) == 0
            prof.start()
            if case['epi'] == 'sum_mask':       # in place, as the training step runs it: the output tensor is the addend
                acc = self.addend.clone()
                y = self.layer(self.x, residual=self.mask, res_mode=4, addend=acc, out=acc, **kw)
            elif case['epi'] == 'mask':
                y = self.layer(self.x, residual=self.mask, res_mode=3, **kw)
            else:
                y = self.layer(self.x, residual=self.res, res_mode=1 if self.res is not None else 0, **kw)
            tags = [t for t, _, _ in prof.stop()]
        finally:
            if plan is not None:
                ops.tune_plan(0, 0)
        assert y.shape[0] == self.r['N'] * self.otn
        return y, tags

    def check(self, y, what):
        """every element of `y` against the float64 reference; prints the worst err / bound and returns it"""
        r, case = self.r, self.case
        got = self.ops.to_ncdhw(y, self.dtype, r['N'], r['Cout'], self.otn).cpu().numpy()
        ref, absref = _ref(case, self.fmt)
        K = nm.conv_k(r['Cin'] // r.get('groups', 1), r['k'])
        err = np.abs(got - ref)
        ratio = float((err / nm.bound(ref, absref, K, self.out_fmt)).max())
        print('windows %s %s %s: max-abs err %.3e, worst err / bound %.3f' % (case['id'], self.fmt + ('x3' if self.x3 else ''), what, err.max(), ratio))
        if self.out_fmt == 'fp32':      # the max-abs limits of tests/test_gpu_kernels.py::test_conv3d stay beside the per-element bound
            assert err.max() < (5e-4 if self.x3 else 2e-4), (what, err.max())
        nm.assert_elementwise(got, ref, absref, K, self.out_fmt, 'windows %s %s' % (case['id'], what))
        return ratio


def _cases(rows, pick=None):
    cs = [c for c in tr.CASES if c['row'] in rows and (pick is None or pick(c))]
    return pytest.mark.parametrize('case', cs, ids=[c['id'] for c in cs])


# ---- generic kernel -----------------------------------------------------------------------------------------------------------------------
@_cases(('dense',))
def test_dense_3x3x3_windows(ops, case):
    """64 -> 128, two clips of four 9 x 13 frames: both tile sizes, split-K (64 channels are ONE chunk: a frame with one valid tap
    leaves split 0 of 2 an empty range, a frame with none leaves both empty), and the table-driven loop (DAT_CONV_NTAP=0)."""
    L = _Launcher(ops, case, '16')
    for plan in ((128, 1), (128, 2), (256, 1)):
        y, tags = L.run(plan)
        assert tags == [_generic_tag(ops, case, '16', plan[0])], (plan, tags)
        L.check(y, 'plan %dx%d' % plan)
    y, tags = _in_fresh_context({'DAT_CONV_NTAP': '0'}, L.run)
    assert tags[0] in (_generic_tag(ops, case, '16', 128), _generic_tag(ops, case, '16', 256)) and len(tags) == 1, tags
    L.check(y, 'table-driven loop')


@_cases(('strips',))
def test_linear_strips_windows(ops, case):
    """64 -> 64 on 12 x 21 maps: one linear strip of positions per frame, bit for bit the 2-D tiling, both inside the bound.
    (The dispatcher tag is the same for both tilings, so it cannot show which ran: at this shape a frame is 4 two-dimensional tiles of
    128 positions against 2 linear ones, which passes the dispatcher's `linear tiles * 10 <= 2-D tiles * 9` rule.)"""
    L = _Launcher(ops, case, '16')
    y_lin, tags = _in_fresh_context({'DAT_CONV_LINEAR': '1'}, L.run)
    y_2d, tags2 = _in_fresh_context({'DAT_CONV_LINEAR': '0'}, L.run)
    assert tags == tags2 and len(tags) == 1 and tags[0] in (_generic_tag(ops, case, '16', 128), _generic_tag(ops, case, '16', 256)), (tags, tags2)
    assert torch.equal(y_lin, y_2d)
    L.check(y_lin, 'linear strips')
    L.check(y_2d, '2-D tiles')


@_cases(('stride2',))
def test_stride2_dense_patch_windows(ops, case):
    L = _Launcher(ops, case, '16')
    for plan in (None, (128, 2)):
        y, tags = L.run(plan)
        assert tags == [_generic_tag(ops, case, '16', 128)], (plan, tags)      # (the dense-patch variant has 128-position tiles only)
        L.check(y, 'plan %r' % (plan,))


@_cases(('k311',))
def test_temporal_k311_windows(ops, case):
    """(3, 1, 1) layers with a window stay on the generic kernel's one-tap variant -- also where the temporal K-streaming kernel takes
    every unwindowed layer (DAT_CONV_TEMPORAL=2, bf16 build)."""
    L = _Launcher(ops, case, '16')

    def run():
        out = L.run()
        prof = ops.ConvProfiler(capacity=8)         # the control: the same layer without a window
        prof.start()
        L.layer(L.x, T=L.r['T'], residual=None, res_mode=0)
        return out, [t for t, _, _ in prof.stop()]
    (y, tags), control = _in_fresh_context({'DAT_CONV_TEMPORAL': '2'}, run)
    assert tags == [_generic_tag(ops, case, '16', 128)], 'a windowed kT x 1 x 1 layer left the generic kernel: tags %r' % (tags,)
    assert control == ([2560351] if ops.L.H16 != 'fp16' else [_generic_tag(ops, case, '16', 128)]), control
    L.check(y, 'one-tap variant')
    # (no split-K run: the planner keeps one-tap layers with fewer than 16 channel chunks at one split, a forced split is ignored)


@_cases(('time_to_channels_3', 'time_to_channels_2'))
def test_time_moved_to_channels(ops, case):
    """KT == T, pad_t = 0, out_t = (0, 1): every tap valid at the single output frame."""
    L = _Launcher(ops, case, '16')
    y, tags = L.run()
    assert tags == [_generic_tag(ops, case, '16', 128)], tags
    L.check(y, 'planner')


@_cases(('short_t1', 'short_t2'))
def test_short_clips(ops, case):
    """T = 1 and T = 2 under 3x3x3: the launcher allows (KT - 1) * chunks = 2 splits, a frame of T = 1 has ONE patch -- split 0 gets
    the empty range [0, 0) and writes zero partial sums."""
    L = _Launcher(ops, case, '16')
    for plan in ((128, 2), (128, 3), None):
        y, tags = L.run(plan)
        assert len(tags) == 1 and tags[0] in (_generic_tag(ops, case, '16', 128), _generic_tag(ops, case, '16', 256)), (plan, tags)
        assert plan is None or tags == [_generic_tag(ops, case, '16', 128)]
        L.check(y, 'plan %r' % (plan,))


FP32_IDS = ['dense-out1+2-inall-affine_res_relu', 'dense-out2+2-in1+1-affine_res_relu', 'stride2-out2+1-inall-affine_res_relu',
            'stride2-outall-in1+1-affine_res_relu', 'k311-out1+2-inall-affine_res_relu', 'k311-outall-in3+1-affine_res_relu']


@pytest.mark.parametrize('cid', FP32_IDS)
def test_fp32_windows(ops, cid):
    """fp32 tensors (32-channel chunks: twice the patches per tap), the planner's plan and split-K (the one-tap k311 rows do not
    split: the planner's plan only)."""
    case = tr.CASES_BY_ID[cid]
    L = _Launcher(ops, case, 'fp32')
    for plan in ((None,) if case['row'] == 'k311' else (None, (128, 2))):
        y, tags = L.run(plan)
        assert len(tags) == 1 and tags[0] in (_generic_tag(ops, case, 'fp32', 128), _generic_tag(ops, case, 'fp32', 256)), (plan, tags)
        L.check(y, 'plan %r' % (plan,))


def test_bf16x3_windows(ops):
    """The split-operand mode (fp32 tensors, x_hi w_hi + x_hi w_lo + x_lo w_hi on bf16 halves) under the fp32 per-element bound and
    its max-abs limit of 5e-4."""
    _bf16_only(ops)
    case = tr.CASES_BY_ID['dense-out1+2-inall-affine_res_relu']
    L = _Launcher(ops, case, 'bf16x3')
    for plan in (None, (128, 2)):
        y, tags = L.run(plan)
        assert len(tags) == 1 and tags[0] in (_generic_tag(ops, case, 'bf16x3', 128), _generic_tag(ops, case, 'bf16x3', 256)), (plan, tags)
        L.check(y, 'plan %r' % (plan,))


# ---- big-tile kernel ----------------------------------------------------------------------------------------------------------------------
@_cases(('big_tile',))
def test_big_tile_windows(ops, case):
    """conv3x3_bt_kernel (DAT_CONV_BT=2 takes it for grids of >= 1.5 blocks per CU): bit for bit the generic kernel under the forced
    (256, 1) plan, and inside the bound.  in_t = (1, 1) leaves frame 3 without a valid tap: the kernel's main loop is skipped."""
    L = _Launcher(ops, case, '16')
    (y, tags), (y_gen, tags_gen) = _in_fresh_context({'DAT_CONV_BT': '2'}, lambda: (L.run(), L.run((256, 1))))
    assert tags == [BT_TAG + 1], 'not the big-tile kernel: tags %r' % (tags,)
    assert tags_gen == [_generic_tag(ops, case, '16', 256)], tags_gen
    assert torch.equal(y, y_gen)
    L.check(y, 'big-tile')


# ---- grouped kernel -----------------------------------------------------------------------------------------------------------------------
@_cases(('grouped', 'grouped_s2'))
def test_grouped_windows(ops, case):
    """conv3d_grouped_kernel, 4 groups of 32 channels; like the project's other grouped-kernel tests these run in the bf16 build."""
    _bf16_only(ops)
    L = _Launcher(ops, case, '16')
    y, tags = L.run()
    assert tags == [GROUPED_TAG + 1], 'not the grouped kernel: tags %r' % (tags,)
    L.check(y, 'grouped')
