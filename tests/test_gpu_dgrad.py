"""The dense data gradient hip_ops.ConvGrad.data -- the data-gradient weight packer, dat_zero_insert2x and the forward conv dispatcher
in its data-gradient role (padding k - 1 - p, residual modes 1 sum / 3 mask / 4 sum + mask) -- against the float64 transpose of the
forward conv (tests/dgrad_refs.dgrad_ref64), every element (large maps: every sampled element) under the per-element bound of
tests/numerics.py, on every kernel the dispatcher picks for such a layer.  Each row asserts the dispatcher tag, so no special kernel
is silently replaced by the generic one; every mode (plain, accumulate_into, mask, mask + accumulate_into) is held against float64,
not against another launch.  tests/test_dgrad_refs_cpu.py shows that every seeded defect of the pipeline leaves this bound.

The bound: K = cout * taps products accumulated in fp32, one rounding to the stored format, and `extra` = the unit roundoff of the
weight format times the sum of absolute products -- the packer's single rounding of w * scale (g, base and mask are rounded to the
16-bit format beforehand; w and scale stay fp32 masters, as in training)."""
import contextlib

import numpy as np
import pytest
import torch

from tests import dgrad_refs as dr
from tests import numerics as nm

pytestmark = pytest.mark.gpu

SPECIAL = {'ws64': 649990, 'pw256': 2560320, 'pwlw': 2560330, 'pwks': 2560340, 'tks': 2560350, 'bt': 2562560}
RATIOS = {}       # dispatcher tag -> worst err / bound seen in this process (printed per check)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


@contextlib.contextmanager
def _env(ops, monkeypatch, env):
    """A context made under the given library switches, and a fresh one afterwards."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ops.drop_ctx()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        for k in env:
            monkeypatch.delenv(k)
        ops.drop_ctx()


def _fmt(ops, mode):
    return 'fp32' if mode == 'fp32' else ('fp16' if ops.L.H16 == 'fp16' else 'bf16')


def _tags(ops, kind, case, dt):
    """the dispatcher tags a row may show: a special kernel's one tag, or the generic kernel's (64- or 128-wide by the data
    gradient's output channels = the forward cin; 128 or 256 positions a block by the planner)"""
    if kind != 'generic':
        return {SPECIAL[kind] + dt}
    wide = 64 if dr.round_up(case['cin'], 4) <= 64 else 128
    return {wide * 10000 + bp * 10 + dt for bp in (128, 256)}


def _ndhwc(a5, cs, tdt):
    """numpy (N, C, T, H, W) -> CUDA [N * T, H, W, cs], channels [C, cs) zero"""
    t = torch.from_numpy(a5)
    n, c, tt, h, w = t.shape
    out = torch.zeros((n * tt, h, w, cs), dtype=torch.float32)
    out[..., :c] = t.permute(0, 2, 3, 4, 1).reshape(n * tt, h, w, c)
    return out.to(tdt).cuda()


class _Row(object):
    """The ConvGrad and the device operands of a case, made on the CURRENT context; run(mode) -> (dx, tags); check(...) holds every
    (sampled) element to the bound.  Small cases: the operands of dr.case_operands and the full reference; large cases: operands drawn
    on the device (torch is plumbing), rounded to the format, and the reference at dr.sample_positions only."""

    def __init__(self, ops, case, mode, sampled=False):
        self.ops, self.case, self.fmt, self.sampled = ops, case, _fmt(ops, mode), sampled
        self.dt = ops.F32 if mode == 'fp32' else ops.BF16
        tdt = ops.tdtype(self.dt)
        c = case
        self.cs_x, self.cs_g = ops.round_up(c['cin'], 64), ops.round_up(c['cout'], 64)
        Ho, Wo = dr.out_hw(c['H'], c['W'], c['k'], c['stride'], c['pads'])
        frames = c['N'] * c['T']
        if not sampled:
            o = dr.case_operands(case, self.fmt)
            self.w, self.scale = o['w'], o['scale']
            self.g = _ndhwc(o['g'], self.cs_g, tdt)
            self.base, self.mask = _ndhwc(o['base'], self.cs_x, tdt), _ndhwc(o['mask'], self.cs_x, tdt)
            self.host = o
        else:
            rs = np.random.RandomState(sum(map(ord, c['name'])))
            k = c['k']
            self.w = (rs.randn(c['cout'], c['cin'], *k) * np.sqrt(2.0 / (c['cin'] * k[0] * k[1] * k[2]))).astype(np.float32)
            self.scale = rs.uniform(0.5, 1.5, c['cout']).astype(np.float32)
            gen = torch.Generator(device='cuda').manual_seed(c['cin'] * 7 + c['cout'])
            draw = lambda shape: torch.randn(shape, device='cuda', generator=gen)
            self.g = draw((frames, Ho, Wo, self.cs_g)).to(tdt)
            self.base = draw((frames, c['H'], c['W'], self.cs_x)).to(tdt)
            self.mask = torch.relu(draw((frames, c['H'], c['W'], self.cs_x))).to(tdt)
            assert self.cs_g == c['cout'] and self.cs_x == c['cin']
            self.pos = dr.sample_positions(c['N'], c['T'], c['H'], c['W'], seed=c['cin'])
            held = dr.sample_holds_the_required(self.pos, c['N'], c['T'], c['H'], c['W'])
            assert all(held.values()) and len(self.pos) >= 2048, held
            self.fidx = torch.from_numpy(self.pos[:, 0] * c['T'] + self.pos[:, 1]).cuda()
            self.hidx, self.widx = torch.from_numpy(self.pos[:, 2]).cuda(), torch.from_numpy(self.pos[:, 3]).cuda()
            g5 = self.g.float().cpu().view(c['N'], c['T'], Ho, Wo, self.cs_g).permute(0, 4, 1, 2, 3)
            self.host = dict(g=g5, base=self._at(self.base), mask=self._at(self.mask))
        self.cg = ops.ConvGrad(torch.from_numpy(self.w).cuda(), torch.from_numpy(self.scale).cuda(), c['stride'], c['pads'], self.dt,
                               self.cs_x, self.cs_g)
        self._refs = {}

    def _at(self, t):
        """[frames, H, W, cs] on the device -> numpy fp32 (P, cs) at the sampled positions"""
        return t[self.fidx, self.hidx, self.widx].float().cpu().numpy()

    def ref(self, mode):
        if mode not in self._refs:
            c = self.case
            base, mask = dr.mode_operands(self.host, mode)
            if self.sampled and base is not None:
                base = base[:, :c['cin']]
            if self.sampled and mask is not None:
                mask = mask[:, :c['cin']]
            self._refs[mode] = dr.dgrad_ref64(self.host['g'], self.w, self.scale, c['stride'], c['pads'], dr.x_shape(c), base, mask,
                                              g_frames=c.get('g_frames'), positions=self.pos if self.sampled else None)
        return self._refs[mode]

    def run(self, mode, inplace=True):
        c, ops = self.case, self.ops
        acc = self.base.clone() if 'accumulate' in mode else None
        prof = ops.ConvProfiler(capacity=8)
        prof.start()
        dx = self.cg.data(self.g, c['T'], c['H'], c['W'], accumulate_into=acc, g_frames=c.get('g_frames'),
                          mask=self.mask if 'mask' in mode else None, inplace=inplace)
        tags = [t for t, _, _ in prof.stop()]
        if acc is not None:
            assert (dx.data_ptr() == acc.data_ptr()) == inplace
            if not inplace:
                assert torch.equal(acc, self.base), 'inplace=False modified the addend'
        return dx, tags

    def check(self, dx, mode, what, tags):
        c = self.case
        assert tuple(dx.shape) == (c['N'] * c['T'], c['H'], c['W'], self.cs_x) and dx.dtype == self.ops.tdtype(self.dt)
        if self.cs_x > c['cin']:
            assert float(dx[..., c['cin']:].float().abs().max()) == 0.0, '%s: padding channels [%d, %d) not zero' % (what, c['cin'], self.cs_x)
        if self.sampled:
            got = self._at(dx)[:, :c['cin']]
        else:
            got = dx.float().cpu().view(c['N'], c['T'], c['H'], c['W'], self.cs_x)[..., :c['cin']].permute(0, 4, 1, 2, 3).numpy()
        ref, absref = self.ref(mode)
        K = nm.conv_k(c['cout'], c['k'])
        extra = nm.unit_roundoff(self.fmt) * absref
        ratio = float((np.abs(got - ref) / nm.bound(ref, absref, K, self.fmt, extra)).max())
        for t in tags:
            RATIOS[t] = max(RATIOS.get(t, 0.0), ratio)
        print('dgrad %s %s %s tag %r: %d elements, worst err / bound %.3f' % (c['name'], self.fmt, what, tags, ref.size, ratio))
        nm.assert_elementwise(got, ref, absref, K, self.fmt, 'dgrad %s %s %s' % (c['name'], self.fmt, what), extra=extra)

    def all_modes(self, kinds, inplace_false=True):
        """kinds: mode -> the kernel the dispatcher must pick.  Every mode against float64; the accumulating modes also into a new
        tensor (inplace=False), which must leave the addend untouched."""
        for mode in dr.MODES:
            if mode not in kinds:
                continue
            want = _tags(self.ops, kinds[mode], self.case, self.dt)
            dx, tags = self.run(mode)
            assert len(tags) == 1 and tags[0] in want, '%s %s: dispatcher tags %r, expected one of %r' % (self.case['name'], mode, tags, sorted(want))
            self.check(dx, mode, mode, tags)
            if 'accumulate' in mode and inplace_false:
                dx, tags = self.run(mode, inplace=False)
                assert len(tags) == 1 and tags[0] in want, (mode, tags)
                self.check(dx, mode, mode + ' into a new tensor', tags)


ALL_GENERIC = {m: 'generic' for m in dr.MODES}
_small = lambda names: pytest.mark.parametrize('name', names)


# ---- generic kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['16', 'fp32'])
@_small(['k333_same', 'k333_pad_t0', 'k311'])
def test_generic_64_wide_table_driven(ops, name, mode):
    """40 <- 24 (3 x 3 x 3, "same" padding and pad_t = 0: the data-gradient padding is 2 on the T axis and 1 on H and W) and 48 <- 32
    (3 x 1 x 1) on two clips of four 9 x 11 frames: the 64-wide generic kernel's table-driven loop."""
    _Row(ops, dr.SMALL_BY_NAME[name], mode).all_modes(ALL_GENERIC)


@pytest.mark.parametrize('mode', ['16', 'fp32'])
def test_generic_nine_tap_split_k(ops, mode):
    """128 <- 64, 1 x 3 x 3 on 4 x 14 x 18: the unrolled nine-tap variant (the planner splits K on this small map)."""
    _Row(ops, dr.SMALL_BY_NAME['k133'], mode).all_modes(ALL_GENERIC)


def test_generic_nine_tap_on_an_roi_head_map_linear_and_2d_tiling(ops, monkeypatch):
    """64 maps of 7 x 7: linear position tiling by default, 2-D tiles under DAT_CONV_LINEAR=0 -- both inside the same bound."""
    case = dr.SMALL_BY_NAME['k133_roi']
    _Row(ops, case, '16').all_modes(ALL_GENERIC)
    with _env(ops, monkeypatch, {'DAT_CONV_LINEAR': '0'}):
        _Row(ops, case, '16').all_modes(ALL_GENERIC, inplace_false=False)


@_small(['k333_s2_13x16', 'k333_s2_12x15', 'k333_s2_12x16'])
def test_zero_insertion_3x3x3_stride2(ops, name):
    """128 <- 64, 3 x 3 x 3, stride 2: dat_zero_insert2x to odd and even extents (13 x 16: 7 x 8 gradients, the last row filled;
    12 x 15 and 12 x 16: a trailing zero row / column), then the generic kernel."""
    _Row(ops, dr.SMALL_BY_NAME[name], '16').all_modes(ALL_GENERIC)
    if name == 'k333_s2_13x16':
        _Row(ops, dr.SMALL_BY_NAME[name], 'fp32').all_modes(ALL_GENERIC, inplace_false=False)


@_small(['k111_s2_13x16', 'k111_s2_12x16'])
def test_zero_insertion_1x1x1_stride2(ops, name):
    """256 <- 128, 1 x 1 x 1, stride 2, no padding: zero insertion + the one-tap variant."""
    _Row(ops, dr.SMALL_BY_NAME[name], '16').all_modes(ALL_GENERIC)


@pytest.mark.parametrize('mode', ['16', 'fp32'])
def test_one_tap_unrolled_padded_channels(ops, mode):
    """256 <- 200, 1 x 1 x 1: 200 output channels of the data gradient in a stride of 256, channels 200..255 exactly zero."""
    _Row(ops, dr.SMALL_BY_NAME['k111_200'], mode).all_modes(ALL_GENERIC)


def test_frame_window_of_the_gradient(ops):
    """g_frames on a single clip, the window not at the clip start: the generic kernel with in_t skips the zero frames' taps."""
    case = dr.SMALL_BY_NAME['k333_window']
    assert case['N'] == 1 and case['g_frames'][0] > 0
    _Row(ops, case, '16').all_modes(ALL_GENERIC)


# ---- special kernels -----------------------------------------------------------------------------------------------------------------------
def test_weights_stationary_3x3_c64(ops):
    """64 <- 64, 1 x 3 x 3 on 2 x 20 x 33: the persistent weights-stationary kernel (plain, accumulate); the masking modes: generic."""
    _Row(ops, dr.SMALL_BY_NAME['ws64'], '16').all_modes({'plain': 'ws64', 'accumulate': 'ws64', 'mask': 'generic', 'mask_accumulate': 'generic'})


def test_weights_stationary_1x1_k64_c256(ops):
    """64 <- 256, 1 x 1 x 1 on 5 x 7 = 35 positions: one full wave tile of 32 and a ragged one."""
    _Row(ops, dr.SMALL_BY_NAME['pw256'], '16').all_modes({'plain': 'pw256', 'accumulate': 'pw256', 'mask': 'generic', 'mask_accumulate': 'generic'})


def test_weights_in_lds_1x1(ops):
    """128 <- 512 on 4 x 127 x 130 = 66 040 positions (pwlw_eligible wants >= 2 * 4 * 256 wave tiles of 32; the last tile is ragged):
    the weights-in-LDS kernel for sum + mask, sum and plain; plain `mask` keeps the generic kernel.  Sampled reference."""
    _Row(ops, dr.LARGE_BY_NAME['pwlw'], '16', sampled=True).all_modes({'plain': 'pwlw', 'accumulate': 'pwlw', 'mask': 'generic', 'mask_accumulate': 'pwlw'})


def test_k_streaming_1x1(ops):
    """512 <- 2048 on 2 x 48 x 64: 24 position blocks x 8 column blocks = 192 blocks, the smallest grid pwks_eligible takes on 256
    CUs; all four modes on the K-streaming kernel.  Sampled reference."""
    _Row(ops, dr.LARGE_BY_NAME['pwks'], '16', sampled=True).all_modes({m: 'pwks' for m in dr.MODES})


def test_temporal_tap_kernel(ops, monkeypatch):
    """256 <- 256, 3 x 1 x 1 on 4 x 7 x 10 = 280 positions under DAT_CONV_TEMPORAL=2: plain and accumulate on the temporal-tap
    K-streaming kernel, the masking modes on the generic one.  The temporal taps carry the factors 1/2, 1, 3/2 (dr.case_operands):
    a missing T flip fails (tests/test_dgrad_refs_cpu.py)."""
    if ops.L.H16 == 'fp16':
        pytest.skip('bf16 build only')
    with _env(ops, monkeypatch, {'DAT_CONV_TEMPORAL': '2'}):
        _Row(ops, dr.SMALL_BY_NAME['tks'], '16').all_modes({'plain': 'tks', 'accumulate': 'tks', 'mask': 'generic', 'mask_accumulate': 'generic'})


def test_big_tile_kernel(ops, monkeypatch):
    """256 <- 256, 1 x 3 x 3 on two clips of 4 x 96 x 128 (48 tiles x 8 frames = 384 blocks = 1.5 per CU, the grid DAT_CONV_BT=2
    asks for): plain and accumulate on the big-tile kernel.  Sampled reference."""
    with _env(ops, monkeypatch, {'DAT_CONV_BT': '2'}):
        _Row(ops, dr.LARGE_BY_NAME['big_tile'], '16', sampled=True).all_modes({'plain': 'bt', 'accumulate': 'bt'})
