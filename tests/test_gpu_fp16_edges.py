"""Edges of the 16-bit formats that the random-operand kernel tests never reach, in whichever build is loaded (bf16 by default,
IEEE half under DAT_H16=fp16, tests/test_gpu_fp16_suite.py): fp32 sums beyond the half range that an affine scale brings back,
outputs that saturate, subnormal operands and outputs, and the exactness of the fp32 -> 16-bit layout conversion.  Each conv edge
runs through the planner's kernel choice, a forced split-K plan, and on shapes that select the weights-stationary 3x3 (ws64), the
big-tile 3x3, the weights-in-LDS 1x1 (lw) and the K-streaming 1x1 (ks) kernels, the grouped 3x3 kernel (two 64-channel slabs of 16
groups) and the dilated 3x3 path of the generic kernel (dilation 2 on a 5 x 5 map: the smallest with an interior output, and the -2
taps leave it on one side, the +2 taps on the other); every expectation is stated per format.  The operand sets and the checks live
in tests/fp16_edge_cases.py, where tests/test_fp16_edges_cpu.py holds them against simulated defects without a GPU."""
import numpy as np
import pytest
import torch

from tests import fp16_edge_cases as fe
from tests import numerics as nm
from tests.dilated_ref import inflate
from tests.grouped_ref import grouped_conv_ref64
from tests.test_gpu_kernels import _dev, _in_fresh_context

pytestmark = pytest.mark.gpu

# name: (kernel taps, Cin, Cout, frames, H, W, environment, forced plan, the kernel's profiler tag(s) or None, groups, dilation)
SELECT = {
    'plan_3x3x3': ((3, 3, 3), 64, 128, 3, 14, 18, {}, None, None, 1, 1),
    'splitk_3x3x3': ((3, 3, 3), 64, 128, 3, 14, 18, {}, (128, 2), None, 1, 1),
    'splitk_1x1': ((1, 1, 1), 64, 128, 2, 12, 20, {}, (128, 2), None, 1, 1),
    'ws64_3x3': ((1, 3, 3), 64, 64, 2, 37, 53, {}, None, None, 1, 1),                      # tests/test_gpu_kernels.py WS64_CASES
    'big_tile_3x3': ((1, 3, 3), 64, 256, 4, 120, 256, {'DAT_CONV_BT': '2'}, None, None, 1, 1),  # BT_CASES '2d_8x32_tiles'
    'lw_1x1': ((1, 1, 1), 64, 64, 2, 192, 200, {}, None, 2560331, 1, 1),                     # LW_CASES 'k64_c64'
    'ks_1x1': ((1, 1, 1), 1024, 256, 2, 192, 200, {}, None, 2560341, 1, 1),                  # KS_CASES 'k1024_c256'
    # tests/test_gpu_grouped_conv.py CASES 'c128_g32x4_1x3x3', one clip: the grouped kernel's tag on 16-bit tensors, as that file asserts it
    'grouped_3x3': ((1, 3, 3), 128, 128, 1, 19, 23, {}, None, 642571, 32, 1),
    # the generic kernel with the dilated mark (tests/test_gpu_dilated_conv.py): 64 channels per block, 128 or 256 positions
    'dilated_3x3': ((1, 3, 3), 64, 64, 2, 5, 5, {}, None, (641286, 642566), 1, 2),
}
IDS = sorted(SELECT)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _conv(ops, sel, x, w, scale, bias):
    """The conv of SELECT[sel] on fp32 operands (quantised to the build's format by the layout conversion and the weight pack);
    returns the stored 16-bit output as (1, Cout, T, H, W) and the float64 (ref, absref)."""
    k, cin, cout, T, H, W, env, plan, tag, groups, dil = SELECT[sel]
    pads = (k[0] // 2, dil * (k[1] // 2), dil * (k[2] // 2))
    layer = ops.ConvLayer(_dev(w), _dev(scale), _dev(bias), stride=(1, 1), pads=pads, relu=False, dtype=ops.BF16, groups=groups,
                          dilation=dil)
    xd = ops.to_ndhwc(_dev(x), ops.BF16)

    def run():
        prof = ops.ConvProfiler(capacity=8)
        try:
            if plan:
                assert ops.tune_plan(*plan) == 0
            prof.start()
            y_ = layer(xd, T=T)
            rec = prof.stop()
        finally:
            ops.tune_plan(0, 0)
        if tag is not None:
            tags = [t for t, _, _ in rec]
            assert len(tags) == 1 and tags[0] in (tag if isinstance(tag, tuple) else (tag,)), \
                'the layer did not take the %s kernel: tags %r' % (sel, tags)
        return y_
    y = _in_fresh_context(env, run) if env else run()
    assert y.dtype == nm.h16()
    got = y[..., :cout].reshape(1, T, H, W, cout).permute(0, 4, 1, 2, 3).cpu()
    # float64: per-group dense convs (tests/grouped_ref.py; one group: numerics.conv_ref64 itself) of the zero-inflated filter
    # (tests/dilated_ref.py; dilation 1: the filter itself)
    ref64, abs64 = grouped_conv_ref64(nm.q16(x), inflate(nm.q16(w), dil), groups, scale, bias, None, (1, 1), pads)
    return got, ref64, abs64


def _shape(sel):
    """(taps, reduction length K = Cin / groups x taps, Cout, shape of x, shape of w)"""
    k, cin, cout, T, H, W = SELECT[sel][:6]
    groups = SELECT[sel][9]
    return k, nm.conv_k(cin // groups, k), cout, (1, cin, T, H, W), (cout, cin // groups) + k


def _interior(sel):
    """Index of the outputs whose every tap lies inside the clip."""
    k, dil = SELECT[sel][0], SELECT[sel][10]
    hw = slice(dil, -dil) if k[1] == 3 else slice(None)
    return (slice(None), slice(None), slice(1, -1) if k[0] == 3 else slice(None), hw, hw)


@pytest.mark.parametrize('sel', IDS)
def test_sums_beyond_the_half_range_brought_back_by_the_affine_scale(ops, sel):
    """Non-negative activations and mostly positive weights: the fp32 sums reach ~4 x 65504, the affine scale 1/16 brings the outputs
    back into the half range.  Finite outputs within the per-element bound: no 16-bit partial sum, split-K partial or staging copy."""
    k, K, cout, xs, ws = _shape(sel)
    x, w, scale, bias = fe.conv_large_sums_operands(K, cout, xs, ws)
    got, ref64, abs64 = _conv(ops, sel, x, w, scale, bias)
    fe.check_conv_large_sums(got, ref64, abs64, bias, K, nm.h16(), sel)


@pytest.mark.parametrize('sel', IDS)
def test_outputs_beyond_the_range_saturate_with_round_to_nearest_even(ops, sel):
    """Every product is 64 * 64 and every sum an exact fp32 integer, so the kernel's fp32 value is sum * scale rounded once; per
    output channel the scale puts the interior outputs at 65504, 65519, 65520, -65520, 65535, 2^17 ...  The stored output equals torch's
    conversion of that fp32 value: fp16 rounds to nearest even (65519 -> 65504, >= 65520 -> +-inf); bf16 keeps them finite."""
    k, K, cout, xs, ws = _shape(sel)
    x, w, scale, bias = fe.conv_saturation_operands(K, cout, xs, ws)
    got, ref64, _ = _conv(ops, sel, x, w, scale, bias)
    # (the sum of an interior output, all taps inside the map: K * 64 * 64)
    fe.check_conv_saturation(got, ref64, scale, float(K * 64 * 64), _interior(sel), nm.h16(), sel)


@pytest.mark.parametrize('sel', IDS)
def test_subnormal_operands_and_outputs(ops, sel):
    """Activations and weights are small multiples of 2^-24 (fp16 subnormals; normal in bf16) -- converted by the layout kernel and the
    weight pack -- and the scales 2^19 .. 2^21 put the outputs in the half format's subnormal range.  Every product and sum is exact
    in fp32, so the stored output must equal torch's rounding of the exact result: subnormals kept, ties to even, no flush to zero."""
    k, K, cout, xs, ws = _shape(sel)
    x, w, scale, bias = fe.conv_subnormal_operands(K, cout, xs, ws)
    np.testing.assert_array_equal(nm.q16(x), x)                  # (representable in both formats: the pack and the layout are exact)
    got, ref64, abs64 = _conv(ops, sel, x, w, scale, bias)
    fe.check_conv_subnormals(got, ref64, abs64, K, nm.h16(), sel)


def test_layout_conversion_is_torch_rounding_bit_for_bit(ops):
    """dat_ncdhw_to_ndhwc (fp32 -> the build's 16-bit format) equals torch's .to() bit for bit on ties of both formats, subnormals of
    both formats, the largest finite values and beyond, and signed zeros; the way back is the exact widening."""
    v = [0.0, -0.0, 1.0, -1.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -9,
         2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -26, -3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -24,
         (1023.5) * 2.0 ** -24, 2.0 ** -126, 2.0 ** -133, 3 * 2.0 ** -134, 2.0 ** -135, -2.0 ** -149, 65504, 65519, 65519.99,
         65520, -65520, 65536, 1e6, -1e6, 3.3895314e38, 3.4028235e38, -3.4028235e38, float('inf'), float('-inf'), 0.1, -2.5e-8]
    x = torch.tensor(v, dtype=torch.float32)
    n = x.numel()
    src = torch.zeros((1, 64, 1, 1, n), dtype=torch.float32)
    src[0, 3, 0, 0, :] = x
    src[0, 60, 0, 0, :] = -x
    nd = ops.to_ndhwc(src.cuda(), ops.BF16, 64)                 # [1, 1, n, 64]
    assert nd.dtype == nm.h16()
    want = src.permute(0, 2, 3, 4, 1).reshape(1, 1, n, 64).to(nm.h16())
    got_bits, want_bits = nd.cpu().view(torch.int16), want.view(torch.int16)
    bad = (got_bits != want_bits).nonzero().tolist()
    assert not bad, 'differs from torch at %d places, e.g. value %r: got bits %#06x, torch %#06x' % (
        len(bad), float(src[0, bad[0][3], 0, 0, bad[0][2]]), int(got_bits[tuple(bad[0])]) & 0xffff, int(want_bits[tuple(bad[0])]) & 0xffff)
    back = ops.to_ncdhw(nd, ops.BF16, 1, 64, 1).cpu()
    assert torch.equal(back.view(torch.int32), want.float().permute(0, 3, 1, 2).reshape(1, 64, 1, 1, n).view(torch.int32))
