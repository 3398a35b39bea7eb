"""Edges of the 16-bit formats that the random-operand kernel tests never reach, in whichever build is loaded (bf16 by default,
IEEE half under DAT_H16=fp16, tests/test_gpu_fp16_suite.py): fp32 sums beyond the half range that an affine scale brings back,
outputs that saturate, subnormal operands and outputs, and the exactness of the fp32 -> 16-bit layout conversion.  Each conv edge
runs through the planner's kernel choice, a forced split-K plan, and on shapes that select the weights-stationary 3x3 (ws64), the
big-tile 3x3, the weights-in-LDS 1x1 (lw) and the K-streaming 1x1 (ks) kernels; every expectation is stated per format."""
import numpy as np
import pytest
import torch

from tests import numerics as nm
from tests.test_gpu_kernels import _dev, _in_fresh_context

pytestmark = pytest.mark.gpu

# name: (kernel taps, Cin, Cout, frames, H, W, environment, forced plan, the kernel's profiler tag or None)
SELECT = {
    'plan_3x3x3': ((3, 3, 3), 64, 128, 3, 14, 18, {}, None, None),
    'splitk_3x3x3': ((3, 3, 3), 64, 128, 3, 14, 18, {}, (128, 2), None),
    'splitk_1x1': ((1, 1, 1), 64, 128, 2, 12, 20, {}, (128, 2), None),
    'ws64_3x3': ((1, 3, 3), 64, 64, 2, 37, 53, {}, None, None),                      # tests/test_gpu_kernels.py WS64_CASES
    'big_tile_3x3': ((1, 3, 3), 64, 256, 4, 120, 256, {'DAT_CONV_BT': '2'}, None, None),  # BT_CASES '2d_8x32_tiles'
    'lw_1x1': ((1, 1, 1), 64, 64, 2, 192, 200, {}, None, 2560331),                     # LW_CASES 'k64_c64'
    'ks_1x1': ((1, 1, 1), 1024, 256, 2, 192, 200, {}, None, 2560341),                  # KS_CASES 'k1024_c256'
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
    k, cin, cout, T, H, W, env, plan, tag = SELECT[sel]
    pads = (k[0] // 2, k[1] // 2, k[2] // 2)
    layer = ops.ConvLayer(_dev(w), _dev(scale), _dev(bias), stride=(1, 1), pads=pads, relu=False, dtype=ops.BF16)
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
            assert [t for t, _, _ in rec] == [tag], 'the layer did not take the %s kernel: tags %r' % (sel, [t for t, _, _ in rec])
        return y_
    y = _in_fresh_context(env, run) if env else run()
    assert y.dtype == nm.h16()
    got = y[..., :cout].reshape(1, T, H, W, cout).permute(0, 4, 1, 2, 3).cpu()
    ref64, abs64 = nm.conv_ref64(nm.q16(x), nm.q16(w), scale, bias, None, (1, 1), pads)
    return got, ref64, abs64


def _shape(sel):
    k, cin, cout, T, H, W = SELECT[sel][:6]
    return k, cin, cout, (1, cin, T, H, W), (cout, cin) + k


@pytest.mark.parametrize('sel', IDS)
def test_sums_beyond_the_half_range_brought_back_by_the_affine_scale(ops, sel):
    """Non-negative activations and mostly positive weights: the fp32 sums reach ~4 x 65504, the affine scale 1/16 brings the outputs
    back into the half range.  Finite outputs within the per-element bound: no 16-bit partial sum, split-K partial or staging copy."""
    k, cin, cout, xs, ws = _shape(sel)
    K = nm.conv_k(cin, k)
    rs = np.random.RandomState(K + cout)
    a = np.sqrt(262144.0 / K)
    x = (rs.uniform(0.5, 1.5, xs) * a).astype(np.float32)
    w = (rs.uniform(0.5, 1.5, ws) * a * np.where(rs.uniform(size=ws) < 0.1, -1.0, 1.0)).astype(np.float32)
    scale = np.full(cout, 1.0 / 16, np.float32)
    bias = (rs.randn(cout) * 4).astype(np.float32)
    got, ref64, abs64 = _conv(ops, sel, x, w, scale, bias)
    assert (np.abs(ref64 - bias.reshape(1, -1, 1, 1, 1)) * 16).max() > 2 * 65504, 'the sums do not leave the half range'
    assert np.abs(ref64).max() < 65504 / 2
    assert torch.isfinite(got).all()
    nm.assert_elementwise(got, ref64, abs64, K, nm.h16(), 'large sums ' + sel)


@pytest.mark.parametrize('sel', IDS)
def test_outputs_beyond_the_range_saturate_with_round_to_nearest_even(ops, sel):
    """Every product is 64 * 64 and every sum an exact fp32 integer, so the kernel's fp32 value is sum * scale rounded once; per
    output channel the scale puts the interior outputs at 65504, 65519, 65520, -65520, 65535, 2^17 ...  The stored output equals torch's
    conversion of that fp32 value: fp16 rounds to nearest even (65519 -> 65504, >= 65520 -> +-inf); bf16 keeps them finite."""
    k, cin, cout, xs, ws = _shape(sel)
    x = np.full(xs, 64.0, np.float32)
    w = np.full(ws, 64.0, np.float32)
    interior = float(nm.conv_k(cin, k) * 64 * 64)                 # the sum of an interior output (all taps inside the map)
    targets = np.array([65504, 65519, 65520, -65520, 65535, -65519, 131072, 60000, -70000, 1.0e6, 32768, 65520.5], np.float64)
    scale = (targets[np.arange(cout) % len(targets)] / interior).astype(np.float32)
    bias = np.zeros(cout, np.float32)
    got, ref64, _ = _conv(ops, sel, x, w, scale, bias)
    # the kernel's fp32 result: the exact sum times the fp32 scale, one fp32 rounding (bias 0 adds nothing)
    sums = ref64 / scale.astype(np.float64).reshape(1, -1, 1, 1, 1)
    want32 = (torch.from_numpy(np.rint(sums).astype(np.float32)) * torch.from_numpy(scale).view(1, -1, 1, 1, 1))
    want = want32.to(nm.h16())
    inner = (slice(None), slice(None), slice(1, -1) if k[0] == 3 else slice(None), slice(1, -1), slice(1, -1))
    if nm.h16() == torch.float16:
        assert torch.isinf(got[inner]).any() and (got[inner] == 65504).any(), 'no saturated / clamped interior outputs'
    else:
        assert torch.isfinite(got).all()
    bad = got.float() != want.float()
    assert not bad.any(), '%s: %d outputs differ from torch\'s rounding, e.g. got %r want %r' % (
        sel, int(bad.sum()), got[bad][:4].tolist(), want[bad][:4].tolist())


@pytest.mark.parametrize('sel', IDS)
def test_subnormal_operands_and_outputs(ops, sel):
    """Activations and weights are small multiples of 2^-24 (fp16 subnormals; normal in bf16) -- converted by the layout kernel and the
    weight pack -- and the scales 2^19 .. 2^21 put the outputs in the half format's subnormal range.  Every product and sum is exact
    in fp32, so the stored output must equal torch's rounding of the exact result: subnormals kept, ties to even, no flush to zero."""
    k, cin, cout, xs, ws = _shape(sel)
    rs = np.random.RandomState(nm.conv_k(cin, k) + 3)
    x = (rs.randint(-15, 16, xs) * 2.0 ** -24).astype(np.float32)
    w = (rs.randint(-15, 16, ws) * 2.0 ** -24).astype(np.float32)
    scale = (2.0 ** rs.randint(19, 22, cout)).astype(np.float32)
    bias = np.zeros(cout, np.float32)
    np.testing.assert_array_equal(nm.q16(x), x)                  # (representable in both formats: the pack and the layout are exact)
    got, ref64, abs64 = _conv(ops, sel, x, w, scale, bias)
    want = torch.from_numpy(ref64).to(nm.h16())                  # exact in fp32, so one rounding of the exact value
    if nm.h16() == torch.float16:
        sub = (want != 0) & (want.abs() < 2.0 ** -14)
        assert sub.float().mean() > 0.3, 'too few subnormal outputs: %.3f' % sub.float().mean()
        assert (got[sub] != 0).all(), 'subnormal outputs flushed to zero'
    bad = got.float() != want.float()
    assert not bad.any(), '%s: %d of %d outputs differ from torch\'s rounding, e.g. got %r want %r' % (
        sel, int(bad.sum()), bad.numel(), got[bad][:4].tolist(), want[bad][:4].tolist())
    nm.assert_elementwise(got, ref64, abs64, nm.conv_k(cin, k), nm.h16(), 'subnormals ' + sel)


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
