"""The per-element bound of tests/numerics.py, checked on the CPU against mutants of a correctly computed conv: it must accept a
float32 conv of quantised operands that is then correctly rounded to the output format, and reject a truncating output conversion,
a result rounded through bf16 when the output is fp16, and one product missing from one output pixel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import numerics as nm

# (the conv cases of tests/test_gpu_kernels.py the mutants were first worked out on: 3x3x3 with residual + ReLU, and the c256 one)
CASES = [('3x3x3', 1, 4, 14, 18, 64, 128, (3, 3, 3), True, True),
         ('3x3x3_c256', 1, 3, 9, 21, 128, 256, (3, 3, 3), False, False)]


def _case(case, fmt):
    name, N, T, H, W, cin, cout, k, relu, with_res = case
    rs = np.random.RandomState(len(name))
    x = nm.q16(rs.randn(N, cin, T, H, W).astype(np.float32), fmt)
    w = nm.q16((rs.randn(cout, cin, *k) * np.sqrt(2.0 / (cin * np.prod(k)))).astype(np.float32), fmt)
    scale = rs.uniform(0.5, 1.5, cout).astype(np.float32)
    bias = (rs.randn(cout) * 0.1).astype(np.float32)
    res = nm.q16(rs.randn(N, cout, T, H, W).astype(np.float32), fmt) if with_res else None
    pads = tuple(v // 2 for v in k)
    ref, absref = nm.conv_ref64(x, w, scale, bias, res, (1, 1), pads, relu)
    # what a correct kernel computes: fp32 accumulation and epilogue, one rounding to the output format at the end
    y = F.conv3d(torch.from_numpy(x), torch.from_numpy(w), None, padding=pads) * torch.from_numpy(scale).view(1, -1, 1, 1, 1) + \
        torch.from_numpy(bias).view(1, -1, 1, 1, 1)
    if res is not None:
        y = y + torch.from_numpy(res)
    if relu:
        y = torch.relu(y)
    return dict(x=x, w=w, scale=scale, pads=pads, ref=ref, absref=absref, y32=y, K=nm.conv_k(cin, k))


def _truncate_bf16(y32):
    b = y32.contiguous().view(torch.int32) & ~0xFFFF
    return b.view(torch.float32)


@pytest.fixture(scope='module', params=CASES, ids=[c[0] for c in CASES])
def case(request):
    return request.param


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
def test_bound_accepts_a_correctly_rounded_fp32_conv(case, fmt):
    c = _case(case, fmt)
    got = c['y32'].to(nm._NAMES[fmt]).float()
    nm.assert_elementwise(got, c['ref'], c['absref'], c['K'], fmt, 'correct %s' % fmt)
    # the fp32 result itself (before the output rounding) is held to the fp32 output bound as well
    nm.assert_elementwise(c['y32'], c['ref'], c['absref'], c['K'], 'fp32', 'fp32 accumulate')


def test_bound_rejects_a_truncating_bf16_output_conversion(case):
    c = _case(case, 'bf16')
    got = _truncate_bf16(c['y32'])
    # the old max-abs tolerance of the kernel tests lets it through ...
    assert np.abs(got.numpy() - c['ref']).max() < 3e-2 * max(1.0, np.abs(c['ref']).max() / 4)
    with pytest.raises(AssertionError, match='outside the per-element bound'):
        nm.assert_elementwise(got, c['ref'], c['absref'], c['K'], 'bf16', 'truncated bf16')


def test_bound_rejects_an_fp16_result_rounded_through_bf16(case):
    c = _case(case, 'fp16')
    got = c['y32'].to(torch.bfloat16).to(torch.float16).float()
    assert np.abs(got.numpy() - c['ref']).max() < 3e-2 * max(1.0, np.abs(c['ref']).max() / 4)
    with pytest.raises(AssertionError, match='outside the per-element bound'):
        nm.assert_elementwise(got, c['ref'], c['absref'], c['K'], 'fp16', 'fp16 through bf16')


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
def test_bound_rejects_one_dropped_product_in_one_pixel(case, fmt):
    c = _case(case, fmt)
    x, w, pads = c['x'], c['w'], c['pads']
    # an interior output pixel that the ReLU keeps (n=0, co=5, t=1) loses its largest single product x * w * scale
    co, t = 5, 1
    inner = c['ref'][0, co, t, 2:-2, 2:-2]
    h, ww = [int(v) + 2 for v in np.unravel_index(int(np.argmax(inner)), inner.shape)]
    kt, kh, kw = w.shape[2:]
    best, arg = 0.0, None
    for a in range(kt):
        for b in range(kh):
            for d in range(kw):
                xs = x[0, :, t + a - pads[0], h + b - pads[1], ww + d - pads[2]]
                p = xs * w[co, :, a, b, d]
                j = int(np.argmax(np.abs(p)))
                if abs(p[j]) > best:
                    best, arg = abs(p[j]), float(p[j])
    y = c['y32'].clone()
    y[0, co, t, h, ww] -= arg * float(c['scale'][co])
    if case[8]:
        y = torch.relu(y)
    got = y.to(nm._NAMES[fmt]).float()
    with pytest.raises(AssertionError, match=r'1 of \d+ elements .* worst at \(0, 5, 1, %d, %d\)' % (h, ww)):
        nm.assert_elementwise(got, c['ref'], c['absref'], c['K'], fmt, 'dropped product')


def test_bound_helpers():
    assert nm.unit_roundoff('bf16') == 2.0 ** -8 and nm.unit_roundoff(torch.float16) == 2.0 ** -11
    assert nm.unit_roundoff('fp32') == 2.0 ** -24
    a = np.array([1.0 + 2.0 ** -9, 65519.0, 65520.0, 2.0 ** -25 * 3], np.float32)
    np.testing.assert_array_equal(nm.q16(a, 'fp16'), torch.from_numpy(a).half().float().numpy())
    assert nm.q16(a, 'fp16')[2] == np.inf and nm.q16(a, 'bf16')[2] == 65536.0
    # NaN in a result never passes
    with pytest.raises(AssertionError):
        nm.assert_elementwise(np.array([np.nan]), np.array([1.0]), np.array([1.0]), 1, 'fp32', 'nan')
