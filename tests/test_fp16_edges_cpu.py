"""The format edges of the later kernel families (tests/fp16_edge_cases.py: the grouped and the dilated conv of
tests/test_gpu_fp16_edges.py, the GroupNorm edges of tests/test_gpu_group_norm.py and tests/test_gpu_gn_roi.py) without a GPU: a plain
fp32 simulation of a correct kernel, stored with correct rounding, passes each edge's check in bf16 and in fp16, and the defect the edge
exists for does not -- subnormal inputs flushed to zero, an output clamped to 65504 instead of overflowing, an fp16 output rounded
through bf16.  (In bf16 the first two defects change nothing: the operands are ordinary normals there and the targets stay finite;
that is asserted too.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fp16_edge_cases as fe
from tests import group_norm_ref as ref
from tests import numerics as nm
from tests.dilated_ref import inflate
from tests.grouped_ref import grouped_conv_ref64
from tests.test_gpu_fp16_edges import SELECT, _interior, _shape
from tests.test_gpu_gn_roi import CASES as ROI_CASES
from tests.test_gpu_group_norm import CASES as CLIP_CASES, EDGE_CASES, EPS

FMTS = ['bf16', 'fp16']
CONVS = ['grouped_3x3', 'dilated_3x3']


# ---- convs -------------------------------------------------------------------------------------------------------------------------------
def _conv_sim(sel, x, w, scale, bias, fmt):
    """-> (y32 torch: fp32 accumulation and epilogue of the operands rounded to fmt, ref64, abs64)"""
    k, cin, cout, T, H, W, env, plan, tag, groups, dil = SELECT[sel]
    pads = (k[0] // 2, dil * (k[1] // 2), dil * (k[2] // 2))
    xq, wq = nm.q16(x, fmt), nm.q16(w, fmt)
    y = F.conv3d(torch.from_numpy(xq), torch.from_numpy(wq), None, padding=pads, dilation=(1, dil, dil), groups=groups)
    y32 = y * torch.from_numpy(scale).view(1, -1, 1, 1, 1) + torch.from_numpy(bias).view(1, -1, 1, 1, 1)
    ref64, abs64 = grouped_conv_ref64(xq, inflate(wq, dil), groups, scale, bias, None, (1, 1), pads)
    return y32, ref64, abs64


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('sel', CONVS)
def test_conv_large_sums_accept_fp32_accumulation_and_reject_a_result_rounded_through_bf16(sel, fmt):
    k, K, cout, xs, ws = _shape(sel)
    x, w, scale, bias = fe.conv_large_sums_operands(K, cout, xs, ws)
    y32, ref64, abs64 = _conv_sim(sel, x, w, scale, bias, fmt)
    fe.check_conv_large_sums(fe.store(y32, fmt), ref64, abs64, bias, K, fmt, sel)
    if fmt == 'fp16':
        with pytest.raises(AssertionError, match='outside the per-element bound'):
            fe.check_conv_large_sums(fe.store_through_bf16(y32), ref64, abs64, bias, K, fmt, sel)
        # (and a sum kept in the 16-bit format overflows before the scale brings it back)
        half_sum = fe.store((y32 - torch.from_numpy(bias).view(1, -1, 1, 1, 1)) * 16, fmt).float() / 16
        with pytest.raises(AssertionError):
            fe.check_conv_large_sums(fe.store(half_sum, fmt), ref64, abs64, bias, K, fmt, sel)


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('sel', CONVS)
def test_conv_saturation_accepts_torch_s_conversion_and_rejects_a_clamp(sel, fmt):
    k, K, cout, xs, ws = _shape(sel)
    x, w, scale, bias = fe.conv_saturation_operands(K, cout, xs, ws)
    y32, ref64, _ = _conv_sim(sel, x, w, scale, bias, fmt)
    args = (ref64, scale, float(K * 64 * 64), _interior(sel), fmt, sel)
    fe.check_conv_saturation(fe.store(y32, fmt), *args)
    if fmt == 'fp16':
        with pytest.raises(AssertionError, match='no saturated / clamped interior outputs'):
            fe.check_conv_saturation(fe.store_clamped(y32, fmt), *args)
        # clamped in one output channel only (target 65520): the others still overflow, the comparison with torch's rounding sees it
        one = fe.store(y32, fmt)
        one[:, 2] = fe.store_clamped(y32, fmt)[:, 2]
        with pytest.raises(AssertionError, match='differ from torch'):
            fe.check_conv_saturation(one, *args)
    else:           # nothing to clamp: every target is finite in bf16
        assert torch.equal(fe.store_clamped(y32, fmt), fe.store(y32, fmt))


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('sel', CONVS)
def test_conv_subnormals_accept_exact_rounding_and_reject_flushed_operands(sel, fmt):
    k, K, cout, xs, ws = _shape(sel)
    x, w, scale, bias = fe.conv_subnormal_operands(K, cout, xs, ws)
    y32, ref64, abs64 = _conv_sim(sel, x, w, scale, bias, fmt)
    fe.check_conv_subnormals(fe.store(y32, fmt), ref64, abs64, K, fmt, sel)
    flushed = _conv_sim(sel, fe.flush_subnormals(x, fmt), fe.flush_subnormals(w, fmt), scale, bias, fmt)[0]
    if fmt == 'fp16':
        assert not flushed.any()
        with pytest.raises(AssertionError, match='flushed to zero'):
            fe.check_conv_subnormals(fe.store(flushed, fmt), ref64, abs64, K, fmt, sel)
        # an output conversion that flushes: the same check
        out = fe.store(y32, fmt)
        out = torch.where(out.abs() < 2.0 ** -14, torch.zeros_like(out), out)
        with pytest.raises(AssertionError, match='flushed to zero'):
            fe.check_conv_subnormals(out, ref64, abs64, K, fmt, sel)
    else:           # the operands are ordinary bf16 numbers
        assert torch.equal(flushed, y32)


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------------
# (kernel family, case) -> [N, M, C] and the groups: the clip kernels' two cases and the per-RoI kernels' smallest
GN = {('clip', n): (CLIP_CASES[n][0], int(np.prod(CLIP_CASES[n][1:4])), CLIP_CASES[n][4], CLIP_CASES[n][6]) for n in EDGE_CASES}
GN[('roi', 'two_per_group')] = (ROI_CASES['two_per_group'][0], int(np.prod(ROI_CASES['two_per_group'][1:4])), ROI_CASES['two_per_group'][4],
                                ROI_CASES['two_per_group'][6])
GN_IDS = sorted(GN)


def _check_y(y, z, G, s, b, eps, fmt, what):
    return ref.check_forward(nm._np64(y), z, G, s.astype(np.float64), b.astype(np.float64), eps, fmt, what)


@pytest.mark.parametrize('fmt', FMTS + ['fp32'])
@pytest.mark.parametrize('key', GN_IDS, ids=['%s-%s' % k for k in GN_IDS])
def test_gn_subnormal_inputs_accept_the_simulation_and_reject_flushed_loads(key, fmt):
    N, M, C, G = GN[key]
    z, s, b = fe.gn_subnormal_case(N, M, C)
    z = nm.q16(z, fmt)
    y32, tables = fe.gn_forward_fp32(z, G, s, b, EPS)
    want, bounds = ref.table_bounds(z, G, s.astype(np.float64), b.astype(np.float64), EPS)
    assert all(np.all(np.abs(t - w) <= d) for t, w, d in zip(tables, want, bounds))
    w = _check_y(fe.store(y32, fmt).float(), z, G, s, b, EPS, fmt, 'subnormal inputs')
    assert np.median(np.abs(y32)) > 1e-3
    zf = fe.flush_subnormals(z, fmt) if fmt != 'fp32' else z
    if fmt == 'fp16':
        assert np.all(np.abs(z) < 2.0 ** -14) and not zf.any()
        yf = fe.gn_forward_fp32(zf, G, s, b, EPS)[0]
        assert not yf.any()
        with pytest.raises(AssertionError, match='outside the per-element bound'):
            _check_y(fe.store(yf, fmt).float(), z, G, s, b, EPS, fmt, 'flushed')
    else:           # bf16 and fp32: the values are ordinary normals
        assert np.array_equal(zf, z)
    print('%s %s: simulation err / bound %.3f' % (key, fmt, w))


@pytest.mark.parametrize('fmt', FMTS + ['fp32'])
@pytest.mark.parametrize('key', GN_IDS, ids=['%s-%s' % k for k in GN_IDS])
def test_gn_saturation_accepts_torch_s_conversion_and_rejects_a_clamp(key, fmt):
    N, M, C, G = GN[key]
    z, s, b, eps, want32, exact = fe.gn_saturation_case(N, M, C, G)
    assert np.array_equal(nm.q16(z, fmt), z)
    y32, tables = fe.gn_forward_fp32(z, G, s, b, eps)
    for t, e in zip(tables, exact):
        assert np.array_equal(t, np.broadcast_to(e, t.shape))
    assert np.array_equal(y32, want32)
    fe.check_gn_saturation(fe.store(y32, fmt), want32, fmt, str(key))
    if fmt == 'fp16':
        with pytest.raises(AssertionError, match='overflow'):
            fe.check_gn_saturation(fe.store_clamped(y32, fmt), want32, fmt, str(key))
        with pytest.raises(AssertionError, match='overflow'):               # 65519 -> 65536 in bf16 -> inf: a wrong overflow
            fe.check_gn_saturation(fe.store_through_bf16(y32), want32, fmt, str(key))
    elif fmt == 'bf16':
        assert torch.equal(fe.store_clamped(y32, fmt), fe.store(y32, fmt))


@pytest.mark.parametrize('fmt', FMTS + ['fp32'])
@pytest.mark.parametrize('key', GN_IDS, ids=['%s-%s' % k for k in GN_IDS])
def test_gn_high_mean_bounds_are_not_vacuous_and_reject_a_result_rounded_through_bf16(key, fmt):
    N, M, C, G = GN[key]
    z, s, b = fe.gn_high_mean_case(N, M, C)
    z = nm.q16(z, fmt)
    s64, b64 = s.astype(np.float64), b.astype(np.float64)
    y64, absref, extra = ref.forward_ref64(z, G, s64, b64, EPS)
    ratio = nm.bound(y64, absref, 2, fmt, extra) / np.maximum(np.abs(y64), 1e-300)
    big = np.abs(y64) >= 0.5
    print('%s %s: bound / |ref| of y: median %.3g, at |ref| >= 0.5: max %.3g (%d of %d elements)' % (
        key, fmt, np.median(ratio), ratio[big].max(), big.sum(), big.size))
    if key == ('roi', 'two_per_group') and fmt == 'bf16':
        # bf16's spacing at 3e4 is 128: the two values of a group are often equal, its variance 0, rstd = eps^-1/2 and the bound of y
        # (|a| d_mu) tens of times |y|.  The GPU test leaves this case out in the bf16 build.
        assert ratio[big].max() > 10
        return
    assert np.median(ratio) < 1 and big.mean() > 0.5 and ratio[big].max() < 1, 'the bound is vacuous here'
    y32, tables = fe.gn_forward_fp32(z, G, s, b, EPS)
    want, bounds = ref.table_bounds(z, G, s64, b64, EPS)
    assert all(np.all(np.abs(t - w) <= d) for t, w, d in zip(tables, want, bounds))
    _check_y(fe.store(y32, fmt).float(), z, G, s, b, EPS, fmt, 'high mean')
    if fmt == 'fp16':
        with pytest.raises(AssertionError, match='outside the per-element bound'):
            _check_y(fe.store_through_bf16(y32).float(), z, G, s, b, EPS, fmt, 'through bf16')
