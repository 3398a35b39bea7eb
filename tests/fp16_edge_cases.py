"""Operands, expectations and checks of the 16-bit format edges (tests/test_gpu_fp16_edges.py, the edge tests of
tests/test_gpu_group_norm.py and tests/test_gpu_gn_roi.py), and plain fp32 simulations of a correct kernel with the defects each
edge exists for (tests/test_fp16_edges_cpu.py): subnormal inputs flushed to zero, an output clamped to the largest finite value
instead of overflowing, an fp16 output rounded through bf16.  Nothing here knows a kernel; the format is always an argument.

Convs.  Three operand sets per shape: sums beyond the half range that the affine scale brings back; exact sums whose scale puts the
interior outputs on the saturation targets; operands and outputs in the fp16 subnormal range.

GroupNorm (y = z a + b', a = s rstd, b' = b - mu a; [N, M, C] arrays, G groups of cg = C / G channels):
  * `gn_subnormal_case`: every z is a multiple of 2^-24 below 2^-14 (an fp16 subnormal; a normal number in bf16 and fp32), so the group
    variance (~1e-9) is far below eps and rstd ~ eps^-1/2; with b = 0 the outputs are normal numbers of the size 1e-2, and a kernel that
    flushes subnormal loads returns zeros.
  * `gn_saturation_case`: every channel is constant -- +1 in the first channel of its group, -1 in the second, 0 in the others -- so that
    every merge of the statistics is exact: mu = 0, var = 2 / cg rounded once, and eps = 4 - var makes var + eps = 4, rstd = 1 / 2.  With
    s = 2 t, b = 0 on the +-1 channels and b = t on the zero channels the fp32 value z a + b' is exactly +t, -t or t for the channel's
    target t (65504, 65519, 65520, ... as in the conv test), and the stored output must be torch's conversion of it.
  * `gn_high_mean_case`: z = 3e4 + N(0, 100^2): the mean sits near the top of the half range (the fp16 spacing there is 16, bf16's 128).
"""
import numpy as np
import torch

from tests import numerics as nm

TARGETS = np.array([65504, 65519, 65520, -65520, 65535, -65519, 131072, 60000, -70000, 1.0e6, 32768, 65520.5], np.float64)
_MAX = {torch.float16: 65504.0, torch.bfloat16: 3.3895313892515355e38}
_MIN_NORMAL = {torch.float16: 2.0 ** -14, torch.bfloat16: 2.0 ** -126}


# ---- the stored output of a correct kernel, and the defects ----------------------------------------------------------------------------
def store(y32, fmt):
    """fp32 values (numpy or torch) -> the format, round to nearest even, overflow to +-inf: torch's conversion.  -> torch tensor."""
    t = y32 if isinstance(y32, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y32, dtype=np.float32))
    return t.to(nm._fmt(fmt))


def store_clamped(y32, fmt):
    """the defect: a conversion that saturates at the largest finite value"""
    fmt = nm._fmt(fmt)
    t = y32 if isinstance(y32, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y32, dtype=np.float32))
    return t.clamp(-_MAX[fmt], _MAX[fmt]).to(fmt)


def store_through_bf16(y32):
    """the defect: an fp16 output that was rounded to bfloat16 on the way"""
    t = y32 if isinstance(y32, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y32, dtype=np.float32))
    return t.to(torch.bfloat16).to(torch.float16)


def flush_subnormals(a, fmt):
    """the defect: a load that reads the format's subnormals as zero (numpy fp32 in, numpy fp32 out)"""
    a = np.asarray(a, dtype=np.float32)
    return np.where(np.abs(a) < _MIN_NORMAL[nm._fmt(fmt)], np.float32(0), a)


# ---- convs -------------------------------------------------------------------------------------------------------------------------------
def conv_large_sums_operands(K, cout, xs, ws):
    """Non-negative activations and mostly positive weights whose fp32 sums over K products reach ~4 x 65504; scale 1 / 16."""
    rs = np.random.RandomState(K + cout)
    a = np.sqrt(262144.0 / K)
    x = (rs.uniform(0.5, 1.5, xs) * a).astype(np.float32)
    w = (rs.uniform(0.5, 1.5, ws) * a * np.where(rs.uniform(size=ws) < 0.1, -1.0, 1.0)).astype(np.float32)
    scale = np.full(cout, 1.0 / 16, np.float32)
    bias = (rs.randn(cout) * 4).astype(np.float32)
    return x, w, scale, bias


def conv_saturation_operands(K, cout, xs, ws):
    """Every product is 64 * 64, every sum an exact fp32 integer; per output channel the scale puts the interior sum K * 4096 on TARGETS."""
    x = np.full(xs, 64.0, np.float32)
    w = np.full(ws, 64.0, np.float32)
    scale = (TARGETS[np.arange(cout) % len(TARGETS)] / float(K * 64 * 64)).astype(np.float32)
    return x, w, scale, np.zeros(cout, np.float32)


def conv_subnormal_operands(K, cout, xs, ws):
    """Small multiples of 2^-24 (exact in both formats), scales 2^19 .. 2^21: outputs in the fp16 subnormal range, every sum exact."""
    rs = np.random.RandomState(K + 3)
    x = (rs.randint(-15, 16, xs) * 2.0 ** -24).astype(np.float32)
    w = (rs.randint(-15, 16, ws) * 2.0 ** -24).astype(np.float32)
    scale = (2.0 ** rs.randint(19, 22, cout)).astype(np.float32)
    return x, w, scale, np.zeros(cout, np.float32)


def worst(got, ref64, abs64, K, fmt, extra=0.0):
    """largest err / bound (inf for a NaN or an infinite output)"""
    g = nm._np64(got)
    return float(np.max(np.where(np.isfinite(g), np.abs(g - ref64), np.inf) / nm.bound(ref64, abs64, K, fmt, extra)))


def check_conv_large_sums(got, ref64, abs64, bias, K, fmt, what):
    """got: the stored output as a torch tensor of the format.  Finite outputs within the per-element bound: no 16-bit partial sum,
    split-K partial or staging copy."""
    assert (np.abs(ref64 - bias.reshape(1, -1, 1, 1, 1)) * 16).max() > 2 * 65504, 'the sums do not leave the half range'
    assert np.abs(ref64).max() < 65504 / 2
    assert torch.isfinite(got).all()
    print('large sums %s: worst err / bound %.3f' % (what, worst(got, ref64, abs64, K, fmt)))
    nm.assert_elementwise(got, ref64, abs64, K, fmt, 'large sums ' + what)


def check_conv_saturation(got, ref64, scale, interior, inner, fmt, what):
    """The kernel's fp32 result is the exact sum times the fp32 scale, one fp32 rounding (bias 0 adds nothing); the stored output equals
    torch's conversion of that value: fp16 rounds to nearest even (65519 -> 65504, >= 65520 -> +-inf); bf16 keeps them finite.
    inner: the index of the outputs whose every tap lies inside the clip (their sum is `interior`)."""
    fmt = nm._fmt(fmt)
    sums = ref64 / scale.astype(np.float64).reshape(1, -1, 1, 1, 1)
    assert np.all(np.rint(sums[inner]) == interior)
    want32 = (torch.from_numpy(np.rint(sums).astype(np.float32)) * torch.from_numpy(scale).view(1, -1, 1, 1, 1))
    want = want32.to(fmt)
    if fmt == torch.float16:
        assert torch.isinf(got[inner]).any() and (got[inner] == 65504).any(), 'no saturated / clamped interior outputs'
    else:
        assert torch.isfinite(got).all()
    bad = got.float() != want.float()
    print('saturation %s: %d of %d outputs differ from torch\'s rounding of the fp32 value' % (what, int(bad.sum()), bad.numel()))
    assert not bad.any(), '%s: %d outputs differ from torch\'s rounding, e.g. got %r want %r' % (
        what, int(bad.sum()), got[bad][:4].tolist(), want[bad][:4].tolist())


def check_conv_subnormals(got, ref64, abs64, K, fmt, what):
    """Every product and sum is exact in fp32, so the stored output must equal torch's rounding of the exact result: subnormals kept,
    ties to even, no flush to zero."""
    fmt = nm._fmt(fmt)
    want = torch.from_numpy(ref64).to(fmt)                       # exact in fp32, so one rounding of the exact value
    if fmt == torch.float16:
        sub = (want != 0) & (want.abs() < 2.0 ** -14)
        assert sub.float().mean() > 0.3, 'too few subnormal outputs: %.3f' % sub.float().mean()
        assert (got[sub] != 0).all(), 'subnormal outputs flushed to zero'
    bad = got.float() != want.float()
    print('subnormals %s: %d of %d outputs differ from torch\'s rounding, worst err / bound %.3f' % (
        what, int(bad.sum()), bad.numel(), worst(got, ref64, abs64, K, fmt)))
    assert not bad.any(), '%s: %d of %d outputs differ from torch\'s rounding, e.g. got %r want %r' % (
        what, int(bad.sum()), bad.numel(), got[bad][:4].tolist(), want[bad][:4].tolist())
    nm.assert_elementwise(got, ref64, abs64, K, fmt, 'subnormals ' + what)


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------------
def gn_subnormal_case(N, M, C, seed=5):
    """-> (z fp32 [N, M, C], s, b): |z| = k 2^-24 < 2^-14 (exact in fp16 and fp32; bf16 rounds the larger k), s in [0.5, 1.5], b = 0."""
    rs = np.random.RandomState(seed)
    z = (rs.randint(-1023, 1024, (N, M, C)) * 2.0 ** -24).astype(np.float32)
    return z, rs.uniform(0.5, 1.5, C).astype(np.float32), np.zeros(C, np.float32)


def gn_saturation_case(N, M, C, G):
    """-> (z, s, b, eps, want32 [N, M, C], tables (mu, rstd, a, b') [C]): see the module docstring; every value is exact in fp32, and z
    in both 16-bit formats."""
    cg = C // G
    assert cg >= 2 and C % G == 0
    j = np.arange(C) % cg
    zc = np.where(j == 0, 1.0, np.where(j == 1, -1.0, 0.0)).astype(np.float32)
    t = TARGETS[np.arange(C) % len(TARGETS)].astype(np.float32)
    s = np.where(j < 2, 2 * t, 1.0).astype(np.float32)
    b = np.where(j < 2, 0.0, t).astype(np.float32)
    assert np.array_equal(s.astype(np.float64), np.where(j < 2, 2 * TARGETS[np.arange(C) % len(TARGETS)], 1.0))
    var = np.float32(2.0) / np.float32(cg)                       # M2 = 2 M over M cg values: one rounding
    eps = np.float32(4.0) - var
    assert np.float32(var + eps) == np.float32(4.0), (cg, var, eps)
    z = np.broadcast_to(zc, (N, M, C)).copy()
    want32 = np.broadcast_to(np.where(j == 1, -t, t).astype(np.float32), (N, M, C)).copy()
    tables = (np.zeros(C, np.float32), np.full(C, 0.5, np.float32), (s * np.float32(0.5)).astype(np.float32), b.copy())
    return z, s, b, float(eps), want32, tables


def gn_high_mean_case(N, M, C, seed=9):
    """-> (z fp32 [N, M, C], s, b): z = 3e4 + N(0, 100^2); the caller rounds z to the tensor format."""
    rs = np.random.RandomState(seed)
    z = (3.0e4 + 100.0 * rs.randn(N, M, C)).astype(np.float32)
    return z, rs.uniform(0.5, 1.5, C).astype(np.float32), (rs.randn(C) * 0.3).astype(np.float32)


def gn_forward_fp32(z, G, s, b, eps):
    """What a correct kernel computes, every operation rounded to fp32: the group mean, the variance around it (two passes), rstd,
    a = s rstd, b' = b - mu a and y = fma(z, a, b').  z: fp32 [N, M, C].  -> (y32 [N, M, C], (mu, rstd, a, b') [N, C])."""
    f = np.float32
    z = np.asarray(z, dtype=f)
    N, M, C = z.shape
    cg = C // G
    zg = z.reshape(N, M, G, cg).transpose(0, 2, 1, 3).reshape(N, G, M * cg)
    n = f(M * cg)
    mu = (zg.sum(axis=2, dtype=f) / n).astype(f)
    d = (zg - mu[:, :, None]).astype(f)
    var = ((d * d).astype(f).sum(axis=2, dtype=f) / n).astype(f)
    rstd = (f(1) / np.sqrt((var + f(eps)).astype(f))).astype(f)
    mu, rstd = np.repeat(mu, cg, axis=1), np.repeat(rstd, cg, axis=1)
    a = (np.asarray(s, dtype=f) * rstd).astype(f)
    bp = (np.asarray(b, dtype=f) - (mu * a).astype(f)).astype(f)
    y = (z.astype(np.float64) * a[:, None, :].astype(np.float64) + bp[:, None, :].astype(np.float64)).astype(f)     # one rounding: the fma
    return y, (mu, rstd, a, bp)


def check_gn_saturation(got, want32, fmt, what):
    """got: the stored output [N, M, C] as a torch tensor of the format; want32: the exact fp32 values.  Equal to torch's conversion,
    which overflows to +-inf at and beyond 65520 in fp16 and stays finite in bf16 and fp32."""
    fmt = nm._fmt(fmt)
    want = store(want32, fmt)
    if fmt == torch.float16:
        assert torch.isinf(want).any() and (want == 65504).any() and (want == -65504).any()
        assert torch.equal(torch.isinf(got), torch.isinf(want)), '%s: %d outputs overflow, torch\'s conversion gives %d' % (
            what, int(torch.isinf(got).sum()), int(torch.isinf(want).sum()))
    else:
        assert torch.isfinite(want).all() and torch.isfinite(got).all()
    bad = got.float() != want.float()
    print('GroupNorm saturation %s: %d of %d outputs differ from torch\'s rounding of the fp32 value' % (what, int(bad.sum()), bad.numel()))
    assert not bad.any(), '%s: %d outputs differ from torch\'s rounding, e.g. got %r want %r' % (
        what, int(bad.sum()), got[bad][:4].tolist(), want[bad][:4].tolist())
