"""Per-element error bounds for the 16-bit kernel tests.

The library ships two builds of the same sources: libdat_hip.so holds bfloat16 in every 16-bit tensor, libdat_hip_f16.so
(DAT_H16=fp16) IEEE half.  A test quantises its operands the way the loaded build will (`q16`), computes the operation in float64
on the CPU from those operands (`ref64`) and the same operation on their absolute values (`absref64`), and then holds every output
element of the kernel to

    |got - ref| <= u_out * |ref|  +  C * sqrt(K) * 2^-24 * absref  (+ the smallest half-ulp of the output format)

u_out is the unit roundoff of the stored output (one correct rounding at the end), the second term the fp32 accumulation and the fp32
epilogue (scale, bias, residual) over a reduction of length K.  A max-abs tolerance scaled by the largest output cannot see rounding
bugs: a truncating output conversion or a result rounded through bf16 in the fp16 build stays inside it; this bound does not.
"""
import numpy as np
import torch

# The fp32 accumulation term's constant: 8 is enough for every kernel order (tile / split-K / tap order) in float64 simulation of
# fp32 accumulation at the shapes of the suite.  One constant for every test: a path that rounds to 16 bits twice adds that term at
# its call site (`extra`), it does not raise C.
C = 8.0

_U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
# half the smallest subnormal: the absolute rounding error of a correctly rounded result below the normal range
_TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}
_NAMES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}


def h16():
    """The loaded library build's 16-bit format (torch.bfloat16 or torch.float16)."""
    from detectandtrack_amd.ops import hip_ops
    return hip_ops.H16_DTYPE


def _fmt(fmt):
    fmt = _NAMES.get(fmt, fmt)
    assert fmt in _U, 'unknown format %r' % (fmt,)
    return fmt


def q16(a, fmt=None):
    """Operands as the kernel sees them: rounded (to nearest even) to the build's 16-bit format, returned in fp32 (numpy in, numpy
    out; torch in, torch out on the same device)."""
    fmt = h16() if fmt is None else _fmt(fmt)
    if isinstance(a, torch.Tensor):
        return a.to(fmt).float()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(fmt).float().numpy()


def unit_roundoff(fmt):
    """Half an ulp at 1.0: bf16 2^-8, fp16 2^-11, fp32 2^-24."""
    return _U[_fmt(fmt)]


def _np64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu()
        return (a.double() if a.is_floating_point() else a).numpy()
    return np.asarray(a, dtype=np.float64)


def bound(ref64, absref64, K, out_fmt, extra=0.0):
    out_fmt = _fmt(out_fmt)
    ref, absref = _np64(ref64), _np64(absref64)
    return unit_roundoff(out_fmt) * np.abs(ref) + C * np.sqrt(float(K)) * 2.0 ** -24 * absref + _TINY[out_fmt] + _np64(extra)


def assert_elementwise(got, ref64, absref64, K, out_fmt, what, extra=0.0):
    """Every element of `got` within the bound of the module docstring.  `extra` (scalar or per element) is an explicitly named
    additional error term of a path that legitimately rounds twice."""
    g, ref = _np64(got), _np64(ref64)
    assert g.shape == ref.shape, '%s: shape %r != reference %r' % (what, g.shape, ref.shape)
    b = bound(ref, absref64, K, out_fmt, extra)
    b = np.broadcast_to(b, ref.shape)
    err = np.abs(g - ref)
    bad = ~(err <= b)                   # NaN / inf in `got` fail
    if bad.any():
        ratio = np.where(bad, np.where(np.isfinite(err), err / np.maximum(b, 1e-300), np.inf), 0.0)
        i = np.unravel_index(int(np.argmax(ratio)), ref.shape)
        raise AssertionError('%s: %d of %d elements outside the per-element bound (K=%d, out=%s); worst at %r: got %.9g, ref %.9g, '
                             '|err| %.3g > bound %.3g' % (what, int(bad.sum()), ref.size, K, str(_fmt(out_fmt)).replace('torch.', ''),
                                                          tuple(int(v) for v in i), g[i], ref[i], err[i], b[i]))


def conv_ref64(x, w, scale=None, bias=None, res=None, stride=(1, 1), pads=(0, 0, 0), relu=False, mask=None):
    """(ref64, absref64) of the fused conv epilogue: conv3d(x, w) * scale + bias + res, ReLU, then `mask > 0 ? v : 0` -- in float64
    on the CPU from the given (already quantised) operands, and the same chain on their absolute values.  x: (N, Cin, T, H, W),
    w: (Cout, Cin, KT, KH, KW); stride is (sh, sw) or (st, sh, sw)."""
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(_np64(a)) if not isinstance(a, torch.Tensor) else a.detach().cpu().double()
    st = tuple(stride) if len(stride) == 3 else (1,) + tuple(stride)
    outs = []
    for absolute in (False, True):
        f = (lambda v: v.abs()) if absolute else (lambda v: v)
        y = F.conv3d(f(t(x)), f(t(w)), None, stride=st, padding=tuple(pads))
        if scale is not None:
            y = y * f(t(scale)).view(1, -1, 1, 1, 1)
        if bias is not None:
            y = y + f(t(bias)).view(1, -1, 1, 1, 1)
        if res is not None:
            y = y + f(t(res))
        if relu and not absolute:
            y = torch.relu(y)
        if mask is not None and not absolute:
            y = torch.where(t(mask) > 0, y, torch.zeros_like(y))
        outs.append(y.numpy())
    return outs[0], outs[1]


def conv_k(cin, k):
    """The reduction length of a conv: input channels times taps."""
    return int(cin) * int(np.prod(k))


def sum_bound(abssum64, n, extra=0.0):
    """Bound on the error of a scalar that a kernel sums from `n` fp32 terms (per-thread partial sums, an LDS tree per block, then
    float atomics across blocks), against the float64 sum of the same terms:

        |got - ref| <= C * sqrt(n) * 2^-24 * sum_i |term_i|  +  extra  (+ the smallest fp32 half-ulp)

    Every addition of a partial sum s rounds once, with error at most 2^-24 * |s| <= 2^-24 * sum_i |term_i|; a sum of n terms in any
    order holds at most n - 1 such roundings, and round-to-nearest errors of independent sign grow like their square root -- the
    C * sqrt(K) term of `bound` with K = n.  The few fp32 roundings of each term's own arithmetic (products, the final multiply by
    the normaliser) stay below C * 2^-24 * |term_i| and are covered by the same term.  A libm call inside a term (expf, log1pf,
    logf: a few ulps of its result, amplified by the argument's rounding) is not: the caller names it in `extra`.  A sum with one
    term missing misses it by |term| and a sum accumulated in bf16 drifts by ~2^-9 per addition -- both far outside the bound at the
    sizes of the suite (tests/test_train_refs_cpu.py)."""
    return C * np.sqrt(float(max(n, 1))) * 2.0 ** -24 * float(abssum64) + float(extra) + _TINY[torch.float32]


def assert_sum(got, ref64, abssum64, n, what, extra=0.0):
    """`got` (a float) within `sum_bound` of the float64 sum `ref64`."""
    b = sum_bound(abssum64, n, extra)
    err = abs(float(got) - float(ref64))
    assert err <= b, '%s: got %.9g, ref %.9g, |err| %.3g > bound %.3g (n=%d, sum|term| %.6g)' % (what, float(got), float(ref64), err, b,
                                                                                               n, float(abssum64))
