"""Reference restatement of GroupNorm (HIP.USE_GN) for the tests.

1. `gn_net(base, ...)`: the oracle graph (`oracle.net3d.Net` or `tests.r2plus1d_ref.Net2plus1d`) with only `affine` overridden by
   `torch.nn.functional.group_norm` on the NC(D)HW view -- per sample (clip), over T x H x W x the cg channels of a group, biased
   variance, the same in training and at test time.

2. float64 NumPy references of the kernels on [clips, M, C] arrays (M = T H W positions of a clip, G groups of cg = C / G channels,
   Mg = M cg values per group) and the error bounds the kernel tests hold them to.  The bounds are built from `tests.numerics.sum_bound`
   / `numerics.bound` only, the way tests/spatial_bn_ref.py builds SpatialBN's, with the group's Mg terms in place of the channel's M:

     d_mu  = sum_bound(mean_i |z_i|, Mg)           mu is a sum of the Mg terms z_i / Mg
     d_M2  = sum_bound(M2, Mg)                     M2 = sum_i (z_i - mu)^2, all terms >= 0 (d M2 / d mu = -2 sum (z_i - mu) = 0: the error
                                                   of mu enters M2 in second order only)
     d_var = d_M2 / Mg
     d_rstd = 1/2 rstd^3 d_var + 2 u rstd          rstd = (var + eps)^-1/2, first order, + its own fp32 roundings (u = 2^-24)
     d_a   = |s| d_rstd + u |a|                    a = s rstd
     d_b'  = |a| d_mu + |mu| d_a + 2 u (|b| + |mu a|)      b' = b - mu a

   y = s (z - mu) rstd + b, so to first order  |dy| <= |s rstd| d_mu + |s (z - mu)| d_rstd: the `extra` of the forward check.  The kernel
   evaluates y as z a + b': the fp32 roundings of that form are the K = 2 accumulation term of `numerics.bound` on
   absref = |z a| + |b'| + |res|.

   Backward.  The kernels get the saved tables (mu, rstd, a) as fp32 INPUTS and the float64 reference is computed from those same
   values, so no statistics error enters.  S1 = sum g, S2 = sum g xhat per (clip, channel): `sum_bound` over the window's rows.
   dz is computed from the sums the kernel returned (fp32 values, taken as exact): with A = sum_c s_c S1_c, B = sum_c s_c S2_c over
   the cg channels of the group, dz = a g + q + r (z - mu), q = -rstd A / Mg, r = -rstd^2 B / Mg.  The kernel sums A and B itself:
   d_A = sum_bound(sum |s S1|, cg), d_q = rstd d_A / Mg + 3 u |q|, likewise d_r = rstd^2 d_B / Mg + 4 u |r| (the fp32 products and the
   division), and dz is held to K = 3 on absref = |a g| + |q| + |r (z - mu)| with extra = d_q + |z - mu| d_r.

   Nothing here was fitted to what the kernels return.
"""
import numpy as np
import torch

from tests import numerics as nm

U32 = 2.0 ** -24


def groups_of(channels, max_groups=32):
    """The documented rule, restated: the largest divisor of `channels` that is <= max_groups."""
    return max(g for g in range(1, max_groups + 1) if channels % g == 0)


# ---- 1. the graph ------------------------------------------------------------------------------------------------------------------------
def gn_net(base, eps, max_groups=32):
    """`base` with `affine` replaced by GroupNorm."""

    class GNNet(base):
        def affine(self, x, name):
            s, b = self.w[name + '_s'], self.w[name + '_b']
            s, b = (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t)) for t in (s, b))
            return torch.nn.functional.group_norm(x, groups_of(x.shape[1], max_groups), s.to(x.dtype), b.to(x.dtype), eps)

    return GNNet


def autograd_reference(base, weights, opts, data, im_info, labels, sampled, scalars, dtype, eps, max_groups=32):
    """One forward + backward of `oracle.train_ref.training_losses` on the GN restatement of `base`, on the CPU in `dtype`
    (torch.float32 or torch.float64).  -> (losses, gradients), NumPy float64.  The oracle modules are patched for the duration of the
    call only (its float32 casts, its Net class)."""
    from oracle import net3d, train_ref
    saved = (net3d._t, train_ref.Net, torch.from_numpy)

    def as_dtype(a):
        t = a if isinstance(a, torch.Tensor) else saved[2](np.ascontiguousarray(a))
        return t.to(dtype) if t.is_floating_point() else t
    wt = {k: saved[2](np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in weights.items()}
    try:
        net3d._t = as_dtype
        train_ref.Net = gn_net(base, eps, max_groups)
        train_ref.torch.from_numpy = as_dtype       # (train_ref wraps its float32 inputs itself)
        losses = train_ref.training_losses(wt, opts, data, im_info, labels, sampled, scalars)
        sum(losses.values()).backward()
    finally:
        net3d._t, train_ref.Net, torch.from_numpy = saved
    grads = {k: v.grad.detach().double().numpy() for k, v in wt.items() if v.grad is not None}
    return {k: float(v.detach()) for k, v in losses.items()}, grads


# ---- 2. kernel references and bounds ---------------------------------------------------------------------------------------------------
def _grouped(z, G):
    """[N, M, C] -> [N, G, M * cg] (the values of each group)"""
    N, M, C = z.shape
    return z.reshape(N, M, G, C // G).transpose(0, 2, 1, 3).reshape(N, G, M * (C // G))


def _per_channel(v, C):
    """[N, G] -> [N, C]"""
    return np.repeat(v, C // v.shape[1], axis=1)


def stats_ref64(z, G, eps):
    """z: [N, M, C] (already quantised).  -> dict of float64 [N, C] (equal within a group): mu, M2, var (biased), rstd."""
    z = np.asarray(z, dtype=np.float64)
    C = z.shape[2]
    zg = _grouped(z, G)
    mu = zg.mean(axis=2)
    M2 = ((zg - mu[:, :, None]) ** 2).sum(axis=2)
    var = M2 / zg.shape[2]
    return {k: _per_channel(v, C) for k, v in dict(mu=mu, M2=M2, var=var, rstd=1.0 / np.sqrt(var + eps)).items()}


def stats_bounds(z, G, eps):
    """The docstring's d_mu, d_var, d_rstd, [N, C]."""
    z = np.asarray(z, dtype=np.float64)
    C = z.shape[2]
    zg = _grouped(z, G)
    Mg = zg.shape[2]
    r = stats_ref64(z, G, eps)
    sb = np.vectorize(lambda v: nm.sum_bound(v, Mg))
    d_mu = _per_channel(sb(np.abs(zg).mean(axis=2)), C)
    d_var = sb(r['M2']) / Mg
    d_rstd = 0.5 * r['rstd'] ** 3 * d_var + 2 * U32 * r['rstd']
    return d_mu, d_var, d_rstd


def table_bounds(z, G, s, b, eps):
    """-> (reference tables mu, rstd, a, b' [N, C], their bounds d_mu, d_rstd, d_a, d_b)"""
    r = stats_ref64(z, G, eps)
    d_mu, _, d_rstd = stats_bounds(z, G, eps)
    a = s * r['rstd']
    d_a = np.abs(s) * d_rstd + U32 * np.abs(a)
    d_b = np.abs(a) * d_mu + np.abs(r['mu']) * d_a + 2 * U32 * (np.abs(b) + np.abs(r['mu'] * a))
    return (r['mu'], r['rstd'], a, b - r['mu'] * a), (d_mu, d_rstd, d_a, d_b)


def forward_ref64(z, G, s, b, eps, res=None, relu=False):
    """-> (y64, absref64, extra) [N, M, C] of y = act(s (z - mu) rstd + b (+ res)) for `numerics.assert_elementwise(K=2)`."""
    z = np.asarray(z, dtype=np.float64)
    r = stats_ref64(z, G, eps)
    d_mu, _, d_rstd = stats_bounds(z, G, eps)
    mu, a = r['mu'][:, None, :], (s * r['rstd'])[:, None, :]
    y = (z - mu) * a + b
    absref = np.abs(z * a) + np.abs(b - mu * a)
    if res is not None:
        y = y + res
        absref = absref + np.abs(res)
    if relu:
        y = np.maximum(y, 0.0)
    extra = np.abs(a) * d_mu[:, None, :] + np.abs(s * (z - mu)) * d_rstd[:, None, :]
    return y, absref, extra


def check_forward(y_got, z, G, s, b, eps, out_fmt, what, res=None, relu=False):
    y, absref, extra = forward_ref64(z, G, s, b, eps, res, relu)
    nm.assert_elementwise(y_got, y, absref, 2, out_fmt, what, extra=extra)
    return float(np.max(np.abs(np.asarray(y_got, dtype=np.float64) - y) / nm.bound(y, absref, 2, out_fmt, extra)))


def backward_sums_ref64(dy, y, z, mu, rstd, lo, n, relu):
    """dy: [N, n, C] = the rows [lo, lo + n) of every clip; y, z: [N, M, C]; mu, rstd: the SAVED tables as the kernels read them (fp32
    values, [N, C]).  -> g [N, n, C], S1, S2 [N, C] and the sums of the terms' magnitudes."""
    dy, z = np.asarray(dy, dtype=np.float64), np.asarray(z, dtype=np.float64)
    g = dy * (np.asarray(y)[:, lo:lo + n] > 0) if relu else dy.copy()
    xh = (z - mu[:, None, :]) * rstd[:, None, :]
    gx = g * xh[:, lo:lo + n]
    return dict(g=g, S1=g.sum(axis=1), S2=gx.sum(axis=1), abs_S1=np.abs(g).sum(axis=1), abs_S2=np.abs(gx).sum(axis=1))


def backward_dz_ref64(g, z, G, s, mu, rstd, S1, S2, lo, a=None):
    """dz [N, M, C] = rstd (s g - A / Mg - xhat B / Mg) from the given tables and sums (all taken as exact), with g = 0 outside the rows
    [lo, lo + n); a: the saved table a = s rstd as the kernel reads it (fp32 values; default: the float64 product).
    -> (dz, absref, extra) for `assert_elementwise(K=3)`, and the coefficients (q, r) with their bounds."""
    z = np.asarray(z, dtype=np.float64)
    N, M, C = z.shape
    cg = C // G
    Mg = M * cg
    gf = np.zeros_like(z)
    gf[:, lo:lo + g.shape[1]] = g
    grp = lambda v: _per_channel(v.reshape(N, G, cg).sum(axis=2), C)
    A, B = grp(s * S1), grp(s * S2)
    sb = np.vectorize(lambda v: nm.sum_bound(v, cg))
    d_A, d_B = sb(grp(np.abs(s * S1))), sb(grp(np.abs(s * S2)))
    q, r = -rstd * A / Mg, -rstd ** 2 * B / Mg
    d_q, d_r = rstd * d_A / Mg + 3 * U32 * np.abs(q), rstd ** 2 * d_B / Mg + 4 * U32 * np.abs(r)
    a = (s * rstd if a is None else np.asarray(a, dtype=np.float64))[:, None, :]
    zc = z - mu[:, None, :]
    dz = a * gf + q[:, None, :] + r[:, None, :] * zc
    absref = np.abs(a * gf) + np.abs(q)[:, None, :] + np.abs(r[:, None, :] * zc)
    extra = d_q[:, None, :] + np.abs(zc) * d_r[:, None, :]
    return dz, absref, extra, (q, r, d_q, d_r)


def full_backward_ref64(dy, z, G, s, eps):
    """The whole GroupNorm backward in float64 from z alone (no ReLU, every row): dz, dscale, dbias -- what autograd gives."""
    z, dy = np.asarray(z, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    r = stats_ref64(z, G, eps)
    sm = backward_sums_ref64(dy, None, z, r['mu'], r['rstd'], 0, z.shape[1], False)
    dz = backward_dz_ref64(sm['g'], z, G, s, r['mu'], r['rstd'], sm['S1'], sm['S2'], 0)[0]
    return dz, sm['S2'].sum(axis=0), sm['S1'].sum(axis=0)


def naive_var_fp32(zg):
    """What the issue forbids: E[x^2] - mu^2 with every operation in fp32, summed in order like a thread's running sum.  zg: [Mg] values
    of one group."""
    zg = np.asarray(zg, dtype=np.float32)
    n = np.float32(zg.shape[0])
    mu = np.cumsum(zg, dtype=np.float32)[-1] / n
    ex2 = np.cumsum(zg * zg, dtype=np.float32)[-1] / n
    return mu, ex2 - mu * mu


def two_pass_var_fp32(zg):
    zg = np.asarray(zg, dtype=np.float32)
    n = np.float32(zg.shape[0])
    mu = np.cumsum(zg, dtype=np.float32)[-1] / n
    d = zg - mu
    return mu, np.cumsum(d * d, dtype=np.float32)[-1] / n


def offset_case(seed=11, frames=2, H=16, W=16, C=64):
    """The cancellation case of the kernel tests: z = 100 + 0.5 N(0, 1), one clip [1, M, C]."""
    rs = np.random.RandomState(seed)
    return (100.0 + 0.5 * rs.randn(1, frames * H * W, C)).astype(np.float32)
