"""Reference restatement of SpatialBN (MODEL.USE_BN) for the tests.

1. `bn_net(base, ...)`: the oracle graph (`oracle.net3d.Net` or `tests.r2plus1d_ref.Net2plus1d`) with only `affine` overridden --
   Caffe2 SpatialBN's public (cuDNN engine) semantics; its source is not part of the reference tree, so parity is unpinned like conv and
   RoIAlign.  Training mode normalises with the batch statistics (biased variance) and records the updated running statistics
   rm <- m rm + (1 - m) mu, riv <- m riv + (1 - m) var M / (M - 1); test mode normalises with rm and riv (a running VARIANCE).

2. float64 NumPy references of the four kernels on [M, C] matrices and the error bounds the kernel tests hold them to.  The bounds
   are built from `tests.numerics.sum_bound` only:

     d_mu  = sum_bound(mean_i |z_i|, M)            mu is a sum of the M terms z_i / M
     d_M2  = sum_bound(M2, M)                      M2 = sum_i (z_i - mu)^2, all terms >= 0 (d M2 / d mu = -2 sum (z_i - mu) = 0: the error
                                                   of mu enters M2 in second order only)
     d_var = d_M2 / M
     d_rstd = 1/2 rstd^3 d_var + 2 u rstd          rstd = (var + eps)^-1/2, first order, + its own fp32 roundings (u = 2^-24)

   y = s (z - mu) rstd + b, so to first order  |dy| <= |s rstd| d_mu + |s (z - mu)| d_rstd: the `extra` of `y_extra`.  The kernel
   evaluates y as z a + b' with a = s rstd, b' = b - mu a: the fp32 roundings of that form are the K = 2 accumulation term of
   `numerics.bound` on absref = |z a| + |b'| + |res|.  Nothing here was fitted to what the kernels return.
"""
import numpy as np
import torch

from tests import numerics as nm

U32 = 2.0 ** -24


# ---- 1. the graph ------------------------------------------------------------------------------------------------------------------------
def bn_net(base, train, eps, momentum, sink=None):
    """`base` with `affine` replaced by SpatialBN.  sink (dict): receives `<name>_rm` / `<name>_riv` after a training-mode forward."""

    class BNNet(base):
        def affine(self, x, name):
            s, b = self.w[name + '_s'], self.w[name + '_b']
            s, b = (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t)).to(x.dtype) for t in (s, b))
            rm, riv = (self.w[name + k] for k in ('_rm', '_riv'))
            rm, riv = (t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t)) for t in (rm, riv))
            rm, riv = rm.to(x.dtype), riv.to(x.dtype)
            shp = [1, -1] + [1] * (x.dim() - 2)
            if train:
                dims = [0] + list(range(2, x.dim()))
                M = x.numel() // x.shape[1]
                mu = x.mean(dim=dims)
                var = ((x - mu.view(shp)) ** 2).mean(dim=dims)
                if sink is not None:
                    sink[name + '_rm'] = (momentum * rm + (1 - momentum) * mu.detach()).numpy()
                    sink[name + '_riv'] = (momentum * riv + (1 - momentum) * var.detach() * M / (M - 1)).numpy()
            else:
                mu, var = rm, riv
            return (x - mu.view(shp)) / torch.sqrt(var.view(shp) + eps) * s.view(shp) + b.view(shp)

    return BNNet


def autograd_reference(base, weights, opts, data, im_info, labels, sampled, scalars, dtype, eps, momentum):
    """One training-mode forward + backward of `oracle.train_ref.training_losses` on the BN restatement of `base`, on the CPU in
    `dtype` (torch.float32 or torch.float64).  -> (losses, gradients, updated running statistics), NumPy float64.  The oracle modules
    are patched for the duration of the call only (its float32 casts, its Net class)."""
    from oracle import net3d, train_ref
    sink = {}
    saved = (net3d._t, train_ref.Net, torch.from_numpy)

    def as_dtype(a):
        t = a if isinstance(a, torch.Tensor) else saved[2](np.ascontiguousarray(a))
        return t.to(dtype) if t.is_floating_point() else t
    wt = {k: saved[2](np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in weights.items()}
    try:
        net3d._t = as_dtype
        train_ref.Net = bn_net(base, True, eps, momentum, sink)
        train_ref.torch.from_numpy = as_dtype       # (train_ref wraps its float32 inputs itself)
        losses = train_ref.training_losses(wt, opts, data, im_info, labels, sampled, scalars)
        sum(losses.values()).backward()
    finally:
        net3d._t, train_ref.Net, torch.from_numpy = saved
    grads = {k: v.grad.detach().double().numpy() for k, v in wt.items() if v.grad is not None}
    return ({k: float(v.detach()) for k, v in losses.items()}, grads, {k: np.asarray(v, dtype=np.float64) for k, v in sink.items()})


# ---- 2. kernel references and bounds ---------------------------------------------------------------------------------------------------
def stats_ref64(z, eps):
    """z: [M, C] (already quantised).  -> dict of float64 [C]: mu, M2, var (biased), rstd."""
    z = np.asarray(z, dtype=np.float64)
    mu = z.mean(axis=0)
    M2 = ((z - mu) ** 2).sum(axis=0)
    var = M2 / z.shape[0]
    return dict(mu=mu, M2=M2, var=var, rstd=1.0 / np.sqrt(var + eps))


def stats_bounds(z, eps):
    """The docstring's d_mu, d_var, d_rstd per channel."""
    z = np.asarray(z, dtype=np.float64)
    M = z.shape[0]
    r = stats_ref64(z, eps)
    d_mu = np.array([nm.sum_bound(v, M) for v in np.abs(z).mean(axis=0)])
    d_var = np.array([nm.sum_bound(v, M) for v in r['M2']]) / M
    d_rstd = 0.5 * r['rstd'] ** 3 * d_var + 2 * U32 * r['rstd']
    return d_mu, d_var, d_rstd


def forward_ref64(z, s, b, eps, res=None, relu=False):
    """-> (y64, absref64, extra) of y = act(s (z - mu) rstd + b (+ res)) for `numerics.assert_elementwise(K=2)`."""
    z = np.asarray(z, dtype=np.float64)
    r = stats_ref64(z, eps)
    d_mu, _, d_rstd = stats_bounds(z, eps)
    a = s * r['rstd']
    y = (z - r['mu']) * a + b
    absref = np.abs(z * a) + np.abs(b - r['mu'] * a)
    if res is not None:
        y = y + res
        absref = absref + np.abs(res)
    if relu:
        y = np.maximum(y, 0.0)
    extra = np.abs(a) * d_mu + np.abs(s * (z - r['mu'])) * d_rstd
    return y, absref, extra


def backward_ref64(dy, y, z, s, mu, rstd, lo, n, relu):
    """dy: the rows [lo, lo + n) of the blob; y, z: all M rows; mu, rstd: the SAVED statistics as the kernels read them (fp32 values).
    -> g [n, C], db, ds [C], dz [M, C], and the per-term magnitudes for the bounds."""
    dy, z = np.asarray(dy, dtype=np.float64), np.asarray(z, dtype=np.float64)
    M = z.shape[0]
    g = dy * (np.asarray(y)[lo:lo + n] > 0) if relu else dy.copy()
    gf = np.zeros_like(z)
    gf[lo:lo + n] = g
    xh = (z - mu) * rstd
    db, ds = gf.sum(axis=0), (gf * xh).sum(axis=0)
    a = s * rstd
    dz = a * (gf - db / M - xh * ds / M)
    absdz = np.abs(a) * (np.abs(gf) + np.abs(db) / M + np.abs(xh * ds) / M)
    return dict(g=g, db=db, ds=ds, dz=dz, absdz=absdz, abs_db=np.abs(gf).sum(axis=0), abs_ds=np.abs(gf * xh).sum(axis=0), xh=xh, a=a)


def naive_var_fp32(z):
    """What the issue forbids: E[x^2] - mu^2 with every operation in fp32, summed in order like a thread's running sum."""
    z = np.asarray(z, dtype=np.float32)
    M = np.float32(z.shape[0])
    mu = np.cumsum(z, axis=0, dtype=np.float32)[-1] / M
    ex2 = np.cumsum(z * z, axis=0, dtype=np.float32)[-1] / M
    return mu, ex2 - mu * mu


def two_pass_var_fp32(z):
    z = np.asarray(z, dtype=np.float32)
    M = np.float32(z.shape[0])
    mu = np.cumsum(z, axis=0, dtype=np.float32)[-1] / M
    d = z - mu
    return mu, np.cumsum(d * d, axis=0, dtype=np.float32)[-1] / M


def offset_case(seed=11, frames=2, H=16, W=16, C=64):
    """The cancellation case of the kernel tests: z = 100 + 0.5 N(0, 1)."""
    rs = np.random.RandomState(seed)
    return (100.0 + 0.5 * rs.randn(frames * H * W, C)).astype(np.float32)


def check_forward(y_got, z, s, b, eps, out_fmt, what, res=None, relu=False):
    y, absref, extra = forward_ref64(z, s, b, eps, res, relu)
    nm.assert_elementwise(y_got, y, absref, 2, out_fmt, what, extra=extra)
