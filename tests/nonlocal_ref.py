"""Reference statements of the spacetime non-local block (HIP.NONLOCAL; Wang et al., CVPR 2018, embedded
Gaussian).  The reference project has no such block: this is the project's own written definition.

  * `reference`: the attention  y_id = sum_j softmax_j(scale * <q_i, k_j>) v_jd  per clip in float64, with the quantities the
    per-element bound is made of.
  * `bound`: that bound, from `tests/numerics` only (C = numerics.C):

        eps_s(i) = max_j[ C sqrt(D) 2^-24 scale sum_d |q_id||k_jd| + 4 2^-24 |s_ij| ] + 4 2^-24 (max_j s_ij - min_j s_ij)
        rel(i)   = u16 (0 on the DAT_F32 path) + expm1(2 eps_s(i)) + 4 2^-23 + C sqrt(L') 2^-24
        bound    = u_out |y| + rel(i) A + tiny,         A_id = sum_j p_ij |v_jd|

    in order: P rounded once to 16 bits; the score error (fp32 accumulation over D, the fp32 scale and the subtraction of the
    maximum), which enters the numerator and the denominator; the hardware exp, used twice; the fp32 accumulation of PV and of the row
    sum over L' keys, tile rescalings included; one output rounding.
  * `simulate`: an fp32 simulation of a fused kernel (online softmax over key tiles, P rounded to the 16-bit format before PV, the row
    sum from the unrounded p) with switchable defects, for tests/test_nonlocal_cpu.py.
  * `CASES` / `make_case`: the operands of the kernel tests, shared by the CPU and the GPU files.
  * `NetNonLocal`: the block on the oracle graph (`oracle.net3d.Net` with `_stage` overridden).
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle.net3d import Net
from tests import numerics as nm

LOG2E = 1.4426950408889634

# name -> (clips, L, L', D)
CASES = {
    'tiny': (1, 1, 1, 64),
    'one_tile': (1, 32, 32, 64),
    'ragged': (1, 70, 45, 64),
    'blocks': (1, 600, 77, 128),
    'growing': (1, 70, 200, 128),
    'big': (1, 40, 100, 256),
    'uniform_ramp': (1, 33, 200, 64),
    'posv': (1, 64, 300, 64),
    'clips': (3, 50, 45, 64),
    'd512': (1, 40, 70, 512),
    'strided': (1, 70, 45, 128),
    'res4_bench': (1, 32256, 8064, 128),
}
CLIP_V_OFFSETS = (100.0, -50.0, 0.0)


def ramp_values(Lk, D):
    """V[j, d] = ((j + 1) / L')^(1 + d mod 3) + d / 64: a different ramp per channel.  Under a uniform P a missing run of keys moves
    the mean of the linear, the quadratic or the cubic channels whichever run it is (a single symmetric ramp hides a middle run)."""
    x = (np.arange(Lk, dtype=np.float64)[:, None] + 1.0) / Lk
    d = np.arange(D)[None, :]
    return x ** (1 + d % 3) + d / 64.0


def make_case(name, fmt):
    """(q, k, v, scale, clips): fp32 arrays [clips * L, D] / [clips * L', D] already rounded to `fmt` ('fp32' | 'bf16' | 'fp16')."""
    clips, L, Lk, D = CASES[name]
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)
    q = rng.randn(clips * L, D)
    k = rng.randn(clips * Lk, D)
    v = rng.randn(clips * Lk, D)
    scale = D ** -0.5
    if name == 'growing':       # key norms grow with the index and q, k are positive: the row maximum rises tile after tile
        q, k = np.abs(q), np.abs(k) * (0.2 + 3.0 * np.arange(Lk)[:, None] / Lk)
    elif name == 'big':         # |s| in the hundreds
        q, k = 8.0 * q, 8.0 * k
    elif name == 'uniform_ramp':
        q, v = 0.0 * q, ramp_values(Lk, D)
    elif name == 'posv':        # same-sign V under a near-uniform P: the mean signed error sees a truncated P
        q, k, v = 0.3 * q, 0.3 * k, rng.uniform(0.5, 1.5, size=v.shape)
    elif name == 'clips':
        v = v + np.repeat(np.asarray(CLIP_V_OFFSETS), Lk)[:, None]
    rnd = (lambda a: np.asarray(a, dtype=np.float32)) if fmt == 'fp32' else (lambda a: nm.q16(a, fmt))
    return rnd(q), rnd(k), rnd(v), scale, clips


def bench_rows(L):
    """The rows of the res4_bench case held to float64: every 97th and the last 64."""
    return np.unique(np.concatenate([np.arange(0, L, 97), np.arange(L - 64, L)]))


def reference(q, k, v, scale, clips=1):
    """float64 (y, A = sum_j p_ij |v_jd|, s, scale * sum_d |q||k|, p); rows of clip c attend the keys of clip c."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    L, Lk = q.shape[0] // clips, k.shape[0] // clips
    out = [[] for _ in range(5)]
    for c in range(clips):
        qc, kc, vc = q[c * L:(c + 1) * L], k[c * Lk:(c + 1) * Lk], v[c * Lk:(c + 1) * Lk]
        s = scale * (qc @ kc.T)
        sabs = abs(scale) * (np.abs(qc) @ np.abs(kc).T)
        e = np.exp(s - s.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        for o, a in zip(out, (p @ vc, p @ np.abs(vc), s, sabs, p)):
            o.append(a)
    return tuple(np.concatenate(o, axis=0) for o in out)


def bound_for(ref, D, fmt):
    """The per-element bound of the module docstring for outputs stored in `fmt`; ref = reference(...), D the channel count."""
    y, A, s, sabs, _ = ref
    Lk = s.shape[1]
    u16 = 0.0 if fmt == 'fp32' else nm.unit_roundoff(fmt)
    u_out = nm.unit_roundoff(fmt)
    e24 = 2.0 ** -24
    eps_s = (nm.C * np.sqrt(float(D)) * e24 * sabs + 4 * e24 * np.abs(s)).max(axis=1) + 4 * e24 * (s.max(axis=1) - s.min(axis=1))
    rel = u16 + np.expm1(2 * eps_s) + 4 * 2.0 ** -23 + nm.C * np.sqrt(float(Lk)) * e24
    return u_out * np.abs(y) + rel[:, None] * A + nm._TINY[nm._fmt(fmt)]



def check(got, ref, D, fmt, what):
    """Every element of `got` inside the bound; returns the worst err / bound."""
    got = np.asarray(got, dtype=np.float64)
    b = bound_for(ref, D, fmt)
    err = np.abs(got - ref[0])
    ratio = np.where(np.isfinite(err), err / b, np.inf)
    worst = float(ratio.max())
    assert worst <= 1.0, '%s (%s): %d of %d elements outside the bound, worst err / bound %.3g at %r' % (
        what, fmt, int((ratio > 1).sum()), ratio.size, worst, np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    return worst


def truncation_statistic(got, ref):
    """mean over all outputs of (got - ref) / A: about 0 for a P rounded to nearest, about -0.6 u16 for a truncated P (same-sign V)."""
    return float(np.mean((np.asarray(got, dtype=np.float64) - ref[0]) / ref[1]))


def round_fmt(a, fmt, truncate=False):
    """fp32 array rounded to `fmt` (to nearest even, or toward zero), returned as fp32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if fmt == 'fp32':
        return a
    t = torch.from_numpy(a)
    r = t.to(nm._fmt(fmt))
    if truncate:
        over = (r.float().abs() > t.abs()).to(torch.int16)
        r = (r.view(torch.int16) - over).view(nm._fmt(fmt))          # sign-magnitude: one unit less in magnitude
    return r.float().numpy()


DEFECTS = ('no_rescale', 'no_scale', 'pad_keys', 'neighbour_clip', 'truncate')


def simulate(q, k, v, scale, fmt, clips=1, tile=32, defect=None, drop=None):
    """The fused kernel in numpy fp32: per clip, key tiles of `tile` rows, running maximum and denominator per query row, P rounded to
    `fmt` for the PV product, the row sum from the unrounded p, one output rounding.  defect: one of DEFECTS; drop: index of a key
    tile that is skipped."""
    assert defect is None or defect in DEFECTS, defect
    f32 = np.float32
    q, k, v = (np.asarray(a, dtype=f32) for a in (q, k, v))
    L, Lk, D = q.shape[0] // clips, k.shape[0] // clips, q.shape[1]
    cst = f32(f32(1.0 if defect == 'no_scale' else scale) * f32(LOG2E))
    ys = []
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(clips):
            cc = (c + 1) % clips if defect == 'neighbour_clip' else c
            qc, kc, vc = q[c * L:(c + 1) * L], k[cc * Lk:(cc + 1) * Lk], v[cc * Lk:(cc + 1) * Lk]
            m = np.full(L, -np.inf, dtype=f32)
            l = np.zeros(L, dtype=f32)
            o = np.zeros((L, D), dtype=f32)
            for t in range((Lk + tile - 1) // tile):
                if drop == t:
                    continue
                n = min(tile, Lk - t * tile)
                kt, vt = np.zeros((tile, D), dtype=f32), np.zeros((tile, D), dtype=f32)
                kt[:n], vt[:n] = kc[t * tile:t * tile + n], vc[t * tile:t * tile + n]
                tt = (qc @ kt.T).astype(f32) * cst
                if defect != 'pad_keys':
                    tt[:, n:] = -np.inf
                m_new = np.maximum(m, tt.max(axis=1))
                alpha = np.exp2(m - m_new).astype(f32)
                if defect == 'no_rescale':
                    alpha = np.ones_like(alpha)
                p = np.exp2(tt - m_new[:, None]).astype(f32)
                l = (l * alpha + p.sum(axis=1, dtype=f32)).astype(f32)
                o = (o * alpha[:, None] + (round_fmt(p, fmt, truncate=defect == 'truncate') @ vt).astype(f32)).astype(f32)
                m = m_new
            ys.append(round_fmt(o / l[:, None], fmt))
    return np.concatenate(ys, axis=0).astype(np.float64)


# ---- the block on the oracle graph ---------------------------------------------------------------------------------------------------------
def parse_spec(spec):
    return [s.strip() for s in str(spec).split(',') if s.strip()]


class NetNonLocal(Net):
    """oracle.net3d.Net with a non-local block behind every body block named in `spec` ('res3_1,res4_0').  A block behind the last
    block of its stage takes the stage's output name (`res{S}_{n-1}_sum`; the body block's own sum becomes `..._sum_nl_in`), any other
    block writes `nonlocal_res{S}_{i}_sum`.  `self.keys_eff[nl]`: median over the query rows of exp(entropy of p)."""

    def __init__(self, weights, opts, spec, maxpool=True, use_scale=True):
        Net.__init__(self, weights, opts)
        self.nl_spec, self.nl_maxpool, self.nl_scale = set(parse_spec(spec)), maxpool, use_scale
        self.keys_eff, self.keys_total = {}, {}

    def _nonlocal(self, x, nl):
        one, zero = [1, 1, 1], [0, 0, 0]
        theta = self.conv_nd(x, nl + '_theta', one, one, zero)
        phi = self.conv_nd(x, nl + '_phi', one, one, zero)
        g = self.conv_nd(x, nl + '_g', one, one, zero)
        if self.nl_maxpool:
            phi = F.max_pool3d(phi, kernel_size=(1, 2, 2), stride=(1, 2, 2))
            g = F.max_pool3d(g, kernel_size=(1, 2, 2), stride=(1, 2, 2))
        N, D = theta.shape[:2]
        rows = lambda a: a.reshape(N, D, -1).transpose(1, 2)             # [N, T*H*W, D], rows in (t, h, w) order
        s = torch.matmul(rows(theta), rows(phi).transpose(1, 2)) * (D ** -0.5 if self.nl_scale else 1.0)
        p = torch.softmax(s.double(), dim=2)
        ent = -(p * torch.log(p.clamp_min(1e-300))).sum(dim=2)
        self.keys_eff[nl], self.keys_total[nl] = float(torch.exp(ent).median()), int(p.shape[2])
        y = torch.matmul(p.float(), rows(g)).transpose(1, 2).reshape(theta.shape)
        self.blobs[nl + '_y'] = y
        z = self.affine(self.conv_nd(y, nl + '_out', one, one, zero, bias=False), nl + '_out_bn')
        return z + x

    def _stage(self, x, stage_id, prefix, n, dim_in, dim_out, kt, stride_init=2):
        trans = self._basic if self.o['trans'] == 'basic' else self._bottleneck
        for i in range(n):
            p = '{}_{}'.format(prefix, i)
            stride = stride_init if (dim_in != dim_out and stage_id != 1) else 1
            tr = trans(x, p, stride, kt)
            if dim_in == dim_out:
                sc = x
            else:
                sc = self.affine(self.conv_nd(x, p + '_branch1', [1, 1, 1], [1, stride, stride], [0, 0, 0], bias=False), p + '_branch1_bn')
            x = F.relu(tr + sc)
            if p in self.nl_spec:
                nl = 'nonlocal_' + p
                if i == n - 1:
                    self.blobs[p + '_sum_nl_in'] = x
                    x = self._nonlocal(x, nl)
                    self.blobs[p + '_sum'] = x
                else:
                    self.blobs[p + '_sum'] = x
                    x = self._nonlocal(x, nl)
                    self.blobs[nl + '_sum'] = x
            else:
                self.blobs[p + '_sum'] = x
            dim_in = dim_out
        return x


def nonlocal_param_shapes(spec, opts):
    """name -> shape of the parameters of the blocks in `spec` (affine default): what the builder must create."""
    dims = opts['feat_dims']
    out = {}
    for p in parse_spec(spec):
        C = dims[int(p[3]) - 1]
        nl = 'nonlocal_' + p
        for b in ('_theta', '_phi', '_g'):
            out[nl + b + '_w'] = (C // 2, C, 1, 1, 1)
            out[nl + b + '_b'] = (C // 2,)
        out[nl + '_out_w'] = (C, C // 2, 1, 1, 1)
        out[nl + '_out_bn_s'] = (C,)
        out[nl + '_out_bn_b'] = (C,)
    return out
