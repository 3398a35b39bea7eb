"""Reference statements of the BACKWARD of the spacetime non-local block's attention (HIP.TRAIN_NONLOCAL) and of
its 2 x 2 max-pool.  The reference project has no such block: this is the project's own written definition.

  * `reference`: float64 gradients of  y = softmax(scale q k^T) v  per clip for an upstream dy,

        p = softmax_j(s),  s = scale q k^T,  dP = dy v^T,  delta_i = sum_d dy_id y_id,  dS = p (dP - delta)
        dv = p^T dy,       dq = scale dS k,   dk = scale dS^T q

    with the quantities the bound is made of, and lse_i = log2 sum_j exp(s_ij) (the kernel's units, c = scale log2(e)).
  * `bounds`: a per-element bound for dq, dk, dv of a kernel that recomputes p from a stored fp32 lse, from `tests/numerics` only
    (C = numerics.C, u = unit_roundoff, e24 = 2^-24, u16 = u(fmt) on the 16-bit path and 0 in fp32, u_y = u(fmt) of the STORED y):

        eps_s(i) = max_j[ C sqrt(D) e24 scale sum_d |q_id||k_jd| + 4 e24 |s_ij| ] + 4 e24 (max_j s_ij - min_j s_ij)
                   + 4 e24 (max_j |s_ij| + |ln 2 lse_i|)
        rel_p(i) = expm1(2 eps_s(i)) + 8 2^-23 + C sqrt(L') e24
        eP_ij    = C sqrt(D) e24 sum_d |dy_id||v_jd|
        eD_i     = (u_y + C sqrt(D) e24) sum_d |dy_id||y_id|
        eS_ij    = (rel_p(i) + u16) |dS_ij| + p_ij (eP_ij + eD_i + 4 e24 (|dP_ij| + |delta_i|)) + t16
        b_dv_jd  = u_out |dv| + sum_i ((rel_p(i) + u16 + C sqrt(L) e24) p_ij + t16) |dy_id| + tiny
        b_dq_id  = (u_out + 2 e24) |dq| + |scale| (sum_j eS_ij |k_jd| + C sqrt(L') e24 sum_j |dS_ij||k_jd|) + tiny
        b_dk_jd  = (u_out + 2 e24) |dk| + |scale| (sum_i eS_ij |q_id| + C sqrt(L)  e24 sum_i |dS_ij||q_id|) + tiny

    in order: the recomputed p -- the score error of the forward bound (fp32 accumulation over D, the fp32 constant, the subtraction) with
    the fp32 product c s and the stored fp32 lse added, entering p twice (through lse and directly); two hardware exps (the forward's
    denominator, the recomputation), the hardware log2 and the lse's fp32 sum over L'; P and dS rounded once to 16 bits (t16 = half the
    smallest subnormal of the 16-bit format, `_TINY`: the absolute error of that rounding below the normal range, which a dS of fp16
    reaches; 0 in fp32); delta from the
    stored, once-rounded y plus its fp32 accumulation over D; dP accumulated over D; the fp32 subtraction and product that make dS; the
    fp32 accumulation over L' (dq) or L (dk, dv); the fp32 multiplication by scale; one output rounding.
  * `lse_bound`: the fp32 lse against the float64 one.
  * `simulate`: an fp32 numpy simulation of the two kernels (query-stationary dq over key tiles, key-stationary dk / dv over query
    tiles, P and dS rounded to the 16-bit format before their products) with switchable defects, for tests/test_nonlocal_grad_cpu.py.
  * `maxpool_bwd`: the max-pool backward for non-overlapping windows; a tie sends the gradient to the first maximum in (h, w) scan order.
  * `GRAD_CASES` / `make_grad_case`: nonlocal_ref.CASES operands plus a seeded dy, shared by the CPU and GPU files.
"""
import zlib

import numpy as np

from tests import nonlocal_ref as R
from tests import numerics as nm

LOG2E = R.LOG2E
LN2 = 1.0 / LOG2E

# the backward cases: names of nonlocal_ref.CASES, plus one that crosses many tiles of both launches
EXTRA_CASES = {'many_tiles': (1, 4100, 1030, 64)}
GRAD_CASES = ('tiny', 'one_tile', 'ragged', 'blocks', 'growing', 'big', 'clips', 'd512', 'many_tiles')


def make_grad_case(name, fmt):
    """(q, k, v, dy, scale, clips): fp32 arrays already rounded to `fmt`."""
    if name in EXTRA_CASES:
        clips, L, Lk, D = EXTRA_CASES[name]
        rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)
        rnd = (lambda a: np.asarray(a, dtype=np.float32)) if fmt == 'fp32' else (lambda a: nm.q16(a, fmt))
        q, k, v, scale = rnd(rng.randn(clips * L, D)), rnd(rng.randn(clips * Lk, D)), rnd(rng.randn(clips * Lk, D)), D ** -0.5
    else:
        q, k, v, scale, clips = R.make_case(name, fmt)
    rng = np.random.RandomState(zlib.crc32(('dy_' + name).encode()) & 0x7fffffff)
    dy = rng.randn(*q.shape)
    dy = np.asarray(dy, dtype=np.float32) if fmt == 'fp32' else nm.q16(np.asarray(dy, dtype=np.float32), fmt)
    return q, k, v, dy, scale, clips


def make_same_sign_case(fmt, seed=5):
    """(q, k, v, dy, scale, 1) where every term dS_ij k_jd of dq has the same sign: P is near uniform (small q), v_j = b_j u with a random
    sign b_j and u in [0.5, 1.5], dy > 0, so dP_ij has the sign b_j and delta_i (a mean of balanced signs) is small; k_j = b_j |k|.  The
    mean signed error of dq then sees a dS that is truncated instead of rounded."""
    rng = np.random.RandomState(seed)
    L, Lk, D = 64, 300, 64
    b = np.where(np.arange(Lk) % 2 == 0, 1.0, -1.0)[:, None]
    q = 0.05 * rng.randn(L, D)
    k = b * rng.uniform(0.5, 1.5, size=(Lk, D))
    v = b * rng.uniform(0.5, 1.5, size=(Lk, D))
    dy = rng.uniform(0.5, 1.5, size=(L, D))
    rnd = (lambda a: np.asarray(a, dtype=np.float32)) if fmt == 'fp32' else (lambda a: nm.q16(np.asarray(a, dtype=np.float32), fmt))
    return rnd(q), rnd(k), rnd(v), rnd(dy), D ** -0.5, 1


def reference(q, k, v, dy, scale, clips=1):
    """float64 dict: dq, dk, dv, y, lse (log2 units of the kernel) and, per clip, the matrices the bound needs."""
    q, k, v, dy = (np.asarray(a, dtype=np.float64) for a in (q, k, v, dy))
    L, Lk = q.shape[0] // clips, k.shape[0] // clips
    out = {n: [] for n in ('dq', 'dk', 'dv', 'y', 'lse')}
    per_clip = []
    for c in range(clips):
        qc, kc, vc, dyc = q[c * L:(c + 1) * L], k[c * Lk:(c + 1) * Lk], v[c * Lk:(c + 1) * Lk], dy[c * L:(c + 1) * L]
        s = scale * (qc @ kc.T)
        m = s.max(axis=1, keepdims=True)
        e = np.exp(s - m)
        l = e.sum(axis=1, keepdims=True)
        p = e / l
        y = p @ vc
        dP = dyc @ vc.T
        delta = (dyc * y).sum(axis=1, keepdims=True)
        dS = p * (dP - delta)
        out['dq'].append(scale * (dS @ kc))
        out['dk'].append(scale * (dS.T @ qc))
        out['dv'].append(p.T @ dyc)
        out['y'].append(y)
        out['lse'].append(((m + np.log(l)) * LOG2E)[:, 0])
        per_clip.append(dict(q=qc, k=kc, v=vc, dy=dyc, s=s, p=p, y=y, dP=dP, delta=delta, dS=dS,
                             sabs=abs(scale) * (np.abs(qc) @ np.abs(kc).T)))
    ref = {n: np.concatenate(a, axis=0) for n, a in out.items()}
    ref['clips'], ref['scale'] = per_clip, scale
    return ref


def _eps_s(c, D):
    e24 = 2.0 ** -24
    s, lse_nat = c['s'], None
    m = s.max(axis=1)
    lse_nat = m + np.log(np.exp(s - m[:, None]).sum(axis=1))
    return ((nm.C * np.sqrt(float(D)) * e24 * c['sabs'] + 4 * e24 * np.abs(s)).max(axis=1) + 4 * e24 * (m - s.min(axis=1)) +
            4 * e24 * (np.abs(s).max(axis=1) + np.abs(lse_nat)))


def _rel_p(c, D):
    Lk = c['s'].shape[1]
    return np.expm1(2 * _eps_s(c, D)) + 8 * 2.0 ** -23 + nm.C * np.sqrt(float(Lk)) * 2.0 ** -24


def bounds(ref, fmt):
    """The per-element bounds of the module docstring: dict dq, dk, dv (arrays shaped like the gradients)."""
    u16 = 0.0 if fmt == 'fp32' else nm.unit_roundoff(fmt)
    u_out = u_y = nm.unit_roundoff(fmt)
    e24 = 2.0 ** -24
    tiny = nm._TINY[nm._fmt(fmt)]
    t16 = 0.0 if fmt == 'fp32' else tiny
    scale = abs(ref['scale'])
    bq, bk, bv = [], [], []
    for c in ref['clips']:
        L, Lk = c['s'].shape
        D = c['q'].shape[1]
        aD = nm.C * np.sqrt(float(D)) * e24
        rel = _rel_p(c, D)[:, None]
        p, dS = c['p'], c['dS']
        eP = aD * (np.abs(c['dy']) @ np.abs(c['v']).T)
        eD = (u_y + aD) * (np.abs(c['dy']) * np.abs(c['y'])).sum(axis=1, keepdims=True)
        eS = (rel + u16) * np.abs(dS) + p * (eP + eD + 4 * e24 * (np.abs(c['dP']) + np.abs(c['delta']))) + t16
        dq, dk, dv = scale * (dS @ c['k']), scale * (dS.T @ c['q']), p.T @ c['dy']
        bv.append(u_out * np.abs(dv) + ((rel + u16 + nm.C * np.sqrt(float(L)) * e24) * p + t16).T @ np.abs(c['dy']) + tiny)
        bq.append((u_out + 2 * e24) * np.abs(dq) + scale * (eS @ np.abs(c['k']) + nm.C * np.sqrt(float(Lk)) * e24 * (np.abs(dS) @ np.abs(c['k']))) + tiny)
        bk.append((u_out + 2 * e24) * np.abs(dk) + scale * (eS.T @ np.abs(c['q']) + nm.C * np.sqrt(float(L)) * e24 * (np.abs(dS).T @ np.abs(c['q']))) + tiny)
    return {'dq': np.concatenate(bq, axis=0), 'dk': np.concatenate(bk, axis=0), 'dv': np.concatenate(bv, axis=0)}


def lse_bound(ref):
    """Bound on |lse_fp32 - lse_float64| (log2 units): the score error and the relative error of the denominator (score error again, one
    hardware exp per term, the fp32 sum over L'), the hardware log2 and the fp32 sum m + log2(l)."""
    out = []
    for c in ref['clips']:
        D, Lk = c['q'].shape[1], c['s'].shape[1]
        eps = _eps_s(c, D)
        m = c['s'].max(axis=1) * LOG2E
        lse = m + np.log2(np.exp(c['s'] - c['s'].max(axis=1, keepdims=True)).sum(axis=1))
        out.append(LOG2E * (eps + np.expm1(2 * eps) + 2 * 2.0 ** -23 + nm.C * np.sqrt(float(Lk)) * 2.0 ** -24) +
                   4 * 2.0 ** -23 * (np.abs(m) + np.abs(lse - m) + np.abs(lse)) + 2.0 ** -126)
    return np.concatenate(out)


def check(got, ref, bnd, name, what, fmt):
    """Every element of `got` inside the bound `bnd[name]`; returns the worst err / bound."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref[name])
    ratio = np.where(np.isfinite(err), err / bnd[name], np.inf)
    worst = float(ratio.max())
    assert worst <= 1.0, '%s of %s (%s): %d of %d elements outside the bound, worst err / bound %.3g at %r' % (
        name, what, fmt, int((ratio > 1).sum()), ratio.size, worst, np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    return worst


def worst_ratio(got, ref, bnd, name):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref[name])
    return float(np.where(np.isfinite(err), err / bnd[name], np.inf).max())


def truncation_statistic(got_dq, ref):
    """mean over dq of (got - ref) / A, A = |scale| sum_j |dS_ij||k_jd|: about 0 for a dS rounded to nearest, clearly negative for a
    truncated one on the same-sign case (where A = dq)."""
    c = ref['clips'][0]
    A = abs(ref['scale']) * (np.abs(c['dS']) @ np.abs(c['k']))
    return float(np.mean((np.asarray(got_dq, dtype=np.float64) - ref['dq']) / A))


DEFECTS = ('rowmax', 'no_delta', 'no_scale_dq', 'no_scale_dk', 'neighbour_clip', 'truncate_ds')


def simulate(q, k, v, dy, scale, fmt, clips=1, tile=32, defect=None, drop_key=None, drop_query=None):
    """The two backward kernels in numpy fp32 -> (dq, dk, dv, lse) as float64 arrays.  The stored y and lse come from an fp32 forward
    (y rounded to `fmt`); delta from the stored y; dq walks key tiles of `tile` rows, dk / dv walk query tiles of `tile` rows; P and dS
    are rounded to `fmt` before their products.  defect: one of DEFECTS; drop_key / drop_query: index of a tile that is skipped."""
    assert defect is None or defect in DEFECTS, defect
    f32 = np.float32
    q, k, v, dy = (np.asarray(a, dtype=f32) for a in (q, k, v, dy))
    L, Lk, D = q.shape[0] // clips, k.shape[0] // clips, q.shape[1]
    cst = f32(f32(scale) * f32(LOG2E))
    sc = f32(scale)
    outs = [[], [], [], []]
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(clips):
            cc = (c + 1) % clips if defect == 'neighbour_clip' else c
            qc, dyc = q[c * L:(c + 1) * L], dy[c * L:(c + 1) * L]
            kf, vf = k[c * Lk:(c + 1) * Lk], v[c * Lk:(c + 1) * Lk]          # the forward always saw the clip's own keys
            kc, vc = k[cc * Lk:(cc + 1) * Lk], v[cc * Lk:(cc + 1) * Lk]
            t = (qc @ kf.T).astype(f32) * cst
            m = t.max(axis=1)
            pf = np.exp2(t - m[:, None]).astype(f32)
            l = pf.sum(axis=1, dtype=f32)
            y = R.round_fmt((R.round_fmt(pf, fmt) @ vf).astype(f32) / l[:, None], fmt)
            lse = (m + np.log2(l).astype(f32)).astype(f32)
            stat = m if defect == 'rowmax' else lse
            delta = np.zeros(L, dtype=f32) if defect == 'no_delta' else (dyc * y).sum(axis=1, dtype=f32)

            def tile_terms(qs, ds_rows, ks):
                """p and dS of query rows `qs` against key rows `ks` (index arrays)"""
                tt = ((qc[qs] @ kc[ks].T).astype(f32) * cst - stat[qs][:, None]).astype(f32)
                p = np.exp2(tt).astype(f32)
                dP = (dyc[qs] @ vc[ks].T).astype(f32)
                dS = (p * (dP - delta[qs][:, None])).astype(f32)
                return p, dS

            allq, allk = np.arange(L), np.arange(Lk)
            dq = np.zeros((L, D), dtype=f32)
            for tk in range((Lk + tile - 1) // tile):
                if drop_key == tk:
                    continue
                ks = allk[tk * tile:(tk + 1) * tile]
                _, dS = tile_terms(allq, None, ks)
                dq = (dq + (R.round_fmt(dS, fmt, truncate=defect == 'truncate_ds') @ kc[ks]).astype(f32)).astype(f32)
            dk, dv = np.zeros((Lk, D), dtype=f32), np.zeros((Lk, D), dtype=f32)
            for tq in range((L + tile - 1) // tile):
                if drop_query == tq:
                    continue
                qs = allq[tq * tile:(tq + 1) * tile]
                p, dS = tile_terms(qs, None, allk)
                dv = (dv + (R.round_fmt(p, fmt).T @ dyc[qs]).astype(f32)).astype(f32)
                dk = (dk + (R.round_fmt(dS, fmt, truncate=defect == 'truncate_ds').T @ qc[qs]).astype(f32)).astype(f32)
            outs[0].append(R.round_fmt(dq * (f32(1.0) if defect == 'no_scale_dq' else sc), fmt))
            outs[1].append(R.round_fmt(dk * (f32(1.0) if defect == 'no_scale_dk' else sc), fmt))
            outs[2].append(R.round_fmt(dv, fmt))
            outs[3].append(lse)
    return tuple(np.concatenate(o, axis=0).astype(np.float64) for o in outs)


def maxpool_bwd(x, dy, k, stride, pad):
    """x [f, h, w, c], dy [f, ho, wo, c] -> dx like x (float64): non-overlapping windows (k <= stride); the FIRST maximum of a window in
    (h, w) scan order takes its gradient; positions outside every window get zero."""
    assert 1 <= k <= stride and 0 <= pad < k
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    f, h, w, c = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    assert dy.shape == (f, ho, wo, c), (dy.shape, (f, ho, wo, c))
    dx = np.zeros_like(x)
    fi, ci = np.meshgrid(np.arange(f), np.arange(c), indexing='ij')
    for oh in range(ho):
        for ow in range(wo):
            pos = [(ih, iw) for ih in range(oh * stride - pad, oh * stride - pad + k) for iw in range(ow * stride - pad, ow * stride - pad + k)
                   if 0 <= ih < h and 0 <= iw < w]
            win = np.stack([x[:, ih, iw, :] for ih, iw in pos], axis=0)           # [positions, f, c] in scan order
            first = np.argmax(win, axis=0)                                       # the first maximum
            ihs = np.asarray([p[0] for p in pos])[first]
            iws = np.asarray([p[1] for p in pos])[first]
            dx[fi, ihs, iws, ci] = dy[:, oh, ow, :]
    return dx
