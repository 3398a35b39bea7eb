"""The four SpatialBN kernels (csrc/batch_norm.hip) through the C ABI against float64 NumPy, in fp32 and in the build's 16-bit format.

Bounds (derived in tests/spatial_bn_ref.py, from `numerics.sum_bound` / `numerics.bound` only):
  * mu and the sums db, ds: `sum_bound` over their M (or window) terms;
  * rstd, a, b', the running statistics: first-order propagation of d_mu and d_M2 = sum_bound(M2, M);
  * y: `assert_elementwise` with K = 2 (y = z a + b', the form the kernel evaluates, on absref = |z a| + |b'| + |res|) and
    extra = |s rstd| d_mu + |s (z - mu)| d_rstd -- the first-order propagation of the mu and M2 sum bounds through rstd:
    dy/dmu = -s rstd, dy/drstd = s (z - mu), d_rstd = 1/2 rstd^3 d_M2 / M + 2 u rstd;
  * dz: the backward kernels are given the saved statistics and the sums as fp32 INPUTS and the float64 reference is computed from
    those same values, so `assert_elementwise` with K = 3 on absref = |a| (|g| + |db| / M + |xhat ds| / M) has no extra term.
"""
import numpy as np
import pytest
import torch

from tests import numerics as nm
from tests import spatial_bn_ref as ref

pytestmark = pytest.mark.gpu
EPS, MOM = 1.0000001e-05, 0.9
U = ref.U32

#        frames H    W    C    cstride
CASES = {'baseline': (2, 5, 7, 64, 64),
         'padding': (2, 5, 7, 24, 64),
         'odd_three_chunks': (3, 37, 53, 192, 192),
         'many_blocks': (8, 96, 168, 64, 64),
         'm2': (1, 1, 2, 64, 64),
         'offset': (2, 16, 16, 64, 64)}


@pytest.fixture(scope='module')
def ops():
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


_CACHE = {}


def _case(name, dtype_name):
    """Inputs of one case, made once: z / res / dy quantised to the tensor format, parameters fp32; float64 statistics."""
    key = (name, dtype_name)
    if key not in _CACHE:
        f, H, W, C, cs = CASES[name]
        rs = np.random.RandomState(sum(map(ord, name)))
        M = f * H * W
        q = (lambda a: nm.q16(a)) if dtype_name == 'h16' else (lambda a: a.astype(np.float32))
        z = ref.offset_case(C=C) if name == 'offset' else (rs.randn(M, C) * rs.uniform(0.5, 3.0, C) + rs.randn(C) * 2).astype(np.float32)
        z = q(z)
        d = dict(z=z, res=q(rs.randn(M, C).astype(np.float32)), dy=q((rs.randn(M, C) * 0.1).astype(np.float32)),
                 s=rs.uniform(0.5, 1.5, C).astype(np.float32), b=(rs.randn(C) * 0.3).astype(np.float32),
                 rm=(rs.randn(C) * 0.2).astype(np.float32), riv=rs.uniform(0.5, 1.5, C).astype(np.float32), M=M, shape=(f, H, W, C, cs))
        d.update(ref.stats_ref64(z, EPS))
        _CACHE[key] = d
    return _CACHE[key]


def _dev(ops, a, shape, dtype_name, junk=1000.0):
    """[M, C] host matrix -> device blob [frames, H, W, cs]; the padding channels hold junk that must never be read into a result."""
    f, H, W, C, cs = shape
    t = torch.full((f * H * W, cs), junk, dtype=torch.float32)
    t[:, :C] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.view(f, H, W, cs).to(nm.h16() if dtype_name == 'h16' else torch.float32).cuda()


def _host(t, C):
    return t.float().cpu().numpy().reshape(-1, t.shape[-1])[:, :C].astype(np.float64), t.float().cpu().numpy().reshape(-1, t.shape[-1])[:, C:]


def _fmt(dtype_name):
    return nm.h16() if dtype_name == 'h16' else torch.float32


def _dt(ops, dtype_name):
    return ops.BF16 if dtype_name == 'h16' else ops.F32


def _vec(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_stats_and_apply_against_float64(ops, name, dtype_name):
    c = _case(name, dtype_name)
    f, H, W, C, cs = c['shape']
    M, dt = c['M'], _dt(ops, dtype_name)
    z = _dev(ops, c['z'], c['shape'], dtype_name)
    rm, riv = _vec(c['rm']), _vec(c['riv'])
    st = ops.bn_stats(z, dt, C, _vec(c['s']), _vec(c['b']), EPS, MOM, rm, riv)
    rm2, riv2 = _vec(c['rm']), _vec(c['riv'])
    st2 = ops.bn_stats(z, dt, C, _vec(c['s']), _vec(c['b']), EPS, MOM, rm2, riv2)
    torch.cuda.synchronize()
    assert torch.equal(st, st2) and torch.equal(rm, rm2) and torch.equal(riv, riv2), 'the same input gave different bits'
    got = st.cpu().numpy().astype(np.float64)
    assert np.all(got[:, C:] == 0), 'padding channels of the statistics are not zero'
    d_mu, d_var, d_rstd = ref.stats_bounds(c['z'], EPS)
    mu, rstd, s, b = c['mu'], c['rstd'], c['s'].astype(np.float64), c['b'].astype(np.float64)
    worst = lambda e, bd: float(np.max(e / bd))
    e_mu, e_rstd = np.abs(got[0, :C] - mu), np.abs(got[1, :C] - rstd)
    print('%s %s: mu err/bound %.3f, rstd err/bound %.3f' % (name, dtype_name, worst(e_mu, d_mu), worst(e_rstd, d_rstd)))
    assert np.all(e_mu <= d_mu), 'mean: worst err/bound %.3g' % worst(e_mu, d_mu)
    assert np.all(e_rstd <= d_rstd), 'rstd: worst err/bound %.3g' % worst(e_rstd, d_rstd)
    a_ref = s * rstd
    b_a = np.abs(s) * d_rstd + U * np.abs(a_ref)
    assert np.all(np.abs(got[2, :C] - a_ref) <= b_a)
    assert np.all(np.abs(got[3, :C] - (b - mu * a_ref)) <= np.abs(a_ref) * d_mu + np.abs(mu) * b_a + 2 * U * (np.abs(b) + np.abs(mu * a_ref)))
    # running statistics: rm <- m rm + (1 - m) mu, riv <- m riv + (1 - m) var M / (M - 1)
    rm_ref = MOM * c['rm'].astype(np.float64) + (1 - MOM) * mu
    riv_ref = MOM * c['riv'].astype(np.float64) + (1 - MOM) * c['var'] * M / (M - 1)
    assert np.all(np.abs(rm.cpu().numpy() - rm_ref) <= (1 - MOM) * d_mu + 3 * U * (np.abs(MOM * c['rm']) + np.abs((1 - MOM) * mu)))
    assert np.all(np.abs(riv.cpu().numpy() - riv_ref) <= (1 - MOM) * d_var * M / (M - 1) + 4 * U * np.abs(riv_ref))
    # apply, with the kernel's own pair: plain, and residual + ReLU
    fmt = _fmt(dtype_name)
    y = ops.bn_apply(z, dt, C, st[2], st[3])
    yv, ypad = _host(y, C)
    assert np.all(ypad == 0), 'padding channels of y are not zero'
    ref.check_forward(yv, c['z'], s, b, EPS, fmt, '%s y' % name)
    res = _dev(ops, c['res'], c['shape'], dtype_name)
    y2 = ops.bn_apply(z, dt, C, st[2], st[3], relu=True, residual=res)
    y2v, y2pad = _host(y2, C)
    assert np.all(y2pad == 0) and (y2v == 0).any() and (y2v > 0).any()
    ref.check_forward(y2v, c['z'], s, b, EPS, fmt, '%s relu(y + res)' % name, res=c['res'].astype(np.float64), relu=True)
    # aliasing: in place over z, and with the residual aliasing the output
    zc, rc = z.clone(), res.clone()
    assert torch.equal(ops.bn_apply(zc, dt, C, st[2], st[3], relu=True, residual=res, out=zc), y2)
    assert torch.equal(ops.bn_apply(z, dt, C, st[2], st[3], relu=True, residual=rc, out=rc), y2)


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_one_position_per_channel_is_an_argument_error(ops, dtype_name):
    from detectandtrack_amd.libdat import DatError
    dt = _dt(ops, dtype_name)
    z = torch.zeros((1, 1, 1, 64), dtype=_fmt(dtype_name), device='cuda')
    one = torch.ones(64, device='cuda')
    with pytest.raises(DatError, match='at least 2 positions'):
        ops.bn_stats(z, dt, 64, one, one, EPS, MOM, one.clone(), one.clone())


def _backward(ops, name, dtype_name, lo, n):
    c = _case(name, dtype_name)
    f, H, W, C, cs = c['shape']
    M, dt, fmt, per = c['M'], _dt(ops, dtype_name), _fmt(dtype_name), H * W
    s = c['s'].astype(np.float64)
    # the saved statistics as fp32 values: inputs of the kernels AND of the reference
    mu32, rstd32 = c['mu'].astype(np.float32), c['rstd'].astype(np.float32)
    a32 = (c['s'] * rstd32).astype(np.float32)
    pad = lambda v: _vec(np.concatenate([v, np.zeros(cs - C, np.float32)]))
    y_host = nm.q16(np.maximum(ref.forward_ref64(c['z'], s, c['b'].astype(np.float64), EPS, c['res'].astype(np.float64))[0], 0)) \
        if dtype_name == 'h16' else np.maximum(ref.forward_ref64(c['z'], s, c['b'].astype(np.float64), EPS, c['res'].astype(np.float64))[0], 0).astype(np.float32)
    z, y = _dev(ops, c['z'], c['shape'], dtype_name), _dev(ops, y_host, c['shape'], dtype_name)
    dy_host = c['dy'][lo * per:(lo + n) * per]
    dy = _dev(ops, dy_host, (n, H, W, C, cs), dtype_name)
    r = ref.backward_ref64(dy_host, y_host, c['z'], a32.astype(np.float64) / rstd32, mu32.astype(np.float64), rstd32.astype(np.float64),
                           lo * per, n * per, True)
    pre_b, pre_g = np.linspace(-1, 1, C).astype(np.float32), np.linspace(2, 3, C).astype(np.float32)
    dbeta, dgamma = _vec(pre_b), _vec(pre_g)
    g, sums = ops.bn_bwd_reduce(dy, y, z, dt, C, pad(mu32), pad(rstd32), frame_lo=lo, relu=True, dbeta=dbeta, dgamma=dgamma)
    gv, gpad = _host(g, C)
    assert np.all(gpad == 0) and np.array_equal(gv, r['g']), 'g is not dy masked by y > 0'
    sm = sums.cpu().numpy().astype(np.float64)
    assert np.all(sm[:, C:] == 0)
    for ch in range(C):
        nm.assert_sum(sm[0, ch], r['db'][ch], r['abs_db'][ch], n * per, '%s db[%d]' % (name, ch))
        nm.assert_sum(sm[1, ch], r['ds'][ch], r['abs_ds'][ch], n * per, '%s ds[%d]' % (name, ch))
    # the caller's gradient buffers ACCUMULATE (the convention of dbias in dat_relu_bias_bwd)
    assert np.array_equal(dbeta.cpu().numpy(), pre_b + sums[0, :C].cpu().numpy()) and np.array_equal(dgamma.cpu().numpy(), pre_g + sums[1, :C].cpu().numpy())
    g_alias, sums_alias = ops.bn_bwd_reduce(dy, y, z, dt, C, pad(mu32), pad(rstd32), frame_lo=lo, relu=True, inplace=True)
    assert g_alias.data_ptr() == dy.data_ptr() and torch.equal(g_alias, g) and torch.equal(sums_alias, sums)
    # dz on EVERY frame, from the kernel's sums taken as exact inputs
    dz = ops.bn_bwd_apply(g, z, dt, C, pad(mu32), pad(rstd32), pad(a32), sums, frame_lo=lo)
    assert tuple(dz.shape) == tuple(z.shape)
    dzv, dzpad = _host(dz, C)
    assert np.all(dzpad == 0)
    gf = np.zeros((M, C))
    gf[lo * per:(lo + n) * per] = r['g']
    a64 = a32.astype(np.float64)
    dz_ref = a64 * (gf - sm[0, :C] / M - r['xh'] * sm[1, :C] / M)
    absdz = np.abs(a64) * (np.abs(gf) + np.abs(sm[0, :C]) / M + np.abs(r['xh'] * sm[1, :C]) / M)
    nm.assert_elementwise(dzv, dz_ref, absdz, 3, fmt, '%s dz' % name)
    return dzv, lo * per, (lo + n) * per


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_backward_over_the_whole_blob_against_float64(ops, name, dtype_name):
    _backward(ops, name, dtype_name, 0, CASES[name][0])


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_backward_of_a_frame_window_fills_every_frame(ops, dtype_name):
    """The gradient covers frame 1 of 3: db / ds are the full-blob sums with g = 0 outside the window, and dz -- checked on ALL frames --
    does not vanish outside it."""
    dz, r0, r1 = _backward(ops, 'odd_three_chunks', dtype_name, 1, 1)
    outside = np.concatenate([dz[:r0], dz[r1:]])
    assert np.count_nonzero(outside) > 0.9 * outside.size
