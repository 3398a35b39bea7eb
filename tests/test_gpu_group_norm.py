"""The GroupNorm kernels (csrc/group_norm.hip, csrc/norm_kernels.h) through the C ABI against float64 NumPy, in fp32 and in the build's
16-bit format.  Shapes: the smallest at which the kernels can go wrong (several groups inside one thread's vector, a group that is a
whole 64-channel chunk, groups that straddle the chunks next to padding channels, one padded group, a wide group over many chunks,
several clips with very different means, more row blocks than one, two values per group, a mean far from zero).

Bounds (derived in tests/group_norm_ref.py, from `numerics.sum_bound` / `numerics.bound` only):
  * mu: `sum_bound` over the Mg = M cg terms of the group; rstd, a, b': first-order propagation of d_mu and d_M2 = sum_bound(M2, Mg);
  * y: `assert_elementwise` with K = 2 (y = z a + b', the form the kernel evaluates, on absref = |z a| + |b'| + |res|) and
    extra = |s rstd| d_mu + |s (z - mu)| d_rstd;
  * S1 = sum g, S2 = sum g xhat per (clip, channel): `sum_bound` over the window's rows; dbeta / dgamma: EXACTLY the fp32 sum over the
    clips, in clip order, added to what the buffer held;
  * the backward kernels are given the saved tables as fp32 INPUTS and the float64 reference is computed from those same values and
    from the sums the kernel returned: the group coefficients q, r carry the sum bound of their cg-term sums A, B, and dz is held to
    K = 3 on absref = |a g| + |q| + |r (z - mu)| with extra = d_q + |z - mu| d_r.
Every test prints its worst err / bound.

Edges of the 16-bit formats (tests/fp16_edge_cases.py), in fp32 and the build's 16-bit format on `two_per_group` and `straddle`: inputs
in the fp16 subnormal range, outputs on and beyond the largest finite half (exact tables, so the stored value is torch's conversion
of a known fp32 value), and a mean of 3e4.
"""
import numpy as np
import pytest
import torch

from tests import fp16_edge_cases as fe
from tests import numerics as nm
from tests import group_norm_ref as ref

pytestmark = pytest.mark.gpu
EPS = 1e-5
U = ref.U32

#        clips frames H   W   C    cstride G
CASES = {'two_per_group': (1, 2, 5, 7, 64, 64, 32),
         'group_is_chunk': (1, 2, 5, 7, 128, 128, 2),
         'straddle': (1, 2, 5, 7, 144, 192, 24),
         'one_group_padded': (1, 2, 5, 7, 24, 64, 1),
         'wide_group': (1, 1, 3, 4, 921, 960, 3),
         'clips': (3, 2, 5, 7, 64, 64, 32),
         'many_blocks': (2, 4, 48, 84, 64, 64, 32),
         'tiny': (1, 1, 1, 1, 64, 64, 32),
         'offset': (1, 2, 16, 16, 64, 64, 32),
         'window': (1, 3, 5, 7, 144, 192, 24)}      # (the frame-window test's clip)
SWEEP = sorted(set(CASES) - {'window'})
CLIP_MEANS = (100.0, -50.0, 0.0)


@pytest.fixture(scope='module')
def ops():
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


_CACHE = {}


def _case(name, dtype_name):
    """Inputs of one case, made once: z / res / dy quantised to the tensor format ([clips, M, C]), parameters fp32; float64 tables."""
    key = (name, dtype_name)
    if key not in _CACHE:
        N, f, H, W, C, cs, G = CASES[name]
        rs = np.random.RandomState(sum(map(ord, name)))
        M = f * H * W
        q = (lambda a: nm.q16(a)) if dtype_name == 'h16' else (lambda a: a.astype(np.float32))
        if name == 'offset':
            z = ref.offset_case(C=C)
        else:
            z = rs.randn(N, M, C) * rs.uniform(0.5, 3.0, C) + rs.randn(C) * 2
            if name == 'clips':         # statistics shared across clips would be off by tens of standard deviations
                z = z + np.array(CLIP_MEANS)[:, None, None]
        z = q(z.astype(np.float32))
        d = dict(z=z, res=q(rs.randn(N, M, C).astype(np.float32)), dy=q((rs.randn(N, M, C) * 0.1).astype(np.float32)),
                 s=rs.uniform(0.5, 1.5, C).astype(np.float32), b=(rs.randn(C) * 0.3).astype(np.float32), M=M, shape=CASES[name])
        d['tables'], d['dtables'] = ref.table_bounds(z, G, d['s'].astype(np.float64), d['b'].astype(np.float64), EPS)
        _CACHE[key] = d
    return _CACHE[key]


def _dev(a, shape, dtype_name, frames=None, junk=1000.0):
    """[clips, M', C] host array -> device blob [clips * frames, H, W, cs]; the padding channels hold junk that must never be read into
    a result."""
    N, f, H, W, C, cs, _ = shape
    f = f if frames is None else frames
    t = torch.full((N * f * H * W, cs), junk, dtype=torch.float32)
    t[:, :C] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, C))
    return t.view(N * f, H, W, cs).to(nm.h16() if dtype_name == 'h16' else torch.float32).cuda()


def _host(t, N, C):
    """device blob -> (real channels [clips, M, C] float64, padding channels)"""
    a = t.float().cpu().numpy().reshape(N, -1, t.shape[-1])
    return a[:, :, :C].astype(np.float64), a[:, :, C:]


def _fmt(dtype_name):
    return nm.h16() if dtype_name == 'h16' else torch.float32


def _dt(ops, dtype_name):
    return ops.BF16 if dtype_name == 'h16' else ops.F32


def _vec(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _worst(err, bd):
    return float(np.max(err / bd))


def _forward(ops, name, dtype_name):
    c = _case(name, dtype_name)
    N, f, H, W, C, cs, G = c['shape']
    z = _dev(c['z'], c['shape'], dtype_name)
    st = ops.gn_stats(z, _dt(ops, dtype_name), C, G, _vec(c['s']), _vec(c['b']), EPS, clips=N)
    return c, z, st


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
@pytest.mark.parametrize('name', SWEEP)
def test_stats_and_apply_against_float64(ops, name, dtype_name):
    c, z, st = _forward(ops, name, dtype_name)
    N, f, H, W, C, cs, G = c['shape']
    dt, fmt = _dt(ops, dtype_name), _fmt(dtype_name)
    st2 = ops.gn_stats(z, dt, C, G, _vec(c['s']), _vec(c['b']), EPS, clips=N)
    torch.cuda.synchronize()
    assert tuple(st.shape) == (4, N, cs) and torch.equal(st, st2), 'the same input gave different bits'
    got = st.cpu().numpy().astype(np.float64)
    assert np.all(got[:, :, C:] == 0), 'padding channels of the tables are not zero'
    ratios = []
    for k, label in enumerate(('mean', 'rstd', 'a', "b'")):
        err, bd = np.abs(got[k, :, :C] - c['tables'][k]), c['dtables'][k]
        ratios.append(_worst(err, bd))
        assert np.all(err <= bd), '%s %s: worst err/bound %.3g' % (name, label, ratios[-1])
    cg = C // G
    assert all(np.all(got[k, :, :C].reshape(N, G, cg) == got[k, :, :C].reshape(N, G, cg)[:, :, :1]) for k in (0, 1)), \
        'mean / rstd differ inside a group'
    # apply, with the kernel's own pair: plain, and residual + ReLU
    s, b = c['s'].astype(np.float64), c['b'].astype(np.float64)
    y = ops.gn_apply(z, dt, C, st[2], st[3], clips=N)
    yv, ypad = _host(y, N, C)
    assert np.all(ypad == 0), 'padding channels of y are not zero'
    w1 = ref.check_forward(yv, c['z'], G, s, b, EPS, fmt, '%s y' % name)
    res = _dev(c['res'], c['shape'], dtype_name)
    y2 = ops.gn_apply(z, dt, C, st[2], st[3], clips=N, relu=True, residual=res)
    y2v, y2pad = _host(y2, N, C)
    assert np.all(y2pad == 0) and (y2v == 0).any() and (y2v > 0).any()
    w2 = ref.check_forward(y2v, c['z'], G, s, b, EPS, fmt, '%s relu(y + res)' % name, res=c['res'].astype(np.float64), relu=True)
    print('%s %s: err/bound mean %.3f rstd %.3f a %.3f b\' %.3f y %.3f relu(y+res) %.3f' % ((name, dtype_name) + tuple(ratios) + (w1, w2)))
    assert torch.equal(ops.gn_apply(z, dt, C, st[2], st[3], clips=N), y), 'the same input gave different bits'
    # aliasing: in place over z, and with the residual aliasing the output
    zc, rc = z.clone(), res.clone()
    assert torch.equal(ops.gn_apply(zc, dt, C, st[2], st[3], clips=N, relu=True, residual=res, out=zc), y2)
    assert torch.equal(ops.gn_apply(z, dt, C, st[2], st[3], clips=N, relu=True, residual=rc, out=rc), y2)


def _backward(ops, name, dtype_name, lo, n):
    c = _case(name, dtype_name)
    N, f, H, W, C, cs, G = c['shape']
    M, dt, fmt, per = c['M'], _dt(ops, dtype_name), _fmt(dtype_name), H * W
    s, b = c['s'].astype(np.float64), c['b'].astype(np.float64)
    # the saved tables as fp32 values: inputs of the kernels AND of the reference
    mu32, rstd32 = c['tables'][0].astype(np.float32), c['tables'][1].astype(np.float32)
    a32 = (c['s'] * rstd32).astype(np.float32)
    pad = lambda v: _vec(np.concatenate([v, np.zeros((N, cs - C), np.float32)], axis=1))
    y64 = np.maximum(ref.forward_ref64(c['z'], G, s, b, EPS, c['res'].astype(np.float64))[0], 0)
    y_host = nm.q16(y64) if dtype_name == 'h16' else y64.astype(np.float32)
    z, y = _dev(c['z'], c['shape'], dtype_name), _dev(y_host, c['shape'], dtype_name)
    dy_host = c['dy'][:, lo * per:(lo + n) * per]
    dy = _dev(dy_host, c['shape'], dtype_name, frames=n)
    mu64, rstd64 = mu32.astype(np.float64), rstd32.astype(np.float64)
    r = ref.backward_sums_ref64(dy_host, y_host, c['z'], mu64, rstd64, lo * per, n * per, True)
    pre_b, pre_g = np.linspace(-1, 1, C).astype(np.float32), np.linspace(2, 3, C).astype(np.float32)
    dbeta, dgamma = _vec(pre_b), _vec(pre_g)
    args = (dy, y, z, dt, C, G, pad(mu32), pad(rstd32), _vec(c['s']))
    g, sums, coef = ops.gn_bwd_reduce(*args, clips=N, frame_lo=lo, relu=True, dbeta=dbeta, dgamma=dgamma)
    gv, gpad = _host(g, N, C)
    assert np.all(gpad == 0) and np.array_equal(gv, r['g']), 'g is not dy masked by y > 0'
    sm = sums.cpu().numpy()
    assert sm.shape == (N, 2, cs) and np.all(sm[:, :, C:] == 0)
    sm64 = sm.astype(np.float64)
    bd1 = np.vectorize(lambda v: nm.sum_bound(v, n * per))(r['abs_S1'])
    bd2 = np.vectorize(lambda v: nm.sum_bound(v, n * per))(r['abs_S2'])
    e1, e2 = np.abs(sm64[:, 0, :C] - r['S1']), np.abs(sm64[:, 1, :C] - r['S2'])
    assert np.all(e1 <= bd1) and np.all(e2 <= bd2), '%s: sum g err/bound %.3g, sum g xhat err/bound %.3g' % (name, _worst(e1, bd1), _worst(e2, bd2))
    # the caller's gradient buffers ACCUMULATE (the convention of dbias in dat_relu_bias_bwd) the fp32 sum over the clips, in clip order
    tb, ts = np.zeros(C, np.float32), np.zeros(C, np.float32)
    for k in range(N):
        tb, ts = tb + sm[k, 0, :C], ts + sm[k, 1, :C]
    assert np.array_equal(dbeta.cpu().numpy(), pre_b + tb) and np.array_equal(dgamma.cpu().numpy(), pre_g + ts)
    g_alias, sums_alias, coef_alias = ops.gn_bwd_reduce(dy.clone(), y, z, dt, C, G, pad(mu32), pad(rstd32), _vec(c['s']), clips=N,
                                                        frame_lo=lo, relu=True)
    assert torch.equal(g_alias, g) and torch.equal(sums_alias, sums) and torch.equal(coef_alias, coef), 'the same input gave different bits'
    dyc = dy.clone()
    g_in, _, _ = ops.gn_bwd_reduce(dyc, y, z, dt, C, G, pad(mu32), pad(rstd32), _vec(c['s']), clips=N, frame_lo=lo, relu=True, inplace=True)
    assert g_in.data_ptr() == dyc.data_ptr() and torch.equal(g_in, g)
    # the group coefficients and dz on EVERY frame, from the kernel's sums taken as exact inputs
    dz_ref, absdz, extra, (q, rr, d_q, d_r) = ref.backward_dz_ref64(r['g'], c['z'], G, s, mu64, rstd64, sm64[:, 0, :C], sm64[:, 1, :C],
                                                                   lo * per, a=a32)
    cf = coef.cpu().numpy().astype(np.float64)
    assert cf.shape == (N, 2, cs) and np.all(cf[:, :, C:] == 0)
    eq, er = np.abs(cf[:, 0, :C] - q), np.abs(cf[:, 1, :C] - rr)
    assert np.all(eq <= d_q) and np.all(er <= d_r), '%s: q err/bound %.3g, r err/bound %.3g' % (name, _worst(eq, d_q), _worst(er, d_r))
    dz = ops.gn_bwd_apply(g, z, dt, C, pad(mu32), pad(a32), coef, clips=N, frame_lo=lo)
    assert tuple(dz.shape) == tuple(z.shape)
    dzv, dzpad = _host(dz, N, C)
    assert np.all(dzpad == 0)
    nm.assert_elementwise(dzv, dz_ref, absdz, 3, fmt, '%s dz' % name, extra=extra)
    wdz = _worst(np.abs(dzv - dz_ref), nm.bound(dz_ref, absdz, 3, fmt, extra))
    print('%s %s: err/bound sum g %.3f, sum g xhat %.3f, q %.3f, r %.3f, dz %.3f' % (name, dtype_name, _worst(e1, bd1), _worst(e2, bd2),
                                                                                  _worst(eq, d_q), _worst(er, d_r), wdz))
    assert torch.equal(ops.gn_bwd_apply(g, z, dt, C, pad(mu32), pad(a32), coef, clips=N, frame_lo=lo), dz), 'the same input gave different bits'
    return dzv, lo * per, (lo + n) * per


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
@pytest.mark.parametrize('name', SWEEP)
def test_backward_over_every_frame_against_float64(ops, name, dtype_name):
    _backward(ops, name, dtype_name, 0, CASES[name][1])


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_backward_of_a_frame_window_fills_every_frame(ops, dtype_name):
    """The gradient covers frame 1 of 3 of one clip: the sums are the clip's sums with g = 0 outside the window, and dz -- checked on ALL
    frames -- does not vanish outside it."""
    dz, r0, r1 = _backward(ops, 'window', dtype_name, 1, 1)
    outside = np.concatenate([dz[:, :r0], dz[:, r1:]], axis=1)
    assert np.count_nonzero(outside) > 0.9 * outside.size


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_every_clip_keeps_the_bits_it_gets_alone(ops, dtype_name):
    """Three clips with means near +100, -50 and 0 in one call: tables, y, g, sums, coefficients and dz of each clip equal bit for bit what
    the clip yields as a blob of its own."""
    c, z, st = _forward(ops, 'clips', dtype_name)
    N, f, H, W, C, cs, G = c['shape']
    dt = _dt(ops, dtype_name)
    s, b = _vec(c['s']), _vec(c['b'])
    res, dy = _dev(c['res'], c['shape'], dtype_name), _dev(c['dy'], c['shape'], dtype_name)
    y = ops.gn_apply(z, dt, C, st[2], st[3], clips=N, relu=True, residual=res)
    g, sums, coef = ops.gn_bwd_reduce(dy, y, z, dt, C, G, st[0], st[1], s, clips=N, relu=True)
    dz = ops.gn_bwd_apply(g, z, dt, C, st[0], st[2], coef, clips=N)
    means = st[0, :, :C].cpu().numpy().mean(axis=1)
    assert np.all(np.abs(means - (np.array(CLIP_MEANS) + means[2])) < 3), means
    for k in range(N):
        fr = slice(k * f, (k + 1) * f)
        zk, rk, dk = z[fr].contiguous(), res[fr].contiguous(), dy[fr].contiguous()
        stk = ops.gn_stats(zk, dt, C, G, s, b, EPS, clips=1)
        assert torch.equal(stk[:, 0], st[:, k]), 'tables of clip %d depend on the other clips' % k
        yk = ops.gn_apply(zk, dt, C, stk[2], stk[3], clips=1, relu=True, residual=rk)
        assert torch.equal(yk, y[fr]), 'y of clip %d depends on the other clips' % k
        gk, sk, ck = ops.gn_bwd_reduce(dk, yk, zk, dt, C, G, stk[0], stk[1], s, clips=1, relu=True)
        assert torch.equal(gk, g[fr]) and torch.equal(sk[0], sums[k]) and torch.equal(ck[0], coef[k])
        assert torch.equal(ops.gn_bwd_apply(gk, zk, dt, C, stk[0], stk[2], ck, clips=1), dz[fr])


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_unsupported_backward_shapes_are_argument_errors_and_launch_nothing(ops, dtype_name):
    """The executor produces every frame of N >= 1 clips, or a frame window of ONE clip.  A window with two clips, a window past the
    clip, a group count that does not divide C and a single value per group are refused before anything is launched: every output
    buffer keeps its sentinel."""
    from detectandtrack_amd.libdat import DatError
    dt, fmt = _dt(ops, dtype_name), _fmt(dtype_name)
    z = torch.randn((2 * 3, 4, 4, 64), device='cuda').to(fmt)
    y = z.clone()
    one = torch.ones(64, device='cuda')
    st = ops.gn_stats(z, dt, 64, 32, one, one, EPS, clips=2)
    dbeta, dgamma = torch.full((64,), 7.0, device='cuda'), torch.full((64,), 9.0, device='cuda')
    dy = torch.full((2 * 1, 4, 4, 64), 3.0, device='cuda').to(fmt)
    with pytest.raises(DatError, match=r'one clip only.*code -1'):
        ops.gn_bwd_reduce(dy, y, z, dt, 64, 32, st[0], st[1], one, clips=2, frame_lo=1, relu=True, dbeta=dbeta, dgamma=dgamma, inplace=True)
    with pytest.raises(DatError, match=r'one clip only.*code -1'):
        ops.gn_bwd_apply(dy, z, dt, 64, st[0], st[2], torch.zeros((2, 2, 64), device='cuda'), clips=2, frame_lo=1)
    z1, st1 = z[:3].contiguous(), st[:, :1].contiguous()
    with pytest.raises(DatError, match=r'window.*code -1'):
        ops.gn_bwd_reduce(dy[:1].contiguous(), y[:3].contiguous(), z1, dt, 64, 32, st1[0], st1[1], one, clips=1, frame_lo=3, relu=True,
                          dbeta=dbeta, dgamma=dgamma)
    with pytest.raises(DatError, match=r'groups.*code -1'):
        ops.gn_stats(z, dt, 64, 24, one, one, EPS, clips=2)
    with pytest.raises(DatError, match=r'at least 2 values.*code -1'):
        ops.gn_stats(torch.zeros((1, 1, 1, 64), device='cuda').to(fmt), dt, 64, 64, one, one, EPS, clips=1)
    torch.cuda.synchronize()
    assert torch.all(dy == 3.0) and torch.all(dbeta == 7.0) and torch.all(dgamma == 9.0)


# ---- edges of the 16-bit formats (operands and expectations: tests/fp16_edge_cases.py) ------------------------------------------------------
EDGE_CASES = ['two_per_group', 'straddle']     # a group inside one thread's vector; groups that straddle the chunks, padding channels
SENTINEL = 77.0


def _edge_forward(ops, name, dtype_name, z, s, b, eps, what):
    """stats + apply of one edge input ([clips, M, C], already in the tensor format): the tables inside `table_bounds`, y inside
    `check_forward`, zero padding channels, and the rows before and behind the output untouched.  -> (tables, y [clips, M, C] tensor)"""
    N, f, H, W, C, cs, G = CASES[name]
    dt, fmt = _dt(ops, dtype_name), _fmt(dtype_name)
    s64, b64 = s.astype(np.float64), b.astype(np.float64)
    tables, dtables = ref.table_bounds(z, G, s64, b64, eps)
    zd = _dev(z, CASES[name], dtype_name)
    st = ops.gn_stats(zd, dt, C, G, _vec(s), _vec(b), eps, clips=N)
    got = st.cpu().numpy().astype(np.float64)
    ratios = []
    for k, label in enumerate(('mean', 'rstd', 'a', "b'")):
        err, bd = np.abs(got[k, :, :C] - tables[k]), dtables[k]
        ratios.append(_worst(err, bd))
        assert np.all(err <= bd), '%s %s %s: worst err/bound %.3g' % (what, name, label, ratios[-1])
    big = torch.full((N * f + 2, H, W, cs), SENTINEL, dtype=torch.float32).to(fmt).cuda()
    y = ops.gn_apply(zd, dt, C, st[2], st[3], clips=N, out=big[1:1 + N * f])
    torch.cuda.synchronize()
    assert torch.all(big[0] == SENTINEL) and torch.all(big[-1] == SENTINEL), 'rows outside the output were written'
    yv, ypad = _host(y, N, C)
    assert np.all(ypad == 0), 'padding channels of y are not zero'
    w1 = ref.check_forward(yv, z, G, s64, b64, eps, fmt, '%s %s y' % (what, name))
    print('%s %s %s: err/bound mean %.3f rstd %.3f a %.3f b\' %.3f y %.3f' % ((what, name, dtype_name) + tuple(ratios) + (w1,)))
    return tables, y[..., :C].reshape(N, -1, C).cpu()


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
@pytest.mark.parametrize('name', EDGE_CASES)
def test_subnormal_inputs_give_normal_outputs(ops, name, dtype_name):
    """Every z is k 2^-24, |k| < 1024: in the fp16 build's 16-bit mode all of them are subnormals (and exact); in bf16 they are ordinary
    normals rounded to 8 bits, in fp32 exact normals.  The variance (~1e-9) is far below eps, rstd ~ eps^-1/2, and the outputs
    s (z - mu) rstd are normal numbers around 1e-2 held to the forward bound; a kernel that flushes subnormal loads returns zeros."""
    N, f, H, W, C, cs, G = CASES[name]
    z, s, b = fe.gn_subnormal_case(N, f * H * W, C)
    if dtype_name == 'h16':
        z = nm.q16(z)
        if nm.h16() == torch.float16:
            assert np.array_equal(z, fe.gn_subnormal_case(N, f * H * W, C)[0]) and np.all(np.abs(z) < 2.0 ** -14)
        else:
            assert np.all((z == 0) | (np.abs(z) >= 2.0 ** -126))
    assert (z != 0).mean() > 0.99
    tables, y = _edge_forward(ops, name, dtype_name, z, s, b, EPS, 'subnormal inputs')
    assert np.all(tables[1] > 0.99 / np.sqrt(EPS))
    y = y.double().numpy()
    assert (y != 0).mean() > 0.99 and np.median(np.abs(y)) > 1e-3, 'the outputs vanished: subnormal inputs flushed to zero'


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
@pytest.mark.parametrize('name', EDGE_CASES)
def test_saturating_outputs_are_the_conversion_of_the_fp32_value(ops, name, dtype_name):
    """Constant channels +1, -1, 0, ... per group and eps = 4 - var: every table is exact (mean 0, rstd 1/2, a = s / 2, b' = b) -- asserted --
    and the fp32 value z a + b' is exactly the channel's target (65504, 65519, 65520, -65520, 2^17, ...).  The stored output equals torch's
    conversion: +-inf at and beyond 65520 in fp16, finite in bf16 and fp32.  The padding channels of z hold 1000 (times a = 2e6 it would
    overflow every format) and come out as zeros; the rows before and behind the output keep their sentinel."""
    N, f, H, W, C, cs, G = CASES[name]
    z, s, b, eps, want32, exact = fe.gn_saturation_case(N, f * H * W, C, G)
    if dtype_name == 'h16':
        assert np.array_equal(nm.q16(z), z)
    dt, fmt = _dt(ops, dtype_name), _fmt(dtype_name)
    zd = _dev(z, CASES[name], dtype_name)
    st = ops.gn_stats(zd, dt, C, G, _vec(s), _vec(b), eps, clips=N)
    got = st.cpu().numpy()
    for k, label in enumerate(('mean', 'rstd', 'a', "b'")):
        assert np.array_equal(got[k, :, :C], np.broadcast_to(exact[k], (N, C))), '%s: the table %s is not exact' % (name, label)
    big = torch.full((N * f + 2, H, W, cs), SENTINEL, dtype=torch.float32).to(fmt).cuda()
    y = ops.gn_apply(zd, dt, C, st[2], st[3], clips=N, out=big[1:1 + N * f])
    torch.cuda.synchronize()
    assert torch.all(big[0] == SENTINEL) and torch.all(big[-1] == SENTINEL), 'rows outside the output were written'
    assert torch.all(y[..., C:] == 0), 'padding channels of y are not zero'
    fe.check_gn_saturation(y[..., :C].reshape(N, -1, C).cpu(), want32, fmt, '%s %s' % (name, dtype_name))


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
@pytest.mark.parametrize('name', EDGE_CASES)
def test_a_mean_near_the_top_of_the_half_range(ops, name, dtype_name):
    """z = 3e4 + N(0, 100^2) rounded to the tensor format (fp16: multiples of 16, bf16: of 128): statistics and outputs inside the
    bounds of the other forward tests.  They are not vacuous here: tests/test_fp16_edges_cpu.py shows bound / |ref| of y below 1."""
    N, f, H, W, C, cs, G = CASES[name]
    z, s, b = fe.gn_high_mean_case(N, f * H * W, C)
    z = nm.q16(z) if dtype_name == 'h16' else z
    assert np.isfinite(z).all() and z.min() > 2.9e4
    _edge_forward(ops, name, dtype_name, z, s, b, EPS, 'high mean')
