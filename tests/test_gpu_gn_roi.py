"""The per-RoI GroupNorm kernels (csrc/group_norm_roi.hip) through the C ABI against float64 NumPy, in fp32 and in the build's 16-bit
format.  The references and bounds are those of tests/group_norm_ref.py with N = R, unchanged (nothing is fitted to the kernel):
  * mean, rstd ([R, G], expanded to [R, C]): `table_bounds`;
  * y: `check_forward` (K = 2 on the form z a + b' the kernel evaluates);
  * S1 = sum g, S2 = sum g xhat per (RoI, channel): `backward_sums_ref64` with `sum_bound` over the RoI's rows;
  * dz: `backward_dz_ref64` from the sums the kernel returned (K = 3);
  * dbeta / dgamma: within `sum_bound` over the live RoIs of the float64 sum of the returned sums plus what the buffer held, and
    bit-identical across two calls.
Shapes: the issue's cases, plus one per register-resident instantiation of the kernels (row slots 4 / 7 / 10 / 13 / 20), the split of a
large RoI into channel slabs (with a slab that is half or all padding), the re-reading path and the stride limit 2048.  Padding channels of every input hold junk.  Every test prints its worst err / bound.

Edges of the 16-bit formats (tests/fp16_edge_cases.py) on `two_per_group`, in fp32 and the build's 16-bit format: inputs in the fp16
subnormal range, outputs on and beyond the largest finite half, a mean of 3e4.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import fp16_edge_cases as fe
from tests import numerics as nm
from tests import group_norm_ref as ref

pytestmark = pytest.mark.gpu
EPS = 1e-5

#        R  Tr H   W   C    cstride G
CASES = {'two_per_group': (3, 1, 1, 1, 64, 64, 32),
         'box_head': (4, 3, 7, 7, 128, 128, 32),
         'group_is_chunk': (3, 1, 7, 7, 128, 128, 2),
         'straddle': (3, 2, 5, 7, 144, 192, 24),
         'wide_group': (2, 1, 3, 4, 921, 960, 3),
         'kps_head': (3, 2, 14, 14, 512, 512, 32),          # 392 rows at stride 512: split into 2 (forward) / 4 (backward) channel slabs
         'reread': (2, 8, 14, 14, 128, 128, 2),             # 1568 rows, groups of 64 channels: two slabs; re-read in fp32 and backward
         'slots_7': (2, 2, 7, 7, 512, 512, 32),             # 16-bit: 7 row slots (the largest resident backward); fp32: 13
         'slots_10': (2, 3, 7, 7, 512, 512, 32),            # the C4 R-18 box head: 16-bit 10 slots, fp32 19
         'slots_13': (2, 1, 14, 14, 512, 512, 32),          # the keypoint head, one frame: 16-bit 13 slots
         'widest': (2, 1, 7, 7, 2048, 2048, 32),            # the stride limit (the R-50 C4 head): 2 / 4 row lanes, 48 KB of LDS in 16-bit
         'split_padded': (2, 8, 14, 14, 144, 192, 24),      # split into two slabs of 96 channels: cg = 6, the second slab half padding
         'split_pad_only': (2, 8, 14, 14, 64, 128, 2),      # split into two slabs of 64 channels: the second is padding only
         'offset': (1, 2, 16, 16, 64, 64, 32),
         'means': (3, 2, 5, 7, 64, 64, 32)}
ROI_MEANS = (100.0, -50.0, 0.0)
COUNTS = (6, 2, 5, 7, 144, 192, 24)


@pytest.fixture(scope='module')
def ops():
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


_CACHE = {}


def _case(name, dtype_name):
    """Inputs of one case, made once: z / res / dy quantised to the tensor format ([R, M, C]), parameters fp32; float64 tables."""
    key = (name, dtype_name)
    if key not in _CACHE:
        R, f, H, W, C, cs, G = CASES[name]
        rs = np.random.RandomState(sum(map(ord, name)))
        M = f * H * W
        q = (lambda a: nm.q16(a)) if dtype_name == 'h16' else (lambda a: a.astype(np.float32))
        if name == 'offset':
            z = ref.offset_case(C=C)
        else:
            z = rs.randn(R, M, C) * rs.uniform(0.5, 3.0, C) + rs.randn(C) * 2
            if name == 'means':         # statistics shared across RoIs would be off by tens of standard deviations
                z = z + np.array(ROI_MEANS)[:, None, None]
        z = q(z.astype(np.float32))
        d = dict(z=z, res=q(rs.randn(R, M, C).astype(np.float32)), dy=q((rs.randn(R, M, C) * 0.1).astype(np.float32)),
                 s=rs.uniform(0.5, 1.5, C).astype(np.float32), b=(rs.randn(C) * 0.3).astype(np.float32), M=M, shape=CASES[name])
        d['tables'], d['dtables'] = ref.table_bounds(z, G, d['s'].astype(np.float64), d['b'].astype(np.float64), EPS)
        _CACHE[key] = d
    return _CACHE[key]


def _dev(a, shape, dtype_name, junk=1000.0):
    """[R, M, C] host array -> device blob [R * Tr, H, W, cs]; the padding channels hold junk that must never reach a result."""
    R, f, H, W, C, cs, _ = shape
    t = torch.full((R * f * H * W, cs), junk, dtype=torch.float32)
    t[:, :C] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, C))
    return t.view(R * f, H, W, cs).to(nm.h16() if dtype_name == 'h16' else torch.float32).cuda()


def _host(t, R, C):
    """device blob -> (real channels [R, M, C] float64, padding channels)"""
    a = t.float().cpu().numpy().reshape(R, -1, t.shape[-1])
    return a[:, :, :C].astype(np.float64), a[:, :, C:]


def _fmt(dtype_name):
    return nm.h16() if dtype_name == 'h16' else torch.float32


def _dt(ops, dtype_name):
    return ops.BF16 if dtype_name == 'h16' else ops.F32


def _vec(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _worst(err, bd):
    return float(np.max(err / bd))


def _per_channel(t, C):
    """fp32 [R, G] device table -> float64 [R, C]"""
    a = t.cpu().numpy().astype(np.float64)
    return np.repeat(a, C // a.shape[1], axis=1)


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_forward_against_float64(ops, name, dtype_name):
    c = _case(name, dtype_name)
    R, f, H, W, C, cs, G = c['shape']
    dt, fmt = _dt(ops, dtype_name), _fmt(dtype_name)
    z, res = _dev(c['z'], c['shape'], dtype_name), _dev(c['res'], c['shape'], dtype_name)
    sv, bv = _vec(c['s']), _vec(c['b'])
    y, mean, rstd = ops.gn_roi_fwd(z, dt, C, G, sv, bv, EPS, R=R)
    y_again, mean_again, rstd_again = ops.gn_roi_fwd(z, dt, C, G, sv, bv, EPS, R=R)
    torch.cuda.synchronize()
    assert tuple(mean.shape) == tuple(rstd.shape) == (R, G)
    assert torch.equal(y, y_again) and torch.equal(mean, mean_again) and torch.equal(rstd, rstd_again), 'the same input gave different bits'
    ratios = []
    for got, k, label in ((mean, 0, 'mean'), (rstd, 1, 'rstd')):
        err, bd = np.abs(_per_channel(got, C) - c['tables'][k]), c['dtables'][k]
        ratios.append(_worst(err, bd))
        assert np.all(err <= bd), '%s %s: worst err/bound %.3g' % (name, label, ratios[-1])
    s, b = c['s'].astype(np.float64), c['b'].astype(np.float64)
    yv, ypad = _host(y, R, C)
    assert np.all(ypad == 0), 'padding channels of y are not zero'
    w1 = ref.check_forward(yv, c['z'], G, s, b, EPS, fmt, '%s y' % name)
    y2, mean2, rstd2 = ops.gn_roi_fwd(z, dt, C, G, sv, bv, EPS, R=R, relu=True, residual=res)
    y2v, y2pad = _host(y2, R, C)
    assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd)
    assert np.all(y2pad == 0) and (y2v == 0).any() and (y2v > 0).any()
    w2 = ref.check_forward(y2v, c['z'], G, s, b, EPS, fmt, '%s relu(y + res)' % name, res=c['res'].astype(np.float64), relu=True)
    print('%s %s: err/bound mean %.3f rstd %.3f y %.3f relu(y+res) %.3f' % ((name, dtype_name) + tuple(ratios) + (w1, w2)))
    # aliasing: in place over z, and with the residual aliasing the output
    zc, rc = z.clone(), res.clone()
    assert torch.equal(ops.gn_roi_fwd(zc, dt, C, G, sv, bv, EPS, R=R, relu=True, residual=res, out=zc)[0], y2)
    assert torch.equal(ops.gn_roi_fwd(z, dt, C, G, sv, bv, EPS, R=R, relu=True, residual=rc, out=rc)[0], y2)


def _saved_tables(c):
    """The saved tables as fp32 values, inputs of the kernel AND of the reference: per channel [R, C] and per group [R, G]."""
    R, f, H, W, C, cs, G = c['shape']
    mu32, rstd32 = c['tables'][0].astype(np.float32), c['tables'][1].astype(np.float32)
    return mu32, rstd32, (c['s'] * rstd32).astype(np.float32), _vec(mu32[:, ::C // G]), _vec(rstd32[:, ::C // G])


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_backward_against_float64(ops, name, dtype_name, relu):
    c = _case(name, dtype_name)
    R, f, H, W, C, cs, G = c['shape']
    M, dt, fmt = c['M'], _dt(ops, dtype_name), _fmt(dtype_name)
    s, b = c['s'].astype(np.float64), c['b'].astype(np.float64)
    mu32, rstd32, a32, mean_g, rstd_g = _saved_tables(c)
    mu64, rstd64 = mu32.astype(np.float64), rstd32.astype(np.float64)
    y64 = np.maximum(ref.forward_ref64(c['z'], G, s, b, EPS, c['res'].astype(np.float64))[0], 0)
    y_host = nm.q16(y64) if dtype_name == 'h16' else y64.astype(np.float32)
    z, y, dy = (_dev(c[k] if k != 'y' else y_host, c['shape'], dtype_name) for k in ('z', 'y', 'dy'))
    r = ref.backward_sums_ref64(c['dy'], y_host, c['z'], mu64, rstd64, 0, M, relu)
    pre_b, pre_g = np.linspace(-1, 1, C).astype(np.float32), np.linspace(2, 3, C).astype(np.float32)
    dbeta, dgamma = _vec(pre_b), _vec(pre_g)
    args = (dy, y if relu else None, z, dt, C, G, mean_g, rstd_g, _vec(c['s']))
    g, dz, sums = ops.gn_roi_bwd(*args, R=R, relu=relu, dbeta=dbeta, dgamma=dgamma)
    gv, gpad = _host(g, R, C)
    assert np.all(gpad == 0) and np.array_equal(gv, r['g']), 'g is not dy masked by y > 0'
    sm = sums.cpu().numpy()
    assert sm.shape == (R, 2, cs) and np.all(sm[:, :, C:] == 0)
    sm64 = sm.astype(np.float64)
    bd1 = np.vectorize(lambda v: nm.sum_bound(v, M))(r['abs_S1'])
    bd2 = np.vectorize(lambda v: nm.sum_bound(v, M))(r['abs_S2'])
    e1, e2 = np.abs(sm64[:, 0, :C] - r['S1']), np.abs(sm64[:, 1, :C] - r['S2'])
    assert np.all(e1 <= bd1) and np.all(e2 <= bd2), '%s: sum g err/bound %.3g, sum g xhat err/bound %.3g' % (name, _worst(e1, bd1), _worst(e2, bd2))
    # dbeta / dgamma ACCUMULATE the sum over the RoIs of the returned sums
    wp = []
    for got, pre, k in ((dbeta, pre_b, 0), (dgamma, pre_g, 1)):
        want = pre.astype(np.float64) + sm64[:, k, :C].sum(axis=0)
        bd = np.vectorize(lambda v: nm.sum_bound(v, R + 1))(np.abs(pre.astype(np.float64)) + np.abs(sm64[:, k, :C]).sum(axis=0))
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        wp.append(_worst(err, bd))
        assert np.all(err <= bd), '%s: %s err/bound %.3g' % (name, ('dbeta', 'dgamma')[k], wp[-1])
    dbeta2, dgamma2 = _vec(pre_b), _vec(pre_g)
    g2, dz2, sums2 = ops.gn_roi_bwd(dy.clone(), y if relu else None, z, dt, C, G, mean_g, rstd_g, _vec(c['s']), R=R, relu=relu, dbeta=dbeta2,
                                    dgamma=dgamma2, inplace=True)
    assert torch.equal(g2, g) and torch.equal(dz2, dz) and torch.equal(sums2, sums), 'the same input gave different bits'
    assert torch.equal(dbeta2, dbeta) and torch.equal(dgamma2, dgamma), 'dbeta / dgamma differ between two calls'
    # dz from the kernel's sums taken as exact inputs
    dz_ref, absdz, extra, _ = ref.backward_dz_ref64(r['g'], c['z'], G, s, mu64, rstd64, sm64[:, 0, :C], sm64[:, 1, :C], 0, a=a32)
    assert tuple(dz.shape) == tuple(z.shape)
    dzv, dzpad = _host(dz, R, C)
    assert np.all(dzpad == 0)
    nm.assert_elementwise(dzv, dz_ref, absdz, 3, fmt, '%s dz' % name, extra=extra)
    wdz = _worst(np.abs(dzv - dz_ref), nm.bound(dz_ref, absdz, 3, fmt, extra))
    print('%s %s relu=%d: err/bound sum g %.3f, sum g xhat %.3f, dbeta %.3f, dgamma %.3f, dz %.3f'
          % (name, dtype_name, relu, _worst(e1, bd1), _worst(e2, bd2), wp[0], wp[1], wdz))
    # the optional outputs: no g, no dz -- the sums do not change
    none_g, none_dz, sums3 = ops.gn_roi_bwd(*args, R=R, relu=relu, want_g=False, want_dz=False)
    assert none_g is None and none_dz is None and torch.equal(sums3, sums)


def _all(ops, c, dtype_name, t, R, count=None):
    """forward (ReLU + residual) and backward of the blobs t = (z, res, dy) -> every output"""
    _, f, H, W, C, cs, G = c['shape']
    dt = _dt(ops, dtype_name)
    s, b = _vec(c['s']), _vec(c['b'])
    z, res, dy = t
    y, mean, rstd = ops.gn_roi_fwd(z, dt, C, G, s, b, EPS, R=R, relu=True, residual=res, count=count)
    dbeta, dgamma = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
    g, dz, sums = ops.gn_roi_bwd(dy, y, z, dt, C, G, mean, rstd, s, R=R, relu=True, count=count, dbeta=dbeta, dgamma=dgamma)
    return dict(y=y, mean=mean, rstd=rstd, g=g, dz=dz, sums=sums, dbeta=dbeta, dgamma=dgamma)


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_every_roi_keeps_the_bits_it_gets_alone(ops, dtype_name):
    """Three RoIs with means near +100, -50 and 0 in one call: every output row of RoI k equals, bit for bit, what the RoI yields as a
    blob of one."""
    c = _case('means', dtype_name)
    R, f, H, W, C, cs, G = c['shape']
    t = tuple(_dev(c[k], c['shape'], dtype_name) for k in ('z', 'res', 'dy'))
    full = _all(ops, c, dtype_name, t, R)
    means = full['mean'].cpu().numpy().mean(axis=1)
    assert np.all(np.abs(means - (np.array(ROI_MEANS) + means[2])) < 3), means
    for k in range(R):
        fr = slice(k * f, (k + 1) * f)
        one = _all(ops, c, dtype_name, tuple(v[fr].contiguous() for v in t), 1)
        for key in ('y', 'g', 'dz'):
            assert torch.equal(one[key], full[key][fr]), '%s of RoI %d depends on the other RoIs' % (key, k)
        for key in ('mean', 'rstd', 'sums'):
            assert torch.equal(one[key][0], full[key][k]), '%s of RoI %d depends on the other RoIs' % (key, k)


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_dead_rois_are_not_read_and_give_zero_rows(ops, dtype_name):
    """R = 6 in three image segments with live counts (0, 1, 2): the dead RoIs' inputs are NaN.  Live RoIs equal the same RoIs run alone
    bit for bit, dead rows are exactly zero, nothing anywhere is NaN, and dbeta / dgamma are the sums over the live RoIs."""
    R, f, H, W, C, cs, G = COUNTS
    rs = np.random.RandomState(5)
    M = f * H * W
    q = (lambda a: nm.q16(a)) if dtype_name == 'h16' else (lambda a: a.astype(np.float32))
    c = dict(shape=COUNTS, s=rs.uniform(0.5, 1.5, C).astype(np.float32), b=(rs.randn(C) * 0.3).astype(np.float32))
    host = [q((rs.randn(R, M, C) * sc + off).astype(np.float32)) for sc, off in ((2.0, 1.0), (1.0, 0.0), (0.1, 0.0))]
    counts, seg = (0, 1, 2), 2
    live = [r for r in range(R) if r % seg < counts[r // seg]]
    assert live == [2, 4, 5]
    for a in host:
        a[[r for r in range(R) if r not in live]] = np.nan
    t = tuple(_dev(a, COUNTS, dtype_name, junk=float('nan')) for a in host)
    cnt = torch.tensor(counts, dtype=torch.int32, device='cuda')
    full = _all(ops, c, dtype_name, t, R, count=cnt)
    torch.cuda.synchronize()
    for key, v in full.items():
        assert not torch.isnan(v.float()).any(), key + ' holds NaN'
    tb, ts, ab, as_ = (np.zeros(C, np.float64) for _ in range(4))
    for k in range(R):
        fr = slice(k * f, (k + 1) * f)
        if k not in live:
            assert all(torch.count_nonzero(full[key][fr]) == 0 for key in ('y', 'g', 'dz')), 'rows of dead RoI %d are not zero' % k
            assert all(torch.count_nonzero(full[key][k]) == 0 for key in ('mean', 'rstd', 'sums'))
            continue
        one = _all(ops, c, dtype_name, tuple(v[fr].contiguous() for v in t), 1)
        for key in ('y', 'g', 'dz'):
            assert torch.equal(one[key], full[key][fr]), '%s of live RoI %d differs from the RoI alone' % (key, k)
        for key in ('mean', 'rstd', 'sums'):
            assert torch.equal(one[key][0], full[key][k]), key
        sm = full['sums'][k].cpu().numpy().astype(np.float64)
        tb, ts, ab, as_ = tb + sm[0, :C], ts + sm[1, :C], ab + np.abs(sm[0, :C]), as_ + np.abs(sm[1, :C])
    for got, want, mag in ((full['dbeta'], tb, ab), (full['dgamma'], ts, as_)):     # (the buffers held zeros)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        bd = np.vectorize(lambda v: nm.sum_bound(v, len(live)))(mag)
        print('%s: dbeta / dgamma over the live RoIs, worst err/bound %.3f' % (dtype_name, _worst(err, bd)))
        assert np.all(err <= bd), float(err.max())


def _raw(ops, name, *args):
    return ops.ctx().call(name, ops._stream(), *args)


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_argument_errors_launch_nothing(ops, dtype_name):
    from detectandtrack_amd.libdat import DatError
    dt, fmt = _dt(ops, dtype_name), _fmt(dtype_name)
    R, C, G = 6, 64, 32
    z = torch.randn((R, 4, 4, C), device='cuda').to(fmt)
    one = torch.ones(C, device='cuda')
    y = torch.full_like(z, 3.0)
    mean, rstd = torch.full((R, G), 5.0, device='cuda'), torch.full((R, G), 5.0, device='cuda')
    sums, dbeta = torch.full((R, 2, C), 7.0, device='cuda'), torch.full((C,), 9.0, device='cuda')
    p, ll, f32 = ops._ptr, ctypes.c_longlong, ctypes.c_float
    cnt4 = torch.ones(4, dtype=torch.int32, device='cuda')
    ws = torch.empty(int(ops.L._lib.dat_gn_roi_workspace_bytes(R, C)), dtype=torch.uint8, device='cuda')
    assert ws.numel() > 0 and ops.L._lib.dat_gn_roi_workspace_bytes(R, 100) == 0 and ops.L._lib.dat_gn_roi_workspace_bytes(0, 64) == 0

    def fwd(zp=p(z), groups=G, count=None, n_seg=1, rows=16, C_=C):
        return _raw(ops, 'dat_gn_roi_fwd', dt, zp, None, p(y), R, ll(rows), C_, C, groups, p(one), p(one), f32(EPS), 0, p(mean), p(rstd),
                    count, n_seg)

    def bwd(dyp=p(z), ws_bytes=ws.numel(), n_seg=1, count=None, sums_p=p(sums)):
        return _raw(ops, 'dat_gn_roi_bwd', dt, dyp, None, p(z), p(mean), p(rstd), p(one), R, ll(16), C, C, G, 0, count, n_seg, p(y), None,
                    sums_p, p(dbeta), None, p(ws), ctypes.c_size_t(ws_bytes))
    with pytest.raises(DatError, match=r'null argument.*code -1'):
        fwd(zp=None)
    with pytest.raises(DatError, match=r'null argument.*code -1'):
        bwd(sums_p=None)
    off = ctypes.c_void_p(z.data_ptr() + 4)
    with pytest.raises(DatError, match=r'16-byte aligned.*code -1'):
        fwd(zp=off)
    with pytest.raises(DatError, match=r'16-byte aligned.*code -1'):
        bwd(dyp=off)
    with pytest.raises(DatError, match=r'equal row segments.*code -1'):
        fwd(count=p(cnt4), n_seg=4)
    with pytest.raises(DatError, match=r'equal row segments.*code -1'):
        bwd(count=p(cnt4), n_seg=4)
    with pytest.raises(DatError, match=r'groups.*code -1'):
        fwd(groups=24)
    wide = torch.zeros((R, 4, 4, 2112), device='cuda').to(fmt)          # past the stride limit of 2048
    with pytest.raises(DatError, match=r'at stride 2112.*at most 2048.*code -1'):
        _raw(ops, 'dat_gn_roi_fwd', dt, p(wide), None, p(wide), R, ll(16), 2112, 2112, 32, p(one), p(one), f32(EPS), 0, p(mean), p(rstd), None, 1)
    assert ops.L._lib.dat_gn_roi_workspace_bytes(R, 2048) > 0 and ops.L._lib.dat_gn_roi_workspace_bytes(R, 2112) == 0
    with pytest.raises(DatError, match=r'at least 2 values.*code -1'):
        fwd(groups=64, rows=1)
    with pytest.raises(DatError, match=r'workspace of \d+ bytes.*code -1'):
        bwd(ws_bytes=ws.numel() - 1)
    torch.cuda.synchronize()
    assert torch.all(y == 3.0) and torch.all(mean == 5.0) and torch.all(sums == 7.0) and torch.all(dbeta == 9.0)


# ---- edges of the 16-bit formats (operands and expectations: tests/fp16_edge_cases.py), on the smallest case ---------------------------------
EDGE = 'two_per_group'
SENTINEL = 77.0


def _edge_forward(ops, dtype_name, z, s, b, eps, what, exact=None):
    """The fused forward on one edge input ([R, M, C], already in the tensor format) written between two sentinel RoIs: mean / rstd inside
    `table_bounds` (exact: equal to these tables), the rows outside the output untouched.  -> (tables, y [R, M, C] tensor, its check)"""
    R, f, H, W, C, cs, G = CASES[EDGE]
    dt, fmt = _dt(ops, dtype_name), _fmt(dtype_name)
    s64, b64 = s.astype(np.float64), b.astype(np.float64)
    tables, dtables = ref.table_bounds(z, G, s64, b64, eps)
    zd = _dev(z, CASES[EDGE], dtype_name)
    big = torch.full((R * f + 2, H, W, cs), SENTINEL, dtype=torch.float32).to(fmt).cuda()
    y, mean, rstd = ops.gn_roi_fwd(zd, dt, C, G, _vec(s), _vec(b), eps, R=R, out=big[1:1 + R * f])
    torch.cuda.synchronize()
    assert torch.all(big[0] == SENTINEL) and torch.all(big[-1] == SENTINEL), 'rows outside the output were written'
    ratios = []
    for got, k, label in ((mean, 0, 'mean'), (rstd, 1, 'rstd')):
        if exact is not None:
            assert np.array_equal(_per_channel(got, C), np.broadcast_to(exact[k].astype(np.float64), (R, C))), 'the table %s is not exact' % label
        err, bd = np.abs(_per_channel(got, C) - tables[k]), dtables[k]
        ratios.append(_worst(err, bd))
        assert np.all(err <= bd), '%s %s: worst err/bound %.3g' % (what, label, ratios[-1])
    yv, ypad = _host(y, R, C)
    assert np.all(ypad == 0)
    check = lambda: ref.check_forward(yv, z, G, s64, b64, eps, fmt, '%s y' % what)
    return tables, y[..., :C].reshape(R, -1, C).cpu(), ratios, check


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_subnormal_inputs_give_normal_outputs(ops, dtype_name):
    """Every z is k 2^-24, |k| < 1024: fp16 subnormals (exact) in the fp16 build's 16-bit mode, ordinary normals in bf16 (rounded to 8 bits)
    and fp32.  rstd ~ eps^-1/2 and the outputs are normal numbers around 1e-2 inside the forward bound; a kernel that flushes subnormal
    loads returns zeros."""
    R, f, H, W, C, cs, G = CASES[EDGE]
    z, s, b = fe.gn_subnormal_case(R, f * H * W, C)
    if dtype_name == 'h16':
        z = nm.q16(z)
        if nm.h16() == torch.float16:
            assert np.array_equal(z, fe.gn_subnormal_case(R, f * H * W, C)[0]) and np.all(np.abs(z) < 2.0 ** -14)
        else:
            assert np.all((z == 0) | (np.abs(z) >= 2.0 ** -126))
    tables, y, ratios, check = _edge_forward(ops, dtype_name, z, s, b, EPS, 'subnormal inputs')
    w = check()
    print('subnormal inputs %s: err/bound mean %.3f rstd %.3f y %.3f' % (dtype_name, ratios[0], ratios[1], w))
    assert np.all(tables[1] > 0.99 / np.sqrt(EPS))
    y = y.double().numpy()
    assert (y != 0).mean() > 0.95 and np.median(np.abs(y)) > 1e-3, 'the outputs vanished: subnormal inputs flushed to zero'


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_saturating_outputs_are_the_conversion_of_the_fp32_value(ops, dtype_name):
    """A group of the two values +1, -1 and eps = 3: mean 0 and rstd 1/2 exactly (asserted), a = s / 2, b' = b, and the fp32 value
    z a + b' is exactly the channel's target (65504, 65519, 65520, -65520, 2^17, ...).  The stored output equals torch's conversion: +-inf
    at and beyond 65520 in fp16, finite in bf16 and fp32; the RoIs before and behind the output keep their sentinel."""
    R, f, H, W, C, cs, G = CASES[EDGE]
    z, s, b, eps, want32, exact = fe.gn_saturation_case(R, f * H * W, C, G)
    assert eps == 3.0 and (dtype_name != 'h16' or np.array_equal(nm.q16(z), z))
    _, y, _, _ = _edge_forward(ops, dtype_name, z, s, b, eps, 'saturation', exact=exact)
    fe.check_gn_saturation(y, want32, _fmt(dtype_name), '%s %s' % (EDGE, dtype_name))


@pytest.mark.parametrize('dtype_name', ['fp32', 'h16'])
def test_a_mean_near_the_top_of_the_half_range(ops, dtype_name):
    """z = 3e4 + N(0, 100^2) rounded to the tensor format: mean, rstd and y inside the bounds of the other forward tests (not vacuous
    in fp32 and fp16: tests/test_fp16_edges_cpu.py).  Left out in bf16: its spacing at 3e4 is 128, the two values of a group are often
    equal, the variance is 0, and the bound of y grows to 40 times |y| (the same CPU test) -- a check that could not fail."""
    R, f, H, W, C, cs, G = CASES[EDGE]
    if dtype_name == 'h16' and nm.h16() == torch.bfloat16:
        pytest.skip('fp16 build only: with two bf16 values per group near 3e4 the bound is vacuous')
    z, s, b = fe.gn_high_mean_case(R, f * H * W, C)
    z = nm.q16(z) if dtype_name == 'h16' else z
    assert np.isfinite(z).all() and z.min() > 2.9e4
    _, _, ratios, check = _edge_forward(ops, dtype_name, z, s, b, EPS, 'high mean')
    w = check()
    print('high mean %s: err/bound mean %.3f rstd %.3f y %.3f' % (dtype_name, ratios[0], ratios[1], w))
