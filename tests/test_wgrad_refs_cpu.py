"""tests/wgrad_refs.py on the CPU, so that tests/test_gpu_wgrad.py holds the weight-gradient kernels to a reference that is itself right
and to a bound that means something:

  * wgrad_ref64 (one float64 matmul per tap) equals torch.nn.grad.conv3d_weight in float64 on every geometry of the GPU tests;
  * a kernel that accumulates in fp32 the way the project's kernels do -- chunks of 64 / 32 positions or 8 x 8 patches with one rounding per
    chunk, K ranges added in a shuffled order, then the scale -- stays inside nm.bound(..., 'fp32') with C = 8 at every shape, the bench's
    reduction length (8 x 24 x 42 positions) included;
  * each seeded defect of wgrad_refs.DEFECTS leaves the bound at every shape it applies to."""
import numpy as np
import pytest
import torch

from tests import numerics as nm
from tests import wgrad_refs as wr

GEOMETRIES = [
    # cin, cout, (kt,kh,kw), stride, N, T, H, W, window
    (5, 7, (3, 3, 3), 1, 1, 3, 9, 17, None),            # 3 x 3 x 3, partial patches on both edges
    (6, 4, (1, 3, 3), 1, 2, 2, 7, 7, None),             # KT 1, two clips, a map smaller than a patch
    (5, 6, (3, 3, 3), 1, 1, 4, 8, 8, (0, 1)),           # window at the first frame (its temporal tap -1 is padding)
    (5, 6, (3, 3, 3), 1, 1, 4, 8, 8, (3, 1)),           # window at the last frame
    (5, 6, (3, 3, 3), 1, 2, 2, 8, 8, (1, 1)),           # two clips: the window is ignored
    (4, 5, (3, 3, 3), 1, 1, 2, 1, 37, None),            # H == 1
    (4, 5, (1, 3, 3), 1, 1, 2, 5, 1, None),             # W == 1
    (6, 5, (3, 3, 3), 2, 1, 3, 9, 11, None),            # stride 2 on odd H and W
    (6, 5, (1, 3, 3), 2, 1, 3, 7, 13, (1, 2)),
    (6, 5, (3, 3, 3), 2, 1, 2, 9, 2, None),             # stride 2, Wo == 1 < Ho with spatial taps
    (7, 3, (1, 1, 1), 1, 1, 2, 13, 19, None),           # pointwise
    (6, 4, (1, 1, 1), 2, 2, 2, 9, 11, None),            # pointwise stride 2, odd map, two clips
    (6, 4, (1, 1, 1), 2, 1, 2, 6, 2, None),             # pointwise stride 2: Wo == 1 < Ho
    (6, 4, (1, 1, 1), 2, 1, 2, 2, 6, None),
    (6, 4, (1, 1, 1), 2, 1, 2, 2, 2, None),
    (6, 4, (1, 1, 1), 2, 1, 3, 1, 5, (1, 1)),
    (9, 5, (3, 1, 1), 1, 1, 4, 6, 7, None),             # kT x 1 x 1 of the (2+1)D bodies
    (9, 5, (3, 1, 1), 1, 1, 3, 9, 1, None),             # ... on a one-column map: Wo == 1 < Ho
    (9, 5, (3, 1, 1), 1, 1, 4, 5, 6, (2, 2)),
    (8, 16, (3, 3, 3), 1, 1, 8, 24, 42, None),          # the bench's reduction length, K = 8064
    (16, 8, (1, 1, 1), 1, 1, 8, 24, 42, None),
    (8, 6, (3, 1, 1), 1, 1, 8, 24, 42, (3, 3)),
]
IDS = ['%dto%d_k%d%d%d_s%d_n%dt%d_%dx%d%s' % (c[0], c[1], c[2][0], c[2][1], c[2][2], c[3], c[4], c[5], c[6], c[7],
                                              '' if c[8] is None else '_win%d+%d' % c[8]) for c in GEOMETRIES]


def _pads(k):
    return (k[0] // 2, k[1] // 2, k[2] // 2)


def _operands(case, fmt, seed=0):
    cin, cout, k, st, N, T, H, W, win = case
    rs = np.random.RandomState(1000 * seed + 17 * cin + cout + H * W)
    Ho, Wo = wr.out_hw(H, W, k, st, _pads(k))
    x = rs.standard_normal((N, cin, T, H, W)).astype(np.float32)
    g = rs.standard_normal((N, cout, T, Ho, Wo)).astype(np.float32)
    scale = (rs.random_sample(cout) + 0.5).astype(np.float32)
    if fmt != 'fp32':
        x, g = nm.q16(x, fmt), nm.q16(g, fmt)
    return x, g, scale


@pytest.mark.parametrize('case', GEOMETRIES, ids=IDS)
def test_wgrad_ref64_equals_torch_conv3d_weight(case):
    cin, cout, k, st, N, T, H, W, win = case
    x, g, scale = _operands(case, 'bf16')
    ref, absref, K = wr.wgrad_ref64(x, g, scale, k, st, _pads(k), win)
    t_lo, t_hi = wr.frame_range(N, T, win)
    assert K == N * (t_hi - t_lo) * g.shape[3] * g.shape[4]
    gz = np.zeros_like(g, dtype=np.float64)
    gz[:, :, t_lo:t_hi] = g[:, :, t_lo:t_hi]
    gz *= scale.astype(np.float64).reshape(1, -1, 1, 1, 1)
    xt, gt = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(gz)
    wgrad = lambda a, b: torch.nn.grad.conv3d_weight(a, (cout, cin) + k, b, stride=(1, st, st), padding=_pads(k)).numpy()
    exp, exp_abs = wgrad(xt, gt), wgrad(xt.abs(), gt.abs())
    np.testing.assert_allclose(ref, exp, rtol=0, atol=1e-12 * float(exp_abs.max()))
    np.testing.assert_allclose(absref, exp_abs, rtol=1e-12)
    assert np.all(absref >= np.abs(ref) * (1 - 1e-12))


def _chunkings(case, fmt):
    k, st = case[2], case[3]
    out = ['linear32' if fmt == 'fp32' else 'linear64']                 # re-pack GEMM (CK 32 in fp32) / direct kernel
    if fmt != 'fp32':
        out.append('linear32')                                              # pointwise kernel: 32-position chunks
        if k[1:] == (3, 3) and st == 1:
            out.append('patch8')                                            # nine-tap kernel
    return out


@pytest.mark.parametrize('fmt', ['bf16', 'fp16', 'fp32'])
def test_fp32_accumulation_in_every_kernel_order_stays_inside_the_bound(fmt):
    """Every element of every simulated kernel result within nm.bound(ref, absref, K, 'fp32'), no case left out.  The largest
    err / bound is printed: the headroom of C = 8 over a correct kernel."""
    worst = (0.0, None)
    for case, cid in zip(GEOMETRIES, IDS):
        cin, cout, k, st, N, T, H, W, win = case
        x, g, scale = _operands(case, fmt)
        ref, absref, K = wr.wgrad_ref64(x, g, scale, k, st, _pads(k), win)
        for chunking in _chunkings(case, fmt):
            parts = wr.chunk_partials(x, g, k, st, _pads(k), win, chunking)
            nch = parts.shape[1]
            for nsplit in sorted({1, 2, 5, 16, nch + 3}):
                got = wr.accumulate_fp32(parts, scale, k, nsplit, np.random.RandomState(nsplit))
                nm.assert_elementwise(got, ref, absref, K, 'fp32', '%s %s split %d' % (cid, chunking, nsplit))
                r = wr.worst_ratio(got, ref, absref, K)
                worst = max(worst, (r, '%s %s split %d' % (cid, chunking, nsplit)))
    print('%s operands: largest simulated err / bound %.4f (%s)' % (fmt, worst[0], worst[1]))
    assert worst[0] < 1.0


@pytest.mark.parametrize('name', wr.DEFECTS)
def test_seeded_defect_leaves_the_bound(name):
    """A kernel with the defect puts at least one element outside the bound at every shape the defect applies to, the bench's reduction
    length included (where the bound is about a fifth of one x * g product: a lost position is seen by the elements whose product there
    is larger).  The smallest worst-element err / bound over the shapes is printed."""
    applied = []
    for case, cid in zip(GEOMETRIES, IDS):
        cin, cout, k, st, N, T, H, W, win = case
        for fmt in ('bf16', 'fp16'):
            x, g, scale = _operands(case, fmt)
            got = wr.defect(name, x, g, scale, k, st, _pads(k), win)
            if got is None:
                continue
            ref, absref, K = wr.wgrad_ref64(x, g, scale, k, st, _pads(k), win)
            r = wr.worst_ratio(got, ref, absref, K)
            applied.append((r, cid, fmt))
            assert r > 1.0, '%s is not caught at %s (%s): largest err / bound %.3f' % (name, cid, fmt, r)
            with pytest.raises(AssertionError):
                nm.assert_elementwise(got, ref, absref, K, 'fp32', name)
    assert applied, name
    weakest = min(applied)
    print('%s: caught at %d shape x format cases; smallest worst-element err / bound %.1f (%s, %s)' % (
        name, len(applied), weakest[0], weakest[1], weakest[2]))
    # (shapes x two formats: 11 shapes pad a spatial border that has a neighbour, 6 have a window on a single clip, 4 a one-column map)
    must = {'border_tap_reads_the_opposite_neighbour': 22, 'window_off_by_one_frame': 12, 'one_column_map_addressing': 8}
    assert len(applied) == must.get(name, 2 * len(GEOMETRIES)), (name, len(applied))
