"""The inference hot path's RoIAlign, keypoint-tail, pooling, reduction and copy kernels (csrc/roi_align.hip, csrc/elementwise.hip,
scatter_words of csrc/labels.hip) element by element against the float64 restatements of tests/infer_refs.py and tests/train_refs.py:
every output element within the per-element bound of tests/numerics.py (copies and maxima exactly), in fp32 and the build's 16-bit
format, at the shapes where these kernels take separate paths -- every lane grouping of RoIAlign over four FPN levels, tubes and key
frames, a second grid pass, the keypoint tail's tile kernel (bit for bit against the per-element kernel), grid-stride loops past the
launch caps, strides wider than the data.  tests/test_infer_refs_cpu.py checks the references and the roi sets on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import infer_refs as ir
from tests import numerics as nm
from tests import train_refs as tr
from tests.test_gpu_train_kernels import IMG_H, IMG_W, LEVEL_SCALES, _roi_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _fmt_name(dtype):
    """'fp32', or the name of the loaded build's 16-bit format for '16'."""
    return 'fp32' if dtype == 'fp32' else {torch.bfloat16: 'bf16', torch.float16: 'fp16'}[nm.h16()]


def _dt(ops, dtype):
    return ops.F32 if dtype == 'fp32' else ops.BF16


def _q(a, fmt):
    a = np.ascontiguousarray(a, np.float32)
    return a if fmt == 'fp32' else nm.q16(a, fmt)


def _dev(a, dtype='fp32'):
    """numpy -> CUDA tensor; '16' gets the build's 16-bit format (exact: the values are quantised first)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if t.is_floating_point():
        t = t.float() if dtype == 'fp32' else t.float().to(nm.h16())
    return t.cuda()


def _poison(shape, tdtype):
    """The care of the suite's DAT_POISON pass without its fixture: a block of the size the wrapper is about to ask for goes back to
    the caching allocator full of NaN (0xFF bytes), so an output cell that no thread writes shows up as NaN, not as a stale value."""
    n = int(np.prod(shape)) * torch.empty((), dtype=tdtype).element_size()
    if n:
        t = torch.empty(n, dtype=torch.uint8, device='cuda')
        t.fill_(0xFF)
        torch.cuda.synchronize()
        del t


# ---- RoIAlign forward -------------------------------------------------------------------------------------------------------------
# name, FPN levels, R, T, Tr, t0, pooled, sampling, C, seed.  The lanes per cell follow C / (16 bytes) (roi_align.hip `grp`): 8 channels
# are one 16-bit vector (64 cells per wave), 72 are 9 (a group of 16 with idle lanes), 256 are 32 (two cells per wave), 520 are 65 (a
# ragged second trip of the channel loop; 130 in fp32: a ragged third), 2048 in fp32 are 512 (eight trips).
ROI_CASES = [
    ('tube2_c64', 4, 40, 2, 2, 0, 7, 2, 64, 1),
    ('tube3_adaptive_c72', 4, 24, 3, 3, 0, 7, 0, 72, 2),
    ('tube2_p14_adaptive_c256', 4, 24, 2, 2, 0, 14, 0, 256, 3),
    ('keyframe_p14_c256', 4, 30, 3, 1, 2, 14, 2, 256, 4),
    ('keyframe_adaptive_c8', 4, 30, 2, 1, 1, 14, 0, 8, 5),
    ('single_adaptive_c520', 4, 24, 1, 1, 0, 7, 0, 520, 6),
    ('single_p14_c72', 4, 30, 1, 1, 0, 14, 2, 72, 7),
    ('single_c8', 4, 40, 1, 1, 0, 7, 2, 8, 8),
    ('one_level_c2048', 1, 16, 1, 1, 0, 7, 2, 2048, 9),
    # more cells than one grid pass holds: 8192 blocks of 4 (fp32) or 8 (16-bit) cells at 256 channels
    ('two_grid_passes_c256', 4, 340, 1, 1, 0, 14, 2, 256, 10),
]
ROI_N = 2                                                  # images
ROI_PARAMS = [(c, d) for c in ROI_CASES for d in ('fp32', '16') if not (c[0] == 'one_level_c2048' and d == '16')]


def roi_inputs(case, fmt, channels=None):
    """(rois, feats, scales) of a case with the maps quantised to `fmt` ('fp32', 'bf16', 'fp16'); `channels` overrides the case's
    channel count (the CPU checks of the roi sets, which do not depend on it)."""
    name, levels, R, T, Tr, t0, P, samp, Cn, seed = case
    Cn = channels or Cn
    rs = np.random.RandomState(seed)
    rois = _roi_set(rs, name, R, Tr, ROI_N)
    scales = LEVEL_SCALES[:levels] if levels > 1 else [1 / 16.]
    feats = [_q(rs.randn(ROI_N * T, int(IMG_H * s), int(IMG_W * s), Cn), fmt) for s in scales]
    return rois, feats, scales


def roi_reference(case, fmt):
    name, levels, R, T, Tr, t0, P, samp, Cn, seed = case
    rois, feats, scales = roi_inputs(case, fmt)
    return (rois, feats, scales) + ir.roi_align_ref(feats, scales, rois, T, Tr, t0, P, samp, 2, 224., 4)


@pytest.mark.parametrize('case,dtype', ROI_PARAMS, ids=['%s-%s' % (c[0], d) for c, d in ROI_PARAMS])
def test_roi_align(ops, case, dtype):
    """Every element of every roi: rois off the map, smaller than a bin, on the FPN level boundaries, jittered tubes (the roi sets of
    the backward tests), two images."""
    name, levels, R, T, Tr, t0, P, samp, Cn, seed = case
    rois, feats, scales, ref, ab, ex, K = roi_reference(case, _fmt_name(dtype))
    ncell = R * Tr * P * P
    if name == 'two_grid_passes_c256':
        assert ncell > 8192 * 4 * (2 if dtype == '16' else 1), 'the grid of dat_roi_align (roi_align.hip) must be capped'
    dfeats = [_dev(f, dtype) for f in feats]
    _poison((R * Tr, P, P, Cn), dfeats[0].dtype)
    out = ops.roi_align(dfeats, scales, _dt(ops, dtype), _dev(rois), T, Tr, t0, P, samp, k_min=2, canon_scale=224., canon_level=4)
    torch.cuda.synchronize()
    assert out.dtype == dfeats[0].dtype and tuple(out.shape) == ref.shape
    nm.assert_elementwise(out.float().cpu().numpy(), ref, ab, K, _fmt_name(dtype), 'roi_align %s %s' % (name, dtype), ex)


# ---- keypoint tail ----------------------------------------------------------------------------------------------------------------
KPS_K = 17
KPS_SHAPES = [(u, t, s, 128) for u in (2, 4) for t in (1, 2) for s in (14, 28)] + [(4, 1, 32, 128), (4, 2, 32, 128)] + \
             [(2, 1, 14, 192), (2, 2, 14, 192), (4, 2, 14, 192)]


def _kps_case(ops, rs, dtype, R, Tr, S, cs, K, up):
    """-> (device input, output, what); the output is already held to the float64 reference.  The channels 4K..cs hold large values
    that no output may see."""
    sub = rs.randn(R * Tr, S, S, cs).astype(np.float32)
    sub[..., 4 * K:] *= 1000.
    sub = _q(sub, _fmt_name(dtype))
    ref = tr.kps_finalize_ref(sub, R, Tr, K, up)
    ab = tr.kps_finalize_ref(np.abs(sub), R, Tr, K, up)
    M = 2 * S * up
    d = _dev(sub, dtype)
    _poison((R, Tr * K, M, M), torch.float32)
    out = ops.kps_finalize(d, _dt(ops, dtype), R, Tr, K, up)
    torch.cuda.synchronize()
    what = 'kps_finalize %s up=%d Tr=%d S=%d cs=%d R=%d' % (dtype, up, Tr, S, cs, R)
    assert tuple(out.shape) == ref.shape == (R, Tr * K, M, M)
    nm.assert_elementwise(out.cpu().numpy(), ref, ab, 4, 'fp32', what)         # two taps per axis (k = 2*up, s = up)
    return d, out, what


def _takes_tile_kernel(R, Tr, S, cs, K, up):
    """The dispatch condition of dat_kps_finalize (csrc/elementwise.hip), restated."""
    M, maps = 2 * S * up, R * Tr * K
    return M <= 256 and (2 * S) * (2 * S) * 4 <= 48 * 1024 and 4 * K <= cs and 1024 <= maps < 2 ** 31


def _per_element_slices(ops, d, dtype, R, Tr, K, up):
    """The same input through the per-element kernel: roi slices of fewer than 1024 maps (the op is independent per map)."""
    step = 1023 // (Tr * K)
    parts = []
    for a in range(0, R, step):
        b = min(R, a + step)
        assert (b - a) * Tr * K < 1024
        parts.append(ops.kps_finalize(d[a * Tr:b * Tr], _dt(ops, dtype), b - a, Tr, K, up))
    torch.cuda.synchronize()
    return torch.cat(parts, 0)


@pytest.mark.parametrize('dtype', ['fp32', '16'])
@pytest.mark.parametrize('up,Tr,S,cs', KPS_SHAPES)
def test_kps_finalize_tile_kernel(ops, up, Tr, S, cs, dtype):
    """The smallest R that takes the tile kernel: M = 56 runs four row groups per block, 112 two, 224 and 256 one; up = 4 its
    general loop.  (a) every element within the bound of the float64 tail, (b) bit-identical to the per-element kernel."""
    K = KPS_K
    R = -(-1024 // (Tr * K))
    M = 2 * S * up
    assert _takes_tile_kernel(R, Tr, S, cs, K, up) and not _takes_tile_kernel(1023 // (Tr * K), Tr, S, cs, K, up)
    assert max(1, min(4, 256 // M)) == {56: 4, 112: 2, 224: 1, 256: 1}[M]
    rs = np.random.RandomState(up * 1000 + Tr * 100 + S + cs)
    d, out, what = _kps_case(ops, rs, dtype, R, Tr, S, cs, K, up)
    per = _per_element_slices(ops, d, dtype, R, Tr, K, up)
    assert torch.equal(out.view(torch.int32), per.view(torch.int32)), what + ': the tile kernel differs from the per-element kernel'


@pytest.mark.parametrize('dtype', ['fp32', '16'])
@pytest.mark.parametrize('up,Tr,S,cs', [(2, 1, 14, 128), (4, 2, 7, 72), (2, 2, 5, 68)])
def test_kps_finalize_few_rois(ops, up, Tr, S, cs, dtype):
    """Fewer than 1024 maps: the per-element kernel, also at a channel stride that is exactly 4K."""
    R = 3
    assert not _takes_tile_kernel(R, Tr, S, cs, KPS_K, up)
    _kps_case(ops, np.random.RandomState(up + Tr + S), dtype, R, Tr, S, cs, KPS_K, up)


def test_kps_finalize_maps_wider_than_a_block_fall_back(ops):
    """M = 264 > 256 fails the tile condition at a map count that passes it: the per-element kernel past its grid cap."""
    R, Tr, S, cs, up = 61, 1, 33, 128, 4
    assert R * Tr * KPS_K >= 1024 and 2 * S * up > 256 and not _takes_tile_kernel(R, Tr, S, cs, KPS_K, up)
    _kps_case(ops, np.random.RandomState(33), '16', R, Tr, S, cs, KPS_K, up)


def test_kps_finalize_no_rois(ops):
    out = ops.kps_finalize(torch.empty((0, 14, 14, 128), device='cuda'), ops.F32, 0, 2, KPS_K, 2)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (0, 2 * KPS_K, 56, 56)


@pytest.mark.parametrize('R', [3, 70])
def test_kps_finalize_rejects_a_stride_narrower_than_the_sub_pixel_channels(ops, R):
    """4K = 68 > cs = 64: both kernels would read the next cell's channels.  The call raises and writes nothing."""
    from detectandtrack_amd.libdat import DatError
    K, S, cs = KPS_K, 7, 64
    sub = torch.randn((R, S, S, cs), device='cuda')
    out = torch.full((R, K, 4 * S, 4 * S), 2.5, device='cuda')
    with pytest.raises(DatError, match='sub-pixel channels'):
        ops.ctx().call('dat_kps_finalize', ops._stream(), ops.F32, ops._ptr(sub), R, 1, S, cs, K, 2, ops._ptr(out))
    torch.cuda.synchronize()
    assert bool((out == 2.5).all())


# ---- mean over time ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', '16'])
@pytest.mark.parametrize('N,T,hwc', [(n, t, (5, 7, 13)) for n in (1, 3) for t in (1, 2, 3, 8)] + [(3, 2, (37, 41, 233))],
                         ids=lambda v: 'x'.join(str(i) for i in v) if isinstance(v, tuple) else str(v))
def test_time_avg(ops, N, T, hwc, dtype):
    """h*w*c = 455 is a multiple of neither the block nor of 8; 3 * 353 461 elements pass the 4096-block grid cap.  The sum is fp32 and
    rounds once, into the output: K = T."""
    rs = np.random.RandomState(N * 10 + T)
    x = _q(rs.randn(*((N * T,) + hwc)) * 3 + 1, _fmt_name(dtype))
    ref, ab = ir.time_avg_ref(x, N, T)
    _poison((N,) + hwc, torch.float32 if dtype == 'fp32' else nm.h16())
    out = ops.time_avg(_dev(x, dtype), _dt(ops, dtype), N, T)
    torch.cuda.synchronize()
    nm.assert_elementwise(out.float().cpu().numpy(), ref, ab, T, _fmt_name(dtype), 'time_avg %s N=%d T=%d %r' % (dtype, N, T, hwc))


# ---- mean over H, W ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', '16'])
@pytest.mark.parametrize('frames,H,W,Cn,Cs', [(3, 1, 1, 200, 208), (4, 7, 7, 200, 256), (2, 14, 14, 72, 128), (8, 7, 7, 2048, 2048),
                                              (5300, 1, 1, 200, 208)])
def test_spatial_mean(ops, frames, H, W, Cn, Cs, dtype):
    """C < Cs with large values in the padding channels, C not a multiple of 64, and frames * C past the 4096-block grid cap."""
    rs = np.random.RandomState(frames + H + Cn)
    x = rs.randn(frames, H, W, Cs).astype(np.float32) + 0.5
    x[..., Cn:] = 1000.
    x = _q(x, _fmt_name(dtype))
    ref, ab = ir.spatial_mean_ref(x, Cn)
    _poison((frames, Cn), torch.float32)
    out = ops.spatial_mean(_dev(x, dtype), _dt(ops, dtype), Cn)
    torch.cuda.synchronize()
    nm.assert_elementwise(out.cpu().numpy(), ref, ab, H * W, 'fp32', 'spatial_mean %s %r' % (dtype, (frames, H, W, Cn, Cs)))


# ---- row softmax ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [0, 1, 100003])
@pytest.mark.parametrize('K,ld', [(1, 3), (2, 8), (5, 7)])
def test_softmax_rows(ops, K, ld, rows):
    """ld_in > K with a large logit in the padding, rows of equal logits, logits at +-90 (their difference leaves fp32's exponent
    range: the small probability is 0 to within the smallest half-ulp), rows past the grid."""
    rs = np.random.RandomState(K * 7 + rows % 1000)
    x = (rs.randn(rows, ld) * 4).astype(np.float32)
    x[:, K:] = 500.
    if rows > 10:
        x[0:4, :K] = [[1.25], [-90.], [90.], [0.]]
        if K > 1:
            x[4, :K], x[4, 0] = -90., 90.
            x[5, :K], x[5, K - 1] = 90., -90.
    p, extra = ir.softmax_rows_ref(x, K)
    _poison((rows, K), torch.float32)
    out = ops.softmax_rows(torch.from_numpy(x).cuda(), K)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (rows, K)
    if rows:
        # p = e / s: the sum of K fp32 terms, each an expf (a few ulps, inside C) of an argument that rounded (`extra`)
        nm.assert_elementwise(out.cpu().numpy(), p, p, K, 'fp32', 'softmax_rows K=%d ld=%d rows=%d' % (K, ld, rows), extra)


# ---- max pooling ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', '16'])
@pytest.mark.parametrize('k,stride,pad', [(3, 2, 1), (1, 2, 0), (2, 2, 0)])
def test_maxpool_hw_is_exact(ops, k, stride, pad, dtype):
    """Negative-only maps with -inf cells and whole -inf windows (a maximum that starts at 0 fails), odd and one-pixel maps."""
    rs = np.random.RandomState(k * 10 + stride)
    for frames, H, W in [(2, 1, 1), (3, 7, 9), (1, 15, 2), (2, 4, 33)]:
        if H + 2 * pad < k or W + 2 * pad < k:
            continue
        for Cn in (8, 64, 200):
            x = -np.abs(rs.randn(frames, H, W, Cn).astype(np.float32)) - 0.5
            x[rs.rand(frames, H, W, Cn) < 0.1] = -np.inf
            x[:, :min(H, 3), :min(W, 3), :Cn // 2] = -np.inf
            x = _q(x, _fmt_name(dtype))
            ref = ir.maxpool_hw_ref(x, k, stride, pad)
            assert np.all(ref < 0) and np.isinf(ref).any()
            _poison(ref.shape, torch.float32 if dtype == 'fp32' else nm.h16())
            out = ops.maxpool_hw(_dev(x, dtype), _dt(ops, dtype), k, stride, pad)
            torch.cuda.synchronize()
            got = out.float().cpu().numpy()
            assert got.shape == ref.shape
            assert np.array_equal(got.astype(np.float64), ref), 'maxpool_hw %s k%d s%d p%d %r C=%d' % (dtype, k, stride, pad, (frames, H, W), Cn)


# ---- hi / lo bf16 split -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('npos,Cn', [(1000, 64), (333, 192), (8192 * 256 // 8 + 37, 64), (8192 * 256 // 24 + 5, 192)])
def test_split_bf16x2_bit_for_bit(ops, npos, Cn):
    """hi = bf16(x), lo = bf16(x - hi) in the documented line layout, past the 8192-block cap (one thread per 8 channels)."""
    if nm.h16() != torch.bfloat16:
        pytest.skip('bf16 build only')
    rs = np.random.RandomState(npos % 1000 + Cn)
    x = (rs.randn(npos, Cn) * np.exp(rs.uniform(-30, 30, (npos, 1)))).astype(np.float32)
    x[0, :8] = [0., 1., -1., 1. + 2. ** -8, 1. + 2. ** -9, 3.0e38, 2. ** -100, -3.3]
    ref = torch.from_numpy(ir.split_bf16x2_ref(x)).to(torch.bfloat16)
    _poison((npos, 2 * Cn), torch.bfloat16)
    out = ops.split_bf16x2(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16)), 'split_bf16x2 npos=%d C=%d' % (npos, Cn)


# ---- frame gather / scatter -------------------------------------------------------------------------------------------------------
def _copy_frames_raw(ops, src, src_idx, dst, dst_idx, n, frame_bytes):
    ia = lambda v: (C.c_int * max(len(v), 1))(*[int(i) for i in v])
    ops.ctx().call('dat_copy_frames', ops._stream(), ops._ptr(src), ia(src_idx), ops._ptr(dst), ia(dst_idx), n, C.c_longlong(frame_bytes))


@pytest.mark.parametrize('n', [0, 1, 128, 129, 300])
@pytest.mark.parametrize('words', [4, 4 * 1000 + 12])
def test_copy_frames(ops, words, n):
    """Frames of one 16-byte vector and of 1003 (not a multiple of a block's 256); index tables of exactly one chunk of 128, one more,
    and three chunks; source frames repeated; every destination frame outside the table keeps its contents."""
    rs = np.random.RandomState(n + words)
    src = rs.randint(-2 ** 31, 2 ** 31 - 1, (n // 2 + 3, words), dtype=np.int64).astype(np.int32)
    dst = np.full((n + 9, words), 0x5A5A5A5A, np.int32)
    src_idx = rs.randint(0, src.shape[0], n)
    dst_idx = rs.permutation(dst.shape[0])[:n]
    if n > 1:
        assert len(set(src_idx)) < n
    ref = ir.copy_frames_ref(src, src_idx, dst, dst_idx)
    d = torch.from_numpy(dst).cuda()
    if n:
        ops.copy_frames(torch.from_numpy(src).cuda(), list(src_idx), d, list(dst_idx))
    else:
        _copy_frames_raw(ops, torch.from_numpy(src).cuda(), [], d, [], 0, words * 4)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), ref)


def test_copy_frames_larger_than_the_capped_grid(ops):
    """A frame above 1024 blocks * 256 threads * 8 vectors: blocks_per_frame is capped and every thread strides (the trunk-cache
    frames of the benchmark are 8 MB)."""
    vecs = 1024 * 256 * 8 + 256 * 3 + 5
    words = vecs * 4
    assert words * 4 > 1024 * 256 * 16 and (vecs + 2047) // 2048 > 1024
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (3, words), dtype=torch.int32, device='cuda')
    dst = torch.full((4, words), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    before = dst.clone()
    ops.copy_frames(src, [2, 0, 2], dst, [3, 0, 1])
    torch.cuda.synchronize()
    assert torch.equal(dst[3], src[2]) and torch.equal(dst[0], src[0]) and torch.equal(dst[1], src[2]) and torch.equal(dst[2], before[2])


def test_copy_frames_rejects_bad_arguments(ops):
    from detectandtrack_amd.libdat import DatError
    src = torch.arange(64, dtype=torch.int32, device='cuda').view(4, 16)
    dst = torch.full((4, 16), 7, dtype=torch.int32, device='cuda')
    with pytest.raises(DatError, match='negative frame index'):
        _copy_frames_raw(ops, src, [1, -1], dst, [0, 2], 2, 64)
    with pytest.raises(DatError, match='negative frame index'):
        _copy_frames_raw(ops, src, [1, 2], dst, [-3, 2], 2, 64)
    with pytest.raises(DatError, match='multiple of 16'):
        ops.copy_frames(src.view(8, 8)[:, :6].contiguous(), [1], dst.view(8, 8)[:, :6].contiguous(), [0])
    torch.cuda.synchronize()
    assert bool((dst == 7).all())


# ---- word scatter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('view', ['float', 'int32'])
@pytest.mark.parametrize('n', [0, 1, 257, 100000])
def test_scatter_words(ops, n, view):
    """Distinct offsets including the first and the last word; offsets below 0 and at / past the end are ignored (the kernel's
    guard); every other word keeps its bits (NaN payloads included)."""
    rs = np.random.RandomState(n + len(view))
    words = 3 * n + 11
    dst = rs.randint(-2 ** 31, 2 ** 31 - 1, words, dtype=np.int64).astype(np.int32)
    offs = (rs.permutation(words - 2)[:n] + 1).astype(np.int32)            # distinct, inside (0, words - 1)
    vals = rs.randint(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32)
    if n >= 1:
        offs[0] = words - 1
    if n > 6:
        offs[1] = 0
        offs[2:6] = [-1, words, words + 5, -2 ** 31]
    ref = ir.scatter_words_ref(dst, offs, vals)
    if n > 6:
        assert ref[0] == vals[1] and ref[-1] == vals[0]
    if view == 'float':
        d, v = torch.from_numpy(dst).view(torch.float32).cuda(), torch.from_numpy(vals).view(torch.float32).cuda()
    else:
        d, v = torch.from_numpy(dst).cuda(), torch.from_numpy(vals).cuda()
    ops.scatter_words(d, torch.from_numpy(offs).cuda(), v)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().view(torch.int32).numpy(), ref)
