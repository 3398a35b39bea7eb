"""The float64 references of tests/infer_refs.py against the operators they restate (the hand-worked RoIAlign answers, the oracle's
fp32 RoIAlign and keypoint tail), the roi sets of tests/test_gpu_infer_kernels.py against the conditions under which every roi and
every element can be compared, and the per-element bound against simulated kernel faults -- on the CPU, before any GPU run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import roi_align as ora
from tests import infer_refs as ir
from tests import numerics as nm
from tests import train_refs as tr
from tests.test_gpu_infer_kernels import ROI_CASES, ROI_N, roi_inputs
from tests.test_oracle_golden import roi_align_known_answers

f32 = np.float32


@pytest.mark.parametrize('case', roi_align_known_answers(), ids=lambda c: c[0])
def test_roi_align_ref_reproduces_the_hand_worked_answers(case):
    """Samples exactly on a validity cut-off included (strict=False: decided in float64, where these coordinates are exact)."""
    name, feat, rois, pooled, scale, sampling, exp = case
    ref, ab, ex, K = ir.roi_align_ref([feat.transpose(0, 2, 3, 1)], [scale], rois, 1, 1, 0, pooled, sampling, strict=False)
    np.testing.assert_array_equal(ref.transpose(0, 3, 1, 2).astype(f32), exp)
    assert np.all(ab >= np.abs(ref)) and np.all(ex >= 0)


def _levels_fp32(rois, Tr, n_levels, k_min, canon_scale, canon_level):
    """The level expression of roi_align_kernel (csrc/roi_align.hip) in float32 numpy: -> (level index, the unfloored level)."""
    r = np.asarray(rois, f32)
    asum = np.zeros(r.shape[0], f32)
    for t in range(Tr):
        w = r[:, 3 + 4 * t] - r[:, 1 + 4 * t] + f32(1)
        h = r[:, 4 + 4 * t] - r[:, 2 + 4 * t] + f32(1)
        asum = asum + w * h
    sarea = np.sqrt(asum / f32(Tr))
    raw = f32(canon_level) + np.log2(sarea / f32(canon_scale) + f32(1e-6))
    assert raw.dtype == f32
    lv = np.clip(np.floor(raw), f32(k_min), f32(k_min + n_levels - 1))
    return lv.astype(np.int64) - k_min, raw


@pytest.mark.parametrize('case', ROI_CASES, ids=lambda c: c[0])
def test_every_roi_of_the_gpu_cases_can_be_compared(case):
    """No sample within fp32 error of a validity cut-off (the reference raises there), every level of a multi-level case receives rois,
    and no roi where the kernel's fp32 level and the reference's float64 level differ or could: the unfloored fp32 level stays two of
    its ulps away from an integer, where log2f (an ulp of a value below 4) and the addition (half an ulp) together move it by less than
    one.  (A side exactly on a boundary sits 1e-6 / (x ln 2) above it, by the 1e-6 of the expression: two ulps at level 5.)"""
    name, levels, R, T, Tr, t0, P, samp, Cn, seed = case
    rois, feats, scales = roi_inputs(case, 'fp32', channels=8)
    assert rois.shape == (R, 4 * Tr + 1) and set(rois[:, 0]) == set(range(ROI_N))
    ref, ab, ex, K = ir.roi_align_ref(feats, scales, rois, T, Tr, t0, P, samp, 2, 224., 4)          # raises on a cut-off sample
    assert K == 4 * samp * samp if samp else K > 16
    lv64 = tr.roi_levels(rois, Tr, levels, 2, 224., 4)
    if levels > 1:
        assert set(lv64) == set(range(levels)), 'levels without rois: %r' % (set(range(levels)) - set(lv64))
        lv32, raw = _levels_fp32(rois, Tr, levels, 2, 224., 4)
        np.testing.assert_array_equal(lv32, lv64)
        assert np.all(np.abs(raw.astype(np.float64) - np.round(raw)) >= 2 * np.spacing(np.abs(raw)).astype(np.float64))
    assert np.all(np.abs(ref).reshape(R * Tr, -1).max(1)[:4 * Tr] > 0)


def _oracle_per_level(case, rois, feats, scales, rows):
    """oracle/roi_align.py (fp32, one level per call) on the first `rows` rois of a case, level by level -> [rows*Tr, P, P, C]."""
    name, levels, R, T, Tr, t0, P, samp, Cn, seed = case
    rois = rois[:rows]
    lv = tr.roi_levels(rois, Tr, levels, 2, 224., 4)
    out = np.zeros((rows * Tr, P, P, feats[0].shape[-1]), f32)
    for li in range(levels):
        sel = np.nonzero(lv == li)[0]
        if len(sel) == 0:
            continue
        f = feats[li]
        if Tr == 1:
            rb = rois[sel].copy()
            rb[:, 0] = rb[:, 0] * T + t0
            y = ora.roi_align_2d(f.transpose(0, 3, 1, 2), rb, P, scales[li], samp).transpose(0, 2, 3, 1)[:, None]
        else:
            f5 = f.reshape((ROI_N, T) + f.shape[1:]).transpose(0, 4, 1, 2, 3)
            y = ora.roi_align_tube(f5, rois[sel], P, scales[li], samp).transpose(0, 2, 3, 4, 1)              # (r, T, P, P, C)
        out.reshape((rows, Tr) + out.shape[1:])[sel] = y
    return out


@pytest.mark.parametrize('case', ROI_CASES, ids=lambda c: c[0])
def test_roi_align_ref_agrees_with_the_oracle_to_fp32_rounding(case):
    """The oracle computes the same operator in fp32 statement by statement: it must lie inside the fp32 bound of the reference (the
    first 48 rois of a set: the hand-placed ones and random ones; three channels)."""
    name, levels, R, T, Tr, t0, P, samp, Cn, seed = case
    rois, feats, scales = roi_inputs(case, 'fp32', channels=3)
    rows = min(R, 48)
    ref, ab, ex, K = ir.roi_align_ref(feats, scales, rois[:rows], T, Tr, t0, P, samp, 2, 224., 4)
    nm.assert_elementwise(_oracle_per_level(case, rois, feats, scales, rows), ref, ab, K, 'fp32', 'oracle RoIAlign ' + name, ex)


@pytest.mark.parametrize('up,Tr', [(2, 1), (4, 1), (2, 2), (4, 3)])
def test_kps_finalize_ref_reproduces_the_oracle_tail(up, Tr):
    """oracle.net3d.Net.kps_outputs_2d (ConvTranspose k4 s2 p1, then the fixed bilinear ConvTranspose) on frames r*Tr + t, its
    kps_score_lowres folded into the sub-pixel channels that dat_kps_finalize reads; channel t*K + k of roi r is frame r*Tr + t."""
    from oracle.net3d import Net, opts_for
    rs = np.random.RandomState(up + Tr)
    R, K, Cin, S, cs = 3, 5, 6, 7, 24
    net = Net({'kps_score_lowres_w': rs.randn(Cin, K, 4, 4).astype(f32), 'kps_score_lowres_b': rs.randn(K).astype(f32)},
              opts_for('R18', kps_up_scale=up))
    out = net.kps_outputs_2d(torch.from_numpy(rs.randn(R * Tr, Cin, S, S).astype(f32))).numpy()
    low = net.blobs['kps_score_lowres'].numpy()                                # [R*Tr, K, 2S, 2S] fp32
    sub = np.full((R * Tr, S, S, cs), 1e6, f32)
    sub[..., :4 * K] = low.reshape(R * Tr, K, S, 2, S, 2).transpose(0, 2, 4, 3, 5, 1).reshape(R * Tr, S, S, 4 * K)
    ref = tr.kps_finalize_ref(sub, R, Tr, K, up)
    ab = tr.kps_finalize_ref(np.abs(sub), R, Tr, K, up)
    M = 2 * S * up
    assert ref.shape == (R, Tr * K, M, M)
    nm.assert_elementwise(out.reshape(R, Tr * K, M, M), ref, ab, 4, 'fp32', 'oracle keypoint tail up=%d Tr=%d' % (up, Tr))


def test_the_one_line_references_on_hand_worked_values():
    x = np.arange(2 * 3 * 1 * 1 * 2, dtype=f32).reshape(6, 1, 1, 2)               # N = 2, T = 3, c = 2
    ref, ab = ir.time_avg_ref(x - 4, 2, 3)
    np.testing.assert_array_equal(ref.reshape(2, 2), [[-2, -1], [4, 5]])
    np.testing.assert_allclose(ab.reshape(2, 2), [[2, 5 / 3.], [4, 5]], rtol=1e-15)
    y = np.array([[[[1, 9], [2, 9]], [[3, 9], [-6, 9]]]], f32)                     # 1 frame, 2 x 2, C = 1 of Cs = 2
    ref, ab = ir.spatial_mean_ref(y, 1)
    assert ref.tolist() == [[0.0]] and ab.tolist() == [[3.0]]
    p, extra = ir.softmax_rows_ref(np.array([[0., np.log(3.), 50.], [7., 7., -50.]]), 2)
    np.testing.assert_allclose(p, [[0.25, 0.75], [0.5, 0.5]], rtol=1e-15)
    assert extra[1].tolist() == [0.0, 0.0] and np.all(extra[0] > 0)
    m = np.full((1, 3, 3, 1), -np.inf, f32)
    m[0, 2, 2, 0], m[0, 0, 1, 0] = -5, -7
    np.testing.assert_array_equal(ir.maxpool_hw_ref(m, 3, 2, 1)[0, :, :, 0], [[-7, -7], [-np.inf, -5]])
    np.testing.assert_array_equal(ir.maxpool_hw_ref(m, 2, 2, 0)[0, :, :, 0], [[-7]])
    v = np.zeros((1, 128), f32)
    v[0, 0], v[0, 1], v[0, 64] = 1 + 2. ** -9 + 2. ** -12, 1 + 2. ** -9 + 2. ** -20, -3
    s = ir.split_bf16x2_ref(v)                                               # chunk 0: hi at 0..63, lo at 64..127; chunk 1: 128.., 192..
    assert s.shape == (1, 256) and s[0, 0] == 1 and s[0, 64] == 2. ** -9 + 2. ** -12 and s[0, 1] == 1 and s[0, 65] == 2. ** -9
    assert s[0, 128] == -3 and s[0, 192] == 0
    src, dst = np.arange(6).reshape(3, 2), np.full((4, 2), -1)
    np.testing.assert_array_equal(ir.copy_frames_ref(src, [2, 2, 0], dst, [0, 3, 1]), [[4, 5], [0, 1], [-1, -1], [4, 5]])
    w = ir.scatter_words_ref(np.zeros((2, 2), f32), [3, -1, 4, 0], np.array([1.5, 9, 9, -2], f32))
    np.testing.assert_array_equal(w, [[-2, 0], [0, 1.5]])


# ---- the bound against simulated kernels ----------------------------------------------------------------------------------------------
def _sim_roi_align(feats, scales, rois, T, Tr, t0, P, samp, fault=None):
    """roi_align_kernel (csrc/roi_align.hip) statement by statement in float32 numpy, one output cell at a time, with one of the
    faults the GPU tests must catch: 'drop_tap' (the last sample of every cell loses its fourth tap), 'inv_fixed' (the average over
    an adaptive grid divides by the fixed 2 x 2), 'tube_t0' (every frame of a tube reads frame t0)."""
    rois = np.asarray(rois, f32)
    lv = tr.roi_levels(rois, Tr, len(feats), 2, 224., 4)
    Cn = feats[0].shape[-1]
    out = np.zeros((rois.shape[0] * Tr, P, P, Cn), f32)
    for r in range(rois.shape[0]):
        f, sc = feats[lv[r]], f32(scales[lv[r]])
        H, W = f.shape[1:3]
        for t in range(Tr):
            frame = int(rois[r, 0]) * T + (t0 if Tr == 1 or fault == 'tube_t0' else t)
            x1, y1, x2, y2 = [v * sc for v in rois[r, 1 + 4 * t:5 + 4 * t]]
            rw, rh = max(x2 - x1, f32(1)), max(y2 - y1, f32(1))
            bw, bh = rw / f32(P), rh / f32(P)
            gh = samp if samp > 0 else int(np.ceil(rh / f32(P)))
            gw = samp if samp > 0 else int(np.ceil(rw / f32(P)))
            inv = f32(1) / f32(4 if fault == 'inv_fixed' else gh * gw)
            for ph in range(P):
                for pw in range(P):
                    acc = np.zeros(Cn, f32)
                    for iy in range(gh):
                        y = y1 + f32(ph) * bh + (f32(iy) + f32(.5)) * bh / f32(gh)
                        for ix in range(gw):
                            x = x1 + f32(pw) * bw + (f32(ix) + f32(.5)) * bw / f32(gw)
                            yy = y
                            if yy < -1 or yy > H or x < -1 or x > W:
                                continue
                            yy, x = max(yy, f32(0)), max(x, f32(0))
                            yl, xl = int(yy), int(x)
                            if yl >= H - 1:
                                yh = yl = H - 1
                                yy = f32(yl)
                            else:
                                yh = yl + 1
                            if xl >= W - 1:
                                xh = xl = W - 1
                                x = f32(xl)
                            else:
                                xh = xl + 1
                            ly, lx = yy - f32(yl), x - f32(xl)
                            hy, hx = f32(1) - ly, f32(1) - lx
                            last = fault == 'drop_tap' and iy == gh - 1 and ix == gw - 1
                            acc += hy * hx * f[frame, yl, xl] + hy * lx * f[frame, yl, xh] + ly * hx * f[frame, yh, xl] + \
                                (f32(0) if last else ly * lx) * f[frame, yh, xh]
                    out[r * Tr + t, ph, pw] = acc * inv
    return out


_SIM = {}


def _sim_case(name, fmt, rows=12):
    """(reference tuple, inputs) of the first rows rois of a GPU case at 8 channels: the hand-placed rois and three random ones."""
    key = (name, fmt)
    if key not in _SIM:
        case = [c for c in ROI_CASES if c[0] == name][0]
        _, levels, R, T, Tr, t0, P, samp, Cn, seed = case
        rois, feats, scales = roi_inputs(case, fmt, channels=8)
        rois = rois[:rows]
        _SIM[key] = (ir.roi_align_ref(feats, scales, rois, T, Tr, t0, P, samp, 2, 224., 4), (feats, scales, rois, T, Tr, t0, P, samp))
    return _SIM[key]


@pytest.mark.parametrize('name', ['tube2_c64', 'tube3_adaptive_c72', 'keyframe_p14_c256'])
def test_the_bound_accepts_an_fp32_roi_align_and_its_16_bit_outputs(name):
    """The kernel's arithmetic in numpy float32 lies inside the bound, as computed and rounded once to either 16-bit format."""
    for fmt in ('fp32', 'bf16', 'fp16'):
        (ref, ab, ex, K), args = _sim_case(name, fmt)
        got = _sim_roi_align(*args)
        nm.assert_elementwise(got if fmt == 'fp32' else nm.q16(got, fmt), ref, ab, K, fmt, 'simulated roi_align %s %s' % (name, fmt), ex)


@pytest.mark.parametrize('name,fault', [('tube2_c64', 'drop_tap'), ('tube3_adaptive_c72', 'drop_tap'), ('tube3_adaptive_c72', 'inv_fixed'),
                                        ('tube2_p14_adaptive_c256', 'inv_fixed'), ('tube2_c64', 'tube_t0'), ('tube3_adaptive_c72', 'tube_t0')])
@pytest.mark.parametrize('fmt', ['fp32', 'bf16'])
def test_the_bound_rejects_a_faulty_roi_align(name, fault, fmt):
    (ref, ab, ex, K), args = _sim_case(name, fmt, rows=12 if fault != 'inv_fixed' or 'p14' not in name else 6)
    got = _sim_roi_align(*args, fault=fault)
    with pytest.raises(AssertionError, match='outside the per-element bound'):
        nm.assert_elementwise(got if fmt == 'fp32' else nm.q16(got, fmt), ref, ab, K, fmt, 'faulty roi_align', ex)


def test_the_bound_rejects_fp32_outputs_rounded_through_bf16():
    """An fp32 path whose result passes through bf16 (2^-9 relative) is far outside the fp32 bound; so is a fp16 output that does."""
    (ref, ab, ex, K), args = _sim_case('tube2_c64', 'fp32')
    got = _sim_roi_align(*args)
    with pytest.raises(AssertionError, match='outside the per-element bound'):
        nm.assert_elementwise(nm.q16(got, 'bf16'), ref, ab, K, 'fp32', 'fp32 roi_align through bf16', ex)
    (ref, ab, ex, K), args = _sim_case('tube2_c64', 'fp16')
    with pytest.raises(AssertionError, match='outside the per-element bound'):
        nm.assert_elementwise(nm.q16(nm.q16(_sim_roi_align(*args), 'bf16'), 'fp16'), ref, ab, K, 'fp16', 'fp16 roi_align through bf16', ex)


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
def test_the_bound_rejects_a_time_avg_that_rounds_its_sum_to_16_bits(fmt, T=3):
    """time_avg_kernel sums in fp32 and rounds once; rounding the sum before the division rounds twice.  On the GPU test's input
    at T = 3: dividing by a power of two commutes with the rounding, so at T = 2 and 8 the two kernels are the same function."""
    rs = np.random.RandomState(30 + T)
    N, hwc = 3, (5, 7, 13)
    x = nm.q16((rs.randn(*((N * T,) + hwc)) * 3 + 1).astype(f32), fmt)
    ref, ab = ir.time_avg_ref(x, N, T)
    s = np.zeros((N,) + hwc, f32)
    for t in range(T):
        s = s + x.reshape((N, T) + hwc)[:, t]
    nm.assert_elementwise(nm.q16(s / f32(T), fmt), ref, ab, T, fmt, 'simulated time_avg')
    with pytest.raises(AssertionError, match='outside the per-element bound'):
        nm.assert_elementwise(nm.q16(nm.q16(s, fmt) / f32(T), fmt), ref, ab, T, fmt, 'time_avg with a 16-bit sum')


def test_the_bound_rejects_a_spatial_mean_on_the_wrong_stride_and_a_softmax_that_reads_its_padding():
    rs = np.random.RandomState(5)
    x = rs.randn(4, 7, 7, 256).astype(f32) + 0.5
    ref, ab = ir.spatial_mean_ref(x, 200)
    good = x[..., :200].reshape(4, 49, 200).sum(1, dtype=f32) / f32(49)
    nm.assert_elementwise(good, ref, ab, 49, 'fp32', 'simulated spatial_mean')
    wrong = x.reshape(-1)[:4 * 49 * 200].reshape(4, 49, 200).sum(1, dtype=f32) / f32(49)          # Cs taken as C
    with pytest.raises(AssertionError, match='outside the per-element bound'):
        nm.assert_elementwise(wrong, ref, ab, 49, 'fp32', 'spatial_mean with Cs = C')
    lg = (rs.randn(50, 8) * 4).astype(f32)
    p, extra = ir.softmax_rows_ref(lg, 5)
    e = np.exp(lg[:, :5] - lg[:, :5].max(1, keepdims=True)).astype(f32)
    nm.assert_elementwise(e / e.sum(1, keepdims=True, dtype=f32), p, p, 5, 'fp32', 'simulated softmax', extra)
    e = np.exp(lg[:, :6] - lg[:, :6].max(1, keepdims=True)).astype(f32)
    with pytest.raises(AssertionError, match='outside the per-element bound'):
        nm.assert_elementwise((e / e.sum(1, keepdims=True, dtype=f32))[:, :5], p, p, 5, 'fp32', 'softmax over K + 1', extra)
