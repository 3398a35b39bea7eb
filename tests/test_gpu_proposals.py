"""The kernels that select and order -- csrc/proposals.hip K0-K3, rpn_emit_kernel, collect_rois_kernel and csrc/detections.hip
det_select_kernel, det_limit_emit_kernel -- against an exact host statement, bit for bit and in order.

The inputs (tests/proposals_cases.py) cluster and tie where the uniform random scores of tests/test_gpu_kernels.py never do, and the
proposal calls run with nms_thresh 2.0: no IoU exceeds 1, so the call returns K3's sorted, filtered list itself and a wrong tie
order or two swapped neighbours show.  The reference is tests/proposals_ref.py (checked on the CPU by
tests/test_proposals_ref_cpu.py, which also shows that every selection case tells a reversed tie rule and a cut moved by one
apart); the detection kernels are compared with oracle/box_results.py on inputs whose size deltas are zero.  Every comparison is
assert_array_equal; the one exception, the mid-range probabilities of the sigmoid path, is stated at that test.

Head tensors are built in torch as [frames, H, W, cstride] (no conversion kernel runs), fp32 or the loaded build's 16-bit format.
"""
import numpy as np
import pytest
import torch

from tests import proposals_cases as pc
from tests import proposals_ref as pr

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def _fmt16(ops):
    return 'fp16' if ops.L.H16 == 'fp16' else 'bf16'


_UPLOADED = {}


def _specs(ops, name, fmt='fp32'):
    """The case's device level specs (heads uploaded once per module run)."""
    if (name, fmt) not in _UPLOADED:
        case = pc.build(name, fmt)
        specs = []
        for head, lv in case.levels:
            t = _dev(head)
            if case.dtype == 1:
                t = t.to(ops.H16_DTYPE)          # exact: the values already are of that format
                assert torch.equal(t.float().cpu(), torch.from_numpy(np.array(head)))
            specs.append(ops.RpnLevelSpec(t, lv.H, lv.W, lv.A, lv.T, lv.feat_stride, lv.cstride, lv.logit_off, lv.delta_off, lv.frame,
                                          _dev(lv.anchors), apply_sigmoid=lv.apply_sigmoid, per_frame=lv.per_frame))
        _UPLOADED[(name, fmt)] = specs
    return _UPLOADED[(name, fmt)]


def _run(ops, name, fmt='fp32'):
    case = pc.build(name, fmt)
    kw = dict(batch_idx=case.batch_idx)
    if case.n_images > 1:
        kw.update(n_images=case.n_images, frame_stride=case.frame_stride)
    rois, probs, counts = ops.rpn_proposals(_specs(ops, name, fmt), case.dtype, case.im_info if case.n_images > 1 else case.im_info[0],
                                            case.pre_nms, case.post_nms, case.nms_thresh, case.min_size, **kw)
    nl = len(case.levels)
    cols = rois.shape[-1]
    return (rois.cpu().numpy().reshape(case.n_images, nl, case.post_nms, cols), probs.cpu().numpy().reshape(case.n_images, nl, case.post_nms),
            counts.cpu().numpy().reshape(case.n_images, nl))


def _assert_exact(got, ref, what, probs_exact=True):
    """counts equal; rois and probs bit-equal and in order; rows past the count are the zeros the wrapper allocated."""
    rois, probs, counts = got
    for i, per_level in enumerate(ref):
        for l, (r_rois, r_probs, _) in enumerate(per_level):
            n = r_rois.shape[0]
            assert counts[i, l] == n, (what, i, l, counts[i, l], n)
            np.testing.assert_array_equal(rois[i, l, :n], r_rois, err_msg='%s image %d level %d' % (what, i, l))
            if probs_exact:
                np.testing.assert_array_equal(probs[i, l, :n], r_probs, err_msg='%s image %d level %d' % (what, i, l))
            assert not rois[i, l, n:].any() and not probs[i, l, n:].any(), (what, i, l)


def _check(ops, name, fmt='fp32'):
    got = _run(ops, name, fmt)
    _assert_exact(got, pc.reference(name, fmt), name)
    return got


# ---- selection ------------------------------------------------------------------------------------------------------------------
def test_one_bin_all_keys_distinct(ops):
    """33 075 distinct keys in one histogram bin: n_gt = 0, the radix select runs over the whole level."""
    _check(ops, 'one_bin_distinct')


@pytest.mark.parametrize('pre', pc.TIE_PRE)
@pytest.mark.parametrize('half', sorted(pc.TIE_V))
def test_cut_inside_a_tie_group(ops, half, pre):
    """The cut divides a group of equal scores that has a higher group above it and members in all three K0 chunks; the last member
    taken has an index above 65535, so the upper index digits of the composite decide.  Even and odd bin: the two halves of K0's
    packed counters.  pre_nms 1024 / 1025: K3's one and two entries per thread."""
    _check(ops, 'tie_cut_%s_%d' % (half, pre))


def test_full_chunk_in_one_bin(ops):
    """66 600 equal scores, pre_nms 16384: 32 768 increments of one packed LDS counter in each of two K0 blocks, the largest LDS sort.
    The rows are the anchors 0 .. 16383 in order."""
    rois, probs, counts = _check(ops, 'full_chunk_one_bin')
    ref_rois, ref_probs, idx = pc.reference('full_chunk_one_bin')[0][0]
    assert counts[0, 0] == 16384 and idx.tolist() == list(range(16384))
    np.testing.assert_array_equal(rois[0, 0, :64], ref_rois[:64])
    np.testing.assert_array_equal(rois[0, 0, 16384 - 64:16384], ref_rois[-64:])


def test_whole_boundary_bin_taken(ops):
    """need == n_bnd: the branch without a radix select; the bin's ten-fold ties still sort by index."""
    _check(ops, 'whole_boundary_bin')


def test_pre_nms_above_the_anchor_count(ops):
    """k_eff = N for a level of one anchor and a level of 700, pre_nms 1000."""
    _check(ops, 'k_eff_n')


def test_cut_among_exact_zeros(ops):
    """The boundary bin is bin 0: composites with a zero score half, next to the sort's zero padding."""
    _check(ops, 'exact_zeros')


def test_large_and_small_level_in_one_launch(ops):
    """Level M (cut inside a tie group) and a 700-anchor level together, pre_nms 700: K0 blocks beyond the small level's anchors
    return, K2's grid is sized by the large level, the small level's k_eff is its N."""
    _check(ops, 'mixed_levels')


# ---- head formats and layouts ---------------------------------------------------------------------------------------------------
def test_16_bit_head(ops):
    """dtype 1: probabilities and deltas in the build's 16-bit format, equal keys throughout the selected rows."""
    _check(ops, 'head16', _fmt16(ops))


@pytest.mark.parametrize('name', ['sigmoid_path', 'sigmoid_zeros'])
def test_sigmoid_path(ops, name):
    """apply_sigmoid (the default): logits -100 -> probability exactly 0; 18, 24, 30 -> exactly 1.0, the index orders them; a grid of
    step 1/64 whose neighbouring probabilities are >= 2^-16 apart relatively, so every expf gives the reference's order.  The cut
    falls inside the grid (pre_nms 700) or among the zeros (5000).  Rows, order and boxes are exact, and so are the probabilities of
    the 1.0 and the 0 group; the grid's probabilities are held to the 1e-6 of test_rpn_proposals_vs_reference_golden against the
    float64 sigmoid (expf is not correctly rounded, so no exact statement of them exists; measured 8.5e-8 in both cases)."""
    got = _run(ops, name)
    ref = pc.reference(name)
    _assert_exact(got, ref, name, probs_exact=False)
    idx = ref[0][0][2]
    head, spec = pc.build(name).levels[0]
    logit = head[0, :, :, spec.logit_off:spec.logit_off + spec.A].reshape(-1)[idx].astype(np.float64)
    probs = got[1][0, 0, :idx.size]
    ones, zeros = logit >= 18, logit == -100
    assert ones.sum() == 300 and zeros.sum() == (500 if name == 'sigmoid_zeros' else 0)
    np.testing.assert_array_equal(probs[ones], np.ones(300, F32))
    np.testing.assert_array_equal(probs[zeros], np.zeros(zeros.sum(), F32))
    exact = np.where(zeros, 0.0, 1 / (1 + np.exp(-logit)))
    print('%s: max |prob - float64 sigmoid| = %.3e' % (name, np.abs(probs - exact).max()))
    np.testing.assert_allclose(probs, exact, rtol=0, atol=1e-6)
    assert (np.diff(probs) <= 0).all()


@pytest.mark.parametrize('per_frame', [0, 1])
def test_tubes(ops, per_frame):
    """T = 3: per_frame 0, and per_frame 1 with frame 1 of a 5-frame head (logits of frames 1..3 added in that order and divided
    by 3, deltas of tube frame t from head frame 1 + t); the averaged logits tie in some anchors and differ by one ulp in others."""
    _check(ops, 'tubes_per_frame%d' % per_frame)


# ---- filter, emit, NMS on -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('min_size', [16, 0, 1000])
def test_min_size_filter(ops, min_size):
    """pre_nms 2048 (two sorted entries per K3 thread) at im_info scale 1.3: min_size 16 (20.8 scaled) drops about a third of the rows
    all through the order, 0 none, 1000 every row -- count 0 and untouched outputs."""
    got = _check(ops, 'min_size_%d' % min_size)
    if min_size == 1000:
        assert got[2][0, 0] == 0 and not got[0].any() and not got[1].any()


def test_min_size_filter_behind_the_largest_sort(ops):
    """pre_nms 16384: sixteen sorted entries per K3 thread, about a third of them dropped by the filter."""
    _check(ops, 'min_size_largest_sort')


@pytest.mark.parametrize('post', [50, 600])
def test_post_nms_below_and_above_the_survivors(ops, post):
    """NMS on (0.7) over tied scores: the kept rows are the reference's, cut at post_nms 50 or all of them (post_nms 600)."""
    _check(ops, 'nms_post_%d' % post)


# ---- batch and reuse ------------------------------------------------------------------------------------------------------------
def test_batch_against_the_host(ops):
    """n_images 3, frame_stride 2 from frame 1 of 6-frame heads, batch_idx 4, two levels, three different im_info rows: every image
    against the host reference of its frame."""
    got = _check(ops, 'batch3')
    assert [got[0][i, 0, 0, 0] for i in range(3)] == [4., 5., 6.]


def test_context_reuse(ops):
    """A large call, a small one and the large one again on one stream and context: nothing a call leaves in the workspace
    (counters, histograms, lists, mask rows) reaches the next."""
    for name in ('full_chunk_one_bin', 'small700', 'full_chunk_one_bin'):
        _check(ops, name)


# ---- collect --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('counts', [[[40, 17, 40, 3, 25]], [[40, 0, 40, 3, 25]], [[0, 0, 0, 0, 0]],
                                    [[40, 17, 0, 3, 25], [0, 0, 0, 0, 1]]], ids=['full', 'empty_level', 'all_empty', 'two_images'])
@pytest.mark.parametrize('post', [50, 200])
def test_collect(ops, counts, post):
    """Probabilities shared across levels (ties go to the earlier level and row), an empty level, all levels empty, post_nms below
    and above the total, two images per launch."""
    rois, probs, counts = pc.collect_inputs(counts)
    ni = counts.shape[0]
    args = (rois, probs, counts) if ni > 1 else (rois[0], probs[0], counts[0])
    out, n_out = ops.collect_rois(*[_dev(a) for a in args], post)
    out, n_out = out.cpu().numpy().reshape(ni, post, 5), n_out.cpu().numpy()
    for i in range(ni):
        ref = pr.collect(rois[i], probs[i], counts[i], post)
        assert n_out[i] == ref.shape[0] == min(post, counts[i].sum())
        np.testing.assert_array_equal(out[i, :ref.shape[0]], ref)
        assert not out[i, ref.shape[0]:].any()


def test_collect_rejects_more_than_16384_candidates(ops):
    from detectandtrack_amd import libdat
    rois, probs, counts = torch.zeros((5, 3277, 5), device='cuda'), torch.zeros((5, 3277), device='cuda'), torch.zeros(5, dtype=torch.int32, device='cuda')
    with pytest.raises(libdat.DatError):
        ops.collect_rois(rois, probs, counts, 100)


# ---- detection select and limit --------------------------------------------------------------------------------------------------
XFORM_CLIP = float(pr.XFORM_CLIP)


def _det_check(ops, rois, n_rois, prob, pred, K, D, out_cap, scale=1.0):
    """dat_box_results against oracle.box_results on the first min(n_rois, cap) rows: both counts, the rows written bit-equal (box,
    score, class; keypoint rois), everything past them zero.  Returns the reference rows."""
    cap = rois.shape[0]
    dets, kp, n_out = ops.box_results(_dev(rois), torch.tensor([n_rois], dtype=torch.int32).cuda(), _dev(prob), _dev(pred), K, 1, scale,
                                      (pc.DET_H, pc.DET_W, 3), pc.DET_WEIGHTS, XFORM_CLIP, float(pc.DET_THRESH), 0.5, D, out_cap)
    n = min(n_rois, cap)
    ref_dets, ref_kp = pc.det_reference(rois[:n], prob[:n], pred[:n], K, D, scale)
    n_out, dets, kp = n_out.cpu().numpy(), dets.cpu().numpy(), kp.cpu().numpy()
    assert n_out[1] == ref_dets.shape[0], (n_out, ref_dets.shape)
    k = min(ref_dets.shape[0], out_cap)
    assert n_out[0] == k
    np.testing.assert_array_equal(dets[:k], ref_dets[:k])
    np.testing.assert_array_equal(kp[:k], ref_kp[:k])
    assert not dets[k:].any() and not kp[k:].any()
    return ref_dets


def test_det_select_two_rows_per_thread(ops):
    """R = 1025 rois: det_select_kernel's threads own two rows each."""
    rois, prob, pred = pc.det_clustered(51, 1025, 1040, 3, 800.0 / 720.0)
    ref = _det_check(ops, rois, 1025, prob, pred, 3, 100, 108, 800.0 / 720.0)
    assert ref.shape[0] == 100


def test_det_limit_emit_several_rows_per_thread(ops):
    """2500 boxes that do not overlap, no limit (D = 0): the one foreground class keeps all 2500 rows, so det_limit_emit_kernel's
    ordered emit owns three rows per thread (and det_select_kernel three)."""
    rois, prob, pred = pc.det_grid(2500, 2512, 2)
    ref = _det_check(ops, rois, 2500, prob, pred, 2, 0, 2512)
    assert ref.shape[0] == 2500


def test_det_limit_radix_select_with_several_rows_per_thread(ops):
    """The same 2500 rows under D = 100 and D = 1500: the radix select reads more rows than the block has threads."""
    rois, prob, pred = pc.det_grid(2500, 2512, 2)
    for D in (100, 1500):
        ref = _det_check(ops, rois, 2500, prob, pred, 2, D, D + 8)
        assert ref.shape[0] == D


def test_det_score_equal_to_the_threshold_is_dropped(ops):
    """score > SCORE_THRESH is strict: rows at exactly float32(0.05) go, rows one float above stay."""
    rois, prob, pred = pc.det_grid(200, 200, 3)
    thr = pc.DET_THRESH
    prob[0:200:4, 1] = thr
    prob[1:200:4, 1] = np.nextafter(thr, F32(1))
    prob[2:200:4, 1] = np.nextafter(thr, F32(0))
    prob[0:200:5, 2] = thr
    ref = _det_check(ops, rois, 200, prob, pred, 3, 0, 400)
    assert ref.shape[0] == 100 + 160 and (ref[:, 4] > thr).all() and (ref[:, 4] == np.nextafter(thr, F32(1))).sum() == 50


def _tie_scores(n_above, ties1, ties2, R=60):
    """Two foreground classes over R non-overlapping boxes: n_above distinct scores above 0.5, rows at exactly 0.5 (ties1 in class 1,
    ties2 in class 2), distinct scores below 0.5 (and above the threshold) for the rest."""
    rois, prob, pred = pc.det_grid(R, R, 3)
    slots = np.random.RandomState(61).permutation(2 * R)          # slot = 2 * row + (class - 1)
    tied = np.concatenate((slots[slots % 2 == 0][:ties1], slots[slots % 2 == 1][:ties2]))
    rest = slots[~np.isin(slots, tied)]
    flat = np.zeros(2 * R, F32)
    flat[tied] = 0.5
    flat[rest[:n_above]] = 0.5 + (1 + np.arange(n_above)) / 256.0
    flat[rest[n_above:]] = 0.5 - (1 + np.arange(rest.size - n_above)) / 512.0
    assert flat.min() > pc.DET_THRESH
    prob[:, 1:] = flat.reshape(R, 2)
    return rois, prob, pred


def test_det_limit_ties_at_the_dth_score(ops):
    """Five rows tie at the D-th best score, three in class 1 and two in class 2: the limit rule keeps D + 4 rows (`>=`), the first
    out_cap = D of them in class-major order are written."""
    D = 20
    rois, prob, pred = _tie_scores(D - 1, 3, 2)
    ref = _det_check(ops, rois, 60, prob, pred, 3, D, D)
    assert ref.shape[0] == D + 4 and (ref[:, 4] == 0.5).sum() == 5 and set(ref[ref[:, 4] == 0.5, 5].tolist()) == {1., 2.}
    _det_check(ops, rois, 60, prob, pred, 3, D, D + 4)          # and with room for all of them


def test_det_counts_at_the_limit(ops):
    """total == D (no select runs), D = 1, and no rois at all."""
    rois, prob, pred = pc.det_grid(60, 60, 3)
    assert _det_check(ops, rois, 60, prob, pred, 3, 120, 120).shape[0] == 120
    assert _det_check(ops, rois, 60, prob, pred, 3, 119, 120).shape[0] == 119
    assert _det_check(ops, rois, 60, prob, pred, 3, 1, 4).shape[0] == 1
    assert _det_check(ops, rois, 0, prob, pred, 3, 10, 10).shape[0] == 0


def test_det_n_rois_is_clamped_to_the_capacity(ops):
    rois, prob, pred = pc.det_grid(60, 60, 3)
    assert _det_check(ops, rois, 1 << 20, prob, pred, 3, 0, 120).shape[0] == 120
