"""tests/proposals_ref.py, the host statement the GPU proposal tests compare bit for bit against, is itself checked here without a
GPU: against the recorded outputs of the real GenerateProposalsOp, against oracle/proposals.py on tie-free inputs, on hand-worked
arrays for every tie rule, and against wrong selection rules (higher index first; the cut moved by one) that every tie case of
tests/proposals_cases.py must tell apart.  The inputs the GPU tests upload are checked too: their exp arguments are ones whose
float32 result does not depend on the last bits of a double exp."""
import numpy as np
import pytest

from oracle import proposals as op
from tests import proposals_cases as pc
from tests import proposals_ref as pr

F32 = np.float32


def _golden_level(golden, name):
    stride, pre, post, thr, min_size = golden[name + '_cfg']
    scores, deltas, anchors = golden[name + '_scores'], golden[name + '_deltas'], golden[name + '_anchors']
    A, T = anchors.shape[0], anchors.shape[1] // 4
    cat = np.concatenate([scores, deltas], axis=1)[0].transpose(1, 2, 0)
    H, W, C = cat.shape
    head = np.full((1, H, W, C + 3), 7.0, F32)
    head[0, :, :, :C] = cat
    return head, pr.Level(H, W, A, T, stride, C + 3, 0, A, 0, anchors), (int(pre), int(post), float(thr), float(min_size))


@pytest.mark.parametrize('name,count', [('gp_fpn3', 300), ('gp_fpn2_min', 200), ('gp_c4_T3', 150)])
def test_reference_matches_the_recorded_generate_proposals_op(golden, name, count):
    """The real GenerateProposalsOp (tests/golden/reference_host.npz): the same count, bit-equal probabilities, boxes within the
    2e-3 the device tests use against the same file (measured 3.1e-5, 7.6e-6, 4.6e-5: the recorded op's np.exp(float32) is a
    1-ulp exp, this reference rounds a float64 exp once)."""
    head, spec, args = _golden_level(golden, name)
    rois, probs, _ = pr.proposals(head, spec, golden[name + '_im_info'][0], *args)
    assert rois.shape == golden[name + '_rois'].shape and rois.shape[0] == count
    np.testing.assert_array_equal(probs, golden[name + '_probs'][:, 0])
    print(name, 'max box difference', np.abs(rois - golden[name + '_rois']).max())
    np.testing.assert_allclose(rois, golden[name + '_rois'], rtol=0, atol=2e-3)


@pytest.mark.parametrize('T,min_size', [(1, 0.), (1, 12.), (3, 0.)])
def test_reference_keeps_the_anchors_the_oracle_keeps(T, min_size):
    """oracle.proposals.generate_proposals on tie-free scores: the same rows in the same order (scores identify the anchors), boxes
    to the oracle's 1-ulp exp."""
    rs = np.random.RandomState(40 + T)
    H, W, A, stride = 14, 18, 3, 16
    anchors = pc.generate_anchors(float(stride), (64,), pc.RATIOS3, time_dim=T)
    scores = rs.permutation(H * W * A).astype(F32).reshape(1, A, H, W) / F32(1024)
    deltas = (rs.randn(1, 4 * A * T, H, W) * 0.4).astype(F32)
    im_info = np.array([[H * stride, W * stride, 1.1]], F32)
    ref_rois, ref_probs = op.generate_proposals(scores, deltas, im_info, anchors, 1. / stride, 300, 120, 0.7, min_size)
    cat = np.concatenate([scores, deltas], axis=1)[0].transpose(1, 2, 0)
    head = np.ascontiguousarray(cat[None])
    spec = pr.Level(H, W, A, T, stride, cat.shape[2], 0, A, 0, anchors)
    rois, probs, idx = pr.proposals(head, spec, im_info[0], 300, 120, 0.7, min_size)
    assert 20 < len(idx) == ref_rois.shape[0]
    np.testing.assert_array_equal(probs, ref_probs[:, 0])
    np.testing.assert_array_equal(pr.keys(head, spec)[idx], probs)
    np.testing.assert_allclose(rois, ref_rois, rtol=0, atol=2e-3)


def test_collect_keeps_the_rows_the_oracle_keeps():
    rs = np.random.RandomState(44)
    counts = [7, 0, 12, 3, 9]
    rois = rs.uniform(0, 100, (5, 12, 5)).astype(F32)
    probs = rs.permutation(60).astype(F32).reshape(5, 12) / 64
    for post in (10, 31, 100):
        ref = op.collect([rois[l, :c] for l, c in enumerate(counts)], [probs[l, :c, None] for l, c in enumerate(counts)], post)
        np.testing.assert_array_equal(pr.collect(rois, probs, counts, post), ref)


# ---- the tie rules on hand-worked arrays ----------------------------------------------------------------------------------------
def test_select_by_hand():
    k = np.array([0.5, 0.75, 0.5, 0.25, 0.75, 0.5, 0.0, 0.5], F32)
    #             0    1     2    3     4     5    6    7      -> 0.75: 1 4 | 0.5: 0 2 5 7 | 0.25: 3 | 0: 6
    assert pr.select(k, 1).tolist() == [1]
    assert pr.select(k, 2).tolist() == [1, 4]
    assert pr.select(k, 4).tolist() == [1, 4, 0, 2]            # the cut inside the 0.5 group: its lowest indices
    assert pr.select(k, 6).tolist() == [1, 4, 0, 2, 5, 7]      # the whole group
    assert pr.select(k, 8).tolist() == pr.select(k, 100).tolist() == [1, 4, 0, 2, 5, 7, 3, 6]       # k_eff = N, zero last
    assert pr.select(np.zeros(3, F32), 2).tolist() == [0, 1]
    ulp = np.array([0.5, np.nextafter(F32(0.5), F32(1)), 0.5], F32)
    assert pr.select(ulp, 3).tolist() == [1, 0, 2]             # one ulp decides before the index does


def test_keys_by_hand():
    """per_frame: ((l0 + l1) + l2) / 3 in float32, frames `frame .. frame + 2`, channel logit_off + a."""
    an = np.zeros((2, 12), F32)
    spec = pr.Level(1, 2, 2, 3, 16, 8, 1, 3, 1, an, per_frame=True)
    head = np.full((5, 1, 2, 8), 7.0, F32)
    l = np.array([[0.1, 0.2, 0.3, 0.4], [1e8, 3.0, 0.25, 0.7], [-1e8, 5.0, 0.5, 0.1]], F32)      # frames 1, 2, 3 x (w, a)
    head[1:4, 0, :, 1:3] = l.reshape(3, 2, 2)
    want = [((F32(l[0, i]) + F32(l[1, i])) + F32(l[2, i])) / F32(3) for i in range(4)]
    got = pr.keys(head, spec)
    assert got.dtype == F32 and got.tolist() == [float(v) for v in want]
    assert got[0] == 0.0            # (0.1 + 1e8) - 1e8 in float32: the order of the additions is part of the statement
    spec0 = pr.Level(1, 2, 2, 3, 16, 8, 1, 3, 2, an)
    assert pr.keys(head, spec0).tolist() == [float(v) for v in l[1]]
    sig = pr.Level(1, 2, 2, 1, 16, 8, 1, 3, 0, an[:, :4], apply_sigmoid=True)
    head[0, 0, :, 1:3] = np.array([-100, 18, 30, 0], F32).reshape(2, 2)
    assert pr.keys(head, sig).tolist() == [0.0, 1.0, 1.0, 0.5]       # exp(100) is inf in float32; exp(-18) vanishes against 1



def test_decode_and_filter_by_hand():
    """One 16 x 16 anchor at (0, 0) .. (15, 15), stride 16, a 3 x 2 map, image 40 x 30 (w x h)."""
    an = np.array([[0, 0, 15, 15]], F32)
    spec = pr.Level(2, 3, 1, 1, 16, 8, 0, 2, 0, an)
    head = np.zeros((1, 2, 3, 8), F32)
    head[0, 0, 1, 2:6] = [0.25, -0.5, 0., 10.]           # idx 1: shift (16, 0); dh clamps to log(1000 / 16)
    head[0, 1, 2, 2:6] = [0., 0., np.log(0.25), 0.]      # idx 5: shift (32, 16); width 4 before the clip
    boxes, ok = pr.decode([0, 1, 5], head, spec, (30., 40., 1.5), 4.)
    np.testing.assert_array_equal(boxes[0], [0, 0, 16, 16])       # zero deltas: centre 8, width 16 -> 8 +- 8 (bbox_transform's + 1)
    # idx 1: centre (16 + 8 + 4, 8 - 8), width 16, height 16 * 62.5 = 1000 -> clipped to the image rows 0 .. 29
    np.testing.assert_array_equal(boxes[1], [20, 0, 36, 29])
    # idx 5: centre x 40, width float32(exp(float64(float32(log 0.25)))) * 16 ~ 4 -> x in [38, 42] clipped to 39
    assert boxes[2, 0] == pytest.approx(38.0, abs=1e-5) and boxes[2].tolist()[1:] == [16.0, 39.0, 29.0]
    # min_size 4 * 1.5 = 6: idx 5 is ~2 wide after the clip and fails; with min_size 1 it passes
    assert ok.tolist() == [True, True, False]
    assert pr.decode([5], head, spec, (30., 40., 1.5), 1.)[1].tolist() == [True]
    assert pr.min_size_scaled(16., 1.3) == F32(16 * np.float64(F32(1.3))) and pr.min_size_scaled(16., 1.3).dtype == F32
    assert pr.min_size_scaled(0., 1.3) == 0


def test_tube_filter_needs_every_frame():
    an = np.tile(np.array([[0, 0, 15, 15]], F32), (1, 2))
    spec = pr.Level(1, 1, 1, 2, 16, 16, 0, 1, 0, an)
    head = np.zeros((1, 1, 1, 16), F32)
    head[0, 0, 0, 1 + 4 + 2] = np.log(0.125)              # frame 1 only: 2 wide
    boxes, ok = pr.decode([0], head, spec, (64., 64., 1.), 4.)
    assert not ok[0] and boxes[0, :4].tolist() == [0, 0, 16, 16]
    assert pr.proposals(head, spec, (64., 64., 1.), 10, 10, 2.0, 4.)[0].shape == (0, 9)
    assert pr.proposals(head, spec, (64., 64., 1.), 10, 10, 2.0, 1.)[0].shape == (1, 9)


def test_proposals_order_nms_switch_and_post_nms_by_hand():
    """Four identical boxes with scores 0.5, 0.75, 0.5, 0.75 and a far one: without suppression the sorted list itself
    (nms_thresh > 1), with it the best of the four and the far one; post_nms cuts after the NMS."""
    an = np.array([[0, 0, 15, 15]], F32)
    spec = pr.Level(1, 5, 1, 1, 0, 8, 0, 1, 0, an)        # feat_stride 0: every cell's anchor at the origin
    head = np.zeros((1, 1, 5, 8), F32)
    head[0, 0, :, 0] = [0.5, 0.75, 0.5, 0.75, 0.25]
    head[0, 0, 4, 1] = 3.0                                  # dx: the fifth box 48 to the right
    im = (64., 128., 1.)
    rois, probs, idx = pr.proposals(head, spec, im, 5, 5, 2.0, 0., batch_idx=3.)
    assert idx.tolist() == [1, 3, 0, 2, 4] and probs.tolist() == [0.75, 0.75, 0.5, 0.5, 0.25] and (rois[:, 0] == 3).all()
    assert pr.proposals(head, spec, im, 3, 5, 2.0, 0.)[2].tolist() == [1, 3, 0]
    assert pr.proposals(head, spec, im, 5, 5, 0.7, 0.)[2].tolist() == [1, 4]
    assert pr.proposals(head, spec, im, 5, 1, 0.7, 0.)[2].tolist() == [1]
    assert pr.proposals(head, spec, im, 5, 5, 1.0, 0.)[2].tolist() == [1, 4]      # IoU 1 >= 1 still suppresses: only > 1 switches it off


def test_collect_by_hand():
    rois = np.arange(3 * 3 * 2, dtype=F32).reshape(3, 3, 2)
    probs = np.array([[0.5, 0.25, 9.], [9., 9., 9.], [0.75, 0.5, 0.25]], F32)
    counts = [2, 0, 3]              # concatenation: L0r0 L0r1 L2r0 L2r1 L2r2
    want = [rois[2, 0], rois[0, 0], rois[2, 1], rois[0, 1], rois[2, 2]]      # ties: the earlier position, i.e. the lower level
    np.testing.assert_array_equal(pr.collect(rois, probs, counts, 100), want)
    np.testing.assert_array_equal(pr.collect(rois, probs, counts, 3), want[:3])
    assert pr.collect(rois, probs, [0, 0, 0], 4).shape == (0, 2)


def test_exp_is_safe_measures_the_distance_to_a_rounding_midpoint():
    """A float32 ulp is 2^29 double ulps, so the midpoints lie 2^29 apart: of random arguments a margin m refuses the share
    2 m / 2^29, exp(0) = 1 lies 2^27 below-side ulps from a midpoint, and arguments are clamped as the decode clamps them."""
    assert pr.exp_is_safe(np.zeros(1, F32), margin=2 ** 27)[0] and not pr.exp_is_safe(np.zeros(1, F32), margin=2 ** 27 + 1)[0]
    x = (np.random.RandomState(0).randn(400000) * 0.5).astype(F32)
    assert pr.exp_is_safe(x).all()
    for m in (2 ** 20, 2 ** 24):
        refused = 1.0 - pr.exp_is_safe(x, margin=m).mean()
        assert 0.8 * m / 2 ** 28 < refused < 1.25 * m / 2 ** 28, (m, refused)
    assert not pr.exp_is_safe(x, margin=2 ** 28 + 1).any()
    big = np.array([50.0, 4.5], F32)
    for m in (16, 2 ** 22, 2 ** 25, 2 ** 27):
        assert (pr.exp_is_safe(big, margin=m) == pr.exp_is_safe(np.array([pr.XFORM_CLIP]), margin=m)[0]).all()


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------
ALL_CASES = [(n, 'fp32') for n in pc.FP32_CASES] + [('head16', 'bf16'), ('head16', 'fp16')]


@pytest.mark.parametrize('name,fmt', ALL_CASES)
def test_gpu_case_inputs_are_decidable(name, fmt):
    """exp_is_safe on every delta a case holds, finite non-negative keys, and an expected output in which no two rows of a level are
    equal -- so a wrong order cannot produce the right rows."""
    case = pc.build(name, fmt)
    assert pr.exp_is_safe(case.deltas()).all()
    if fmt != 'fp32':
        for head, _ in case.levels:
            np.testing.assert_array_equal(head, pc.nm.q16(head.copy(), fmt))
    for per_level in pc.reference(name, fmt):
        for rois, probs, idx in per_level:
            assert np.unique(rois, axis=0).shape[0] == rois.shape[0] == np.unique(idx).shape[0]
            assert rois.shape[0] <= case.post_nms and (np.diff(probs) <= 0).all()


def _higher_index_first(k, pre_nms):
    k = np.asarray(k, F32)
    return np.lexsort((-np.arange(k.shape[0]), -k))[:min(int(pre_nms), k.shape[0])]


def _cut_moved_by_one(k, pre_nms):
    order = np.argsort(-np.asarray(k, F32), kind='stable')
    n = min(int(pre_nms), order.shape[0])
    return np.concatenate((order[:n - 1], order[n:n + 1])) if n < order.shape[0] else order[:n]


NOT_SELECTION = ('min_size_16', 'min_size_0', 'min_size_1000', 'min_size_largest_sort', 'nms_post_50', 'nms_post_600', 'batch3')      # filter, NMS, batch


@pytest.mark.parametrize('name,fmt', [(n, f) for n, f in ALL_CASES if n not in NOT_SELECTION])
def test_selection_cases_bite(name, fmt):
    """A reference with the tie rule reversed (higher index first) or with the cut moved by one (the last selected anchor replaced by
    the first one left out) expects other rows: no selection case is one that any order would satisfy."""
    case = pc.build(name, fmt)
    assert case.bites, name
    good = pc.reference(name, fmt)
    wrong = {'tie': _higher_index_first, 'cut': _cut_moved_by_one}
    for what in case.bites:
        bad = case.reference(wrong[what])
        changed = [not np.array_equal(g[0], b[0]) for gi, bi in zip(good, bad) for g, b in zip(gi, bi)]
        assert any(changed), (name, what)


def test_the_gpu_comparison_itself_bites():
    """tests/test_gpu_proposals._assert_exact, fed the reference's own rows as the device output, passes; fed the rows of a wrong
    selection rule it fails -- the comparison the GPU tests rest on sees a reversed tie and a moved cut."""
    from tests.test_gpu_proposals import _assert_exact

    def as_output(case, ref):
        cols = ref[0][0][0].shape[1]
        rois = np.zeros((case.n_images, len(case.levels), case.post_nms, cols), F32)
        probs = np.zeros(rois.shape[:3], F32)
        counts = np.zeros(rois.shape[:2], np.int32)
        for i, per_level in enumerate(ref):
            for l, (r, p, _) in enumerate(per_level):
                rois[i, l, :len(r)], probs[i, l, :len(p)], counts[i, l] = r, p, len(r)
        return rois, probs, counts
    for name in ('tie_cut_odd_bin_1025', 'mixed_levels'):
        case, good = pc.build(name), pc.reference(name)
        _assert_exact(as_output(case, good), good, name)
        for wrong in (_higher_index_first, _cut_moved_by_one):
            with pytest.raises(AssertionError):
                _assert_exact(as_output(case, case.reference(wrong)), good, name)
    # two neighbours swapped, one stale row past the count
    case, good = pc.build('small700'), pc.reference('small700')
    rois, probs, counts = as_output(case, good)
    rois[0, 0, [10, 11]] = rois[0, 0, [11, 10]]
    with pytest.raises(AssertionError):
        _assert_exact((rois, probs, counts), good, 'swapped')
    case, good = pc.build('nms_post_600'), pc.reference('nms_post_600')
    rois, probs, counts = as_output(case, good)
    rois[0, 0, -1, 2] = 1.0
    with pytest.raises(AssertionError):
        _assert_exact((rois, probs, counts), good, 'stale row')


def test_case_score_structure():
    """The structure the case descriptions promise, read off the keys."""
    # the tie group of every tie_cut case: members in all three K0 chunks (pre > 1), on both sides of index 65536, cut above it
    for b, v in pc.TIE_V.items():
        for pre in pc.TIE_PRE:
            case = pc.build('tie_cut_%s_%d' % (b, pre))
            head, spec = case.levels[0]
            k = pr.keys(head, spec)
            member = np.flatnonzero(k == F32(v))
            assert (k.view(np.uint32)[member] >> 16 == (0x3F00 if b == 'even_bin' else 0x3F01)).all()
            idx = pr.select(k, pre)
            taken = idx[k[idx] == F32(v)]
            assert 0 < taken.size < member.size and taken.max() >= 65536 and (k[idx] > F32(v)).sum() == pre // 3
            if pre > 1:
                assert set((member // 32768).tolist()) == {0, 1, 2} and member.min() < 65536
    # whole boundary bin: the selected set is everything at or above the bin, the bin holds ties
    case = pc.build('whole_boundary_bin')
    k = pr.keys(*case.levels[0])
    bins = k.view(np.uint32) >> 16
    assert (bins > 0x3F00).sum() == 200 and (bins == 0x3F00).sum() == 500 and np.unique(k[bins == 0x3F00]).size == 50
    # exact zeros: the cut falls among them
    case = pc.build('exact_zeros')
    k = pr.keys(*case.levels[0])
    assert (k > 0).sum() == 16000 < case.pre_nms < k.size and (k == 0).sum() > k.size // 2
    # tubes, per_frame: averaged logits that tie and averaged logits one float32 ulp apart
    for name in ('tubes_per_frame0', 'tubes_per_frame1'):
        case = pc.build(name)
        bits = np.unique(pr.keys(*case.levels[0]).view(np.uint32), return_counts=True)
        assert (bits[1] > 1).any() and (np.diff(bits[0].astype(np.int64)) == 1).any(), name
    # sigmoid grid: neighbouring probabilities at least 2^-16 apart, relatively (in float64)
    p = 1.0 / (1.0 + np.exp(-pc.SIGMOID_GRID.astype(np.float64)))
    assert (np.diff(p) / p[1:] >= 2.0 ** -16).all()
    assert np.exp(np.float64(-18)) < 2.0 ** -25
    # 16-bit heads: equal keys among the selected
    for fmt in ('bf16', 'fp16'):
        case = pc.build('head16', fmt)
        k = pr.keys(*case.levels[0])
        assert np.unique(k[pr.select(k, case.pre_nms)]).size < case.pre_nms
    # the min-size filter drops about a third, through the whole order; 0 drops nothing; 1000 everything
    n16 = pc.reference('min_size_16')[0][0][2].size
    assert 0.5 * 2048 < n16 < 0.8 * 2048, n16
    assert pc.reference('min_size_0')[0][0][2].size == 2048 and pc.reference('min_size_1000')[0][0][2].size == 0
    assert pr.min_size_scaled(16., 1.3) != np.round(pr.min_size_scaled(16., 1.3))
    n_big = pc.reference('min_size_largest_sort')[0][0][2].size
    assert 0.5 * 16384 < n_big < 0.8 * 16384, n_big
    # NMS on: post_nms 50 binds, 600 does not
    assert pc.reference('nms_post_50')[0][0][2].size == 50 < pc.reference('nms_post_600')[0][0][2].size < 600
    # batch: the images' counts differ (clip bounds and min_size * scale are per image)
    assert len({tuple(r[2].size for r in per_level) for per_level in pc.reference('batch3')}) == 3


def test_detection_reference_inputs():
    """The detection cases' zero size deltas make oracle.box_results exact (exp(0) = 1), and the grid's boxes never overlap."""
    rois, prob, pred = pc.det_grid(2500, 2512, 2)
    assert not pred[:, 2::4].any() and not pred[:, 3::4].any()
    dets, kp = pc.det_reference(rois[:2500], prob[:2500], pred[:2500], 2, 0, 1.0)
    assert dets.shape == (2500, 6) and kp.shape == (2500, 5)
