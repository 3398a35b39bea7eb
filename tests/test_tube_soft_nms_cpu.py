"""CPU tests of Soft-NMS and box voting for tubes (cfg.HIP.TUBE_SOFT_NMS): the definition restated in NumPy
(tests/tube_soft_nms_ref.py) against today's box arithmetic at T = 1, against the host twin dat_soft_nms_tubes_host, and -- method
`hard` -- against the reference's tube NMS; the host dispatch and the device-path predicate with the switch on and off."""
import numpy as np
import pytest

from tests import soft_nms_cases as sc
from tests import tube_soft_nms_ref as tr

TWIN_T = (2, 3, 5)
TWIN_N = (0, 1, 2, 65, 200)


@pytest.mark.parametrize('method', tr.METHODS)
def test_the_restatement_at_one_frame_is_todays_soft_nms(method):
    """T = 1: the tube definition (float32 sum of one IoU from 0, divided by float32(1); re-score iff ov > 0) is dat_soft_nms_host bit
    for bit -- rows, order, indices, scores -- and so is the tube host twin."""
    for name, dets in (('golden', sc.golden_dets()), ('ties', sc.tie_dets(200, 1200)), ('smooth', sc.smooth_dets(300, 16))):
        ref_d, ref_i = sc.host_soft_nms(dets, method)
        assert 0 < len(ref_d) < len(dets)
        for what, (d, i) in (('numpy', tr.serial_soft_nms(dets, 1, method)), ('twin', tr.host_soft_nms_tubes(dets, 1, method))):
            np.testing.assert_array_equal(i, ref_i, err_msg='%s %s' % (name, what))
            np.testing.assert_array_equal(d, ref_d, err_msg='%s %s' % (name, what))


@pytest.mark.parametrize('method', tr.METHODS)
@pytest.mark.parametrize('T', TWIN_T)
def test_the_host_twin_equals_the_restatement(T, method):
    """dat_soft_nms_tubes_host against the NumPy serial loop: rows, order, indices and scores bit for bit, on dense continuous inputs
    and on tie-heavy ones with duplicated rows.  Gaussian too: the rule tests/test_soft_nms_cpu.py applies to the box host twin (NumPy's
    float64 exp and the C library's are the same function here)."""
    rescored = removed = False
    for n in TWIN_N:
        for gen in (tr.smooth_tubes, tr.tie_tubes):
            dets = gen(n, T, 7 + n)
            ref_d, ref_i = tr.serial_soft_nms(dets, T, method)
            got_d, got_i = tr.host_soft_nms_tubes(dets, T, method)
            np.testing.assert_array_equal(got_i, ref_i, err_msg='%s n=%d' % (gen.__name__, n))
            np.testing.assert_array_equal(got_d, ref_d, err_msg='%s n=%d' % (gen.__name__, n))
            np.testing.assert_array_equal(got_d[:, :-1], dets[got_i, :-1])
            removed |= len(got_i) < n
            rescored |= bool(np.any(got_d[:, -1] != dets[got_i, -1]))
    assert removed and (rescored or method == 'hard')          # (hard: a re-scored row has weight 1 or is removed)


HARD_CASES = [(T, n, 40 + n + T) for T in (2, 3) for n in (1, 2, 65, 200)]


@pytest.mark.parametrize('T,n,seed', HARD_CASES)
def test_method_hard_keeps_what_the_reference_tube_nms_keeps(T, n, seed):
    """With method `hard` a row whose overlap with a selected row is > Nt gets score 0 and is removed; one with 0 < ov <= Nt keeps
    its score: the loop selects rows in score order and drops exactly what lib/nms/py_cpu_nms_tubes.py:17-53 (oracle/nms.nms_tubes,
    keep while the mean IoU <= thresh) drops.  The two form the per-frame IoU in different arithmetic (float32 `+ 1` there, a double
    constant here), so the inputs must keep every overlap away from Nt -- asserted first, on the restatement's own overlaps -- and
    have distinct scores (the tie order of the reference's argsort is an accident)."""
    from oracle import nms as oracle_nms
    dets = tr.grid_tubes(n, T, seed)
    assert len(np.unique(dets[:, -1])) == n
    audit = {}
    rows, inds = tr.serial_soft_nms(dets, T, 'hard', nt=0.3, thresh=0.001, audit=audit)
    assert audit.get('nt_gap', np.inf) >= 1e-5, audit
    keep = oracle_nms.nms_tubes(dets, 0.3)
    assert list(inds) == list(keep)
    np.testing.assert_array_equal(rows, dets[keep])
    assert n < 65 or 1 < len(keep) < n


def test_the_gaussian_inputs_of_the_device_comparison_qualify():
    """The rule of tests/test_soft_nms_cpu.py for the cases tests/test_gpu_tube_soft_nms.py runs with method gaussian: the device's
    double exp may move a score by one float ulp per re-scoring, so identical rows in identical order can be demanded only of inputs on
    which no decision of the run is closer than that allowance.  Every case must qualify (one that did not would get another seed in
    tube_soft_nms_ref.GAUSSIAN_CASES, not a skip)."""
    from detectandtrack_amd.ops import hip_ops
    assert hip_ops.soft_nms_tubes_max_boxes(5) == tr.CAPACITY_T5
    for T, n, seed in tr.GAUSSIAN_CASES:
        dets = tr.smooth_tubes(n, T, seed)
        audit = {}
        d, i, k = tr.serial_soft_nms(dets, T, 'gaussian', count_rescorings=True, audit=audit)
        ref_d, ref_i = tr.host_soft_nms_tubes(dets, T, 'gaussian')
        np.testing.assert_array_equal(i, ref_i)
        np.testing.assert_array_equal(d, ref_d)
        s = ref_d[:, -1].astype(np.float64)
        consecutive = np.all(s[:-1] - s[1:] > (k[:-1] + k[1:]) * tr.ULP * s[:-1]) if len(s) > 1 else True
        assert audit.get('slack', np.inf) > 0 and consecutive, (T, n, seed, audit)
        if n >= 64:
            assert audit['rescored'] > 0 and len(ref_i) < n


def test_the_capacity_per_tube_length():
    """dat_soft_nms_tubes_max_boxes: 16T + 11 bytes a row in the 160 KB of a workgroup less 512 bytes for the static arrays, down to a
    multiple of 64, never above DAT_SOFT_NMS_MAX_BOXES: 2048 up to T = 4, then falling -- T = 16 no longer holds the reference's 1000
    rois; 0 outside 1 .. 16."""
    from detectandtrack_amd.ops import hip_ops
    cap = [hip_ops.soft_nms_tubes_max_boxes(T) for T in range(0, 18)]
    assert cap[0] == cap[17] == 0
    assert cap[1:5] == [hip_ops.SOFT_NMS_MAX_BOXES] * 4 == [2048] * 4
    assert cap[5] == 1792 and cap[16] == 576 < 1000
    for T in range(1, 17):
        assert cap[T] % 64 == 0 and cap[T] <= 2048 and cap[T] * (16 * T + 11) <= 160 * 1024 - 512
        assert cap[T] == 2048 or (cap[T] + 64) * (16 * T + 11) > 160 * 1024 - 512
        assert T == 1 or cap[T] <= cap[T - 1]


def _tube_cfg(T=3):
    from detectandtrack_amd.core.config import cfg
    cfg.MODEL.FASTER_RCNN = True
    cfg.MODEL.VIDEO_ON, cfg.VIDEO.BODY_HEAD_LINK, cfg.VIDEO.NUM_FRAMES_MID = True, '', T


def test_predicate_and_dispatch_with_the_switch_on():
    """HIP.TUBE_SOFT_NMS: device_results_supported admits tube configs with either TEST switch; the Soft-NMS capacity is that of the
    clip's T (an over-capacity config goes to the host loop, which has none; voting reads global memory and has none either);
    nms_wrapper.soft_nms of tube rows runs the host twin."""
    from detectandtrack_amd.core import nms_wrapper, test as engine
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.ops import hip_ops
    reset_cfg()
    try:
        _tube_cfg(3)
        cfg.HIP.TUBE_SOFT_NMS = True
        assert engine.device_results_supported()
        for soft, vote in ((True, False), (False, True), (True, True)):
            cfg.TEST.SOFT_NMS.ENABLED, cfg.TEST.BBOX_VOTE.ENABLED = soft, vote
            cfg.TEST.RPN_POST_NMS_TOP_N = 1000
            assert engine.device_results_supported(), (soft, vote)
            cfg.TEST.RPN_POST_NMS_TOP_N = hip_ops.soft_nms_tubes_max_boxes(3)
            assert engine.device_results_supported(), (soft, vote)
            cfg.TEST.RPN_POST_NMS_TOP_N = hip_ops.soft_nms_tubes_max_boxes(3) + 1
            assert engine.device_results_supported() == (not soft), (soft, vote)
        # sixteen frames: the reference's 1000 rois no longer fit
        cfg.VIDEO.NUM_FRAMES_MID, cfg.TEST.RPN_POST_NMS_TOP_N = 16, 1000
        cfg.TEST.SOFT_NMS.ENABLED, cfg.TEST.BBOX_VOTE.ENABLED = True, False
        assert not engine.device_results_supported()
        cfg.TEST.RPN_POST_NMS_TOP_N = hip_ops.soft_nms_tubes_max_boxes(16)
        assert engine.device_results_supported()
        cfg.TEST.SOFT_NMS.ENABLED, cfg.TEST.BBOX_VOTE.ENABLED, cfg.TEST.RPN_POST_NMS_TOP_N = False, True, 1000
        assert engine.device_results_supported()
        # boxes keep their bound whatever the switch
        cfg.VIDEO.BODY_HEAD_LINK = 'slice-center'
        cfg.TEST.SOFT_NMS.ENABLED, cfg.TEST.RPN_POST_NMS_TOP_N = True, sc.CAPACITY
        assert engine.device_results_supported()
        cfg.TEST.RPN_POST_NMS_TOP_N = sc.CAPACITY + 1
        assert not engine.device_results_supported()
        dets = tr.smooth_tubes(65, 3, 9)
        assert dets.shape[1] == 13
        rows, inds = nms_wrapper.soft_nms(dets, sigma=tr.SIGMA, overlap_thresh=tr.NT, score_thresh=tr.THRESH, method='linear')
        ref_d, ref_i = tr.serial_soft_nms(dets, 3, 'linear')
        assert inds.dtype == np.int64 and rows.dtype == np.float32 and 0 < len(inds) < 65
        np.testing.assert_array_equal(inds, ref_i)
        np.testing.assert_array_equal(rows, ref_d)
        empty_rows, empty_inds = nms_wrapper.soft_nms(dets[:0])
        assert empty_rows.shape == (0, 13) and empty_inds.shape == (0,)
    finally:
        reset_cfg()


def _parent_box_voting(top_dets, all_dets, thresh):
    """utils/boxes.box_voting as it is without the switch (lib/utils/boxes.py:294-310): four columns, column 4 as the weights."""
    from detectandtrack_amd.utils import boxes as bu
    out = top_dets.copy()
    overlaps = bu.bbox_overlaps(top_dets[:, :4], all_dets[:, :4])
    for k in range(out.shape[0]):
        vote = np.where(overlaps[k] >= thresh)[0]
        out[k, :4] = np.average(all_dets[vote, :4], axis=0, weights=all_dets[vote, 4])
    return out


def test_predicate_and_dispatch_with_the_switch_off():
    """The default: everything as before the switch existed.  The expectations of
    tests/test_soft_nms_cpu.py::test_device_results_predicate_with_soft_nms_and_voting restated; nms_wrapper.soft_nms of tube rows is
    the reference's NotImplementedError; utils/boxes.box_voting of tube rows touches the first four columns only."""
    from detectandtrack_amd.core import nms_wrapper, test as engine
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import boxes as bu
    reset_cfg()
    try:
        assert cfg.HIP.TUBE_SOFT_NMS is False
        cfg.MODEL.FASTER_RCNN = True
        assert engine.device_results_supported()
        cfg.TEST.SOFT_NMS.ENABLED = True
        assert cfg.TEST.RPN_POST_NMS_TOP_N <= engine.SOFT_NMS_MAX_BOXES == sc.CAPACITY
        assert engine.device_results_supported()
        cfg.TEST.RPN_POST_NMS_TOP_N = sc.CAPACITY + 1
        assert not engine.device_results_supported()
        cfg.TEST.SOFT_NMS.ENABLED, cfg.TEST.BBOX_VOTE.ENABLED = False, True
        assert engine.device_results_supported()
        cfg.TEST.RPN_POST_NMS_TOP_N = 1000
        _tube_cfg(3)
        assert not engine.device_results_supported()
        cfg.TEST.BBOX_VOTE.ENABLED = False
        assert engine.device_results_supported()
        cfg.TEST.SOFT_NMS.ENABLED = True
        assert not engine.device_results_supported()
        cfg.VIDEO.BODY_HEAD_LINK = 'slice-center'
        assert engine.device_results_supported()
        dets = tr.smooth_tubes(40, 3, 10)
        with pytest.raises(NotImplementedError):
            nms_wrapper.soft_nms(dets)
        top = dets[::5]
        got = bu.box_voting(top, dets, 0.5)
        np.testing.assert_array_equal(got, _parent_box_voting(top, dets, 0.5))
        np.testing.assert_array_equal(got[:, 4:], top[:, 4:])
    finally:
        reset_cfg()


@pytest.mark.parametrize('T', [2, 3, 5])
def test_host_tube_voting_is_the_float64_mean(T):
    """utils/boxes.box_voting of tube rows with the switch on: all 4T coordinates within one float32 ulp of the float64 score-weighted
    mean over the voters the float32 tube overlap selects (utils/boxes.tube_overlaps: the explicit frame-order sum, equal to the
    restatement's overlap bit for bit); scores untouched; box rows untouched by the switch."""
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import boxes as bu
    reset_cfg()
    try:
        cfg.HIP.TUBE_SOFT_NMS = True
        for n_all, n_top, th in ((300, 64, 0.5), (65, 7, 0.3), (1, 1, 0.8)):
            all_dets = tr.smooth_tubes(n_all, T, 20 + n_all)
            top = all_dets[np.random.RandomState(n_all).permutation(n_all)[:n_top]]
            ov = bu.tube_overlaps(top[:, :-1], all_dets[:, :-1])
            assert ov.dtype == np.float32
            for k in range(n_top):
                np.testing.assert_array_equal(ov[k], tr.tube_ov(top[k], all_dets, T))
            got = bu.box_voting(top, all_dets, th)
            ref, voters, _ = tr.vote_f64(top, all_dets, T, th)
            assert got.dtype == np.float32 and got.shape == top.shape
            assert n_all == 1 or voters.max() > 1
            assert np.all(np.abs(got[:, :-1] - ref[:, :-1]) <= tr.one_ulp(ref[:, :-1]))
            np.testing.assert_array_equal(got[:, -1], top[:, -1])
        boxes = sc.smooth_dets(100, 3)
        on = bu.box_voting(boxes[:20], boxes, 0.5)
        cfg.HIP.TUBE_SOFT_NMS = False
        np.testing.assert_array_equal(on, bu.box_voting(boxes[:20], boxes, 0.5))
    finally:
        reset_cfg()


def test_host_post_processing_of_tubes_with_the_switch_on():
    """core/test.box_results_with_nms_and_limit on tube rows, TEST.SOFT_NMS + TEST.BBOX_VOTE + HIP.TUBE_SOFT_NMS: per class the serial
    loop (overlap threshold TEST.NMS, score threshold 0.0001), then voting of the re-scored rows by the class's selected rows, then
    the DETECTIONS_PER_IM rule on the re-scored scores."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.config import cfg, reset_cfg
    T, K, R, D = 3, 3, 60, 20
    rs = np.random.RandomState(4)
    boxes = np.hstack([tr.smooth_tubes(R, T, 30 + j)[:, :-1] for j in range(K)])
    scores = rs.uniform(0.0, 1.0, (R, K)).astype(np.float32)
    reset_cfg()
    try:
        cfg.MODEL.NUM_CLASSES, cfg.HIP.TUBE_SOFT_NMS = K, True
        cfg.TEST.SCORE_THRESH, cfg.TEST.NMS, cfg.TEST.DETECTIONS_PER_IM = 0.05, 0.5, D
        cfg.TEST.SOFT_NMS.ENABLED, cfg.TEST.SOFT_NMS.METHOD, cfg.TEST.SOFT_NMS.SIGMA = True, 'linear', 0.5
        cfg.TEST.BBOX_VOTE.ENABLED, cfg.TEST.BBOX_VOTE.VOTE_TH = True, 0.7
        s, b, cls_boxes = engine.box_results_with_nms_and_limit(scores.copy(), boxes.copy())
    finally:
        reset_cfg()
    per_class = []
    for j in range(1, K):
        sel = scores[:, j] > 0.05
        dets = np.hstack((boxes[sel, 4 * T * j:4 * T * (j + 1)], scores[sel, j][:, None])).astype(np.float32)
        rows, _ = tr.serial_soft_nms(dets, T, 'linear', sigma=0.5, nt=0.5, thresh=0.0001)
        ref, voters, _ = tr.vote_f64(rows, dets, T, 0.7)
        per_class.append((rows, ref))
    all_scores = np.concatenate([r[:, -1] for r, _ in per_class])
    assert len(all_scores) > D
    cut = np.sort(all_scores)[-D]
    assert b.shape == (len(s), 4 * T) and len(s) >= D
    off = 0
    for j, (rows, ref) in enumerate(per_class, start=1):
        keep = rows[:, -1] >= cut
        m = int(keep.sum())
        np.testing.assert_array_equal(cls_boxes[j][:, -1], rows[keep, -1])
        np.testing.assert_array_equal(s[off:off + m], rows[keep, -1])
        assert np.all(np.abs(b[off:off + m] - ref[keep, :-1]) <= tr.one_ulp(ref[keep, :-1]))
        off += m
    assert off == len(s)


def test_the_shipped_tube_soft_nms_config_takes_the_device_path():
    """configs/test_r18_c4_tube_softnms_synthetic.yaml: a tube model (T = 3) with both TEST switches and HIP.TUBE_SOFT_NMS loads, builds
    and stays on the device path; the same file without the switch goes to the host path."""
    import os
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.config import cfg, cfg_from_file, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    reset_cfg()
    try:
        cfg_from_file(os.path.join(sc.REPO, 'configs', 'test_r18_c4_tube_softnms_synthetic.yaml'))
        assert_and_infer_cfg()
        assert cfg.TEST.SOFT_NMS.ENABLED and cfg.TEST.BBOX_VOTE.ENABLED and cfg.HIP.TUBE_SOFT_NMS
        assert engine._tube_detections() and cfg.VIDEO.NUM_FRAMES_MID == 3
        assert engine.device_results_supported()
        model = model_builder.create(cfg.MODEL.TYPE, train=False)
        assert model.keypoint_net is not None
        cfg.HIP.TUBE_SOFT_NMS = False
        assert not engine.device_results_supported()
    finally:
        reset_cfg()
