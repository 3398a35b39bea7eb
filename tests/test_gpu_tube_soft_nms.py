"""GPU tests of Soft-NMS and box voting for tubes (cfg.HIP.TUBE_SOFT_NMS; csrc/detections.hip: soft_nms_kernel,
box_vote_kernel, dat_box_results_ex with tubes_enabled) and of the engine paths the switch opens for tube models."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from detectandtrack_amd.utils import boxes as bu
from tests import tube_soft_nms_ref as tr
from tests.model_util import c4_tube_kps_cfg

pytestmark = pytest.mark.gpu
XFORM_CLIP = float(np.float32(np.log(1000. / 16.)))


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_soft_nms(ops, dets, T, method):
    d, inds, cnt = ops.soft_nms_tubes(_dev(dets), T, sigma=tr.SIGMA, overlap_thresh=tr.NT, score_thresh=tr.THRESH, method=method)
    m = int(cnt.item())
    return d[:m].cpu().numpy(), inds[:m].cpu().numpy()


def _assert_exercised(dets, ref_d, ref_i, name, rescored=True):
    """On the HOST result: the run removed a row and (methods that can change a kept row's score) re-scored a kept one."""
    assert len(ref_i) < len(dets), name
    assert not rescored or np.any(ref_d[:, -1] != dets[ref_i, -1]), name


# ---- dat_soft_nms_tubes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['hard', 'linear'])
@pytest.mark.parametrize('T', [1, 2, 3])
def test_soft_nms_tubes_hard_and_linear_are_bit_identical_to_the_host_twin(ops, T, method):
    """Methods 0 and 1 have no transcendental: rows, order, indices and scores of dat_soft_nms_tubes equal dat_soft_nms_tubes_host bit
    for bit, from no row to the capacity, across the wave and block boundaries (63 / 64 / 65, 257), on dense continuous inputs and
    on tie-heavy ones with duplicated rows (positions decide nearly every arg-max, so a compaction that leaves a row in another slot
    shows)."""
    assert ops.soft_nms_tubes_max_boxes(T) == tr.GPU_SIZES[-1]
    for n in tr.GPU_SIZES:
        for gen in (tr.smooth_tubes, tr.tie_tubes):
            name = '%s n=%d' % (gen.__name__, n)
            dets = gen(n, T, 500 + n)
            ref_d, ref_i = tr.host_soft_nms_tubes(dets, T, method)
            got_d, got_i = _device_soft_nms(ops, dets, T, method)
            np.testing.assert_array_equal(got_i, ref_i, err_msg=name)
            np.testing.assert_array_equal(got_d, ref_d, err_msg=name)
            if n >= 64:
                _assert_exercised(dets, ref_d, ref_i, name, rescored=method != 'hard')


@pytest.mark.parametrize('method', ['hard', 'linear'])
def test_soft_nms_tubes_at_the_capacity_of_five_frames(ops, method):
    """T = 5: 91 bytes a row no longer leave room for 2048 rows.  The capacity itself is bit-identical to the host twin; one row
    more is an argument error, not a truncation."""
    from detectandtrack_amd import libdat
    cap = ops.soft_nms_tubes_max_boxes(5)
    assert cap == tr.CAPACITY_T5 < 2048
    for gen in (tr.smooth_tubes, tr.tie_tubes):
        dets = gen(cap, 5, 77)
        ref_d, ref_i = tr.host_soft_nms_tubes(dets, 5, method)
        got_d, got_i = _device_soft_nms(ops, dets, 5, method)
        np.testing.assert_array_equal(got_i, ref_i, err_msg=gen.__name__)
        np.testing.assert_array_equal(got_d, ref_d, err_msg=gen.__name__)
        _assert_exercised(dets, ref_d, ref_i, gen.__name__, rescored=method != 'hard')
    with pytest.raises(libdat.DatError):
        ops.soft_nms_tubes(_dev(tr.smooth_tubes(cap + 1, 5, 78)), 5)
    with pytest.raises(libdat.DatError):
        ops.soft_nms_tubes(_dev(tr.smooth_tubes(2049, 2, 79)), 2)


def test_soft_nms_tubes_gaussian_matches_the_host_twin(ops):
    """Method 2 on the cases tests/test_tube_soft_nms_cpu.py qualifies (no decision of the run is closer than the allowance): the
    same rows in the same order with the same indices, coordinates bit-identical, scores within one float ulp per re-scoring the
    row received (include/dat_hip.h: the device's double exp is accurate to an ulp of a double, not correctly rounded)."""
    for T, n, seed in tr.GAUSSIAN_CASES:
        name = 'T=%d n=%d' % (T, n)
        dets = tr.smooth_tubes(n, T, seed)
        ref_d, ref_i = tr.host_soft_nms_tubes(dets, T, 'gaussian')
        _, _, k = tr.serial_soft_nms(dets, T, 'gaussian', count_rescorings=True)
        got_d, got_i = _device_soft_nms(ops, dets, T, 'gaussian')
        np.testing.assert_array_equal(got_i, ref_i, err_msg=name)
        np.testing.assert_array_equal(got_d[:, :-1], ref_d[:, :-1], err_msg=name)
        rel = np.abs(got_d[:, -1].astype(np.float64) - ref_d[:, -1]) / np.abs(ref_d[:, -1].astype(np.float64))
        print('gaussian %-12s rows %4d  max |score diff| = %.3f ulp (allowed: up to %d)' % (
            name, len(ref_d), (rel / tr.ULP).max() if len(rel) else 0, k.max() if len(k) else 0))
        assert np.all(rel <= k * tr.ULP), name
        if n >= 64:
            _assert_exercised(dets, ref_d, ref_i, name)


# ---- dat_box_voting_tubes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 2, 3])
def test_box_voting_tubes_is_the_float64_mean_and_repeats_bit_for_bit(ops, T):
    """All 4T coordinates within one float32 ulp of the float64 score-weighted mean over the voters the float32 tube overlap selects;
    scores untouched; two runs bit-identical (fixed summation order); in place (out is top) equals out of place."""
    several = False
    for n_top in (1, 7, 64):
        for n_all in (1, 65, 300):
            all_dets = tr.smooth_tubes(n_all, T, 900 + n_all)
            top = all_dets[np.random.RandomState(n_top).randint(0, n_all, n_top)]
            ref, voters, _ = tr.vote_f64(top, all_dets, T, 0.5)
            several |= bool(voters.max() > 1)
            a = ops.box_voting_tubes(_dev(top), _dev(all_dets), T, 0.5).cpu().numpy()
            b = ops.box_voting_tubes(_dev(top), _dev(all_dets), T, 0.5).cpu().numpy()
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a[:, -1], top[:, -1])
            err = np.abs(a[:, :-1] - ref[:, :-1])
            assert np.all(err <= tr.one_ulp(ref[:, :-1])), (n_top, n_all, float((err / tr.one_ulp(ref[:, :-1])).max()))
            inplace = _dev(top)
            assert ops.box_voting_tubes(inplace, _dev(all_dets), T, 0.5, out=inplace) is inplace
            np.testing.assert_array_equal(inplace.cpu().numpy(), a)
    assert several


def test_box_voting_tubes_of_more_frames_than_one_register_chunk(ops):
    """T = 5 and 16: the kernel forms the sums four frames at a time and walks the voters once per chunk; every chunk must find the
    same voters, in place too (the kept row's coordinates stay in registers while the row is overwritten)."""
    for T in (5, 16):
        all_dets = tr.smooth_tubes(130, T, 40 + T)
        top = all_dets[::3]
        ref, voters, _ = tr.vote_f64(top, all_dets, T, 0.5)
        assert voters.max() > 1
        a = ops.box_voting_tubes(_dev(top), _dev(all_dets), T, 0.5).cpu().numpy()
        assert np.all(np.abs(a[:, :-1] - ref[:, :-1]) <= tr.one_ulp(ref[:, :-1]))
        np.testing.assert_array_equal(a[:, -1], top[:, -1])
        inplace = _dev(top)
        ops.box_voting_tubes(inplace, _dev(all_dets), T, 0.5, out=inplace)
        np.testing.assert_array_equal(inplace.cpu().numpy(), a)


# ---- dat_box_results_ex with tubes_enabled ---------------------------------------------------------------------------------------------
H, W, SCALE = 720, 1280, 2.0
WEIGHTS = (10., 10., 5., 5.)
T3, K2, CAP, R = 3, 2, 64, 50
VOTE_TH = 0.7


def _image_inputs(seed):
    """About 50 tube proposals of three frames around eight objects, class probabilities and deltas of one image.  The host path
    decodes tubes in float64 and rounds once (utils/boxes.split_tube_into_boxes promotes, as the reference's does), the device in
    float32, so the two agree bit for bit only where every step of the decode is exact -- and the comparison below needs both paths to
    see the same tubes.  Hence: integer proposal corners, the scale a power of two, centre deltas that are multiples of 1/8 after the
    division by the regression weight, and zero size deltas (exp(0) = 1 on both sides)."""
    rs = np.random.RandomState(seed)
    centres = np.stack([rs.randint(200, int(W * SCALE) - 700, 8), rs.randint(200, int(H * SCALE) - 700, 8)], axis=1)
    xy = centres[rs.randint(0, 8, CAP)][:, None, :] + rs.randint(-16, 17, (CAP, 1, 2)) + rs.randint(-6, 7, (CAP, T3, 2))
    wh = rs.randint(360, 521, (CAP, 1, 2))
    rois = np.zeros((CAP, 4 * T3 + 1), np.float32)
    rois[:, 1:] = np.concatenate((xy, xy + wh), axis=2).reshape(CAP, 4 * T3)
    prob = rs.uniform(0.06, 0.99, (CAP, K2)).astype(np.float32)
    eighths = rs.randint(-1, 2, (CAP, K2 * 4 * T3)) / 8.0
    pred = (eighths * np.tile([WEIGHTS[0], WEIGHTS[1], 0.0, 0.0], K2 * T3)).astype(np.float32)
    return rois, prob, pred


def _host_box_results(rois, prob, pred, D, soft, vote):
    """core/test.box_results_with_nms_and_limit with HIP.TUBE_SOFT_NMS on the host-decoded tubes, and the class's selected rows."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    cfg.MODEL.NUM_CLASSES, cfg.HIP.TUBE_SOFT_NMS = K2, True
    cfg.TEST.SCORE_THRESH, cfg.TEST.NMS, cfg.TEST.DETECTIONS_PER_IM = 0.05, 0.5, D
    cfg.TEST.SOFT_NMS.ENABLED = soft is not None
    if soft is not None:
        cfg.TEST.SOFT_NMS.METHOD, cfg.TEST.SOFT_NMS.SIGMA = soft, 0.5
    cfg.TEST.BBOX_VOTE.ENABLED, cfg.TEST.BBOX_VOTE.VOTE_TH = bool(vote), VOTE_TH
    try:
        boxes = bu.clip_tiled_boxes(bu.bbox_transform(rois[:, 1:] / np.float32(SCALE), pred, WEIGHTS), (H, W, 3))
        s, b, cls_boxes = engine.box_results_with_nms_and_limit(prob.copy(), boxes.copy())
        keep = prob[:, 1] > 0.05
        sel = np.hstack((boxes[keep, 4 * T3:8 * T3], prob[keep, 1][:, None])).astype(np.float32)
    finally:
        reset_cfg()
    return s, b, sel


def _unvoted(voted_scores, sel, soft):
    """The kept rows before voting: voting leaves scores alone, and the scores (continuous random values, re-scored or not) identify
    the rows; with Soft-NMS the host loop is run again."""
    rows = sel if soft is None else tr.host_soft_nms_tubes(sel, T3, soft, sigma=0.5, nt=0.5, thresh=0.0001)[0]
    by_score = {float(s): r for r, s in enumerate(rows[:, -1])}
    assert len(by_score) == len(rows)
    return rows[[by_score[float(s)] for s in voted_scores]]


def _box_results(ops, per, ni, D, soft, vote, tubes=True):
    rois, prob, pred = (np.concatenate([p[c] for p in per]) for c in range(3))
    out_cap = D + 8 if D > 0 else CAP * (K2 - 1)
    return ops.box_results(_dev(rois), torch.tensor([R] * ni, dtype=torch.int32).cuda(), _dev(prob), _dev(pred), K2, T3, SCALE,
                           (H, W, 3), WEIGHTS, XFORM_CLIP, 0.05, 0.5, D, out_cap, n_images=ni,
                           soft_nms=dict(method=soft, sigma=0.5, score_thresh=0.0001) if soft else None,
                           bbox_vote=VOTE_TH if vote else None, tubes=tubes), out_cap


MODES = [('linear', False), ('gaussian', False), (None, True), ('linear', True)]


@pytest.mark.parametrize('soft,vote', MODES, ids=['soft_linear', 'soft_gaussian', 'vote_only', 'soft_linear_vote'])
@pytest.mark.parametrize('ni', [1, 4])
@pytest.mark.parametrize('D', [5, 0], ids=['limit_binds', 'no_limit'])
def test_box_results_for_tubes_match_the_host_path(ops, soft, vote, ni, D):
    """dat_box_results_ex with tubes_enabled, T = 3, against core/test.box_results_with_nms_and_limit with the switch on, fed the same
    scores and decoded tubes -- the criteria of tests/test_gpu_soft_nms.py for boxes: the same rows in the same order, scores
    bit-identical (linear) or within an ulp per re-scoring (gaussian), coordinates bit-identical without voting and, voted, within
    (m + 2) * 2^-24 * max|coordinate of the row's m voters| of the float64 mean and of the host path; keypoint_rois =
    float32(float64(tube) * scale).  The same call without tubes_enabled is an argument error."""
    from detectandtrack_amd import libdat
    per = [_image_inputs(700 + 10 * ni + i) for i in range(ni)]
    (dets, kp, n_out), out_cap = _box_results(ops, per, ni, D, soft, vote)
    n = n_out.cpu().numpy().reshape(ni, 2)
    cols = 4 * T3 + 1
    d_all, kp_all = dets.cpu().numpy().reshape(ni, out_cap, cols + 1), kp.cpu().numpy().reshape(ni, out_cap, cols)
    for i in range(ni):
        ref_s, ref_b, sel = _host_box_results(per[i][0][:R], per[i][1][:R], per[i][2][:R], D, soft, vote)
        assert n[i, 0] == n[i, 1] == len(ref_s), (i, n[i], len(ref_s))
        assert len(ref_s) == D if D > 0 else D < len(ref_s) <= len(sel)
        k = int(n[i, 0])
        d = d_all[i, :k]
        np.testing.assert_array_equal(d[:, -1], np.ones(k, np.float32))
        if soft == 'gaussian':
            audit = {}
            hits = tr.serial_soft_nms(sel, T3, soft, sigma=0.5, nt=0.5, thresh=0.0001, count_rescorings=True, audit=audit)
            assert audit['slack'] > 0                               # (the input qualifies: no decision inside the allowance)
            allowed = dict(zip((float(s) for s in hits[0][:, -1]), hits[2]))
            rel = np.abs(d[:, -2].astype(np.float64) - ref_s) / ref_s.astype(np.float64)
            assert np.all(rel <= np.array([allowed[float(s)] for s in ref_s]) * tr.ULP)
        else:
            np.testing.assert_array_equal(d[:, -2], ref_s)
        if soft is not None:
            rows, inds = tr.host_soft_nms_tubes(sel, T3, soft, sigma=0.5, nt=0.5, thresh=0.0001)
            assert np.any(rows[:, -1] != sel[inds, -1])             # (the class's run re-scored a row it kept; the limit may cut it)
            assert D > 0 or np.any(~np.isin(ref_s, sel[:, -1]))
        if vote:
            before = _unvoted(ref_s, sel, soft)
            ref64, voters, tol = tr.vote_f64(before, sel, T3, VOTE_TH)
            assert voters.max() > 1
            e64, eh = np.abs(d[:, :4 * T3] - ref64[:, :4 * T3]), np.abs(d[:, :4 * T3] - ref_b)
            print('image %d voting: max error / bound = %.3f (float64 mean), %.3f (host path)' % (i, (e64 / tol).max(), (eh / tol).max()))
            assert np.all(e64 <= tol) and np.all(eh <= tol)
            assert np.abs(ref_b - before[:, :4 * T3]).max() > 0.01    # (voting moved a tube)
        else:
            np.testing.assert_array_equal(d[:, :4 * T3], ref_b)
        exp_kp = np.hstack((np.full((k, 1), i, np.float32), (d[:, :4 * T3].astype(np.float64) * SCALE).astype(np.float32)))
        np.testing.assert_array_equal(kp_all[i, :k], exp_kp)
        assert not kp_all[i, k:].any() and not d_all[i, k:].any()
    with pytest.raises(libdat.DatError):
        _box_results(ops, per, ni, D, soft, vote, tubes=False)


def test_box_results_ex_for_tubes_with_both_switches_off_is_box_results_batch(ops):
    """tubes_enabled alone changes nothing: with TEST.SOFT_NMS and TEST.BBOX_VOTE off, dat_box_results_ex of tube rows is
    dat_box_results_batch -- byte-identical outputs, the same workspace size."""
    from detectandtrack_amd import libdat as L
    ni, D = 4, 10
    per = [_image_inputs(950 + i) for i in range(ni)]
    rois, prob, pred = (_dev(np.concatenate([p[c] for p in per])) for c in range(3))
    n_rois = torch.tensor([R] * ni, dtype=torch.int32).cuda()
    base = ops.box_results(rois, n_rois, prob, pred, K2, T3, SCALE, (H, W, 3), WEIGHTS, XFORM_CLIP, 0.05, 0.5, D, D + 8, n_images=ni)
    opts = L.DetOpts()
    opts.tubes_enabled = 1
    ws_bytes = L.lib().dat_box_results_ex_workspace_bytes(CAP, K2, T3, C.byref(opts))
    assert ws_bytes == L.lib().dat_box_results_workspace_bytes(CAP, K2, T3)
    ds = (L.DetDesc * ni)()
    for d in ds:
        d.num_classes, d.T, d.cls_agnostic_bbox_reg, d.detections_per_im = K2, T3, 0, D
        d.im_scale, d.im_scale_f64, d.im_h, d.im_w = SCALE, SCALE, H, W
        for q in range(4):
            d.reg_weights[q] = WEIGHTS[q]
        d.xform_clip, d.score_thresh, d.nms_thresh = XFORM_CLIP, 0.05, 0.5
    cols = 4 * T3 + 1
    wsb = torch.empty(ni * ws_bytes, dtype=torch.uint8, device='cuda')
    dets = torch.full((ni * (D + 8), cols + 1), -7.0, device='cuda')
    kp = torch.full((ni * (D + 8), cols), -7.0, device='cuda')
    n_out = torch.full((ni, 2), -7, dtype=torch.int32, device='cuda')
    ops.ctx().call('dat_box_results_ex', ops._stream(), ops._ptr(rois), ops._ptr(n_rois), CAP, ops._ptr(prob), K2, ops._ptr(pred),
                   4 * T3 * K2, ds, C.byref(opts), ni, ops._ptr(wsb), D + 8, ops._ptr(dets), ops._ptr(kp), ops._ptr(n_out))
    assert int(n_out.cpu().numpy()[0, 0]) > 1
    for a, b in zip(base, (dets, kp, n_out)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- model level -----------------------------------------------------------------------------------------------------------------------
T_E2E, H_E2E, W_E2E = 3, 96, 128
VOTE_TH_E2E = 0.6      # not the default 0.8: a threshold that did not travel from cfg to the kernel would show
# The two paths do not see bit-identical tubes: the host decodes a tube in float64 and rounds once (utils/boxes.split_tube_into_boxes
# promotes, as the reference's does), the device decodes in float32 -- five roundings (w, centre, product, sum, corner) of values
# below 128, each at most half an ulp of 2^-17: under 2e-5 pixels; DECODE_ATOL allows 1e-4.  A re-scored score is a product of factors
# 1 - ov: moving the eight corners of a pair by 2e-5 pixels moves the per-frame IoU of boxes at least 16 pixels wide (the smallest
# anchor) by under 8 * 2e-5 / 16 = 1e-5, and a factor 1 - ov >= 0.03 by under 3.3e-4 relative (typically 1e-5); SCORE_RTOL allows
# 1e-3 for a product of such factors.  (Measured on the MI355X: score difference 0, tube difference 7.6e-6 pixels.)
DECODE_ATOL, SCORE_RTOL = 1e-4, 1e-3


def _tube_cfg(device=True, mode='soft', **hip):
    c = c4_tube_kps_cfg(T=T_E2E, dtype='fp32', pre=300, post=64)
    # (proposal NMS at 0.9: the 64 proposals overlap, so the detections re-score one another and kept tubes have several voters)
    c['TEST'].update(SCALES=(H_E2E,), MAX_SIZE=max(H_E2E, W_E2E), SCORE_THRESH=0.0, DETECTIONS_PER_IM=15, RPN_NMS_THRESH=0.9,
                     SOFT_NMS={'ENABLED': mode == 'soft', 'METHOD': 'linear', 'SIGMA': 0.5},
                     BBOX_VOTE={'ENABLED': mode == 'vote', 'VOTE_TH': VOTE_TH_E2E})
    c['HIP'].update(DEVICE_BOX_RESULTS=device, TUBE_SOFT_NMS=True, **hip)
    return c


def _zero_size_deltas(weights):
    """The width / height rows of the tube head's per-frame delta conv `bbox_pred_1` (rows: class, then dx dy dw dh; the frames share
    it) zeroed: dw = dh = 0 in every frame, so a clip's detections keep the size of their proposals and overlap."""
    from detectandtrack_amd.core.config import cfg
    for name in ('bbox_pred_1_w', 'bbox_pred_1_b'):
        w = np.array(weights[name], copy=True)
        assert w.shape[0] == 4 * cfg.MODEL.NUM_CLASSES
        w[2::4] = 0
        w[3::4] = 0
        weights[name] = w
    return weights


def _build_without_size_deltas(cfg_dict, seed=3):
    """tests/test_gpu_soft_nms.py's helper for the tube model."""
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    reset_cfg()
    cfg_from_cfg(cfg_dict)
    assert_and_infer_cfg()
    model = model_builder.create(cfg.MODEL.TYPE, train=False)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    for k, v in _zero_size_deltas(net_utils.synthetic_params(model, seed)).items():
        ws.set_param(k, v)
    ws.CreateNet(model.net)
    ws.CreateNet(model.conv_body_net)
    ws.CreateNet(model.keypoint_net)
    return model, ws


@pytest.mark.parametrize('mode', ['soft', 'vote'])
def test_im_detect_all_of_a_tube_model_takes_the_device_path_and_matches_the_host_path(monkeypatch, mode):
    """R-18 C4 tube model, T = 3, with HIP.TUBE_SOFT_NMS and TEST.SOFT_NMS (linear) or TEST.BBOX_VOTE: im_detect_all never calls
    box_results_with_nms_and_limit (patched to raise) and returns what it returns with cfg.HIP.DEVICE_BOX_RESULTS False -- the same
    rows in the same order, scores bit-identical; tubes bit-identical (soft) or within the voting bound of the float64 mean over what
    the host path's box_voting was given, and of the host path's tubes (vote); keypoints within a pixel for 95 %."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.ops import hip_ops
    rs = np.random.RandomState(21)
    ims = [[rs.randint(0, 255, (H_E2E, W_E2E, 3)).astype(np.uint8) for _ in range(T_E2E)] for _ in range(2)]

    def boom(*a, **k):
        raise AssertionError('the host post-processing ran with HIP.TUBE_SOFT_NMS on')
    assert hip_ops.tune_plan(0, 1) == 0          # no split-K: a clip's sums do not depend on the path
    votes, softs = [], []
    real_voting, real_soft = bu.box_voting, engine.soft_nms

    def recording_voting(top, all_dets, thresh):
        assert thresh == VOTE_TH_E2E and top.shape[1] == 4 * T_E2E + 1
        votes.append((top.copy(), all_dets.copy()))
        return real_voting(top, all_dets, thresh)

    def recording_soft(dets, **kw):
        rows, inds = real_soft(dets, **kw)
        softs.append((dets.copy(), rows.copy(), inds.copy()))
        return rows, inds
    try:
        model, ws = _build_without_size_deltas(_tube_cfg(device=False, mode=mode))
        assert not engine.device_results_supported()
        monkeypatch.setattr(bu, 'box_voting', recording_voting)
        monkeypatch.setattr(engine, 'soft_nms', recording_soft)
        host = [engine.im_detect_all(model, im, None) for im in ims]
        monkeypatch.setattr(bu, 'box_voting', real_voting)
        monkeypatch.setattr(engine, 'soft_nms', real_soft)
        assert (len(votes), len(softs)) == ((len(ims), 0) if mode == 'vote' else (0, len(ims)))
        model, ws = _build_without_size_deltas(_tube_cfg(mode=mode))
        assert engine.device_results_supported()
        monkeypatch.setattr(engine, 'box_results_with_nms_and_limit', boom)
        device = [engine.im_detect_all(model, im, None) for im in ims]
    finally:
        hip_ops.tune_plan(0, 0)
    for i in range(len(ims)):
        hb, db = host[i][0][1], device[i][0][1]
        assert hb.shape == db.shape and hb.shape[0] > 1 and hb.shape[1] == 4 * T_E2E + 1
        if mode == 'vote':
            np.testing.assert_array_equal(db[:, -1], hb[:, -1])                    # (hard NMS: the scores are cls_prob's)
        else:
            print('clip %d: %d rows, max relative score difference %.3g, max tube difference %.3g pixels' % (
                i, len(hb), np.abs(db[:, -1] / hb[:, -1] - 1).max(), np.abs(db[:, :-1] - hb[:, :-1]).max()))
            np.testing.assert_allclose(db[:, -1], hb[:, -1], rtol=SCORE_RTOL, atol=0)
        if mode == 'vote':
            top, all_dets = votes[i]
            ref64, voters, tol = tr.vote_f64(top, all_dets, T_E2E, VOTE_TH_E2E)
            rows = []
            for r, sv in enumerate(hb[:, -1]):       # a kept row is the `top` row of its score; among duplicates the nearest mean
                cand = np.where(top[:, -1] == sv)[0]
                rows.append(int(cand[np.abs(ref64[cand, :-1] - hb[r, :-1]).max(axis=1).argmin()]))
            e64, eh = np.abs(db[:, :-1] - ref64[rows, :-1]), np.abs(db[:, :-1] - hb[:, :-1])
            assert np.all(e64 <= tol[rows] + DECODE_ATOL) and np.all(eh <= tol[rows] + DECODE_ATOL)
            assert voters[rows].max() > 1 and (np.abs(hb[:, :-1] - top[rows, :-1]).max(axis=1) > 0.01).any()
        else:
            np.testing.assert_allclose(db[:, :-1], hb[:, :-1], rtol=0, atol=DECODE_ATOL)
            dets, rows, inds = softs[i]
            assert len(rows) > 1 and np.any(rows[:, -1] != dets[inds, -1])         # (the run re-scored a kept row)
        hk, dk = np.stack(host[i][2][1]), np.stack(device[i][2][1])
        assert hk.shape == dk.shape and hk.shape[2] == 17 * T_E2E
        assert (np.abs(hk[:, :2] - dk[:, :2]) < 1.0).mean() > 0.95


def test_pipelined_engine_of_a_tube_model_writes_the_eager_loop_detections(tmp_path):
    """test_net over a short clip list, tube model with HIP.TUBE_SOFT_NMS + TEST.SOFT_NMS: the pipelined engine (forwards in flight,
    hipGraph replay) accepts the list and writes the detections of the one-clip-at-a-time loop, bit for bit."""
    from detectandtrack_amd.core import test_engine
    from detectandtrack_amd.core.config import cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd import workspace
    rs = np.random.RandomState(5)
    roidb = [{'image': [rs.randint(0, 255, (H_E2E, W_E2E, 3)).astype(np.uint8) for _ in range(T_E2E)], 'height': H_E2E, 'width': W_E2E}
             for _ in range(4)]

    def run(depth, graph, out):
        c = _tube_cfg(PIPELINE_DEPTH=depth, IMS_PER_FORWARD=1, CLIP_GRAPH=graph)
        c['RNG_SEED'] = 3
        reset_cfg()
        cfg_from_cfg(c)
        assert_and_infer_cfg()
        workspace.ResetWorkspace()
        os.makedirs(out, exist_ok=True)
        return test_engine.test_net(roidb, None, out), test_engine.test_net.last_stats
    eager, st0 = run(0, False, str(tmp_path / 'eager'))
    assert st0 is None
    got, st = run(3, True, str(tmp_path / 'piped'))
    assert st is not None and st['clips'] == 4 and st['per_forward'] == 1      # the pipelined engine took the list
    for i in range(4):
        assert eager['all_boxes'][1][i].shape[0] > 1 and eager['all_boxes'][1][i].shape[1] == 4 * T_E2E + 1
        np.testing.assert_array_equal(got['all_boxes'][1][i], eager['all_boxes'][1][i])
        assert len(got['all_keyps'][1][i]) == len(eager['all_keyps'][1][i]) > 1
        for a, b in zip(got['all_keyps'][1][i], eager['all_keyps'][1][i]):
            np.testing.assert_array_equal(a, b)
    reset_cfg()
