"""GPU tests of Soft-NMS and box voting in the device detection post-processing (csrc/detections.hip: soft_nms_kernel, box_vote_kernel,
dat_box_results_ex) and of the engine paths they open (core/test.device_results_supported with TEST.SOFT_NMS / TEST.BBOX_VOTE)."""
import os

import numpy as np
import pytest
import torch

from detectandtrack_amd.utils import boxes as bu
from tests import soft_nms_cases as sc
from tests.model_util import fpn3d_kps_cfg

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XFORM_CLIP = float(np.float32(np.log(1000. / 16.)))


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _reference_soft_nms(dets, method):
    """The reference's own compiled Cython (oracle/_ref) when it is there, else dat_soft_nms_host (pinned to the golden file by
    tests/test_host_cpu.py)."""
    from oracle import build_ref
    ref = build_ref.load()
    if ref is None or len(dets) == 0:
        return sc.host_soft_nms(dets, method)
    d, inds = ref[0].soft_nms(np.ascontiguousarray(dets), np.float32(sc.SIGMA), np.float32(sc.NT), np.float32(sc.THRESH),
                              np.uint8(sc.METHODS.index(method)))
    return np.asarray(d), np.asarray(inds)


def _device_soft_nms(ops, dets, method):
    d, inds, cnt = ops.soft_nms(_dev(dets), sigma=sc.SIGMA, overlap_thresh=sc.NT, score_thresh=sc.THRESH, method=method)
    m = int(cnt.item())
    return d[:m].cpu().numpy(), inds[:m].cpu().numpy()


# ---- 3. dat_soft_nms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['hard', 'linear'])
def test_soft_nms_hard_and_linear_are_bit_identical_to_the_reference(ops, method):
    """Methods 0 and 1 have no transcendental: boxes, scores and indices of dat_soft_nms equal the reference's compiled Cython bit
    for bit -- on the golden input, on the tie-heavy inputs of the CPU specification test (positions decide nearly every arg-max,
    so a compaction that leaves a row in another slot shows), and at the kernel's capacity."""
    cases = [('golden', sc.golden_dets())] + [('ties_n%d' % n, sc.tie_dets(n, 1000 + n)) for n in sc.TIE_SIZES]
    cases += [('ties_capacity', sc.tie_dets(sc.CAPACITY, 77)), ('smooth_capacity', sc.smooth_dets(sc.CAPACITY, 18))]
    for name, dets in cases:
        ref_d, ref_i = _reference_soft_nms(dets, method)
        got_d, got_i = _device_soft_nms(ops, dets, method)
        np.testing.assert_array_equal(got_i, ref_i, err_msg=name)
        np.testing.assert_array_equal(got_d, ref_d, err_msg=name)
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'reference_postproc.npz'))
    got_d, got_i = _device_soft_nms(ops, g['soft_dets'], method)
    np.testing.assert_array_equal(got_i, g['soft_%s_inds' % method])
    np.testing.assert_array_equal(got_d, g['soft_%s_dets' % method])


def test_soft_nms_gaussian_is_bit_identical_to_the_reference(ops):
    """Method 2: identical indices in identical order, boxes AND scores bit-identical.  The device's double exp is accurate to 1 ulp
    of a double, not correctly rounded, so a float ulp per re-scoring (k * 2^-23 relative after k re-scorings) was the bar this test
    started with; the measured difference was zero on every row of every case (the double error almost never crosses a float
    rounding boundary), so the assertion is the tight one.  Inputs: the golden one and the cases tests/test_soft_nms_cpu.py
    qualifies (no decision of the reference run is closer than the k-ulp allowance), up to the kernel's capacity."""
    cases = [('golden', sc.golden_dets())] + [('smooth_n%d' % n, sc.smooth_dets(n, seed)) for n, seed in sc.GAUSSIAN_CASES]
    for name, dets in cases:
        ref_d, ref_i = _reference_soft_nms(dets, 'gaussian')
        got_d, got_i = _device_soft_nms(ops, dets, 'gaussian')
        rel = np.abs(got_d[:len(ref_d), 4].astype(np.float64) - ref_d[:len(got_d), 4]) / np.abs(ref_d[:len(got_d), 4].astype(np.float64))
        print('gaussian %-14s rows %4d  max |score diff| = %.3f ulp' % (name, len(ref_d), (rel / sc.ULP).max() if len(rel) else 0))
        np.testing.assert_array_equal(got_i, ref_i, err_msg=name)
        np.testing.assert_array_equal(got_d, ref_d, err_msg=name)
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'reference_postproc.npz'))
    got_d, got_i = _device_soft_nms(ops, g['soft_dets'], 'gaussian')
    np.testing.assert_array_equal(got_i, g['soft_gaussian_inds'])
    np.testing.assert_array_equal(got_d, g['soft_gaussian_dets'])


def test_soft_nms_rejects_more_rows_than_its_capacity_and_tubes(ops):
    from detectandtrack_amd import libdat
    assert ops.SOFT_NMS_MAX_BOXES == sc.CAPACITY
    with pytest.raises(libdat.DatError):
        ops.soft_nms(_dev(sc.smooth_dets(sc.CAPACITY + 1, 5)))
    with pytest.raises(NotImplementedError):
        ops.soft_nms(torch.zeros((4, 9), device='cuda'))


# ---- 4. dat_box_voting -----------------------------------------------------------------------------------------------------------
def _vote_f64(top, all_dets, thresh):
    """float64 score-weighted mean over the voters the reference's float32 IoU selects, and the float32 accumulation bound
    (m + 2) * 2^-24 * max|coordinate| for m voters."""
    ov = bu.bbox_overlaps(top[:, :4], all_dets[:, :4])
    out = top.astype(np.float64)
    tol = np.zeros((len(top), 1))
    for k in range(len(top)):
        v = np.where(ov[k] >= thresh)[0]
        w = all_dets[v, 4].astype(np.float64)
        out[k, :4] = (all_dets[v, :4].astype(np.float64) * w[:, None]).sum(axis=0) / w.sum()
        tol[k] = (len(v) + 2) * 2.0 ** -24 * np.abs(all_dets[v, :4]).max()
    return out, tol


def test_box_voting_matches_the_reference_and_repeats_bit_for_bit(ops):
    """dat_box_voting against the golden output of the reference's box_voting (the bar of tests/test_host_cpu.py: atol 1e-4), against
    utils/boxes.box_voting, and against a float64 weighted mean within the float32 accumulation bound; scores untouched; two runs
    bit-identical."""
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'reference_postproc.npz'))
    all_dets, top = g['soft_dets'], g['vote_top']
    got = ops.box_voting(_dev(top), _dev(all_dets), 0.8).cpu().numpy()
    np.testing.assert_allclose(got, g['vote_out'], rtol=0, atol=1e-4)
    np.testing.assert_allclose(got, bu.box_voting(top, all_dets, 0.8), rtol=0, atol=1e-4)
    for seed, n_all, n_top, th in ((1, 700, 90, 0.8), (2, 1500, 300, 0.5), (3, 65, 65, 0.3), (4, 1, 1, 0.8)):
        all_dets = sc.smooth_dets(n_all, seed)
        top = all_dets[np.random.RandomState(seed).permutation(n_all)[:n_top]]
        a = ops.box_voting(_dev(top), _dev(all_dets), th).cpu().numpy()
        b = ops.box_voting(_dev(top), _dev(all_dets), th).cpu().numpy()
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a[:, 4], top[:, 4])
        ref, tol = _vote_f64(top, all_dets, th)
        err = np.abs(a[:, :4] - ref[:, :4])
        print('voting n_all %4d n_top %3d: max error / bound = %.3f' % (n_all, n_top, (err / tol).max()))
        assert np.all(err <= tol), float((err / tol).max())


# ---- 5. dat_box_results_ex ---------------------------------------------------------------------------------------------------------
H, W, SCALE = 720, 1280, 800.0 / 720.0
WEIGHTS = (10., 10., 5., 5.)


def _image_inputs(seed, R, cap, K):
    """Proposals, class probabilities and deltas of one image.  The size deltas are zero, so the decode has no exp that NumPy and the
    device round differently: the host path below sees bit for bit the boxes the device decodes."""
    rs = np.random.RandomState(seed)
    xy = np.stack([rs.uniform(0, W * SCALE - 60, cap), rs.uniform(0, H * SCALE - 60, cap)], axis=1)
    # proposals cluster around a few objects, as after an RPN: overlaps are common
    centres = np.stack([rs.uniform(100, W * SCALE - 300, 12), rs.uniform(100, H * SCALE - 300, 12)], axis=1)
    xy = centres[rs.randint(0, 12, cap)] + rs.uniform(-40, 40, (cap, 2))
    wh = rs.uniform(60, 260, (cap, 2))
    rois = np.zeros((cap, 5), np.float32)
    rois[:, 1:3] = xy
    rois[:, 3:5] = xy + wh
    logits = rs.randn(cap, K).astype(np.float32) * 2
    prob = (np.exp(logits) / np.exp(logits).sum(axis=1, keepdims=True)).astype(np.float32)
    pred = (rs.randn(cap, K * 4) * np.tile([1.0, 1.0, 0.0, 0.0], K)).astype(np.float32)
    return rois, prob, pred


def _host_box_results(rois, prob, pred, K, D, soft, vote):
    """core/test.box_results_with_nms_and_limit (the comparison path) on the host-decoded boxes."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    cfg.MODEL.NUM_CLASSES = K
    cfg.TEST.SCORE_THRESH, cfg.TEST.NMS, cfg.TEST.DETECTIONS_PER_IM = 0.05, 0.5, D
    cfg.TEST.SOFT_NMS.ENABLED = soft is not None
    if soft is not None:
        cfg.TEST.SOFT_NMS.METHOD, cfg.TEST.SOFT_NMS.SIGMA = soft, 0.5
    cfg.TEST.BBOX_VOTE.ENABLED, cfg.TEST.BBOX_VOTE.VOTE_TH = bool(vote), 0.8
    try:
        # (core/test._read_bbox_outputs: float32 / float32(scale), bbox_transform, clip)
        scores = prob
        boxes = bu.clip_tiled_boxes(bu.bbox_transform(rois[:, 1:] / np.float32(SCALE), pred, WEIGHTS), (H, W, 3))
        s, b, cls_boxes = engine.box_results_with_nms_and_limit(scores.copy(), boxes.copy())
        # what the voting read: the class's selected rows, for the bound of the voted coordinates
        sel = [None] + [np.hstack((boxes[scores[:, j] > 0.05, 4 * j:4 * j + 4], scores[scores[:, j] > 0.05, j][:, None])).astype(np.float32)
                        for j in range(1, K)]
    finally:
        reset_cfg()
    return s, b, cls_boxes, sel


MODES = [('linear', False), ('gaussian', False), (None, True), ('linear', True)]


@pytest.mark.parametrize('soft,vote', MODES, ids=['soft_linear', 'soft_gaussian', 'vote_only', 'soft_linear_vote'])
@pytest.mark.parametrize('ni', [1, 4])
@pytest.mark.parametrize('D', [40, 0], ids=['limit_binds', 'no_limit'])
def test_box_results_with_soft_nms_and_voting_match_the_host_path(ops, soft, vote, ni, D):
    """dat_box_results_ex against core/test.box_results_with_nms_and_limit fed the same scores and decoded boxes, one image and
    four images per launch, DETECTIONS_PER_IM binding (40) and off: the same rows in the same order (class column, and the
    coordinates bit-identical without voting); scores bit-identical in every mode, gaussian included (the k * 2^-23 allowance of
    the stand-alone comparison measured zero and was tightened there, so it is tight here too); voted coordinates within
    (m + 2) * 2^-24 * max|coordinate of the row's m voters| of a float64 mean and of the host path's; keypoint_rois =
    float32(float64(box) * scale)."""
    K, R, cap = 3, 600, 640
    per = [_image_inputs(500 + 10 * ni + i, R, cap, K) for i in range(ni)]
    rois, prob, pred = (np.concatenate([p[c] for p in per]) for c in range(3))
    out_cap = D + 8 if D > 0 else cap * (K - 1)
    dets, kp, n_out = ops.box_results(_dev(rois), torch.tensor([R] * ni, dtype=torch.int32).cuda(), _dev(prob), _dev(pred), K, 1, SCALE,
                                      (H, W, 3), WEIGHTS, XFORM_CLIP, 0.05, 0.5, D, out_cap, n_images=ni,
                                      soft_nms=dict(method=soft, sigma=0.5, score_thresh=0.0001) if soft else None,
                                      bbox_vote=0.8 if vote else None)
    n = n_out.cpu().numpy().reshape(ni, 2)
    d_all, kp_all = dets.cpu().numpy().reshape(ni, out_cap, 6), kp.cpu().numpy().reshape(ni, out_cap, 5)
    for i in range(ni):
        ref_s, ref_b, cls_boxes, sel = _host_box_results(per[i][0][:R], per[i][1][:R], per[i][2][:R], K, D, soft, vote)
        assert n[i, 0] == n[i, 1] == len(ref_s), (i, n[i], len(ref_s))
        assert len(ref_s) > (D if D > 0 else 100) - 1
        k = int(n[i, 0])
        d = d_all[i, :k]
        ref_cls = np.concatenate([np.full((len(cls_boxes[j]),), j, np.float32) for j in range(1, K)])
        np.testing.assert_array_equal(d[:, 5], ref_cls)
        # (gaussian too: the standalone comparison measured a zero difference on every row, and the host path runs dat_soft_nms_host,
        #  itself bit-identical to the reference's Cython -- so the bar is bit-identity for every mode)
        np.testing.assert_array_equal(d[:, 4], ref_s)
        if vote:
            off = 0
            for j in range(1, K):
                m = len(cls_boxes[j])
                # the bar of the stand-alone voting test, per row: (m + 2) * 2^-24 * max|coordinate of its m voters|, voters counted for
                # the kept row as it was BEFORE voting (what the host path's box_voting was given) -- against the float64 mean, and
                # against the host path's own float32 np.average
                before = _unvoted(cls_boxes[j], sel[j], soft)
                ref64, tol = _vote_f64(before, sel[j], 0.8)
                err64 = np.abs(d[off:off + m, :4] - ref64[:, :4])
                err = np.abs(d[off:off + m, :4] - cls_boxes[j][:, :4])
                print('image %d class %d voting: max error / bound = %.3f (float64 mean), %.3f (host path)' % (
                    i, j, (err64 / tol).max() if m else 0, (err / tol).max() if m else 0))
                assert np.all(err64 <= tol) and np.all(err <= tol)
                off += m
        else:
            np.testing.assert_array_equal(d[:, :4], ref_b)
        exp_kp = np.hstack((np.full((k, 1), i, np.float32), (d[:, :4].astype(np.float64) * SCALE).astype(np.float32)))
        np.testing.assert_array_equal(kp_all[i, :k], exp_kp)
        assert not kp_all[i, k:].any() and not d_all[i, k:].any()


def _unvoted(voted, sel, soft):
    """The kept rows before voting: voting leaves scores alone and, without Soft-NMS, scores identify the selected rows (continuous
    random scores); with Soft-NMS the host loop is run again."""
    if soft is None:
        order = {float(s): r for r, s in enumerate(sel[:, 4])}
        return sel[[order[float(s)] for s in voted[:, 4]]]
    from detectandtrack_amd.core import nms_wrapper
    rows, _ = nms_wrapper.soft_nms(sel, sigma=0.5, overlap_thresh=0.5, score_thresh=0.0001, method=soft)
    by_score = {float(s): r for r, s in enumerate(rows[:, 4])}
    return rows[[by_score[float(s)] for s in voted[:, 4]]]


def test_box_results_ex_with_both_switches_off_is_box_results_batch(ops):
    """dat_box_results_ex with an all-off options struct runs dat_box_results_batch: byte-identical outputs, same workspace size."""
    import ctypes as C
    from detectandtrack_amd import libdat as L
    K, R, cap, ni, D = 3, 600, 640, 4, 40
    per = [_image_inputs(900 + i, R, cap, K) for i in range(ni)]
    rois, prob, pred = (_dev(np.concatenate([p[c] for p in per])) for c in range(3))
    n_rois = torch.tensor([R] * ni, dtype=torch.int32).cuda()
    base = ops.box_results(rois, n_rois, prob, pred, K, 1, SCALE, (H, W, 3), WEIGHTS, XFORM_CLIP, 0.05, 0.5, D, D + 8, n_images=ni)
    opts = L.DetOpts()
    assert L.lib().dat_box_results_ex_workspace_bytes(cap, K, 1, C.byref(opts)) == L.lib().dat_box_results_workspace_bytes(cap, K, 1)
    ds = (L.DetDesc * ni)()
    for d in ds:
        d.num_classes, d.T, d.cls_agnostic_bbox_reg, d.detections_per_im = K, 1, 0, D
        d.im_scale, d.im_scale_f64, d.im_h, d.im_w = SCALE, SCALE, H, W
        for q in range(4):
            d.reg_weights[q] = WEIGHTS[q]
        d.xform_clip, d.score_thresh, d.nms_thresh = XFORM_CLIP, 0.05, 0.5
    wsb = torch.empty(ni * L.lib().dat_box_results_workspace_bytes(cap, K, 1), dtype=torch.uint8, device='cuda')
    dets = torch.full((ni * (D + 8), 6), -7.0, device='cuda')
    kp = torch.full((ni * (D + 8), 5), -7.0, device='cuda')
    n_out = torch.full((ni, 2), -7, dtype=torch.int32, device='cuda')
    ops.ctx().call('dat_box_results_ex', ops._stream(), ops._ptr(rois), ops._ptr(n_rois), cap, ops._ptr(prob), K, ops._ptr(pred), 4 * K, ds,
                   C.byref(opts), ni, ops._ptr(wsb), D + 8, ops._ptr(dets), ops._ptr(kp), ops._ptr(n_out))
    for a, b in zip(base, (dets, kp, n_out)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # Soft-NMS above the kernel's capacity is an argument error, not a truncation
    from detectandtrack_amd import libdat
    big = sc.CAPACITY + 8
    r2, p2, q2 = (_dev(a) for a in _image_inputs(1, 100, big, K))
    with pytest.raises(libdat.DatError):
        ops.box_results(r2, torch.tensor([100], dtype=torch.int32).cuda(), p2, q2, K, 1, SCALE, (H, W, 3), WEIGHTS, XFORM_CLIP, 0.05, 0.5, D, D,
                        soft_nms=dict(method='linear'))


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------
VOTE_TH_E2E = 0.7      # not the default 0.8: a threshold that did not travel from cfg to the kernel would show


def _soft_cfg(T, Hh, Ww, method='linear', device=True, mode='soft', **hip):
    c = fpn3d_kps_cfg('18', T=T, dtype='fp32', pre=300, post=100)
    c['TEST'].update(SCALES=(Hh,), MAX_SIZE=max(Hh, Ww), SCORE_THRESH=0.0, DETECTIONS_PER_IM=15,
                     SOFT_NMS={'ENABLED': mode == 'soft', 'METHOD': method, 'SIGMA': 0.5},
                     BBOX_VOTE={'ENABLED': mode == 'vote', 'VOTE_TH': VOTE_TH_E2E})
    c['HIP'].update(DEVICE_BOX_RESULTS=device, **hip)
    return c


def _build_without_size_deltas(cfg_dict, seed=3):
    """tests/model_util.build_product with the width / height rows of `bbox_pred` zeroed: dw = dh = 0, so the box decode has no exp
    that NumPy (host path) and the device round differently, both paths see bit for bit the same boxes and the linear Soft-NMS
    scores can be compared exactly."""
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
    weights = net_utils.synthetic_params(model, seed)
    for name in ('bbox_pred_w', 'bbox_pred_b'):
        w = np.array(weights[name], copy=True)
        assert w.shape[0] == 4 * cfg.MODEL.NUM_CLASSES
        w[2::4] = 0
        w[3::4] = 0
        weights[name] = w
    for k, v in weights.items():
        ws.set_param(k, v)
    ws.CreateNet(model.net)
    ws.CreateNet(model.conv_body_net)
    ws.CreateNet(model.keypoint_net)
    return model, ws


@pytest.mark.parametrize('mode', ['soft', 'vote'])
def test_im_detect_all_with_soft_nms_takes_the_device_path_and_matches_the_host_path(monkeypatch, mode):
    """mode 'vote': the same with TEST.BBOX_VOTE (hard NMS, VOTE_TH 0.7) in place of Soft-NMS -- scores bit-identical, voted boxes within
    the voting bound (m + 2) * 2^-24 * max|coordinate of the row's voters| of the float64 mean over what the host path's box_voting
    was given, and of the host path's boxes.  mode 'soft':
    TEST.SOFT_NMS.ENABLED no longer leaves the device path: im_detect_all never calls box_results_with_nms_and_limit (patched to
    raise), and returns what it returns with cfg.HIP.DEVICE_BOX_RESULTS False -- the same rows in the same order, boxes and linear
    scores bit-identical (the model predicts no size deltas, see _build_without_size_deltas), keypoints within a pixel for 95 % (the
    bar of the several-images-per-forward test); four clips in one forward (im_detect_all_batch) give every clip the detections it
    gets alone."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.ops import hip_ops
    T, Hh, Ww, B = 2, 96, 128, 4
    rs = np.random.RandomState(21)
    ims = [[rs.randint(0, 255, (Hh, Ww, 3)).astype(np.uint8) for _ in range(T)] for _ in range(B)]
    def boom(*a, **k):
        raise AssertionError('the host post-processing ran with TEST.SOFT_NMS / TEST.BBOX_VOTE on')
    assert hip_ops.tune_plan(0, 1) == 0          # no split-K: a clip's sums depend neither on the batch size nor on the path
    votes = []                                   # (top_dets, all_dets) of every host box_voting call, in clip order
    real_voting = bu.box_voting

    def recording_voting(top, all_dets, thresh):
        assert thresh == VOTE_TH_E2E
        votes.append((top.copy(), all_dets.copy()))
        return real_voting(top, all_dets, thresh)
    try:
        model, ws = _build_without_size_deltas(_soft_cfg(T, Hh, Ww, device=False, mode=mode))
        assert not engine.device_results_supported()
        monkeypatch.setattr(bu, 'box_voting', recording_voting)
        host = [engine.im_detect_all(model, im, None) for im in ims]
        monkeypatch.setattr(bu, 'box_voting', real_voting)
        assert len(votes) == (B if mode == 'vote' else 0)
        model, ws = _build_without_size_deltas(_soft_cfg(T, Hh, Ww, mode=mode))
        assert engine.device_results_supported()
        monkeypatch.setattr(engine, 'box_results_with_nms_and_limit', boom)
        singles = [engine.im_detect_all(model, im, None) for im in ims]
        batch = engine.im_detect_all_batch(model, ims)
    finally:
        hip_ops.tune_plan(0, 0)
    for i in range(B):
        hb, db = host[i][0][1], singles[i][0][1]
        assert hb.shape == db.shape and hb.shape[0] >= 15
        np.testing.assert_array_equal(db[:, 4], hb[:, 4])
        if mode == 'vote':
            top, all_dets = votes[i]
            ref64, tol = _vote_f64(top, all_dets, VOTE_TH_E2E)
            # the limit kept a subset of `top`; voting leaves scores alone, so a kept row is the `top` row of its score -- among rows of
            # one score (duplicate proposals), the one whose float64 mean is nearest to the host path's voted box
            rows = []
            for r, sv in enumerate(hb[:, 4]):
                cand = np.where(top[:, 4] == sv)[0]
                rows.append(int(cand[np.abs(ref64[cand, :4] - hb[r, :4]).max(axis=1).argmin()]))
            np.testing.assert_array_equal(top[rows, 4], hb[:, 4])
            e64, eh = np.abs(db[:, :4] - ref64[rows, :4]), np.abs(db[:, :4] - hb[:, :4])
            print('clip %d voting: max error / bound = %.3f (float64 mean), %.3f (host path); rows moved by voting: %d' % (
                i, (e64 / tol[rows]).max(), (eh / tol[rows]).max(), int((np.abs(hb[:, :4] - top[rows, :4]).max(axis=1) > 0.01).sum())))
            assert np.all(e64 <= tol[rows]) and np.all(eh <= tol[rows])
            assert (np.abs(hb[:, :4] - top[rows, :4]).max(axis=1) > 0.01).any()      # (voting did move boxes)
        else:
            np.testing.assert_array_equal(db[:, :4], hb[:, :4])
        assert hb[:, 4].min() < 0.999 * hb[:, 4].max()
        hk, dk = np.stack(host[i][2][1]), np.stack(singles[i][2][1])
        assert (np.abs(hk[:, :2] - dk[:, :2]) < 1.0).mean() > 0.95
        np.testing.assert_array_equal(batch[i][0][1], db, err_msg='detections of clip %d in the batch' % i)
        for a, b in zip(batch[i][2][1], singles[i][2][1]):
            np.testing.assert_array_equal(a, b, err_msg='keypoints of clip %d in the batch' % i)


def test_pipelined_engine_with_soft_nms_writes_the_eager_loop_detections(tmp_path):
    """test_net over a short clip list with TEST.SOFT_NMS on: the pipelined engine (forwards in flight, hipGraph replay) accepts the
    list and writes the detections of the one-clip-at-a-time loop, bit for bit (one clip per forward: the same kernels)."""
    from detectandtrack_amd.core import test_engine
    from detectandtrack_amd.core.config import cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd import workspace
    T, Hh, Ww = 2, 96, 128
    rs = np.random.RandomState(5)
    roidb = [{'image': [rs.randint(0, 255, (Hh, Ww, 3)).astype(np.uint8) for _ in range(T)], 'height': Hh, 'width': Ww} for _ in range(5)]

    def run(depth, graph, out):
        c = _soft_cfg(T, Hh, Ww, PIPELINE_DEPTH=depth, IMS_PER_FORWARD=1, CLIP_GRAPH=graph)
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
    assert st is not None and st['clips'] == 5 and st['per_forward'] == 1      # the pipelined engine took the list
    for i in range(5):
        np.testing.assert_array_equal(got['all_boxes'][1][i], eager['all_boxes'][1][i])
        assert len(got['all_keyps'][1][i]) == len(eager['all_keyps'][1][i]) >= 15
        for a, b in zip(got['all_keyps'][1][i], eager['all_keyps'][1][i]):
            np.testing.assert_array_equal(a, b)
    reset_cfg()
