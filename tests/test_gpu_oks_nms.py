"""GPU tests of KRCNN.NMS_OKS on the device (csrc/oks_nms.hip: dat_oks_nms): the kernel against its host twin
dat_oks_nms_host, the reference's golden cases, and the engine paths the switch opens (im_detect_all on the device path against the
host path, the pipelined engine with two clips per forward)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import oks_nms_ref as R
from tests.model_util import c4_tube_kps_cfg, fpn2d_kps_cfg, fpn3d_kps_cfg

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = R.K


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_and_compare(ops, images, T, cap, thresh=R.THRESH):
    """images: [(kps [n, 4, 17T], dets [n, 4T+2])] -> one dat_oks_nms call over all of them, `cap` rows per image, the dead rows filled
    with NaN (they must never be read as data), compared with dat_oks_nms_host image by image: keep, n_keep, the gathered rows and the
    zero tail exactly; n_out and the inputs unchanged; a second run writes identical bytes.  Asserts the margins on the host values."""
    ni, ld = len(images), 4 * T + 2
    kps_all = np.full((ni * cap, 4, K * T), np.nan, dtype=np.float32)
    dets_all = np.full((ni * cap, ld), np.nan, dtype=np.float32)
    n_out = np.zeros((ni, 2), dtype=np.int32)
    for i, (kps, dets) in enumerate(images):
        n = len(dets)
        assert n <= cap
        kps_all[i * cap:i * cap + n] = kps
        dets_all[i * cap:i * cap + n] = dets
        n_out[i] = (n, n)
    kps_d, dets_d, n_d = _dev(kps_all), _dev(dets_all), _dev(n_out)
    n_rows = n_d[0:1, 0] if ni == 1 else n_d[:, 0]            # the strided column the engine passes
    out1 = ops.oks_nms(kps_d, dets_d, n_rows, ni, T, K, thresh)
    out2 = ops.oks_nms(kps_d, dets_d, n_rows, ni, T, K, thresh)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in out1]
    for a, b in zip(got, out2):
        assert a.tobytes() == b.cpu().numpy().tobytes()      # no atomics: the same bytes run after run
    assert kps_d.cpu().numpy().tobytes() == kps_all.tobytes() and dets_d.cpu().numpy().tobytes() == dets_all.tobytes()
    assert np.array_equal(n_d.cpu().numpy(), n_out)
    g_dets, g_kps, g_keep, g_n = got
    assert g_dets.shape == (ni * cap, ld) and g_kps.shape == (ni * cap, 4, K * T) and g_keep.shape == (ni, cap) and g_n.shape == (ni,)
    kept = []
    for i, (kps, dets) in enumerate(images):
        keep, scores, oks = ops.oks_nms_host(kps, dets, T, thresh, want_oks=True)
        m_oks, m_score = R.margins(scores, oks, thresh)
        print('image %d: %d rows, %d kept, margins: OKS %.3g, score %.3g' % (i, len(dets), len(keep), m_oks, m_score))
        assert m_oks > R.OKS_MARGIN and m_score > R.SCORE_MARGIN
        nk = len(keep)
        assert int(g_n[i]) == nk
        assert g_keep[i, :nk].tolist() == keep.tolist() and np.all(g_keep[i, nk:] == -1)
        lo = i * cap
        assert g_dets[lo:lo + nk].tobytes() == np.ascontiguousarray(dets[keep]).tobytes()
        assert g_kps[lo:lo + nk].tobytes() == np.ascontiguousarray(kps[keep]).tobytes()
        assert not g_dets[lo + nk:lo + cap].view(np.uint32).any() and not g_kps[lo + nk:lo + cap].view(np.uint32).any()
        kept.append(keep)
    return kept


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65, 104, 300])
def test_kernel_equals_the_host_twin(ops, n, T):
    kps, dets = R.clustered_poses(n, T, R.seed_for(n, T))
    keep, = _run_and_compare(ops, [(kps, dets)], T, cap=n + 3)
    assert n < 63 or 1 < len(keep) < n            # rows were removed, and not all of them


@pytest.mark.parametrize('T', [1, 3])
def test_three_images_in_one_call(ops, T):
    images = [R.clustered_poses(n, T, R.seed_for(n, T)) for n in (104, 0, 17)]
    kept = _run_and_compare(ops, images, T, cap=104)
    assert len(kept[0]) > 1 and len(kept[1]) == 0 and 1 < len(kept[2]) < 17


def test_kernel_on_the_reference_cases(ops):
    """tests/golden/reference_oks_nms.json: the kernel returns the keep lists the reference's own nms_oks returned."""
    with open(os.path.join(REPO, 'tests', 'golden', 'reference_oks_nms.json')) as f:
        g = json.load(f)
    names = sorted(g['sets'])
    images, cap = [], 0
    for name in names:
        s = g['sets'][name]
        kps, rois = np.asarray(s['kps'], dtype=np.float32), np.asarray(s['rois'], dtype=np.float32)
        images.append((kps, np.hstack([rois, np.full((len(rois), 2), 1.0, dtype=np.float32)])))
        cap = max(cap, len(rois) + 1)
    kept = _run_and_compare(ops, images, 1, cap, thresh=float(g['thresh']))
    for name, keep in zip(names, kept):
        assert keep.tolist() == g['sets'][name]['keep'], name


def test_more_rows_than_the_kernel_holds_are_refused(ops):
    from detectandtrack_amd import libdat
    cap = ops.OKS_NMS_MAX_ROWS + 1
    kps = torch.zeros((cap, 4, K), device='cuda')
    dets = torch.zeros((cap, 6), device='cuda')
    n = torch.tensor([2], dtype=torch.int32, device='cuda')
    outs = [torch.full((cap, 6), -7.0, device='cuda'), torch.full((cap, 4, K), -7.0, device='cuda'),
            torch.full((1, cap), -7, dtype=torch.int32, device='cuda'), torch.full((1,), -7, dtype=torch.int32, device='cuda')]

    def call(cap_, T=1, k=K):
        ops.ctx().call('dat_oks_nms', ops._stream(), ops._ptr(kps), ops._ptr(dets), 6, ops._ptr(n), 1, cap_, 1, T, k, 0.3,
                       ops._ptr(outs[2]), ops._ptr(outs[3]), ops._ptr(outs[0]), ops._ptr(outs[1]))
    for bad in (dict(cap_=cap), dict(cap_=8, T=0), dict(cap_=8, T=17), dict(cap_=8, k=16)):
        with pytest.raises(libdat.DatError):
            call(**bad)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == -7).all())            # nothing was launched
    call(8)
    torch.cuda.synchronize()
    assert int(outs[3].item()) == 1 and outs[2][0, :8].tolist() == [1] + [-1] * 7      # two equal rows: the later one is kept


# ---- model level -----------------------------------------------------------------------------------------------------------------------
H_E2E, W_E2E, T_TUBE, T_CLIP = 96, 128, 3, 2


def _model_cfg(kind, device=True, oks=False, thresh=R.THRESH, **hip):
    if kind in ('boxes', 'clips'):          # 'clips': the 3D body with slice-center 2D heads of the other pipeline tests -- box detections
        c = fpn2d_kps_cfg('18', pre=300, post=100, dtype='fp32') if kind == 'boxes' else fpn3d_kps_cfg('18', T=T_CLIP, dtype='fp32', pre=300, post=100)
        c['TEST'].update(SCALES=(H_E2E,), MAX_SIZE=max(H_E2E, W_E2E), SCORE_THRESH=0.0, DETECTIONS_PER_IM=15)
    else:
        c = c4_tube_kps_cfg(T=T_TUBE, dtype='fp32', pre=300, post=64)
        # (proposal NMS at 0.9, as tests/test_gpu_tube_soft_nms.py: the detections overlap)
        c['TEST'].update(SCALES=(H_E2E,), MAX_SIZE=max(H_E2E, W_E2E), SCORE_THRESH=0.0, DETECTIONS_PER_IM=15, RPN_NMS_THRESH=0.9)
    c['KRCNN']['NMS_OKS'] = bool(oks)
    c['HIP'].update(DEVICE_BOX_RESULTS=device, TUBE_NMS_OKS=(kind == 'tubes'), NMS_OKS_THRESH=float(thresh), **hip)
    return c


def _build(kind, cfg_dict):
    """The models of the Soft-NMS tests: no size deltas, so both paths decode (nearly) the same boxes."""
    if kind != 'tubes':
        from tests.test_gpu_soft_nms import _build_without_size_deltas as build
    else:
        from tests.test_gpu_tube_soft_nms import _build_without_size_deltas as build
    return build(cfg_dict)[0]


def _clips(kind, n, seed):
    rs = np.random.RandomState(seed)
    T = {'boxes': 1, 'tubes': T_TUBE, 'clips': T_CLIP}[kind]
    return [[rs.randint(0, 255, (H_E2E, W_E2E, 3)).astype(np.uint8) for _ in range(T)] for _ in range(n)]


def _pick_threshold(results):
    """Random weights give OKS values near zero, so 0.3 would remove nothing.  From the poses of runs WITHOUT the switch: the threshold
    in the widest relative gap between two neighbouring OKS values for which the host loop, on every clip, removes at least one row and
    keeps at least two.  Returns (threshold, the keep lists, the smallest |log(OKS / threshold)| over all pairs)."""
    from detectandtrack_amd.utils import keypoints as kp
    mats, poses = [], []
    for cls_boxes, _, cls_keyps in results:
        boxes, kps = np.asarray(cls_boxes[1])[:, :-1], np.stack(cls_keyps[1])
        oks = kp.compute_oks if boxes.shape[1] == 4 else kp.compute_oks_tubes
        m = np.stack([oks(kps[i], boxes[i], kps, boxes) for i in range(len(kps))])
        mats.append(m[~np.eye(len(kps), dtype=bool)])
        poses.append((kps, boxes))
    vals = np.unique(np.concatenate(mats))
    vals = vals[vals > 1e-300]
    gaps = np.log(vals[1:] / vals[:-1])
    for g in np.argsort(gaps, kind='stable')[::-1]:           # widest gap first
        th = float(np.sqrt(vals[g] * vals[g + 1]))
        keeps = [[int(i) for i in kp.nms_oks(kps, boxes, th)] for kps, boxes in poses]
        if all(2 <= len(k) < len(p[0]) for k, p in zip(keeps, poses)):
            return th, keeps, 0.5 * float(gaps[g])
    raise AssertionError('no threshold removes a row and keeps two on every clip')


@pytest.mark.parametrize('kind', ['boxes', 'tubes'])
def test_im_detect_all_on_the_device_path_matches_the_host_path(monkeypatch, kind):
    """R-18 FPN 2D keypoint model (boxes) and R-18 C4 tube model with HIP.TUBE_NMS_OKS (T = 3): with KRCNN.NMS_OKS im_detect_all stays on
    the device path (box_results_with_nms_and_limit patched to raise) and returns what the host path (HIP.DEVICE_BOX_RESULTS False)
    returns: the same rows in the same order -- scores bit-identical, boxes bit-identical (boxes) or within the decode bound of
    tests/test_gpu_tube_soft_nms.py (tubes: float64 on the host, float32 on the device, 1e-4 pixels), keypoints at the bar of the other
    two-path tests (within a pixel for 95 %).  The host result removes at least one row and keeps at least two."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.ops import hip_ops
    ims = _clips(kind, 2, 21)

    def boom(*a, **k):
        raise AssertionError('the host post-processing ran with KRCNN.NMS_OKS on')
    assert hip_ops.tune_plan(0, 1) == 0          # no split-K: a clip's sums do not depend on the path
    try:
        model = _build(kind, _model_cfg(kind, device=False))
        assert not engine.device_results_supported()
        plain = [engine.im_detect_all(model, im, None) for im in ims]
        thresh, keeps, gap = _pick_threshold(plain)
        print('%s: HIP.NMS_OKS_THRESH = %.6g, keep lists %s of %s rows, log-margin %.3g' % (kind, thresh, keeps, [len(p[0][1]) for p in plain], gap))
        cfg.KRCNN.NMS_OKS, cfg.HIP.NMS_OKS_THRESH = True, thresh
        host = [engine.im_detect_all(model, im, None) for im in ims]
        model = _build(kind, _model_cfg(kind, oks=True, thresh=thresh))
        assert engine.device_results_supported()
        monkeypatch.setattr(engine, 'box_results_with_nms_and_limit', boom)
        device = [engine.im_detect_all(model, im, None) for im in ims]
    finally:
        hip_ops.tune_plan(0, 0)
    for i in range(len(ims)):
        pb, hb, db = plain[i][0][1], host[i][0][1], device[i][0][1]
        assert 2 <= len(hb) < len(pb) and len(hb) == len(keeps[i])            # not vacuous: a row went, two stayed
        np.testing.assert_array_equal(hb, pb[keeps[i]])                       # the host path filtered and reordered boxes ...
        for a, j in zip(host[i][2][1], keeps[i]):
            np.testing.assert_array_equal(a, plain[i][2][1][j])               # ... and poses by one keep list
        assert db.shape == hb.shape
        np.testing.assert_array_equal(db[:, -1], hb[:, -1])                   # the same rows in the same order
        if kind == 'boxes':
            np.testing.assert_array_equal(db, hb)
        else:
            np.testing.assert_allclose(db[:, :-1], hb[:, :-1], rtol=0, atol=1e-4)
        hk, dk = np.stack(host[i][2][1]), np.stack(device[i][2][1])
        assert hk.shape == dk.shape == (len(hb), 4, K * (1 if kind == 'boxes' else T_TUBE))
        assert (np.abs(hk[:, :2] - dk[:, :2]) < 1.0).mean() > 0.95


def test_pipelined_engine_with_two_clips_per_forward_returns_what_im_detect_all_returns():
    """core/pipeline.ClipPipeline with hipGraph replay, two clips per forward, KRCNN.NMS_OKS on: dat_oks_nms is part of the captured
    graph and every clip comes back with the rows im_detect_all gives it alone, bit for bit (no split-K, as the batch tests: a clip's
    sums do not depend on the batch size).  The second forward replays the graph the first one captured."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.core.pipeline import ClipPipeline
    from detectandtrack_amd import workspace
    from detectandtrack_amd.ops import hip_ops
    kind = 'clips'
    clips = _clips(kind, 4, 33)
    assert hip_ops.tune_plan(0, 1) == 0
    pipe = None
    try:
        model = _build(kind, _model_cfg(kind))
        plain = [engine.im_detect_all(model, im, None) for im in clips]
        thresh, keeps, gap = _pick_threshold(plain)
        cfg.KRCNN.NMS_OKS, cfg.HIP.NMS_OKS_THRESH = True, thresh
        assert engine.device_results_supported()
        ref = [engine.im_detect_all(model, im, None) for im in clips]
        pipe = ClipPipeline(model, workspace.GlobalWorkspace(), depth=1, graph=True)
        with torch.cuda.stream(pipe.slots[0].stream):
            assert hip_ops.tune_plan(0, 1) == 0
        out = []
        for pair in (clips[:2], clips[2:]):
            pipe.submit_frames(pair, tag='x')
            (_, res), = pipe.drain()
            out.extend(res)
        assert pipe.graphs_captured == 1 and pipe.rerun_images == 0 and pipe.host_path_images == 0
    finally:
        if pipe is not None:
            with torch.cuda.stream(pipe.slots[0].stream):
                hip_ops.tune_plan(0, 0)
        hip_ops.tune_plan(0, 0)
    for i in range(len(clips)):
        assert 2 <= len(ref[i][0][1]) < len(plain[i][0][1]) and len(ref[i][0][1]) == len(keeps[i])
        np.testing.assert_array_equal(ref[i][0][1][:, -1], plain[i][0][1][keeps[i], -1])
        np.testing.assert_array_equal(out[i][0][1], ref[i][0][1])
        assert len(out[i][2][1]) == len(ref[i][2][1])
        for a, b in zip(out[i][2][1], ref[i][2][1]):
            np.testing.assert_array_equal(a, b)
