"""KRCNN.NMS_OKS without a GPU: the host restatements of the reference's nms_oks / compute_oks against vectors
the reference itself produced (tests/golden/reference_oks_nms.json, tests/golden/make_golden_oks_nms.py), the C host twin
dat_oks_nms_host, the tube form, the tie rule, the wiring of core/test.py's host path and the C ABI."""
import ctypes
import json
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dat_oks_nms', 'dat_oks_nms_host')
K = 17


@pytest.fixture(scope='module')
def golden_oks():
    with open(os.path.join(REPO, 'tests', 'golden', 'reference_oks_nms.json')) as f:
        g = json.load(f)
    sets = {name: dict(kps=np.asarray(s['kps'], dtype=np.float32), rois=np.asarray(s['rois'], dtype=np.float32), keep=list(s['keep']),
                       oks=np.asarray(s['oks'], dtype=np.float64)) for name, s in g['sets'].items()}
    return float(g['thresh']), sets


@pytest.fixture
def default_cfg():
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    yield cfg
    reset_cfg()


SETS = ('near_duplicates', 'asymmetric_area', 'asymmetric_area_reversed', 'chain', 'removes_all', 'none_removed')


def test_the_golden_file_holds_the_cases(golden_oks):
    thresh, sets = golden_oks
    assert thresh == 0.3 and sorted(sets) == sorted(SETS)
    o = sets['asymmetric_area']['oks']
    assert o[0, 1] < thresh < o[1, 0]          # the result depends on whose area is used
    assert sets['asymmetric_area']['keep'] == [0, 1] and sets['asymmetric_area_reversed']['keep'] == [1]
    o = sets['chain']['oks']                     # rows: B, C, A
    assert o[2, 0] > thresh and o[0, 1] > thresh and o[2, 1] < thresh and sets['chain']['keep'] == [2, 1]


# ---- the NumPy restatements against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SETS)
def test_nms_oks_returns_the_reference_keep_lists(golden_oks, name):
    from detectandtrack_amd.utils import keypoints as kp
    thresh, sets = golden_oks
    s = sets[name]
    assert [int(i) for i in kp.nms_oks(s['kps'], s['rois'], thresh)] == s['keep']


@pytest.mark.parametrize('name', SETS)
def test_compute_oks_equals_the_reference_values(golden_oks, name):
    """float64 values in [0, 1]; 17 terms of summation-order slack are about 2e-15."""
    from detectandtrack_amd.utils import keypoints as kp
    s = golden_oks[1][name]
    for i in range(len(s['kps'])):
        got = kp.compute_oks(s['kps'][i], s['rois'][i], s['kps'], s['rois'])
        assert got.dtype == np.float64 and np.abs(got - s['oks'][i]).max() < 1e-12
        tube = kp.compute_oks_tubes(s['kps'][i], s['rois'][i], s['kps'], s['rois'])
        assert np.array_equal(tube, got)          # the tube form at T = 1, bit for bit


# ---- the C host twin ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SETS)
def test_c_host_loop_returns_the_reference_keep_lists(golden_oks, name):
    from detectandtrack_amd.ops import hip_ops as ops
    thresh, sets = golden_oks
    s = sets[name]
    keep, scores, oks = ops.oks_nms_host(s['kps'], s['rois'], 1, thresh, want_oks=True)
    assert keep.tolist() == s['keep']
    assert np.abs(scores - np.mean(s['kps'][:, 2, :].astype(np.float64), axis=1)).max() < 1e-12
    seen = ~np.isnan(oks)
    assert seen.sum() >= len(s['kps']) - 1 and not seen.diagonal().any()         # (the first kept row meets all the others)
    assert np.abs(oks[seen] - s['oks'][seen]).max() < 1e-12
    # its own tube form: three copies of the frame are a tube whose per-frame values are all the box value
    kps3 = np.concatenate([s['kps']] * 3, axis=2)
    rois3 = np.concatenate([s['rois']] * 3, axis=1)
    keep3, scores3, oks3 = ops.oks_nms_host(kps3, rois3, 3, thresh, want_oks=True)
    assert keep3.tolist() == keep.tolist() and np.array_equal(np.isnan(oks3), np.isnan(oks))
    assert np.abs(oks3[seen] - oks[seen]).max() < 1e-15 and np.abs(scores3 - scores).max() < 1e-14


def test_c_host_loop_reads_boxes_in_place_from_detection_rows(golden_oks):
    """The boxes may sit at the start of wider rows ([4T | score | class]): the columns behind them are not read."""
    from detectandtrack_amd.ops import hip_ops as ops
    thresh, sets = golden_oks
    s = sets['near_duplicates']
    wide = np.hstack([s['rois'], np.full((len(s['rois']), 2), np.nan, dtype=np.float32)])
    assert ops.oks_nms_host(s['kps'], wide, 1, thresh)[0].tolist() == s['keep']


def test_c_host_loop_refuses_bad_arguments():
    from detectandtrack_amd import libdat
    f = libdat.lib().dat_oks_nms_host
    kps = np.zeros((2, 4, K), dtype=np.float32)
    box = np.zeros((2, 4), dtype=np.float32)
    keep = np.zeros(2, dtype=np.int32)
    nk = ctypes.c_int(-7)
    pf, pi = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)

    def call(n=2, T=1, k=K, ld=4):
        return f(kps.ctypes.data_as(pf), box.ctypes.data_as(pf), ld, n, T, k, 0.3, keep.ctypes.data_as(pi), ctypes.byref(nk), None, None)
    assert call() == 0 and nk.value == 1 and keep[0] == 1           # two identical poses with equal scores: the later row is visited first
    assert call(n=0) == 0 and nk.value == 0
    for bad in (dict(T=0), dict(T=17), dict(k=16), dict(ld=3), dict(n=-1)):
        assert call(**bad) == -1, bad


# ---- ties, tubes ----------------------------------------------------------------------------------------------------------------------------
def _far_apart_poses(n, T=1, seed=5):
    rs = np.random.RandomState(seed)
    kps = np.zeros((n, 4, K * T), dtype=np.float32)
    rois = np.zeros((n, 4 * T), dtype=np.float32)
    for i in range(n):
        for t in range(T):
            x0, y0 = 300.0 * i, 40.0 * t
            rois[i, 4 * t:4 * t + 4] = (x0, y0, x0 + 60, y0 + 120)
            kps[i, 0, t * K:(t + 1) * K] = rs.uniform(x0, x0 + 60, K)
            kps[i, 1, t * K:(t + 1) * K] = rs.uniform(y0, y0 + 120, K)
    return kps, rois


def test_equal_scores_are_visited_in_stable_reversed_order():
    """np.argsort(scores, kind='stable')[::-1]: among equal scores the later row comes first -- a definition (the reference's argsort leaves
    ties undefined)."""
    from detectandtrack_amd.ops import hip_ops as ops
    from detectandtrack_amd.utils import keypoints as kp
    kps, rois = _far_apart_poses(5)
    logits = np.random.RandomState(9).uniform(1, 3, K).astype(np.float32)
    kps[:, 2, :] = logits                     # five equal scores
    kps[2, 2, :] = logits + np.float32(1)     # and one better row in the middle
    want = [2, 4, 3, 1, 0]
    assert [int(i) for i in kp.nms_oks(kps, rois, 0.3)] == want
    assert ops.oks_nms_host(kps, rois, 1, 0.3)[0].tolist() == want


def _hand_worked_tubes():
    """Two tubes of T = 3, identical in frames 0 and 1 (per-frame OKS exactly 1) and 1000 px apart in frame 2 (exp(-huge) = 0): the mean is
    exactly 2 / 3."""
    kps, rois = _far_apart_poses(1, T=3)
    kps, rois = np.concatenate([kps, kps]), np.concatenate([rois, rois])
    kps[1, 0, 2 * K:] += np.float32(1000)
    kps[0, 2, :], kps[1, 2, :] = 5.0, 4.0
    return kps, rois


def test_hand_worked_tube_case():
    from detectandtrack_amd.ops import hip_ops as ops
    from detectandtrack_amd.utils import keypoints as kp
    kps, rois = _hand_worked_tubes()
    oks = kp.compute_oks_tubes(kps[0], rois[0], kps[1:], rois[1:])
    assert oks[0] == 2.0 / 3.0
    assert [int(i) for i in kp.nms_oks(kps, rois, 0.3)] == [0]              # 2/3 > 0.3: the second tube goes
    assert [int(i) for i in kp.nms_oks(kps, rois, 0.7)] == [0, 1]           # 2/3 <= 0.7: it stays
    keep, _, m = ops.oks_nms_host(kps, rois, 3, 0.3, want_oks=True)
    assert keep.tolist() == [0] and m[0, 1] == 2.0 / 3.0
    assert ops.oks_nms_host(kps, rois, 3, 0.7)[0].tolist() == [0, 1]


# ---- core/test.py: the host path -----------------------------------------------------------------------------------------------------------
def _peaked_heatmaps(cells, logits, M=14):
    """[N, 17 T, M, M] maps with one peak per keypoint: cells [N, 17 T, 2] (row, column), logits [N]."""
    n, c = cells.shape[:2]
    maps = np.full((n, c, M, M), -4.0, dtype=np.float32)
    for i in range(n):
        for k in range(c):
            maps[i, k, cells[i, k, 0], cells[i, k, 1]] = logits[i]
    return maps


def _box_case():
    """Four person detections: rows 0 and 2 are the same pose in boxes one pixel apart (OKS close to 1), rows 1 and 3 lie elsewhere.  Row 2
    has the higher logits, so it is visited before row 0 and removes it: keep = [2, 1, 3] in score order."""
    rs = np.random.RandomState(11)
    cells = rs.randint(2, 12, (4, K, 2))
    cells[2] = cells[0]
    boxes = np.array([[20, 30, 80, 150], [200, 40, 260, 170], [21, 30, 81, 150], [400, 50, 470, 190]], dtype=np.float32)
    maps = _peaked_heatmaps(cells, [1.0, 10.0, 40.0, 4.0])
    dets = np.hstack([boxes, np.array([[0.9], [0.8], [0.7], [0.6]], dtype=np.float32)])
    return maps, boxes, dets, [2, 1, 3]


def test_keypoint_results_filters_and_reorders_boxes_and_poses(default_cfg):
    """(On the commit before KRCNN.NMS_OKS worked this raised NotImplementedError.)"""
    from detectandtrack_amd.core import test as engine
    cfg = default_cfg
    cfg.MODEL.NUM_CLASSES, cfg.KRCNN.NUM_KEYPOINTS = 2, K
    maps, boxes, dets, want = _box_case()
    cls_boxes = [[], dets.copy()]
    plain = engine.keypoint_results(cls_boxes, maps, boxes)
    assert len(plain[1]) == 4 and np.array_equal(cls_boxes[1], dets)
    cfg.KRCNN.NMS_OKS = True
    got = engine.keypoint_results(cls_boxes, maps, boxes)
    assert len(got[1]) == len(want) and len(cls_boxes[1]) == len(want)
    assert np.array_equal(cls_boxes[1], dets[want])
    for row, i in zip(got[1], want):
        assert np.array_equal(row, plain[1][i])
    # the threshold is the key HIP.NMS_OKS_THRESH: above every similarity nothing is removed, and the rows come in score order
    cfg.HIP.NMS_OKS_THRESH = 1.5
    cls_boxes = [[], dets.copy()]
    got = engine.keypoint_results(cls_boxes, maps, boxes)
    assert np.array_equal(cls_boxes[1], dets[[2, 1, 3, 0]]) and len(got[1]) == 4


def test_tubes_need_the_opt_in_switch(default_cfg):
    from detectandtrack_amd.core import test as engine
    cfg = default_cfg
    cfg.MODEL.NUM_CLASSES, cfg.KRCNN.NUM_KEYPOINTS = 2, K
    cfg.KRCNN.NMS_OKS = True
    maps, boxes, dets, _ = _box_case()
    maps2, boxes2 = np.concatenate([maps, maps], axis=1), np.hstack([boxes, boxes])
    dets2 = np.hstack([boxes2, dets[:, 4:]])
    assert not cfg.HIP.TUBE_NMS_OKS
    with pytest.raises(NotImplementedError, match='Handle tubes'):
        engine.keypoint_results([[], dets2.copy()], maps2, boxes2)
    cfg.HIP.TUBE_NMS_OKS = True
    cls_boxes = [[], dets2.copy()]
    got = engine.keypoint_results(cls_boxes, maps2, boxes2)
    assert np.array_equal(cls_boxes[1], dets2[[2, 1, 3]]) and len(got[1]) == 3 and got[1][0].shape == (4, 2 * K)


def test_more_than_one_foreground_class_is_refused(default_cfg):
    from detectandtrack_amd.core import test as engine
    cfg = default_cfg
    cfg.KRCNN.NMS_OKS = True
    cfg.MODEL.NUM_CLASSES, cfg.KRCNN.NUM_KEYPOINTS = 3, K
    maps, boxes, dets, _ = _box_case()
    with pytest.raises(ValueError, match='NUM_CLASSES'):
        engine.keypoint_results([[], dets.copy(), dets[:0].copy()], maps, boxes)
    cfg.MODEL.NUM_CLASSES = 2
    cfg.KRCNN.NUM_KEYPOINTS = 16
    with pytest.raises(ValueError, match='NUM_KEYPOINTS'):
        engine.keypoint_results([[], dets.copy()], maps[:, :16], boxes)


# ---- wiring and C ABI -----------------------------------------------------------------------------------------------------------------------
def test_device_path_admits_the_switch_where_the_kernel_covers_it(default_cfg):
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.config import cfg_from_file, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.ops import hip_ops as ops
    cfg = default_cfg
    cfg_from_file(os.path.join(REPO, 'configs', 'test_r18_fpn3d_oks_synthetic.yaml'))
    assert_and_infer_cfg()
    assert cfg.KRCNN.NMS_OKS and cfg.HIP.NMS_OKS_THRESH == 0.3 and engine.device_results_supported()
    cfg.MODEL.NUM_CLASSES = 3                   # the host path raises for it
    assert not engine.device_results_supported()
    cfg.MODEL.NUM_CLASSES = 2
    cfg.TEST.DETECTIONS_PER_IM = ops.OKS_NMS_MAX_ROWS       # + the spare rows: more than the kernel holds -> the host loop
    assert not engine.device_results_supported()
    cfg.TEST.DETECTIONS_PER_IM = 100
    assert engine.device_results_supported() and engine.rerun_rows_supported(ops.OKS_NMS_MAX_ROWS)
    assert not engine.rerun_rows_supported(ops.OKS_NMS_MAX_ROWS + 1)
    reset_cfg()
    cfg_from_file(os.path.join(REPO, 'configs', 'test_r18_c4_tube_oks_synthetic.yaml'))
    assert_and_infer_cfg()
    assert cfg.KRCNN.NMS_OKS and cfg.HIP.TUBE_NMS_OKS and engine.device_results_supported()
    cfg.HIP.TUBE_NMS_OKS = False
    assert not engine.device_results_supported()
    cfg.KRCNN.NMS_OKS = False
    assert engine.device_results_supported() and engine.rerun_rows_supported(10 ** 6)


def test_defaults_leave_the_switch_off(default_cfg):
    cfg = default_cfg
    assert cfg.KRCNN.NMS_OKS is False and cfg.HIP.TUBE_NMS_OKS is False and cfg.HIP.NMS_OKS_THRESH == 0.3


@pytest.mark.parametrize('lib', ['libdat_hip.so', 'libdat_hip_f16.so'])
def test_both_library_flavours_export_the_entry_points(lib):
    h = ctypes.CDLL(os.path.join(REPO, 'detectandtrack_amd', lib))
    for name in NEW_SYMBOLS:
        assert hasattr(h, name), '%s does not export %s' % (lib, name)
    from detectandtrack_amd import libdat
    from detectandtrack_amd.ops import hip_ops as ops
    assert set(NEW_SYMBOLS) <= set(libdat.EXPORTS)
    with open(os.path.join(REPO, 'include', 'dat_hip.h')) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert 'int %s(' % name in header
    assert '#define DAT_OKS_NMS_MAX_ROWS %d\n' % ops.OKS_NMS_MAX_ROWS in header
