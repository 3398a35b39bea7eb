"""CPU tests of the host side: C-ABI exports, product/oracle separation, config, builders, tracker, sharding."""
import ast
import glob
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_library_exports_every_declared_symbol():
    """libdat_hip.so loads (no GPU needed) and exports every function include/dat_hip.h declares."""
    import ctypes
    hdr = open(os.path.join(REPO, 'include', 'dat_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = sorted(set(re.findall(r'\b(dat_[a-z0-9_]+|_nms)\s*\(', hdr)))   # `_nms`: the reference's own C symbol (gpu_nms.hpp:3-9)
    assert '_nms' in declared
    assert len(declared) >= 25
    lib = ctypes.CDLL(os.path.join(REPO, 'detectandtrack_amd', 'libdat_hip.so'))
    missing = [n for n in declared if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.dat_version() >= 1 and lib.dat_h16_format() == 0
    # the IEEE-half flavour of the same sources (cfg.HIP.DTYPE 'fp16'): the same exports, the other 16-bit format
    lib16 = ctypes.CDLL(os.path.join(REPO, 'detectandtrack_amd', 'libdat_hip_f16.so'))
    assert not [n for n in declared if not hasattr(lib16, n)]
    assert lib16.dat_version() == lib.dat_version() and lib16.dat_h16_format() == 1
    from detectandtrack_amd import libdat
    assert sorted(libdat.EXPORTS) == declared, set(declared) ^ set(libdat.EXPORTS)


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: no module of the product package, tools/ or bench's hot path imports it
    (bench.py may use it ONLY inside its cpu_* baseline legs)."""
    offenders = []
    for path in glob.glob(os.path.join(REPO, 'detectandtrack_amd', '**', '*.py'), recursive=True) + \
            glob.glob(os.path.join(REPO, 'tools', '*.py')):
        tree = ast.parse(open(path).read())
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom) and node.module:
                names = [node.module]
            if any(n == 'oracle' or n.startswith('oracle.') for n in names):
                offenders.append(path)
    assert not offenders, offenders
    src = open(os.path.join(REPO, 'bench.py')).read()
    tree = ast.parse(src)
    for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
        uses = any(isinstance(n, ast.ImportFrom) and n.module and n.module.startswith('oracle') for n in ast.walk(fn))
        assert (not uses) or fn.name.startswith('cpu_'), fn.name      # the CPU-baseline legs: cpu_baseline, cpu_proposal_path, ...


def test_ops_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from detectandtrack_amd import libdat
    with pytest.raises(libdat.DatError):
        libdat.Ctx(0)


# ---- config ----------------------------------------------------------------------------------------------------------------
def test_cfg_defaults_and_merge(tmp_path):
    from detectandtrack_amd.core.config import cfg, cfg_from_file, cfg_from_list, assert_and_infer_cfg, reset_cfg
    reset_cfg()
    assert cfg.TEST.NMS == 0.3 and cfg.RPN.SIZES == (64, 128, 256, 512) and cfg.RNG_SEED == 3
    assert abs(cfg.BBOX_XFORM_CLIP - np.log(1000. / 16.)) < 1e-12
    y = tmp_path / 'c.yaml'
    y.write_text('MODEL:\n  TYPE: keypoint_rcnn\n  FASTER_RCNN: True\nVIDEO:\n  NUM_FRAMES: 3\n  TIME_KERNEL_DIM: 3\n'
                 'TEST:\n  SCALES: (256,)\n  NMS: 0.5\n')
    cfg_from_file(str(y))
    cfg_from_list(['TEST.MAX_SIZE', '333', 'NUM_GPUS', '1'])
    assert_and_infer_cfg()
    assert cfg.VIDEO.TIME_KERNEL_DIM.BODY == 3 and cfg.VIDEO.TIME_KERNEL_DIM.HEAD_KPS == 3   # config.py:839-850
    assert cfg.VIDEO.NUM_FRAMES_MID == 3 and cfg.RPN.ON and cfg.TEST.SCALES == (256,) and cfg.TEST.MAX_SIZE == 333
    with pytest.raises(KeyError):
        from detectandtrack_amd.core.config import cfg_from_cfg
        cfg_from_cfg({'NOT_A_KEY': 1})
    with pytest.raises(ValueError):
        from detectandtrack_amd.core.config import cfg_from_cfg
        cfg_from_cfg({'TEST': {'NMS': 'high'}})
    reset_cfg()


REF_CONFIGS = os.path.join(REPO, 'tests', 'golden', 'reference_configs')     # the reference's shipped yaml files (make_golden.py golden_cfg_files)


def test_every_shipped_reference_yaml_loads():
    from detectandtrack_amd.core.config import cfg, cfg_from_file, assert_and_infer_cfg, reset_cfg
    files = sorted(glob.glob(os.path.join(REF_CONFIGS, 'video', '*', '*.yaml')))
    assert len(files) == 12
    for f in files:
        reset_cfg()
        cfg_from_file(f)
        assert_and_infer_cfg()
        assert cfg.MODEL.TYPE == 'keypoint_rcnn'
    reset_cfg()


# ---- builders ----------------------------------------------------------------------------------------------------------------
def _build(cfg_dict):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    reset_cfg()
    cfg_from_cfg(cfg_dict)
    assert_and_infer_cfg()
    return model_builder.create(cfg.MODEL.TYPE, train=False)


def test_builder_r18_fpn3d_graph_and_params():
    from tests.model_util import fpn3d_kps_cfg
    m = _build(fpn3d_kps_cfg('18', T=8))
    convs = [op for op in m.net.ops if op.type == 'Conv']
    body_fpn = [op for op in m.conv_body_net.ops if op.type == 'Conv']
    assert len(body_fpn) == 28          # 1 stem + 16 block convs + 3 shortcuts + 4 laterals + 4 post-hoc
    # every AffineChannelNd / Relu / Sum is folded into a conv epilogue
    assert not [op for op in m.net.ops if op.type in ('AffineChannel', 'Relu', 'Sum', 'UpsampleNearest2x')]
    lat = [op for op in body_fpn if op.outputs[0] == 'fpn_inner_res4_1_sum'][0]
    assert lat.args['res_mode'] == 2 and lat.args['residual'] == 'fpn_inner_res5_1_sum'
    blk = [op for op in body_fpn if op.outputs[0] == 'res3_1_sum'][0]
    assert blk.args['relu'] and blk.args['res_mode'] == 1 and blk.args['kernels'] == [3, 3, 3]
    # reference parameter names / shapes
    ps = m.param_specs
    assert ps['conv1_w']['shape'] == (64, 3, 1, 7, 7) and ps['res_conv1_bn_s']['shape'] == (64,)
    assert ps['res2_0_branch2a_w']['shape'] == (64, 64, 1, 3, 3)          # kT = 1 in res2 (ResNet3D.py:270-272)
    assert ps['res3_0_branch2a_w']['shape'] == (128, 64, 3, 3, 3)
    assert ps['res3_0_branch1_w']['shape'] == (128, 64, 1, 1, 1)
    assert ps['fpn_inner_res4_1_sum_lateral_w']['shape'] == (256, 256, 1, 1, 1)
    assert ps['fpn_res2_1_sum_w']['shape'] == (256, 256, 3, 3, 3)
    assert ps['conv_rpn_fpn2_w']['shape'] == (256, 256, 3, 3) and 'conv_rpn_fpn3_w' not in ps   # shared (FPN.py:246)
    assert ps['fc6_w']['shape'] == (1024, 256 * 49) and ps['kps_score_lowres_w']['shape'] == (512, 17, 4, 4)
    assert [op.type for op in m.keypoint_net.ops] == ['RoIFeatureTransform'] + ['Conv'] * 8 + ['ConvTranspose', 'BilinearInterpolation']
    # frozen: affine params and the bilinear kernel never train (detector.py:57-65, 378-379)
    tr = m.TrainableParams()
    assert 'res2_0_branch2a_bn_s' not in tr and 'kps_score_w' not in tr and 'conv1_w' in tr
    from detectandtrack_amd.core.config import reset_cfg
    reset_cfg()


def test_builder_r50_and_c4_tube_graphs():
    from tests.model_util import fpn3d_kps_cfg
    m = _build(fpn3d_kps_cfg('50', T=4))
    ps = m.param_specs
    assert ps['res2_0_branch2a_w']['shape'] == (64, 64, 1, 1, 1) and ps['res3_0_branch2b_w']['shape'] == (128, 128, 3, 3, 3)
    assert ps['res5_2_branch2c_w']['shape'] == (2048, 512, 1, 1, 1)
    assert len([op for op in m.conv_body_net.ops if op.type == 'Conv']) == 1 + 16 * 3 + 4 + 4 + 4
    # shipped 3D config: C4 body + res5 tube head + 3D keypoint head (configs/video/3d/04_*.yaml)
    c4 = {'MODEL': {'TYPE': 'keypoint_rcnn', 'CONV_BODY': 'ResNet3D.add_ResNet18_conv4_body',
                    'ROI_HEAD': 'ResNet3D.add_ResNet18_roi_conv5_head', 'NUM_CLASSES': 2, 'FASTER_RCNN': True,
                    'KEYPOINTS_ON': True, 'VIDEO_ON': True},
          'FAST_RCNN': {'ROI_XFORM_METHOD': 'RoIAlign', 'ROI_XFORM_RESOLUTION': 7, 'ROI_XFORM_SAMPLING_RATIO': 2},
          'KRCNN': {'ROI_KEYPOINTS_HEAD': 'keypoint_rcnn_heads.add_roi_pose_head_v1convX_3d', 'NUM_STACKED_CONVS': 8,
                    'NUM_KEYPOINTS': 17, 'USE_DECONV_OUTPUT': True, 'CONV_INIT': 'MSRAFill', 'CONV_HEAD_DIM': 512,
                    'UP_SCALE': 2, 'HEATMAP_SIZE': 56, 'ROI_XFORM_METHOD': 'RoIAlign', 'ROI_XFORM_RESOLUTION': 14,
                    'ROI_XFORM_SAMPLING_RATIO': 2, 'NO_3D_DECONV_TIME_TO_CH': True},
          'VIDEO': {'NUM_FRAMES': 3, 'TIME_KERNEL_DIM': 3, 'BODY_HEAD_LINK': '', 'WEIGHTS_INFLATE_MODE': 'center-only'}}
    m = _build(c4)
    ps = m.param_specs
    assert ps['conv_rpn_w']['shape'] == (256, 256, 3, 3, 3) and ps['rpn_cls_logits_1_w']['shape'] == (12, 256, 1, 1, 1)
    assert ps['res5_0_branch2a_w']['shape'] == (512, 256, 1, 3, 3)      # res5 head is kT = 1 (ResNet3D.py:314-316)
    assert ps['conv_fcn1_w']['shape'] == (512, 256, 3, 3, 3)
    gp = [op for op in m.net.ops if op.type == 'GenerateProposals'][0]
    assert gp.args['anchors'].shape == (12, 12)                          # A = 12 tube anchors x 4*T
    from detectandtrack_amd.core.config import reset_cfg
    reset_cfg()


def test_product_anchors_boxes_match_reference_golden(golden):
    from detectandtrack_amd.core.config import reset_cfg
    from detectandtrack_amd.modeling.generate_anchors import generate_anchors
    import detectandtrack_amd.utils.boxes as bu
    reset_cfg()
    np.testing.assert_array_equal(generate_anchors(16., (64, 128, 256, 512), (0.5, 1, 2), time_dim=3), golden['anchors_c4_T3'])
    for lvl in range(2, 7):
        np.testing.assert_array_equal(generate_anchors(2. ** lvl, (32 * 2. ** (lvl - 2),), (0.5, 1, 2)), golden['anchors_fpn%d' % lvl])
    np.testing.assert_array_equal(bu.bbox_transform(golden['bt_boxes'].astype(np.float64), golden['bt_deltas'], (10., 10., 5., 5.)),
                                  golden['bt_out_w10'])
    tt = bu.bbox_transform(golden['tt_boxes'].astype(np.float64), golden['tt_deltas'], (10., 10., 5., 5.))
    np.testing.assert_array_equal(tt, golden['tt_out'])
    np.testing.assert_array_equal(bu.clip_tiled_boxes(tt.copy(), (256, 320)), golden['clip_out'])
    np.testing.assert_array_equal(bu.bbox_transform_inv(golden['bt_boxes'], golden['inv_gt'], (10., 10., 5., 5.)), golden['inv_out'])
    np.testing.assert_array_equal(bu.bbox_overlaps(golden['iou_a'], golden['iou_b']), golden['iou_out'])
    np.testing.assert_array_equal(bu.bbox_overlaps(golden['iou_ta'], golden['iou_tb']), golden['iou_tube_out'])
    import detectandtrack_amd.modeling.FPN as fpn
    np.testing.assert_array_equal(fpn.map_rois_to_fpn_levels(golden['lvl_rois'][:, 1:], 2, 5), golden['lvl_out'])


def test_weight_inflation_matches_reference(golden):
    from detectandtrack_amd.utils.net import inflate_weights
    src = golden['inflate_src']
    tgt = np.zeros((8, 4, 3, 3, 3), np.float32)
    for mode in ('mean-repeat', 'repeat', 'center-only'):
        np.testing.assert_array_equal(inflate_weights(src, tgt, 'x_w', mode), golden['inflate_' + mode.replace('-', '_')])


def test_weights_file_roundtrip(tmp_path):
    from tests.model_util import fpn3d_kps_cfg
    from detectandtrack_amd.utils import net as nu
    m = _build(fpn3d_kps_cfg('18', T=2))

    class WS(object):
        def __init__(self):
            self.params = {}

        def set_param(self, k, v):
            self.params[k] = np.asarray(v, np.float32)
    ws = WS()
    nu.initialize_params(m, ws, seed=1)
    assert set(ws.params) == set(m.params)
    assert ws.params['res2_0_branch2a_bn_s'].min() == 1.0 and abs(ws.params['rpn_cls_logits_fpn2_w'].std() - 0.01) < 2e-3
    f = str(tmp_path / 'w.pkl')
    nu.save_model_to_weights_file(f, m, ws)
    ws2 = WS()
    nu.initialize_params(m, ws2, seed=2)
    nu.initialize_from_weights_file(m, ws2, f)
    for k in m.params:
        np.testing.assert_array_equal(ws.params[k], ws2.params[k])
    # 2D checkpoint -> 3D model: conv weights inflate centre-only (VIDEO.WEIGHTS_INFLATE_MODE)
    import pickle
    blobs = {k: (v[:, :, 1] if v.ndim == 5 and v.shape[2] == 3 else v) for k, v in ws.params.items()}
    with open(f, 'wb') as fh:
        pickle.dump({'blobs': blobs}, fh, protocol=2)
    ws3 = WS()
    nu.initialize_params(m, ws3, seed=2)
    nu.initialize_from_weights_file(m, ws3, f)
    w = ws3.params['res3_0_branch2a_w']
    assert w.shape[2] == 3 and np.all(w[:, :, 0] == 0) and np.all(w[:, :, 2] == 0)
    np.testing.assert_array_equal(w[:, :, 1], ws.params['res3_0_branch2a_w'][:, :, 1])
    from detectandtrack_amd.core.config import reset_cfg
    reset_cfg()


def test_backbone_only_weights_file_overlays_an_initialised_workspace(tmp_path):
    """Fine-tuning from an ImageNet-style file (reference train_net.py:100-118, utils/net.py:164-249): parameters absent from the
    file (fpn_*, rpn_*, heads) keep their init, 2D convs inflate, blobs that cannot be inflated (class-count mismatch) keep their
    init instead of turning into zeros; `<param>_momentum` blobs round-trip."""
    import pickle
    from tests.model_util import fpn3d_kps_cfg
    from detectandtrack_amd.utils import net as nu
    from detectandtrack_amd.core.config import reset_cfg
    m = _build(fpn3d_kps_cfg('18', T=2))

    class WS(object):
        def __init__(self):
            self.params = {}

        def set_param(self, k, v):
            self.params[k] = np.asarray(v, np.float32)
    full = WS()
    nu.initialize_params(m, full, seed=5)
    body = {k: (v[:, :, 1] if v.ndim == 5 and v.shape[2] == 3 else v) for k, v in full.params.items()
            if k.startswith(('conv1', 'res'))}
    body['cls_score_w'] = np.ones((81, 1024), np.float32)          # COCO class count: not inflatable to 2 classes
    body['conv1_w_momentum'] = np.full(full.params['conv1_w'].shape, 0.25, np.float32)
    f = str(tmp_path / 'imagenet.pkl')
    with open(f, 'wb') as fh:
        pickle.dump({'blobs': body}, fh, protocol=2)
    ws = WS()                                                      # blank workspace: the loader must initialise it itself
    mom = {}
    kept = nu.initialize_from_weights_file(m, ws, f, momentum=mom)
    assert set(ws.params) == set(m.params)
    assert 'fpn_inner_res5_1_sum_w' in kept and 'cls_score_w' in kept and 'conv1_w' not in kept
    assert ws.params['cls_score_w'].shape == (2, 1024) and abs(ws.params['cls_score_w'].std() - 0.01) < 3e-3   # Gaussian init kept
    assert ws.params['rpn_cls_logits_fpn2_w'].std() > 0
    w = ws.params['res3_0_branch2a_w']
    assert np.all(w[:, :, 0] == 0) and np.array_equal(w[:, :, 1], full.params['res3_0_branch2a_w'][:, :, 1])
    np.testing.assert_array_equal(mom['conv1_w'], body['conv1_w_momentum'])
    out = str(tmp_path / 'snap.pkl')
    nu.save_model_to_weights_file(out, m, ws, {'conv1_w': mom['conv1_w']})
    assert 'conv1_w_momentum' in nu.load_weights_file(out)
    reset_cfg()


# ---- host utils ----------------------------------------------------------------------------------------------------------------
def test_image_resize_and_blob_prep():
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import image as iu, blob as bu
    reset_cfg()
    im = np.arange(12, dtype=np.float32).reshape(3, 4)
    np.testing.assert_allclose(iu.resize_bilinear(im, 4, 3), im)
    np.testing.assert_allclose(iu.resize_bicubic(im, 4, 3), im, atol=1e-6)
    up = iu.resize_bilinear(im, 8, 6)
    assert up.shape == (6, 8) and abs(up.mean() - im.mean()) < 1e-4
    const = iu.resize_bicubic(np.full((5, 7, 2), 3.0, np.float32), 11, 9)
    np.testing.assert_allclose(const, 3.0, atol=1e-5)
    # S-B of SURVEY.md §8: 720x1280 @ scale 800 / max 1333 -> 750x1333 -> pad32 -> 768x1344
    cfg.FPN.FPN_ON = True
    cfg.MODEL.VIDEO_ON = True
    cfg.VIDEO.NUM_FRAMES = 2
    ims, sc = bu.prep_im_for_blob(np.zeros((720, 1280, 3), np.uint8), cfg.PIXEL_MEANS, (800,), 1333)
    assert ims[0].shape == (750, 1333, 3) and abs(sc[0] - 1333. / 1280.) < 1e-9
    blob = bu.im_list_to_blob([ims[0], ims[0]])
    assert blob.shape == (1, 3, 2, 768, 1344)
    reset_cfg()


def test_host_resamplers_and_keypoint_decode_match_the_cv2_oracle():
    """The product's host cv2.resize stand-ins (utils/image.py) and heatmaps_to_keypoints (utils/keypoints.py) against the independent
    restatement of OpenCV's algorithm in oracle/resize.py -- bit-identical images (same float32 operation order), identical
    keypoint rows; the prep_im_for_blob path uses the GIVEN scale for the sampling step (blob.py:86-87)."""
    from oracle import resize as R
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import image as iu, blob as bu, keypoints as ku
    reset_cfg()
    rs = np.random.RandomState(4)
    for (h, w, c), (ow, oh) in (((56, 56, 17), (43, 91)), ((56, 56, 3), (200, 17)), ((9, 13, 1), (13, 9)), ((20, 31, 2), (7, 5)),
                                ((4, 4, 1), (1, 1)), ((3, 5, 2), (64, 48))):
        im = (rs.randn(h, w, c) * 3).astype(np.float32)
        np.testing.assert_array_equal(iu.resize_bicubic(im, ow, oh), R.resize_cubic(im, dsize=(ow, oh)))
        np.testing.assert_array_equal(iu.resize_bilinear(im, ow, oh), R.resize_linear(im, dsize=(ow, oh)))
    im = rs.uniform(-120, 140, (72, 128, 3)).astype(np.float32)
    for s in (1333.0 / 1280.0, 800.0 / 600.0, 0.37):
        np.testing.assert_array_equal(iu.resize_bilinear(im, fx=s, fy=s), R.resize_linear(im, fx=s, fy=s))
    frame = rs.randint(0, 255, (72, 128, 3)).astype(np.uint8)
    ims, sc = bu.prep_im_for_blob(frame, cfg.PIXEL_MEANS, (80,), 133)
    ref = R.resize_linear(frame.astype(np.float32) - cfg.PIXEL_MEANS, fx=sc[0], fy=sc[0])
    np.testing.assert_array_equal(ims[0], ref)
    # heatmap decoding (lib/utils/keypoints.py:94-149)
    maps = (rs.randn(6, 17, 56, 56) * 2).astype(np.float32)
    xy = rs.uniform(0, 200, (6, 2)).astype(np.float32)
    rois = np.hstack((xy, xy + rs.uniform(0.4, 150, (6, 2)).astype(np.float32)))
    cfg.KRCNN.NUM_KEYPOINTS = 17
    for ms in (0, 40):
        cfg.KRCNN.INFERENCE_MIN_SIZE = ms
        np.testing.assert_array_equal(ku.heatmaps_to_keypoints(maps, rois), R.heatmaps_to_keypoints(maps, rois, ms))
    reset_cfg()


def test_soft_nms_and_box_voting_match_the_real_reference():
    """core/nms_wrapper.soft_nms (dat_soft_nms_host: the loop of lib/utils/cython_nms.pyx:98-203 in C float) and utils/boxes.box_voting
    (lib/utils/boxes.py:294-310) against outputs of the REAL reference (its Cython compiled into oracle/_ref, its boxes.py run under
    py3 shims; tests/golden/reference_postproc.npz): bit-identical re-scored boxes, order and indices."""
    from detectandtrack_amd.core import nms_wrapper
    from detectandtrack_amd.utils import boxes as bu
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'reference_postproc.npz'))
    dets = g['soft_dets']
    for method in ('hard', 'linear', 'gaussian'):
        d, inds = nms_wrapper.soft_nms(dets, sigma=0.5, overlap_thresh=0.3, score_thresh=0.001, method=method)
        np.testing.assert_array_equal(inds, g['soft_%s_inds' % method])
        np.testing.assert_array_equal(d, g['soft_%s_dets' % method])
    assert 0 < len(g['soft_linear_inds']) <= len(dets)
    np.testing.assert_allclose(bu.box_voting(g['vote_top'], dets, 0.8), g['vote_out'], rtol=0, atol=1e-4)
    with pytest.raises(ValueError):
        nms_wrapper.nms(dets, 0.5, soft_nms=True)
    d0, i0 = nms_wrapper.soft_nms(np.zeros((0, 5), np.float32))
    assert d0.shape == (0, 5) and i0.shape == (0,)


def test_tracker_hungarian_greedy_and_ids():
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.core import tracking_engine as te
    reset_cfg()
    C = np.array([[0.1, 0.9, 0.8], [0.2, 0.15, 0.7]])
    m = te._compute_matches(None, None, None, None, 'hungarian', C=C)
    assert m.tolist() == [0, 1, -1]
    m = te._compute_matches(None, None, None, None, 'greedy', C=C)
    assert m.tolist() == [0, 1, -1]
    # two people crossing: identities follow overlap
    b0 = np.array([[0, 0, 50, 100, 0.99], [200, 0, 250, 100, 0.98]], np.float32)
    b1 = np.array([[205, 0, 255, 100, 0.97], [5, 0, 55, 100, 0.99], [400, 0, 450, 100, 0.96]], np.float32)
    json_data = [{'image': 'v/a/%d.jpg' % i, 'height': 200, 'width': 500} for i in range(2)]
    dets = {'all_boxes': [[], [b0, b1]], 'all_keyps': [[], [[np.zeros((4, 17))] * 2, [np.zeros((4, 17))] * 3]]}
    cfg.TRACKING.DISTANCE_METRIC_WTS = (1.0, 0.0, 0.0)
    out = te.compute_matches_tracks(json_data, dets)
    assert out['all_tracks'][1] == [[0, 1], [1, 0, 2]]
    # centre-frame selection + pruning (tracking_engine.py:731-755)
    tube = np.array([[0, 0, 10, 10, 20, 20, 60, 60, 40, 40, 50, 50, 0.99], [0, 0, 1, 1, 0, 0, 2, 2, 0, 0, 1, 1, 0.99]], np.float32)
    d = {'all_boxes': [[], [tube]], 'all_keyps': [[], [[np.zeros((4, 51)), np.zeros((4, 51))]]]}
    cfg.KRCNN.NUM_KEYPOINTS = 17
    te._center_detections(d)
    assert d['all_boxes'][1][0].tolist()[0] == [20, 20, 60, 60, np.float32(0.99)] and d['all_keyps'][1][0][0].shape == (4, 17)
    te._prune_bad_detections(d, [{'height': 100, 'width': 100}], 0.95)
    assert d['all_boxes'][1][0].shape == (1, 5)
    reset_cfg()


def test_shard_range_matches_array_split():
    from detectandtrack_amd.utils.dist import shard_range
    for n in (0, 1, 7, 50, 101):
        for w in (1, 2, 3, 8):
            parts = np.array_split(np.arange(n), w)
            for r in range(w):
                s, e = shard_range(n, w, r)
                assert list(range(s, e)) == parts[r].tolist()


def _gloo_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    from detectandtrack_amd.utils import dist as du
    from detectandtrack_amd.core.test_engine import merge_range_results
    dist = du.init_process_group('gloo')
    s, e = du.shard_range(11, world, rank)
    local = {'all_boxes': [[], [np.full((1, 5), i, np.float32) for i in range(s, e)]], 'all_keyps': [[], [[] for _ in range(s, e)]]}
    parts = du.gather_in_range_order([local], dist)
    t = du.max_over_ranks(1.0 + rank, dist)
    dist.barrier()
    if rank == 0:
        merged = merge_range_results(parts)
        q.put(([int(b[0, 0]) for b in merged['all_boxes'][1]], t))
    dist.destroy_process_group()


def test_multi_gpu_sharding_protocol_gloo_world2():
    """N>1 path on CPU (gloo, world_size 2): contiguous clip ranges, range-order merge on rank 0, MAX timing."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    order, tmax = q.get(timeout=120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert order == list(range(11)) and tmax == 2.0


def _allreduce_worker(rank, world, port, q):
    import os
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from detectandtrack_amd.training import GradExchange
    per = 4096 // 4                # force several buckets
    g = torch.Generator().manual_seed(100 + rank)
    # the Trainer's flat gradient buffer with per-parameter views into it (training.py): reduced in bucket-sized slices, in place
    sizes = (7, 300, 1500, 64, 2000, 5)
    flat_g = torch.randn(sum(sizes), generator=g)
    tensors, off = [], 0
    for n in sizes:
        tensors.append(flat_g[off:off + n])
        off += n
    local = [x.clone() for x in tensors]
    n = flat_g.numel()
    GradExchange(flat_g, [(off, min(off + per, n)) for off in range(0, n, per)], dist, overlap=False).finish()
    q.put((rank, [x.numpy() for x in local], [x.numpy() for x in tensors]))
    dist.destroy_process_group()


def test_gradient_allreduce_buckets_gloo_world2():
    """The training exchange step (model_builder.py:932-942): bucketed sum all-reduce over 2 ranks on the gloo backend."""
    import multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_allreduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs])
    for p in procs:
        p.join(timeout=60)
    (_, l0, r0), (_, l1, r1) = res
    for a, b, x, y in zip(l0, l1, r0, r1):
        np.testing.assert_allclose(x, a + b, rtol=1e-6)
        np.testing.assert_allclose(y, a + b, rtol=1e-6)


def _exchange_worker(rank, world, port, q):
    import os
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from detectandtrack_amd.training import GradExchange
    g = torch.Generator().manual_seed(500 + rank)
    n = 5000
    buckets = [(0, 1800), (1800, 1800), (1800, 4100), (4100, 5000)]      # (one empty bucket)
    final = torch.randn(n, generator=g)               # what this rank's backward will have produced at the end
    results = {}
    for mode in ('serial', 'overlap'):
        flat = torch.full((n,), float('nan'))         # a gradient is garbage until its producer has run
        x = GradExchange(flat, buckets, dist, overlap=(mode == 'overlap'))
        x.begin()
        for k, (lo, hi) in enumerate(buckets):        # the backward pass: bucket k becomes final, is handed over, the pass continues
            flat[lo:hi] = final[lo:hi]
            x.ready(k)
        x.finish()
        results[mode] = (flat.clone().numpy(), list(x.order))
    q.put((rank, final.numpy(), results))
    dist.destroy_process_group()


def test_overlapped_bucket_exchange_equals_the_serial_one_gloo_world2():
    """gradient buckets all-reduced AS THEY BECOME FINAL (GradExchange.ready(k) from the backward pass, collectives
    in flight while later buckets are still being written) give exactly the serial result -- the sum over the ranks of every
    element -- and start in completion order; overlap=False starts nothing before finish()."""
    import multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + ((os.getpid() + 17) % 1000)
    procs = [ctx.Process(target=_exchange_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, f0, r0), (_, f1, r1) = res
    for r in (r0, r1):
        for mode in ('serial', 'overlap'):
            got, order = r[mode]
            np.testing.assert_array_equal(got, f0 + f1)        # (two addends: the sum is order-independent, bit for bit)
            assert order == [0, 1, 2, 3]
    np.testing.assert_array_equal(r0['overlap'][0], r0['serial'][0])


def test_gradient_completion_order_of_the_training_graph():
    """The static rule the overlapped exchange rests on (training.param_ready_index): a parameter's gradient is final once the op
    with the SMALLEST index that uses it has been differentiated (the backward pass runs the op list from the end).  On the
    R-18 FPN3D training graph: the heads complete before the FPN, the FPN before res5 ... res3; the RPN conv shared by the five FPN
    levels completes with its FIRST use; both fused RPN head convs complete at the fused launch's index; frozen parameters
    (conv1 / res2, below StopGradient) are not trainable at all."""
    from detectandtrack_amd.core.config import cfg, cfg_from_file, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.training import param_ready_index
    from detectandtrack_amd.workspace import Executor
    reset_cfg()
    cfg_from_file(os.path.join(REPO, 'configs', 'train_r18_fpn3d_synthetic.yaml'))
    assert_and_infer_cfg()
    m = model_builder.create(cfg.MODEL.TYPE, train=True)
    ex = Executor.__new__(Executor)
    ex.net = m.net
    ex._plan_rpn_siblings()
    assert ex._fused, 'the RPN logits / deltas convs of every level are fused'
    idx = param_ready_index(m.net, ex._fused)
    train = list(m.TrainableParams())
    assert all(n in idx for n in train), [n for n in train if n not in idx]
    # conv1 / res2 sit below StopGradient: the model lists them as trainable, they are final at once (and the Trainer, which reads
    # this index, keeps them out of its update: tests/test_gpu_trainer_state.py)
    frozen = [n for n in train if n.startswith(('conv1', 'res2'))]
    assert frozen and all(idx[n] == len(m.net.ops) for n in frozen)
    uses = {}
    for i, op in enumerate(m.net.ops):
        for key in ('w', 'b'):
            n = op.args.get(key) if isinstance(op.args, dict) else None
            if isinstance(n, str) and n:
                uses.setdefault(n, []).append(i)
    for n in train:
        assert n in frozen or idx[n] <= min(uses[n]), n   # never later than the first use
    shared = [n for n in train if len(uses[n]) > 1]
    assert shared and all(idx[n] == min(uses[n]) or n.startswith('rpn_') for n in shared)
    for first, (lo, do, _gi) in ex._fused.items():
        for op in (lo, do):
            assert idx[op.args['w']] <= first and idx[op.args['b']] <= first
    # heads -> FPN -> res5 -> res4 -> res3 in completion (= backward) order
    def done(prefix):
        return max(idx[n] for n in train if n.startswith(prefix))
    def last_done(prefix):
        return min(idx[n] for n in train if n.startswith(prefix))
    assert last_done('kps_score') > done('fpn_') or last_done('conv_fcn') > done('fpn_')
    assert last_done('fc') > done('fpn_inner')
    assert last_done('res5') > done('res4') > 0 and last_done('res4') > done('res3')
    reset_cfg()


def test_roi_data_matches_the_real_reference_golden():
    """detectandtrack_amd/roi_data (host label generation for training) against vectors produced by the REAL reference
    lib/roi_data + json_dataset + utils/keypoints under py3 shims (tests/golden/make_golden.py:golden_roi_data): same seeded
    numpy.random stream, so labels / sampled rois / keypoint cells must be identical."""
    import numpy.random as npr
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.roi_data import rpn, fast_rcnn
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'reference_roi_data.npz'))
    reset_cfg()
    cfg.FPN.FPN_ON = cfg.FPN.MULTILEVEL_RPN = cfg.FPN.MULTILEVEL_ROIS = True
    cfg.MODEL.KEYPOINTS_ON = True
    cfg.MODEL.NUM_CLASSES = 2
    cfg.KRCNN.NUM_KEYPOINTS, cfg.KRCNN.HEATMAP_SIZE = 17, 56
    cfg.TRAIN.MAX_SIZE, cfg.TRAIN.BATCH_SIZE_PER_IM = 333, 64
    H, W = [int(v) for v in g['rd_hw']]
    boxes, kps, props = g['rd_boxes'], g['rd_kps'], g['rd_props']
    n = boxes.shape[0]
    foas = rpn.fpn_fields(1)
    npr.seed(77)
    per_level = rpn.get_rpn_blobs(float(H), float(W), foas, boxes, np.full((n, 1), True), npr)
    for i, b in enumerate(per_level):
        for k, v in b.items():
            ref = g['rd_%s_fpn%d' % (k, i + 2)]
            assert v.shape == ref.shape and v.dtype == ref.dtype, (k, i, v.shape, ref.shape, v.dtype, ref.dtype)
            if 'labels' in k:
                np.testing.assert_array_equal(v, ref)
            else:
                np.testing.assert_allclose(v, ref, rtol=1e-6, atol=1e-7)
    ov = np.zeros((n, 2), np.float32)
    ov[:, 1] = 1.0
    entry = dict(boxes=boxes.copy(), gt_classes=np.ones((n,), np.int32), is_crowd=np.zeros((n,), np.bool_), gt_overlaps=ov,
                 box_to_gt_ind_map=np.arange(n, dtype=np.int32), gt_keypoints=kps.copy(), height=H, width=W)
    e = fast_rcnn.merge_proposals_into_entry(entry, props)
    np.testing.assert_allclose(e['max_overlaps'], g['rd_merged_max_overlaps'], rtol=1e-6)
    np.testing.assert_array_equal(e['box_to_gt_ind_map'], g['rd_merged_b2g'])
    npr.seed(78)
    sb = fast_rcnn.sample_rois(e, 1.0, 0, npr)
    for k in ('labels_int32', 'rois', 'bbox_targets', 'bbox_inside_weights', 'bbox_outside_weights', 'keypoint_rois',
              'keypoint_locations_int32', 'keypoint_weights'):
        ref = g['rd_s_' + k]
        assert sb[k].shape == ref.shape, (k, sb[k].shape, ref.shape)
        if sb[k].dtype.kind == 'i':
            np.testing.assert_array_equal(sb[k], ref, err_msg=k)
        else:
            np.testing.assert_allclose(sb[k], ref, rtol=1e-5, atol=1e-6, err_msg=k)
    # ---- the same chain on tubes (T = 3): tube IoU in the merge, 4T-wide targets, first-frame visibility test, per-frame heatmap cells
    T = 3
    tubes, tkps, tprops = g['rt_boxes'], g['rt_kps'], g['rt_props']
    n = tubes.shape[0]
    assert tubes.shape == (n, 4 * T) and tkps.shape == (n, 3, 17 * T) and tprops.shape[1] == 4 * T and len(tprops) > 100
    ov = np.zeros((n, 2), np.float32)
    ov[:, 1] = 1.0
    entry = dict(boxes=tubes.copy(), gt_classes=np.ones((n,), np.int32), is_crowd=np.zeros((n,), np.bool_), gt_overlaps=ov,
                 box_to_gt_ind_map=np.arange(n, dtype=np.int32), gt_keypoints=tkps.copy(), height=H, width=W)
    e = fast_rcnn.merge_proposals_into_entry(entry, tprops)
    np.testing.assert_allclose(e['max_overlaps'], g['rt_merged_max_overlaps'], rtol=1e-6)
    np.testing.assert_array_equal(e['box_to_gt_ind_map'], g['rt_merged_b2g'])
    npr.seed(79)
    sb = fast_rcnn.sample_rois(e, 1.25, 0, npr)
    for k in ('labels_int32', 'rois', 'bbox_targets', 'bbox_inside_weights', 'bbox_outside_weights', 'keypoint_rois',
              'keypoint_locations_int32', 'keypoint_weights'):
        ref = g['rt_s_' + k]
        assert sb[k].shape == ref.shape, (k, sb[k].shape, ref.shape)
        if sb[k].dtype.kind == 'i':
            np.testing.assert_array_equal(sb[k], ref, err_msg='tubes: ' + k)
        else:
            np.testing.assert_allclose(sb[k], ref, rtol=1e-5, atol=1e-5, err_msg='tubes: ' + k)
    assert g['rt_s_rois'].shape[1] == 1 + 4 * T and g['rt_s_bbox_targets'].shape[1] == 2 * 4 * T
    # tube RPN labels: anchors of T frames, per-frame visibility of the tracks in the inside weights (rpn.py:285-300)
    npr.seed(80)
    per_level = rpn.get_rpn_blobs(float(H), float(W), rpn.fpn_fields(T), tubes, g['rt_vis'], npr)
    n_fg = 0
    for i, b in enumerate(per_level):
        for k, v in b.items():
            if 'vis' in k:
                continue
            ref = g['rt_%s_fpn%d' % (k, i + 2)]
            assert v.shape == ref.shape and v.dtype == ref.dtype, ('tubes', k, i, v.shape, ref.shape, v.dtype, ref.dtype)
            if 'labels' in k:
                np.testing.assert_array_equal(v, ref)
                n_fg += int((ref == 1).sum())
            else:
                np.testing.assert_allclose(v, ref, rtol=1e-6, atol=1e-7)
    assert n_fg >= 4 and g['rt_rpn_bbox_targets_wide_fpn2'].shape[1] == 3 * 4 * T
    assert g['rt_s_keypoint_locations_int32'].shape[0] == g['rt_s_keypoint_rois'].shape[0] * 17 * T
    reset_cfg()


def test_posetrack_annorect_matches_the_real_reference_golden():
    """core/mpii_eval_engine.convert_data_to_annorect_struct (the per-frame structure of the JSON poseval reads) against the
    REAL reference function run under py3 shims (tests/golden/reference_posetrack_annorect.json), all KP_CONF_TYPEs."""
    import json
    import tempfile
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.core import mpii_eval_engine as me
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'reference_posetrack_annorect.json')) as f:
        g = json.load(f)
    reset_cfg()
    boxes = np.asarray(g['boxes'], dtype=np.float32)
    poses = [np.asarray(p, dtype=np.float32) for p in g['poses']]
    for case in g['cases']:
        cfg.TRACKING.KP_CONF_TYPE = case['conf_type']
        cfg.EVAL.EVAL_MPII_KPT_THRESHOLD = -float('inf') if case['thr'] is None else case['thr']
        got = json.loads(json.dumps(me.convert_data_to_annorect_struct(boxes, poses, g['tracks'])))
        assert got == case['annorect'], case['conf_type']
    assert me.convert_data_to_annorect_struct(np.zeros((0, 5), np.float32), [], []) == g['empty']
    # the per-video files
    reset_cfg()
    names = ['images/vidA/%06d.jpg' % i for i in range(3)] + ['images/vidB/000000.jpg']
    dets = {'all_boxes': [[], [boxes, boxes[:2], np.zeros((0, 5), np.float32), boxes[:1]]],
            'all_keyps': [[], [poses, poses[:2], [], poses[:1]]],
            'all_tracks': [[], [g['tracks'], g['tracks'][:2], [], g['tracks'][:1]]]}
    with tempfile.TemporaryDirectory() as d:
        files = me.write_posetrack_json(names, dets, d)
        assert sorted(os.path.basename(f) for f in files) == ['vidA.json', 'vidB.json']
        with open(os.path.join(d, 'vidA.json')) as f:
            a = json.load(f)['annolist']
        assert [e['imagenum'] for e in a] == [[0], [1], [2]] and a[2]['annorect'][0]['score'] == [0]
    reset_cfg()


def _loader_cfg(tube_T=1):
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    cfg.MODEL.KEYPOINTS_ON = True
    cfg.MODEL.NUM_CLASSES = 2
    cfg.KRCNN.NUM_KEYPOINTS, cfg.KRCNN.HEATMAP_SIZE = 17, 56
    cfg.TRAIN.MAX_SIZE, cfg.TRAIN.BATCH_SIZE_PER_IM = 333, 64
    if tube_T == 1:
        cfg.FPN.FPN_ON = cfg.FPN.MULTILEVEL_RPN = cfg.FPN.MULTILEVEL_ROIS = True
    return cfg


def _loader_source(tube_T=1, h=200, w=320):
    from detectandtrack_amd.roi_data import synthetic

    def source(i):
        rs = np.random.RandomState(500 + i)
        data = rs.randn(1, 3, 2, h, w).astype(np.float32)
        return data, synthetic.synthetic_roidb_entry(h, w, n_persons=1 + i % 4, seed=i, T=tube_T), 1.0
    return source


@pytest.mark.parametrize('tube_T', [1, 2])
def test_sparse_rpn_labels_dense_and_scatter_plan_agree(tube_T):
    """The three consumers of the sparse labels — host dense blobs (the golden-pinned layout), the flat-buffer scatter plan
    the device path uses, and the loss normaliser's window count — describe the same tensors."""
    from detectandtrack_amd.core.config import reset_cfg
    from detectandtrack_amd.roi_data import loader
    _loader_cfg(tube_T)
    _, entry, _ = _loader_source(tube_T)(3)
    sparse, per_level, names, im_info = loader.label_clip_host(entry, 1.0, np.random.RandomState(5))
    assert len(sparse.idx) > 0 and (sparse.labels == 1).any() and (sparse.labels == 0).any()
    offs, vals, views, words = sparse.scatter_plan()
    flat = np.zeros((words,), np.uint32)
    for lv in views:
        o, shape = lv['rpn_labels_int32_wide']
        flat[o:o + int(np.prod(shape))] = np.uint32(0xFFFFFFFF)
    flat[offs] = vals
    for l, (lv, dense) in enumerate(zip(views, per_level)):
        for name, (o, shape) in lv.items():
            got = flat[o:o + int(np.prod(shape))].view(dense[name].dtype).reshape(shape)
            np.testing.assert_array_equal(got, dense[name], err_msg='%s level %d' % (name, l))
        lab = dense['rpn_labels_int32_wide']
        for (h, w) in ((lab.shape[2], lab.shape[3]), (lab.shape[2] // 2, lab.shape[3] // 3)):
            assert sparse.count_in_window(l, h, w) == int((lab[:, :, :h, :w] >= 0).sum())
    reset_cfg()


def test_roi_data_loader_is_ordered_and_reproducible():
    """roi_data.loader (reference lib/roi_data/loader.py): the k-th minibatch is the same for any worker count, equals the
    synchronous rpn.add_rpn_blobs labelling of the same clip with the same RNG, every clip of an epoch is visited once, and
    a failing source surfaces in the consumer."""
    from detectandtrack_amd.core.config import reset_cfg
    from detectandtrack_amd.roi_data import loader, rpn
    _loader_cfg(1)
    src = _loader_source(1)
    runs = []
    for workers in (1, 3):
        ld = loader.RoIDataLoader(src, num_items=5, num_workers=workers, queue_size=3, device=None, seed=11)
        mbs = [ld.get_next_minibatch(timeout=60) for _ in range(10)]
        ld.shutdown()
        runs.append(mbs)
    seen = []
    for a, b in zip(*runs):
        assert a.index == b.index and sorted(a.blobs) == sorted(b.blobs)
        for k in a.blobs:
            np.testing.assert_array_equal(a.blobs[k], b.blobs[k], err_msg=k)
        seen.append(int(a.entry['boxes'].shape[0]))
    # epoch coverage: the permutation visits the 5 clips once per epoch (identify a clip by its data tensor)
    for ep in (0, 1):
        sums = sorted(float(m.blobs['data'].sum()) for m in runs[0][5 * ep:5 * ep + 5])
        assert sums == sorted(float(src(i)[0].sum()) for i in range(5))
    # the same labels as the synchronous host path with that minibatch's RNG
    m = runs[0][2]
    ref = rpn.add_rpn_blobs({}, 1.0, m.entry, np.random.RandomState((11 + 104729 * 3) % 2 ** 32))
    for k, v in ref.items():
        np.testing.assert_array_equal(m.blobs[k], v, err_msg=k)

    def bad(i):
        raise ValueError('no such clip')
    ld = loader.RoIDataLoader(bad, num_items=2, num_workers=2, device=None, seed=0)
    with pytest.raises(ValueError):
        ld.get_next_minibatch(timeout=60)
    ld.shutdown()
    reset_cfg()


def test_trunk_split_finds_the_per_frame_prefix():
    """Executor.trunk_split (cfg.HIP.FRAME_TRUNK_CACHE): conv1 / pool1 / res2 (time kernel 1, ResNet3D.py:258-275) form the
    per-frame prefix with ONE live-out blob; a 2D model is per-frame up to the first multi-consumer point as well."""
    from tests.model_util import fpn3d_kps_cfg
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.workspace import Executor
    for arch, want in (('18', (7, 'res2_1_sum')), ('50', (13, 'res2_2_sum'))):
        reset_cfg()
        cfg_from_cfg(fpn3d_kps_cfg(arch, T=4))
        assert_and_infer_cfg()
        m = model_builder.create(cfg.MODEL.TYPE, train=False)
        n, live = Executor.trunk_split(m.net)
        assert (n, live) == want
        assert all(op.args.get('kernels', [1])[0] == 1 for op in m.net.ops[:n] if op.type == 'Conv')
        assert m.net.ops[n].type == 'Conv' and m.net.ops[n].inputs[0] == live
    reset_cfg()


def test_lr_policy_matches_the_real_reference_golden():
    """utils/lr_policy.get_lr_at_iter against schedules produced by the REAL reference lib/utils/lr_policy.py
    (tests/golden/make_golden.py:golden_lr_policy): all three policies, both warm-up methods, iterations past MAX_ITER."""
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import lr_policy
    gdir = os.path.join(os.path.dirname(__file__), 'golden')
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_cases', os.path.join(gdir, 'make_golden.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)                      # importing the generator only defines its tables and functions
    cases = mg.LR_CASES
    g = np.load(os.path.join(gdir, 'reference_lr_policy.npz'))
    assert len(cases) == len([k for k in g.files if k.startswith('lr_case')]) == 4
    for i, (pol, base, gamma, step_size, steps, lrs, max_iter, wi, wf, wm) in enumerate(cases):
        reset_cfg()
        so = cfg.SOLVER
        so.LR_POLICY, so.BASE_LR, so.GAMMA, so.STEP_SIZE, so.STEPS, so.LRS = pol, base, gamma, step_size, list(steps), list(lrs)
        so.MAX_ITER, so.WARM_UP_ITERS, so.WARM_UP_FACTOR, so.WARM_UP_METHOD = max_iter, wi, wf, wm
        got = np.array([lr_policy.get_lr_at_iter(it) for it in range(max_iter + 10)], dtype=np.float32)
        np.testing.assert_array_equal(got, g['lr_case%d' % i], err_msg='case %d (%s)' % (i, pol))
    reset_cfg()
    cfg.SOLVER.LR_POLICY = 'cosine'
    with pytest.raises(NotImplementedError):
        lr_policy.get_lr_at_iter(0)
    reset_cfg()


def test_roidb_clip_source_feeds_the_loader():
    """roi_data.minibatch.RoidbClipSource (reference roi_data/minibatch.py:59-103): frames of a roidb entry -> scaled,
    mean-subtracted, stride-padded clip; through the loader the labels are computed at that scale."""
    from detectandtrack_amd.core.config import reset_cfg
    from detectandtrack_amd.roi_data import loader, rpn, synthetic
    from detectandtrack_amd.roi_data.minibatch import RoidbClipSource
    import detectandtrack_amd.utils.blob as blob_utils
    cfg = _loader_cfg(1)
    cfg.MODEL.VIDEO_ON = True
    cfg.VIDEO.NUM_FRAMES = 2
    cfg.TRAIN.SCALES, cfg.TRAIN.MAX_SIZE = (96,), 160
    rs = np.random.RandomState(2)
    roidb = []
    for i in range(3):
        e = synthetic.synthetic_roidb_entry(60, 90, n_persons=2, seed=i, T=1)
        e['image'] = [rs.randint(0, 255, (60, 90, 3)).astype(np.uint8) for _ in range(2)]
        e['flipped'] = (i == 1)
        roidb.append(e)
    src = RoidbClipSource(roidb, seed=5)
    data, entry, scale = src(1)
    assert scale == 96.0 / 60.0 and data.shape == (1, 3, 2, 96, 160) and data.dtype == np.float32   # 96 x 144 padded to /32
    ref0, _ = blob_utils.prep_im_for_blob(roidb[1]['image'][0][:, ::-1, :], cfg.PIXEL_MEANS, [96], 160)
    np.testing.assert_array_equal(data[0, :, 0, :96, :144], ref0[0].transpose(2, 0, 1))
    assert np.all(data[0, :, :, :, 144:] == 0)
    ld = loader.RoIDataLoader(src, num_items=len(src), num_workers=2, device=None, seed=3, widths=src.widths, heights=src.heights)
    mb = ld.get_next_minibatch(timeout=60)
    ld.shutdown()
    np.testing.assert_allclose(mb.blobs['im_info'], [[96.0, 144.0, 1.6]])
    want = rpn.add_rpn_blobs({}, 1.6, mb.entry, np.random.RandomState((3 + 104729) % 2 ** 32))
    for k, v in want.items():
        np.testing.assert_array_equal(mb.blobs[k], v, err_msg=k)
    reset_cfg()


def test_own_configs_load_and_build():
    """Every yaml under configs/ loads and its graph builds (training configs in training mode)."""
    import glob
    from detectandtrack_amd.core.config import cfg, cfg_from_file, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(__file__)), 'configs', '*.yaml')))
    assert len(files) >= 4
    for f in files:
        reset_cfg()
        cfg_from_file(f)
        assert_and_infer_cfg()
        train = os.path.basename(f).startswith('train_')
        m = model_builder.create(cfg.MODEL.TYPE, train=train)
        assert len(m.net.ops) > 40 and (train or m.keypoint_net is not None), f
        # what tools/train_net.py asserts before it builds anything (round 4: the shipped training configs inherited the default 2 and
        # the README's own command line failed)
        assert not train or cfg.TRAIN.IMS_PER_BATCH == 1, f
        assert cfg.TEST.RPN_PRE_NMS_TOP_N <= 4096 or train
    reset_cfg()



def test_bench_kernel_names_and_side_run_table():
    """bench.py host logic: the conv launch tags of the C ABI's profiler map to the kernel that ran, and the side runs appended to
    the default line name existing workloads / modes."""
    import bench
    assert bench.conv_kernel_name(1282561, 'bf16') == 'conv3d_igemm_kernel<bf16,128,256>'
    assert bench.conv_kernel_name(641284, 'bf16') == 'conv3d_igemm_kernel<bf16,64,128,tps3>'
    assert bench.conv_kernel_name(649991, 'bf16') == 'conv3x3_c64_ws_kernel<bf16>'
    assert bench.conv_kernel_name(2560321, 'bf16') == 'conv1x1_k64_c256_ws_kernel<bf16>'
    assert bench.conv_kernel_name(2562561, 'bf16') == 'conv3x3_bt_kernel<bf16,256,256>'
    assert bench.conv_kernel_name(2560331, 'bf16') == 'conv1x1_lw_kernel<bf16>'
    import inspect
    src = inspect.getsource(bench.other_configs)
    for w in ('2d_r50_fpn', '3d_r50_fpn3d', "'--mode', 'train'"):
        assert w in src


def test_bench_gpus_n_without_n_ranks_never_prints_an_n_gpu_line():
    """`python bench.py --gpus 2` started WITHOUT a launcher must not print a line with n_gpus 2 from one
    process.  It re-executes itself under torch.distributed.run with 2 ranks when 2 devices are visible and exits non-zero
    otherwise (here: no GPU at all); under a launcher with the wrong rank count it exits non-zero too.  The other_configs
    labels follow BASELINE.json (config 4 = R-50 training, config 5 = R-50 inference)."""
    import subprocess
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0'], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode != 0
    assert b'n_gpus' not in p.stdout, p.stdout
    assert b'only 0 GPU(s) visible' in p.stderr, p.stderr
    # with enough devices the process would turn into the launcher: N ranks on 127.0.0.1, same arguments
    cmd = bench.ensure_ranks(4, 1, ['--gpus', '4', '--steps', '7'], device_count=8, do_exec=False)
    assert cmd[1:3] == ['-m', 'torch.distributed.run'] and '--nproc-per-node' in cmd and cmd[cmd.index('--nproc-per-node') + 1] == '4'
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1' and cmd[-4:] == ['--gpus', '4', '--steps', '7']
    assert cmd[-5].endswith('bench.py')
    assert bench.ensure_ranks(4, 4, [], device_count=8, do_exec=False) is None         # launched correctly: nothing to do
    for n, world, have in ((4, 1, 2), (4, 2, 8), (2, 8, 8)):                            # too few devices / wrong launcher size
        with pytest.raises(SystemExit) as e:
            bench.ensure_ranks(n, world, [], device_count=have, do_exec=False)
        assert e.value.code not in (0, None)
    # ranks_seen must cover N distinct processes / devices
    seen = [{'rank': r, 'local_rank': r, 'pid': 100 + r, 'device': 'GPU-%d' % r, 'pci': '0000:0%d:00' % r} for r in range(4)]
    bench.check_ranks_seen(seen, 4)
    dup = [dict(s) for s in seen]
    dup[3]['device'], dup[3]['pci'] = dup[2]['device'], dup[2]['pci']
    for bad in (seen[:3], dup):
        with pytest.raises(SystemExit):
            bench.check_ranks_seen(bad, 4)
    import inspect
    src = inspect.getsource(bench.other_configs)
    assert "'config4_3d_r50_fpn3d_training', ['--workload', '3d_r50_fpn3d', '--mode', 'train']" in src
    assert "'config5_3d_r50_fpn3d_inference', ['--workload', '3d_r50_fpn3d']" in src
    ap_src = inspect.getsource(bench.main)
    assert "'--steps', type=int, default=100" in ap_src


def test_segmented_row_counts_and_test_scale_host_logic():
    """Round 3 host logic that needs no GPU: (a) a row-counted blob of a forward with several images holds equal row segments with one
    count per image and is fetched as the images' live rows concatenated (what the reference's batched blobs hold, column 0 = image);
    (b) `utils.blob.test_scale` is the scale `prep_im_for_blob` applies (lib/utils/blob.py:78-85); (c) the pipeline's geometry key
    separates forwards that must not share a captured graph."""
    import torch
    from detectandtrack_amd import workspace as W
    from detectandtrack_amd.utils import blob as blob_utils
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    b = W.Blob(torch.zeros(12, 5), 'rois')
    arr = np.arange(60, dtype=np.float32).reshape(12, 5)
    b.count = torch.tensor([2, 0, 3], dtype=torch.int32)
    got = W._valid_rows(b, arr)
    np.testing.assert_array_equal(got, np.concatenate([arr[0:2], arr[8:11]]))
    np.testing.assert_array_equal(W._valid_rows(b, arr.reshape(3, 4, 5)), got)           # [n_images, rows, cols] view of a per-level blob
    b.count = torch.tensor([7], dtype=torch.int32)
    np.testing.assert_array_equal(W._valid_rows(b, arr), arr[:7])
    b.count = None
    assert W._valid_rows(b, arr) is arr
    rs = np.random.RandomState(0)
    for h, w, target, mx in ((720, 1280, 800, 1333), (600, 800, 800, 1333), (97, 53, 64, 100), (480, 854, 800, 1333), (1080, 1920, 800, 1333)):
        im = rs.randint(0, 255, (h, w, 3)).astype(np.uint8)
        ims, scales = blob_utils.prep_im_for_blob(im, cfg.PIXEL_MEANS, (target,), mx)
        s = blob_utils.test_scale((h, w), target, mx)
        assert s == scales[0] and ims[0].shape[:2] == (int(np.rint(h * s)), int(np.rint(w * s)))
    # (the key is a pure function of blob shape, im_info rows and unscaled image sizes)
    import importlib
    key = None
    try:
        pipeline = importlib.import_module('detectandtrack_amd.core.pipeline')
        key = pipeline.ClipPipeline._geometry
    except ImportError:
        pytest.skip('pipeline imports the device library')
    k1 = key((4, 3, 8, 768, 1344), np.tile([[768, 1344, 1.04]], (4, 1)), [(720, 1280, 3)] * 4)
    assert k1 == key((4, 3, 8, 768, 1344), np.tile([[768, 1344, 1.04]], (4, 1)), [(720, 1280, 3)] * 4)
    assert k1 != key((2, 3, 8, 768, 1344), np.tile([[768, 1344, 1.04]], (2, 1)), [(720, 1280, 3)] * 2)
    assert k1 != key((4, 3, 8, 768, 1344), np.tile([[768, 1344, 1.11]], (4, 1)), [(720, 1280, 3)] * 4)
    assert k1 != key((4, 3, 8, 768, 1344), np.tile([[768, 1344, 1.04]], (4, 1)), [(719, 1280, 3)] * 4)


def test_clips_given_as_image_files_are_decoded_to_bgr_frames(tmp_path):
    """roidb entries whose `image` holds file paths (what the reference's dataset layer produces, lib/utils/video.py:149-201) are
    decoded by core/test_engine.load_clip to HxWx3 uint8 BGR -- cv2.imread's layout -- and a sliding window decodes each file once."""
    from PIL import Image
    from detectandtrack_amd.core import test_engine
    rs = np.random.RandomState(2)
    frames = [rs.randint(0, 255, (36, 52, 3)).astype(np.uint8) for _ in range(5)]        # BGR
    paths = []
    for i, f in enumerate(frames):
        p = str(tmp_path / ('%06d.png' % i))
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(p)                        # files hold RGB
        paths.append(p)
    test_engine._FRAME_CACHE = None
    clip_a = test_engine.load_clip({'image': paths[0:4]})
    clip_b = test_engine.load_clip({'image': paths[1:5]})
    for got, ref in zip(clip_a + clip_b[-1:], frames):
        assert got.dtype == np.uint8 and got.flags['C_CONTIGUOUS']
        np.testing.assert_array_equal(got, ref)
    assert clip_b[0] is clip_a[1] and len(test_engine._FRAME_CACHE) == 5              # shared frames were not decoded again
    mixed = test_engine.load_clip({'image': [frames[0], paths[1]]})                     # arrays pass through untouched
    assert mixed[0] is frames[0] and mixed[1] is clip_a[1]
    # the cached arrays are shared between clips: read-only, and the EXIF orientation is applied as cv2.imread applies it
    assert not clip_a[1].flags.writeable
    with pytest.raises(ValueError):
        clip_a[1][0, 0, 0] = 0
    ex = Image.Exif()
    ex[0x0112] = 6                                       # "rotate 90 degrees clockwise to display"
    p = str(tmp_path / 'rotated.png')
    Image.fromarray(np.ascontiguousarray(frames[0][:, :, ::-1])).save(p, exif=ex)
    np.testing.assert_array_equal(test_engine.read_frame(p), np.rot90(frames[0], -1))
    test_engine._FRAME_CACHE = None


def test_gradient_contributions_of_a_blob_are_summed_over_their_frame_windows():
    """GradLedger.take (train_plan.py): contributions (tensor, first frame, masked) of one blob -- full-window tensors, shorter
    windows, another dtype (the fp32 RoIAlign accumulators) -- come back as ONE tensor over the union of the windows; a single
    contribution is passed through untouched and keeps its `masked` flag; the inputs are not modified."""
    import torch
    from detectandtrack_amd.train_plan import GradLedger
    from detectandtrack_amd.ops import hip_ops as ops
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g)
    for dt in (ops.F32, ops.BF16):
        tdt = ops.tdtype(dt)        # (the 16-bit format is the loaded build's)
        led = GradLedger()
        take = lambda name: led.take(name, dt)
        assert take('none') == (None, 0, False)
        # one contribution: the tensor itself, the mask flag survives
        t = rnd(3, 2, 2, 4).to(tdt)
        led.add('a', t, 1, masked=True)
        out, lo, masked = take('a')
        assert out is t and lo == 1 and masked and not led.waiting('a')
        # two full windows + a one-frame window + an fp32 accumulator marked as the RoIAlign backward's
        a, b = rnd(3, 2, 2, 4).to(tdt), rnd(3, 2, 2, 4).to(tdt)
        c = rnd(1, 2, 2, 4).to(tdt)
        r = led.roi_accumulator('b', (3, 2, 2, 4), 'cpu')       # (waits for frames [0, 3) like every RoIAlign accumulator)
        assert led.roi_accumulator('b', (3, 2, 2, 4), 'cpu') is r and led.contributions('b') == 1
        r.copy_(rnd(3, 2, 2, 4))
        keep = [x.clone() for x in (a, b, c, r)]
        led.add('b', a, 0)
        led.add('b', c, 1)
        led.add('b', b, 0)
        out, lo, masked = take('b')
        assert lo == 0 and out.dtype == tdt and tuple(out.shape) == (3, 2, 2, 4) and not masked
        ref = a.float() + b.float() + r
        ref[1:2] += c.float()
        tol = 1e-6 if tdt == torch.float32 else 0.05
        assert (out.float() - ref).abs().max() < tol
        for x, k in zip((a, b, c, r), keep):
            assert torch.equal(x, k)
        # windows that only overlap: the union is allocated
        led.add('c', c, 0)
        led.add('c', rnd(2, 2, 2, 4).to(tdt), 1)
        out, lo, _ = take('c')
        assert lo == 0 and tuple(out.shape) == (3, 2, 2, 4)
        assert (out[0:1].float() - c.float()).abs().max() < tol


def test_create_net_drops_the_cached_reader_scans():
    """the lazy-SliceKeyFrame / unread-padding / conv-reader decisions are cached per (net, blob) from a scan of the nets
    registered at that moment; registering another net must invalidate them (a later reader would otherwise see an N*T-frame tensor
    labelled T = 1, or unzeroed padding channels), packed layers must survive, and forks share the same cache."""
    from detectandtrack_amd.workspace import Workspace

    class Net(object):
        def __init__(self, name):
            self.name, self.ops = name, []
    ws = Workspace(0)
    fork = ws.fork()
    ws._layers[('slice_lazy', 'net', 'fpn_2')] = True
    ws._layers[('pad_unread', 'net', 'cls_score')] = True
    ws._layers[('conv_reader', 'net', 'res2_0_sum')] = False
    ws._layers[('net', 3)] = 'a packed conv layer'
    ws._layers[('net', ('rpnhead', 'w', 'b'))] = 'a fused head layer'
    fork.CreateNet(Net('late_reader'))
    assert sorted(ws._layers, key=str) == sorted([('net', 3), ('net', ('rpnhead', 'w', 'b'))], key=str)
    assert fork._layers is ws._layers and 'late_reader' in ws.nets


def test_reference_affine_op_library_is_built_from_the_reference_source_and_exports_its_entry_points():
    """oracle/_ref/libref_affine.so = /root/reference/lib/ops/affine_channel_nd_op.cu compiled where it lies by oracle/build_ref.py
    (hipcc, gfx950, against the Caffe2 stand-in of oracle/ref_affine/shim): loads without a GPU, exports the two C entry points of
    the test driver and contains the REFERENCE's kernels (caffe2::(anonymous)::ScaleBiasForward<float> / ScaleForward<float>).
    Test infrastructure only: tracked files hold no copy of the reference source (the driver #includes it by path at build time)."""
    from oracle import build_ref
    if os.path.isdir('/root/reference'):
        assert build_ref.build_affine()
    lib = build_ref.load_affine()
    if lib is None:
        pytest.skip('no /root/reference and no prebuilt oracle/_ref/libref_affine.so')
    assert hasattr(lib, 'ref_affine_channel_nd_fwd') and hasattr(lib, 'ref_affine_channel_nd_bwd')
    blob = open(build_ref.AFFINE_SO, 'rb').read()
    assert b'ScaleBiasForwardIfEE' in blob and b'ScaleForwardIfEE' in blob
    drv = open(os.path.join(REPO, 'oracle', 'ref_affine', 'ref_affine_driver.hip')).read()
    assert '#include REF_AFFINE_CU' in drv and 'CUDA_1D_KERNEL_LOOP' not in drv and '__global__' not in drv


def test_bench_dump_outputs_writes_the_last_timed_step(tmp_path):
    """bench.py --dump-outputs: the results of the LAST step only (forwards of the step in order, images in order), boxes of every
    foreground class [n, 5] and the person keypoint rows [n, 4, K] as float32 .npy files; --full and --dump-outputs are options."""
    import bench
    rs = np.random.RandomState(0)

    def image(n):
        kps = [rs.rand(4, 17).astype(np.float32) for _ in range(n)]
        return ([[], rs.rand(n, 5).astype(np.float32)], None, [[], kps] if n else None)
    step0 = [((0, 0), [image(3)]), ((0, 1), [image(1)])]
    step1 = [((1, 1), [image(0), image(2)]), ((1, 0), [image(4)])]      # (completion order differs from submission order)
    bench.dump_outputs(str(tmp_path / 'out'), {'results': step0 + step1, 'steps': 2})
    names = sorted(os.listdir(str(tmp_path / 'out')))
    assert names == ['im%02d_%s.npy' % (k, w) for k in range(3) for w in ('boxes', 'keypoints')]
    want = [step1[1][1][0], step1[0][1][0], step1[0][1][1]]
    for k, (cls_boxes, _, cls_keyps) in enumerate(want):
        b = np.load(str(tmp_path / 'out' / ('im%02d_boxes.npy' % k)))
        kp = np.load(str(tmp_path / 'out' / ('im%02d_keypoints.npy' % k)))
        assert b.dtype == np.float32 and kp.dtype == np.float32
        np.testing.assert_array_equal(b, cls_boxes[1])
        if cls_keyps:
            np.testing.assert_array_equal(kp, np.stack(cls_keyps[1]))
        else:
            assert kp.size == 0 and b.shape == (0, 5)
    src = open(os.path.join(REPO, 'bench.py')).read()
    assert "'--full', action='store_true'" in src and "'--dump-outputs'" in src


def test_bench_power_sampler_reads_an_amdgpu_hwmon_tree(tmp_path):
    """bench.py's `roofline.power_over_timed_region`: the hwmon directory is found by PCI address (or as the only one), power is read from
    power1_average | power1_input in microwatts, the clock from freq1_input in Hz; a box without the files reports None."""
    import importlib.util
    import time
    spec = importlib.util.spec_from_file_location('bench_for_power_test', os.path.join(REPO, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    root = tmp_path / 'drm'
    devs = tmp_path / 'pci'
    for card, pci, pf in (('card0', '0000:05:00.0', 'power1_average'), ('card1', '0000:85:00.0', 'power1_input')):
        hw = devs / pci / 'hwmon' / 'hwmon3'
        hw.mkdir(parents=True)
        (hw / pf).write_text('750000000\n' if card == 'card1' else '1000000\n')
        (hw / 'power1_cap').write_text('1400000000\n')
        (hw / 'freq1_input').write_text('1780000000\n')
        (root / card).mkdir(parents=True)
        os.symlink(str(devs / pci), str(root / card / 'device'))
    (root / 'card2' / 'device').mkdir(parents=True)        # (a display-only node without hwmon)
    assert bench.find_hwmon('0000:85:00', root=str(root)).endswith('card1/device/hwmon/hwmon3')
    assert bench.find_hwmon(None, root=str(root)) is None                 # two candidates and no address: no guess
    assert bench.find_hwmon('0000:ff:00', root=str(root)) is None
    ps = bench.PowerSampler(bench.find_hwmon('0000:85:00', root=str(root)), period_s=0.002).start()
    time.sleep(0.05)
    rep = ps.stop()
    assert rep['avg_w'] == 750.0 and rep['max_w'] == 750.0 and rep['cap_w'] == 1400.0 and rep['sclk_mhz_avg'] == 1780.0
    assert rep['samples'] >= 3 and 'power1_input' in rep['source']
    assert bench.PowerSampler(None).start().stop() is None
    assert bench.find_hwmon(None, root=str(tmp_path / 'nothing')) is None


def test_integration_md_names_every_entry_point_of_the_c_abi():
    """INTEGRATION.md is the map a maintainer of the reference binds from: every function `include/dat_hip.h` declares has a row there
    (a sizing helper may ride on its function's row as `(+_workspace_bytes)`)."""
    import re
    with open(os.path.join(REPO, 'include', 'dat_hip.h')) as f:
        names = sorted(set(re.findall(r'\b(dat_[a-z0-9_]+|_nms)\s*\(', f.read())))
    with open(os.path.join(REPO, 'INTEGRATION.md')) as f:
        text = f.read()
    assert len(names) >= 70
    missing = []
    for n in names:
        if n in text:
            continue
        m = re.match(r'(dat_[a-z0-9_]+?)(_workspace_bytes|_ws_bytes|_weight_bytes)$', n)
        if m and m.group(1) in text and ('+`%s`' % m.group(2)) in text:
            continue
        missing.append(n)
    assert not missing, 'no row in INTEGRATION.md: %s' % missing


def test_tracker_matches_the_real_reference_golden():
    """core/tracking_engine.py against lib/core/tracking_engine.py ITSELF (run under the py3 shims of tests/golden/make_golden.py --
    golden_tracker -- on seeded detections): centre-frame selection of tube detections, confidence / size pruning with in-place clipping,
    video splitting (entries of a video arrive shuffled and are sorted by their KEY-frame path, utils/image.py:44-48; the last video is
    taken as it comes, :683-684), Hungarian and greedy matching, track-id assignment.  The test regenerates the inputs from the
    generator's seeds and compares with the committed outputs."""
    import json
    import importlib.util
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.core import tracking_engine as te
    spec = importlib.util.spec_from_file_location('make_golden_for_tracker', os.path.join(REPO, 'tests', 'golden', 'make_golden.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    with open(os.path.join(REPO, 'tests', 'golden', 'reference_tracker.json')) as f:
        cases = json.load(f)['cases']
    assert len(cases) == 5 and {c['algo'] for c in cases} == {'hungarian', 'greedy'} and {c['T'] for c in cases} == {1, 3, 4}
    reset_cfg()
    try:
        for c in cases:
            cfg.TRACKING.BIPARTITE_MATCHING_ALGO = c['algo']
            cfg.KRCNN.NUM_KEYPOINTS = 17
            assert cfg.TRACKING.KEEP_CENTER_DETS_ONLY and float(cfg.TRACKING.CONF_FILTER_INITIAL_DETS) == c['conf']
            json_data, dets = mg.tracker_case(c['seed'], c['T'], tuple(c['frames_per_video']), c['algo'])
            te._center_detections(dets)
            assert [list(b.shape) for b in dets['all_boxes'][1]] == c['centred_shapes']
            dets = te._prune_bad_detections(dets, json_data, cfg.TRACKING.CONF_FILTER_INITIAL_DETS)
            out = te.compute_matches_tracks(json_data, dets)
            assert len(out['all_tracks'][1]) == len(c['tracks']) == sum(c['frames_per_video'])
            n_rows = 0
            for i, (b, want) in enumerate(zip(out['all_boxes'][1], c['pruned_boxes'])):
                want = np.asarray(want, dtype=np.float64)
                assert len(b) == len(want), (c['seed'], i)
                if len(want):       # (a frame without detections keeps the shape it came with, :87-88)
                    assert b.shape == want.shape == (len(want), 5), (c['seed'], i)
                    np.testing.assert_allclose(b, want, atol=1e-4)
                n_rows += len(want)
            assert n_rows > 2 * len(c['tracks'])            # (the cases are not degenerate)
            assert [len(k) for k in out['all_keyps'][1]] == c['pruned_pose_counts']
            assert [list(k[0].shape) if len(k) else None for k in out['all_keyps'][1]] == c['pose_shapes']
            assert [[int(t) for t in tr] for tr in out['all_tracks'][1]] == c['tracks'], 'track ids of case seed %d' % c['seed']
    finally:
        reset_cfg()


def test_blob_utils_match_the_real_reference_golden():
    """utils/blob.py against lib/utils/blob.py ITSELF (tests/golden/make_golden.py golden_blob): the `data` blob's layout -- common size,
    FPN.COARSEST_STRIDE padding, NCHW, clips along a time axis -- and prep_im_for_blob's scale rule, mean subtraction and the (fx, fy,
    INTER_LINEAR) it hands to the resampler (the resampler itself is pinned by known answers: OpenCV is not in this image)."""
    import importlib.util
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import blob as blob_utils
    spec = importlib.util.spec_from_file_location('make_golden_for_blob', os.path.join(REPO, 'tests', 'golden', 'make_golden.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'reference_blob.npz'))
    reset_cfg()
    try:
        for name, c in mg.BLOB_CASES:
            cfg.MODEL.VIDEO_ON, cfg.FPN.FPN_ON, cfg.VIDEO.NUM_FRAMES = c['video'], c['fpn'], c['T']
            got = blob_utils.im_list_to_blob(mg.blob_case_images(name, c['shapes']))
            assert got.shape == g[name].shape and got.dtype == g[name].dtype == np.float32, (name, got.shape, g[name].shape)
            np.testing.assert_array_equal(got, g[name])
        assert g['b3d_fpn_T4'].shape == (2, 3, 4, 32, 64) and g['b2d_fpn'].shape == (2, 3, 64, 64) and g['b3d_c4_T3'].shape == (1, 3, 3, 33, 41)
        means = np.array([[[102.9801, 115.9465, 122.7717]]])
        for k, (h, w, target, max_size) in enumerate(mg.PREP_CASES):
            rec = g['prep%d' % k]
            assert tuple(rec[:4]) == (h, w, target, max_size)
            assert rec[5] == rec[6] == rec[4] and rec[7] == 1            # fx = fy = the returned scale, INTER_LINEAR
            assert blob_utils.test_scale((h, w, 3), target, max_size) == rec[4], (h, w, target, max_size)
            px = g['prep%d_pixel' % k]
            im = np.ascontiguousarray(np.broadcast_to(px[:3].astype(np.uint8).reshape(1, 1, 3), (4, 6, 3)))
            ims, scales = blob_utils.prep_im_for_blob(im, means, [4], 1000)      # (a tiny image: what is checked is the mean subtraction)
            np.testing.assert_allclose(ims[0][0, 0], px[3:], rtol=0, atol=1e-5)
            if h * w <= 600 * 800:       # (the NumPy resampler on a full HD frame takes seconds; the rule itself is test_scale above)
                _, scales = blob_utils.prep_im_for_blob(np.zeros((h, w, 3), np.uint8), means, [target], max_size)
                assert scales[0] == rec[4]
    finally:
        reset_cfg()


def test_keypoint_decode_matches_the_reference_body_around_the_restated_resampler():
    """lib/utils/keypoints.py:94-149 / :210-216 ITSELF, run with the oracle's INTER_CUBIC restatement in place of the absent cv2.resize
    (tests/golden/make_golden.py golden_decode), against the oracle's restatement of that function and the product's host decode: roi
    clamp / ceil / INFERENCE_MIN_SIZE, first-maximum argmax, the continuous-coordinate formula, logit and spatial-softmax probability
    are pinned to the reference's own code (the resampler by known answers, tests/test_oracle_golden.py)."""
    import importlib.util
    from oracle import resize as R
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import keypoints as ku
    spec = importlib.util.spec_from_file_location('make_golden_for_decode', os.path.join(REPO, 'tests', 'golden', 'make_golden.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'reference_decode.npz'))
    reset_cfg()
    try:
        for name in ('dec_k17', 'dec_k17_min40', 'dec_k3_min8'):
            seed, n, K, min_size = [int(v) for v in g[name + '_cfg']]
            maps, rois = mg.decode_case_inputs(seed, n, K)
            want = g[name]
            assert want.shape == (n, 4, K) and want.dtype == np.float32
            np.testing.assert_array_equal(R.heatmaps_to_keypoints(maps, rois, min_size), want)
            cfg.KRCNN.NUM_KEYPOINTS, cfg.KRCNN.INFERENCE_MIN_SIZE = K, min_size
            np.testing.assert_array_equal(ku.heatmaps_to_keypoints(maps, rois), want)
        # the constant map decodes to its first cell, the twice-attained maximum to its first position
        seed, n, K, _ = [int(v) for v in g['dec_k17_cfg']]
        maps, rois = mg.decode_case_inputs(seed, n, K)
        w1 = max(rois[1, 2] - rois[1, 0], 1.0)
        assert abs(g['dec_k17'][1, 0, 2] - (rois[1, 0] + 0.5 * w1 / np.ceil(w1))) < 1e-4
        np.testing.assert_array_equal(R.scores_to_probs(g['probs_in']), g['probs_out'])
        np.testing.assert_array_equal(ku.scores_to_probs(g['probs_in'].copy()), g['probs_out'])
        # tube detections through core/test.py:865-894 keypoint_results and the keypoint net's roi blob (:77-121)
        from detectandtrack_amd.core import test as engine
        seed, n, K, T = [int(v) for v in g['tube_cfg']]
        cfg.KRCNN.NUM_KEYPOINTS, cfg.KRCNN.INFERENCE_MIN_SIZE, cfg.MODEL.NUM_CLASSES, cfg.KRCNN.NMS_OKS = K, 0, 2, False
        maps, rois = mg.tube_decode_inputs(seed, n, K, T)
        kps = engine.keypoint_results([[], rois], maps, rois)
        assert len(kps) == 2 and kps[0] == [] and g['tube_keyps'].shape == (n, 4, K * T)
        np.testing.assert_array_equal(np.stack(kps[1]), g['tube_keyps'])
        blob = engine._get_rois_blob(rois, np.array([1.0414]))
        assert blob.dtype == g['tube_rois_blob'].dtype == np.float32 and blob.shape == (n, 1 + 4 * T)
        np.testing.assert_array_equal(blob, g['tube_rois_blob'])
    finally:
        reset_cfg()


def test_cfg_has_every_key_and_default_of_the_real_reference_config():
    """core/config.py against lib/core/config.py ITSELF (tests/golden/make_golden.py golden_cfg_defaults: the reference's `cfg` flattened
    right after import): every reference key exists here under the same name -- a bare `ON` in embedded YAML is the boolean true in
    YAML 1.1, which once hid RPN.ON -- with the same default; the two site paths of the author's cluster are blank here; the HIP.* keys
    are this build's additions."""
    import json
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()

    def flat(d, pre=''):
        out = {}
        for k, v in d.items():
            assert isinstance(k, str), 'non-string config key %r under %r' % (k, pre)
            if isinstance(v, dict):
                out.update(flat(v, pre + k + '.'))
            else:
                out[pre + k] = v.tolist() if isinstance(v, np.ndarray) else (list(v) if isinstance(v, tuple) else v)
        return out
    mine = flat(cfg)
    with open(os.path.join(REPO, 'tests', 'golden', 'reference_cfg_defaults.json')) as f:
        ref = json.load(f)
    assert len(ref) >= 269
    missing = sorted(set(ref) - set(mine))
    assert not missing, 'reference config keys without a counterpart: %s' % missing
    extra = sorted(k for k in set(mine) - set(ref) if not k.startswith('HIP.'))
    assert not extra, 'keys the reference does not have (outside HIP.*): %s' % extra
    site_paths = {'EXT_PATHS.POSEVAL_CODE_PATH', 'VOC_DIR', 'ROOT_DIR'}     # (ROOT_DIR = wherever the tree lies: checked on the next line)
    assert os.path.realpath(mine['ROOT_DIR']) == os.path.realpath(REPO)
    diff = [(k, ref[k], mine[k]) for k in sorted(ref) if k not in site_paths and json.loads(json.dumps(mine[k])) != ref[k]]
    assert not diff, 'defaults that differ from the reference: %s' % diff[:10]
    assert cfg.RPN.ON is False


def test_every_shipped_yaml_gives_the_effective_config_the_real_reference_computes():
    """cfg_from_file + assert_and_infer_cfg against lib/core/config.py ITSELF on all 12 shipped configs (tests/golden/make_golden.py
    golden_cfg_files): yaml load, the type rules of _merge_a_into_b, the TIME_KERNEL_DIM int-to-dict mapping (:826-858) and the inferred
    keys (RPN.ON, NUM_FRAMES_MID) -- the whole set of keys that differ from the defaults, per file."""
    import json
    from detectandtrack_amd.core.config import cfg, cfg_from_file, assert_and_infer_cfg, reset_cfg
    with open(os.path.join(REPO, 'tests', 'golden', 'reference_cfg_files.json')) as f:
        ref = json.load(f)
    assert len(ref) == 12

    def flat(d, pre=''):
        out = {}
        for k, v in d.items():
            if isinstance(v, dict):
                out.update(flat(v, pre + str(k) + '.'))
            else:
                v = v.tolist() if isinstance(v, np.ndarray) else (list(v) if isinstance(v, tuple) else v)
                out[pre + str(k)] = json.loads(json.dumps(v))
        return out
    reset_cfg()
    base = flat(cfg)
    try:
        for rel, want in sorted(ref.items()):
            reset_cfg()
            cfg_from_file(os.path.join(REF_CONFIGS, rel))
            assert_and_infer_cfg()
            now = flat(cfg)
            got = {k: v for k, v in now.items() if not k.startswith('HIP.') and (k not in base or base[k] != v)}
            assert sorted(got) == sorted(want), (rel, sorted(set(got) ^ set(want)))
            bad = [(k, want[k], got[k]) for k in want if got[k] != want[k]]
            assert not bad, (rel, bad[:5])
    finally:
        reset_cfg()


def test_model_builder_emits_the_graph_the_reference_builders_emit():
    """modeling/* against the REFERENCE's own builder code (tests/golden/make_golden.py golden_builders: lib/modeling/model_builder.py
    create() -> build_generic_fast_rcnn_model with ResNet3D / ResNet / FPN3D / FPN / head_builder / keypoint_rcnn_heads and the output
    functions, executed on a recorder made of this package's helper): for the 3D R-18 / R-50 / R-101 FPN3D and the 2D R-50-FPN keypoint
    models, inference and training -- the same ops with the same inputs, outputs, kernels, strides, pads and init specs in the same
    order, the same parameter list, the same split into net / keypoint_net / conv_body_net.  The reference appends its loss ops at the
    end (:283-303); here they are fused ops next to their heads: their hyper-parameters are compared with the recorded Caffe2 ops'."""
    import gzip
    import importlib.util
    import json
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from tests import model_util
    spec = importlib.util.spec_from_file_location('make_golden_for_builders', os.path.join(REPO, 'tests', 'golden', 'make_golden.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    with gzip.open(os.path.join(REPO, 'tests', 'golden', 'reference_builder_nets.json.gz')) as f:
        ref = json.loads(f.read().decode())
    assert len(ref) == 8
    sig = lambda net: json.loads(json.dumps(mg.net_signature(net)))
    mine_loss = {'SoftmaxLoss', 'SmoothL1Loss', 'KeypointLoss', 'RpnLoss'}
    try:
        for name, rec in sorted(ref.items()):
            reset_cfg()
            cfg_from_cfg(getattr(model_util, rec['cfg_fn'])(**rec['cfg_kw']))
            if rec['train']:
                cfg.TRAIN.DATASET = 'synthetic'
            assert_and_infer_cfg()
            model = model_builder.create(cfg.MODEL.TYPE, train=rec['train'])
            assert [str(p) for p in model.params] == rec['params'], name
            if not rec['train']:
                assert sig(model.net) == rec['net'], name
                assert sig(model.keypoint_net) == rec['keypoint_net'], name
                assert len(model.conv_body_net.ops) == rec['conv_body_net_ops'], name
                # what one RoIFeatureTransform op stands for: the reference helper's own expansion (detector.py:216-310) of the same call
                mine_rt = [o for o in sig(model.net) + sig(model.keypoint_net) if o[0] == 'RoIFeatureTransform']
                assert len(mine_rt) == len(rec['roi_transforms']) == 2, name
                k_min = cfg.FPN.ROI_MIN_LEVEL
                for o, rt in zip(mine_rt, rec['roi_transforms']):
                    assert o == rt['fused'], name
                    n_feat, a = o[3]['n_feat'], o[3]
                    per_level = [e for e in rt['expansion'] if e[0] == 'RoIAlign']
                    assert len(per_level) == n_feat == cfg.FPN.ROI_MAX_LEVEL - k_min + 1
                    for i, e in enumerate(per_level):           # input i of the fused op IS pyramid level k_min + i, with scale i
                        assert e[1] == [o[1][i], '%s_fpn%d' % (o[1][n_feat], k_min + i)], (name, e)
                        assert e[3] == {'pooled_h': a['resolution'], 'pooled_w': a['resolution'], 'sampling_ratio': a['sampling_ratio'],
                                        'spatial_scale': a['scales'][i]}, (name, e)
                    cat, perm = rt['expansion'][n_feat], rt['expansion'][n_feat + 1]
                    assert cat[0] == 'Concat' and cat[1] == [e[2][0] for e in per_level] and cat[3] == {'axis': 0}
                    assert perm[0] == 'BatchPermutation' and perm[1][1] == o[1][n_feat] + '_idx_restore_int32'
                    assert len(rt['expansion']) == n_feat + 2
                continue
            got = sig(model.net)
            first_loss = [i for i, o in enumerate(rec['net']) if o[0] == 'SoftmaxWithLoss'][0]
            assert [o for o in got if o[0] not in mine_loss] == rec['net'][:first_loss], name
            tail = {tuple(o[2]): o for o in rec['net'][first_loss:]}
            fused = {o[0] + ':' + o[2][-1 if o[0] != 'SoftmaxLoss' else 1]: o for o in got if o[0] in mine_loss}
            assert fused['SoftmaxLoss:loss_cls'][3]['scale'] == tail[('cls_prob', 'loss_cls')][3]['scale']
            assert fused['SmoothL1Loss:loss_bbox'][3]['scale'] == tail[('loss_bbox',)][3]['scale'] and fused['SmoothL1Loss:loss_bbox'][3]['beta'] == 1.0
            assert 'beta' not in tail[('loss_bbox',)][3]                 # (Caffe2's default beta = 1)
            assert fused['KeypointLoss:loss_kps'][3]['scale'] == tail[('kps_prob', 'loss_kps')][3]['scale']
            assert tail[('kps_score_reshaped', '_kps_score_old_shape')][3]['shape'] == [-1, cfg.KRCNN.HEATMAP_SIZE ** 2]
            for lvl in range(cfg.FPN.RPN_MIN_LEVEL, cfg.FPN.RPN_MAX_LEVEL + 1):
                mine = fused['RpnLoss:loss_rpn_bbox_fpn%d' % lvl][3]
                sce, sl1 = tail[('loss_rpn_cls_fpn%d' % lvl,)][3], tail[('loss_rpn_bbox_fpn%d' % lvl,)][3]
                assert mine['cls_scale'] == sce['scale'] and mine['normalize'] == sce['normalize'] == 0, (name, lvl)
                assert mine['beta'] == sl1['beta'] and mine['bbox_scale'] == sl1['scale'], (name, lvl)
    finally:
        reset_cfg()


def test_heatmap_outputs_of_a_3d_head_emit_what_the_reference_function_emits():
    """model_builder.add_heatmap_outputs on a T = 3 tube head against the REFERENCE's own function run on the recorder
    (tests/golden/make_golden.py golden_builders -> reference_heatmap_outputs.json; lib/modeling/model_builder.py:755-870).
    KRCNN.NO_3D_DECONV_TIME_TO_CH False -- the reference default, core/config.py:472 -- : op for op the same (time -> channels,
    ConvTranspose dim*T -> K*T with group = T, bilinear deconv on K*T maps).  True (the shipped 3D configs): time -> batch, the 2D
    deconvs, batch -> time and time -> channels (views of what dat_kps_finalize wrote).  Both op for op, parameter for parameter."""
    import json
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.modeling.detector import DetectionModelHelper
    from tests import model_util
    with open(os.path.join(REPO, 'tests', 'golden', 'reference_heatmap_outputs.json')) as f:
        ref = json.load(f)
    sig = lambda net: json.loads(json.dumps([[o.type, [str(b) for b in o.inputs], [str(b) for b in o.outputs], dict(o.args)] for o in net.ops]))
    try:
        for no_t2c in (False, True):
            reset_cfg()
            cfg_from_cfg(model_util.c4_tube_kps_cfg(T=3, deconv='time_to_batch' if no_t2c else 'grouped'))
            assert_and_infer_cfg()
            m = DetectionModelHelper(name='heat', train=False, num_classes=cfg.MODEL.NUM_CLASSES)
            ret = model_builder.add_heatmap_outputs(m, 'conv_fcn8', cfg.KRCNN.CONV_HEAD_DIM, 3, True)
            rec = ref['no_3d_deconv_time_to_ch_%s' % no_t2c]
            assert [str(p) for p in m.params] == rec['params'] and str(ret) == rec['returns']
            got = sig(m.net)
            assert got == rec['ops'], no_t2c
            if not no_t2c:
                assert got[1][3]['group'] == 3 and got[1][3]['dim_in'] == 3 * 512 and got[1][3]['dim_out'] == got[2][3]['dim'] == 3 * 17
            else:
                assert [o[0] for o in got] == ['TimeToBatch', 'ConvTranspose', 'BilinearInterpolation', 'BatchToTime', 'TimeToChannel']
                assert got[-1][2] == ['kps_score'] and str(ret) == 'kps_score_prefinal'     # (the reference returns the pre-move blob)
    finally:
        reset_cfg()


def test_momentum_correction_matches_the_reference_set_new_lr():
    """utils.lr_policy.momentum_correction against lib/modeling/detector.py:606-616 _SetNewLr ITSELF (tests/golden/make_golden.py
    golden_lr_policy: the method run unbound, its _CorrectMomentum recorded): WHEN the update history is rescaled at a learning-rate
    change (ratio either way above SOLVER.SCALE_MOMENTUM_THRESHOLD, old lr above 1e-7, switch on) and BY WHAT (new / old)."""
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import lr_policy
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'reference_lr_policy.npz'))['momentum_correction']
    assert g.shape == (24, 5) and g[:, 3].sum() >= 6
    reset_cfg()
    try:
        for mode, cur, new, called, factor in g:
            cfg.SOLVER.SCALE_MOMENTUM = bool(mode)
            got = lr_policy.momentum_correction(float(cur), float(new))
            assert (got is not None) == bool(called), (mode, cur, new, got)
            if called:
                assert abs(got - factor) <= 1e-6 * max(abs(factor), 1e-12) + 1e-12, (cur, new, got, factor)
        cfg.SOLVER.SCALE_MOMENTUM = True
        assert lr_policy.momentum_correction(None, 0.02) is None            # the first iteration
    finally:
        reset_cfg()


def test_checkpoint_loading_matches_the_real_reference():
    """utils.net.initialize_from_weights_file against lib/utils/net.py:163-249 initialize_gpu_0_from_weights_file ITSELF (run on a
    dict-backed workspace, tests/golden/make_golden.py golden_weights): exact matches, 2D -> 3D inflation, repeat-inflation of a
    T-times-wider predictor, a shape that cannot be inflated (keeps its initialisation), a parameter the file lacks, `_[xyz]_foo <- foo`
    only when the file has no `_[xyz]_foo`, momentum restored from a checkpoint but not from a `trainedCOCO` initialisation."""
    import importlib.util
    import pickle
    import types
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import net as net_utils
    spec = importlib.util.spec_from_file_location('make_golden_for_weights', os.path.join(REPO, 'tests', 'golden', 'make_golden.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'reference_weights_load.npz'))
    shapes, init, blobs = mg.weights_case()
    reset_cfg()
    cfg.VIDEO.WEIGHTS_INFLATE_MODE = 'center-only'
    import tempfile
    d = tempfile.mkdtemp()
    try:
        for tag, fname in (('resume', 'model_iter99.pkl'), ('first', 'R-50_trainedCOCO.pkl')):
            path = os.path.join(d, fname)
            with open(path, 'wb') as f:
                pickle.dump({'blobs': blobs}, f, protocol=2)
            params = {n: v.copy() for n, v in init.items()}
            ws = types.SimpleNamespace(params=params, set_param=lambda n, v, params=params: params.__setitem__(n, np.asarray(v, np.float32)))
            model = types.SimpleNamespace(params=[n for n, _ in shapes],
                                          param_specs={n: {'shape': sh, 'init': ('GaussianFill', {'std': 0.01})} for n, sh in shapes})
            momentum = {}
            kept = net_utils.initialize_from_weights_file(model, ws, path, momentum=momentum)
            fed = [str(n) for n in g[tag + '_fed']]
            for n, sh in shapes:
                want = g[tag + ':gpu_0/' + n] if 'gpu_0/' + n in fed else init[n]
                assert params[n].shape == tuple(sh) == want.shape, (tag, n)
                np.testing.assert_array_equal(params[n], want, err_msg='%s %s' % (tag, n))
            assert 'new_head_w' in kept and 'odd_w' in kept
            np.testing.assert_array_equal(params['odd_w'], init['odd_w'])
            np.testing.assert_array_equal(params['_[pose]_fc_w'], blobs['fc_w'])            # shared initialisation
            np.testing.assert_array_equal(params['_[mask]_fc_w'], blobs['_[mask]_fc_w'])    # the file's own entry wins
            want_m = sorted(n[len('gpu_0/'):-len('_momentum')] for n in fed if n.endswith('_momentum'))
            assert sorted(momentum) == want_m == (['conv1_w', 'res2_b'] if tag == 'resume' else []), (tag, sorted(momentum), want_m)
            for n in momentum:
                np.testing.assert_array_equal(momentum[n], g[tag + ':gpu_0/' + n + '_momentum'])
    finally:
        reset_cfg()


def test_clip_assembly_matches_the_reference_get_clip():
    """utils.video.clip_frame_ids against lib/utils/video.py:149-201 get_clip ITSELF (tests/golden/make_golden.py golden_clips): which
    frames make the clip of every key frame -- odd and even T (the key frame sits at index T // 2), videos shorter than a clip, border
    replication towards the key frame, VIDEO.TIME_INTERVAL > 1 -- and the synthetic-video tools build their clips with it."""
    import json
    from detectandtrack_amd.utils.video import clip_frame_ids
    with open(os.path.join(REPO, 'tests', 'golden', 'reference_clips.json')) as f:
        cases = json.load(f)
    assert len(cases) == 5
    for c in cases:
        T, step = c['T'], c['time_interval']
        got = [clip_frame_ids(k, 1, n, T, step) for n in c['videos'] for k in range(1, n + 1)]
        assert got == c['clips'], (T, step)
        assert all(clip[T // 2] == k for clip, k in zip(got, [k for n in c['videos'] for k in range(1, n + 1)]))
    for tool in ('tools/test_net.py', 'tools/bench_config5.py'):
        with open(os.path.join(REPO, tool)) as f:
            assert 'clip_frame_ids(k, 0, n_frames - 1, T)' in f.read(), tool


def test_device_roi_sampler_checks_the_kernel_limits_up_front_and_draws_its_seed_lazily():
    """(1) the limits of dat_sample_rois (4096 candidates, every person a keypoint roi, 8 frames per tube) are checked against
    cfg and the entry in DeviceRoiSampler.__init__ -- where make_sampler's fallback to the host restatement catches them -- not by a launch
    error in the middle of an iteration; (2) the seed of the device draw is taken from the minibatch RNG only when the device sampler is
    really built: the host path, documented as bit-compatible with the reference's numpy.random stream, loses no draw."""
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.roi_data import synthetic
    from detectandtrack_amd.roi_data.device_sampler import DeviceRoiSampler, make_sampler
    reset_cfg()
    try:
        cfg.MODEL.KEYPOINTS_ON, cfg.MODEL.NUM_CLASSES = True, 2
        entry = synthetic.synthetic_roidb_entry(128, 160, n_persons=5, seed=2)
        asked = []
        seed = lambda: asked.append(1) or 7
        cfg.TRAIN.RPN_POST_NMS_TOP_N = 4092                      # 5 + 4092 > 4096 candidates
        with pytest.raises(AssertionError, match='candidates'):
            DeviceRoiSampler(entry, seed=seed)
        cfg.TRAIN.RPN_POST_NMS_TOP_N = 2000
        cfg.TRAIN.BATCH_SIZE_PER_IM = 16                         # 4 foreground rois per image for 5 persons
        with pytest.raises(AssertionError, match='persons'):
            DeviceRoiSampler(entry, seed=seed)
        assert not asked
        rng = np.random.RandomState(5)
        state = rng.get_state()[1].copy()
        s = make_sampler(entry, rng, seed=lambda: int(rng.randint(0, 2 ** 31 - 1)))       # (no GPU here: the host sampler)
        assert not isinstance(s, DeviceRoiSampler) and np.array_equal(rng.get_state()[1], state)
    finally:
        reset_cfg()
