"""An image's head results do not depend on the images it shares a forward with (cfg.HIP.IMS_PER_FORWARD), under
the planner's OWN plans -- no test here calls `tune_plan`.  Every comparison is bit equality.

1. Layer level (tests/batch_cases.py): every per-RoI layer family of the shipped heads through the C ABI, the rows of B images in one
   launch with `dat_conv_desc.plan_frames` = one image's rows against each image's rows alone; the rows behind the last image keep their
   sentinel.  Per family, the table holds shapes at which the batched result DIFFERS when the hint is withheld.
2. Executor level (tests/head_alone.py): the heads as `workspace.Executor` runs them, on the RoI features of one image of a B-clip
   forward, against that image's segment of the forward.
3. Whole model: a clip gets the same proposals, boxes and keypoints in slot 0 of [X, Y] and in slot 1 of [Z, X]."""
import numpy as np
import pytest
import torch

from tests import batch_cases as BC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _need_build(ops, mode):
    if mode == 'bf16x3' and ops.H16_DTYPE != torch.bfloat16:
        pytest.skip('bf16 build only')


# ---- 1. layer level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family,R,B,mode', [(f, R, B, m) for f in BC.FAMILIES for (R, B, m) in BC.table(f)])
def test_rows_of_an_image_in_a_batched_launch_equal_the_launch_alone(ops, family, R, B, mode):
    _need_build(ops, mode)
    equal, untouched = BC.run_case(ops, family, R, B, mode, hint=True)
    assert untouched, 'rows behind the last image were written'
    assert all(equal), 'images %r of %d differ from their launch alone' % ([i for i, e in enumerate(equal) if not e], B)


@pytest.mark.parametrize('family', [f for f in BC.FAMILIES if BC.DIFFERS_WITHOUT_HINT[f]])
def test_table_can_fail(ops, family):
    """Without the hint at least one case of the family's table is not bit-equal: the table holds shapes at which the planner's choice
    moves between one image's rows and B images' rows, so the test above can fail."""
    recorded = [c for c in BC.DIFFERS_WITHOUT_HINT[family] if not (c[2] == 'bf16x3' and ops.H16_DTYPE != torch.bfloat16)]
    rest = [c for c in BC.table(family) if c not in recorded and not (c[2] == 'bf16x3' and ops.H16_DTYPE != torch.bfloat16)]
    for R, B, mode in recorded + rest:
        equal, _ = BC.run_case(ops, family, R, B, mode, hint=False)
        if not all(equal):
            print('%s: R %d, B %d, %s differs without the hint' % (family, R, B, mode))
            return
    pytest.fail('no case of the %s table differs without the hint' % family)


# ---- 2. executor level ---------------------------------------------------------------------------------------------------------------------
# DETECTIONS_PER_IM 46 + the 4 spare rows = 50 keypoint RoIs per image, RPN_POST_NMS_TOP_N 100 (60 for the tube heads) box RoIs: rows at
# which section 1 measured that the sub-pixel deconv (both forms, 16-bit and fp32, B 2 and 4), the 3 x 3 and 3 x 3 x 3 head convs and --
# at B = 4 in 16 bit -- fc7 differ without the hint.  fc6 itself has no such shape below 512 rows (tests/batch_cases.py).
DETECTIONS = 46


def _h16_mode(ops):
    return 'fp16' if ops.H16_DTYPE == torch.float16 else 'bf16'


def _model_cfg(name, dtype):
    from tests.model_util import fpn3d_kps_cfg, c4_tube_kps_cfg, fpn2d_kps_cfg
    if name == 'r18_fpn3d':
        c, T, H, W = fpn3d_kps_cfg('18', T=4, dtype=dtype, pre=300, post=100), 4, 96, 128
    elif name == 'c4_tube_gn':
        c, T, H, W = c4_tube_kps_cfg(T=3, dtype=dtype, pre=300, post=60), 3, 64, 96
        c['HIP'].update(USE_GN=True)
    elif name == 'gn_kps_head':
        c, T, H, W = fpn3d_kps_cfg('18', T=2, dtype=dtype, pre=300, post=100), 2, 64, 96
        c['HIP'].update(USE_GN=True, GN_KPS_HEAD=True)
    elif name == 'time_to_channel':
        c, T, H, W = c4_tube_kps_cfg(T=3, dtype=dtype, pre=300, post=60, deconv='grouped'), 3, 64, 96
    else:
        assert name == 'r50_fpn2d'
        c, T, H, W = fpn2d_kps_cfg('50', dtype=dtype, pre=400, post=100), 1, 128, 192
    c['TEST'].update(SCALES=(H,), MAX_SIZE=max(H, W), SCORE_THRESH=0.0, DETECTIONS_PER_IM=DETECTIONS)
    return c, T, H, W


def _clips(B, T, H, W, seed=11):
    rs = np.random.RandomState(seed)
    return [[(rs.randint(0, 255, (H, W, 3)) // (1 + (i % 2))).astype(np.uint8) for _ in range(T)] for i in range(B)]


def _forward(model, ims):
    """B clips through ONE forward and the device post-processing (what core.test.im_detect_all_batch runs, without its host re-run of an
    image whose ties overflowed the detection rows -- that would replace the workspace's blobs).  Returns the per-image results."""
    from detectandtrack_amd import workspace
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.config import cfg
    B, T = len(ims), len(ims[0])
    data, im_scales = engine._get_image_blob([f for clip in ims for f in clip], num_frames=T if cfg.MODEL.VIDEO_ON else None)
    assert data.shape[0] == B
    workspace.FeedBlob('data', data)
    workspace.FeedBlob('im_info', np.tile(np.array([[data.shape[-2], data.shape[-1], im_scales[0]]], dtype=np.float32), (B, 1)))
    workspace.RunNet(model.net.Proto().name)
    dev = engine.enqueue_results_on_device(model, [clip[0].shape for clip in ims], [im_scales[0]] * B)
    return engine.read_batch_results_from_device(*dev)


@pytest.mark.parametrize('dtype', ['h16', 'fp32'])
@pytest.mark.parametrize('name,B', [('r18_fpn3d', 2), ('r18_fpn3d', 4), ('c4_tube_gn', 2), ('gn_kps_head', 2), ('time_to_channel', 2), ('r50_fpn2d', 2)])
def test_heads_on_one_image_of_a_batch_equal_the_heads_alone(ops, name, B, dtype):
    """Box head and keypoint head as the executor runs them: every blob the heads write for image i in a forward of B clips equals, bit for
    bit, the same ops run on image i's RoI features alone (one count, so nothing is planned per image).  A call site that forgets
    `plan_frames` fails here: the layer tests pass the hint themselves."""
    from tests.model_util import build_product
    from tests import head_alone
    c, T, H, W = _model_cfg(name, _h16_mode(ops) if dtype == 'h16' else 'fp32')
    model, ws, _ = build_product(c)
    _forward(model, _clips(B, T, H, W))
    for net, must in ((model.net, {'cls_prob', 'bbox_pred'}), (model.keypoint_net, {'conv_fcn8', 'kps_score_lowres', 'kps_score'})):
        for i in range(B):
            one = head_alone.run_head_alone(ws, net, i, B)
            differing, compared = head_alone.compare_head(ws, one, net, i, B)
            assert must <= set(compared), (must, compared)
            assert not differing, '%s, image %d of %d: %r differ from the head alone (of %r)' % (net.name, i, B, differing, compared)
    feat = ws.blobs[model.net.ops[head_alone.head_ops(model.net)[0]].outputs[0]]
    counts = feat.count.cpu().numpy().reshape(-1)
    print('%s B %d %s: box RoIs per image %s of %d' % (name, B, dtype, counts.tolist(), feat.N // B))


# ---- 3. whole model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['r18_fpn3d', 'c4_tube_gn'])
def test_a_clip_does_not_depend_on_its_companion_or_its_slot(ops, name):
    """Clip X in slot 0 of [X, Y] and in slot 1 of [Z, X] (Y another clip, Z flat grey: nearly empty) gets bit-equal proposals, boxes and
    keypoints, in the 16-bit mode under the planner's own plans.  The grid is the same in both forwards, so this holds whatever the
    body's plans are; a wrong im_info row, batch index or per-image count breaks it."""
    from tests.model_util import build_product
    c, T, H, W = _model_cfg(name, _h16_mode(ops))
    c['TEST'].update(RPN_POST_NMS_TOP_N=300)        # (= the pre-NMS count: every clip keeps what its NMS leaves, so the live counts differ)
    model, ws, _ = build_product(c)
    X, Y = _clips(2, T, H, W, seed=5)
    Z = [np.full((H, W, 3), 128, dtype=np.uint8) for _ in range(T)]
    seen = []
    for ims, slot in (([X, Y], 0), ([Z, X], 1)):
        res = _forward(model, ims)
        rois = ws.FetchBlob('rois')
        n = [int((rois[:, 0] == i).sum()) for i in range(2)]
        assert res[slot] is not None, 'ties at the detection limit overflowed the device rows of clip X'
        seen.append((rois[rois[:, 0] == slot][:, 1:].copy(), res[slot][0][1], res[slot][1][1], n))
    (ra, ba, ka, na), (rb, bb, kb, nb) = seen
    print('%s: proposals per image %s with Y, %s with Z' % (name, na, nb))
    assert na[0] == nb[1] > 0 and len(ba) > 0 and len(ka) == len(ba)
    assert nb[0] != na[1], 'Y and Z have the same number of proposals'
    np.testing.assert_array_equal(ra, rb, err_msg='proposals')
    np.testing.assert_array_equal(ba, bb, err_msg='boxes')
    assert len(ka) == len(kb)
    for a, b in zip(ka, kb):
        np.testing.assert_array_equal(a, b, err_msg='keypoints')
