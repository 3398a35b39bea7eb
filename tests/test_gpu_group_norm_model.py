"""GroupNorm (HIP.USE_GN) in the model on the GPU, at T = 2, 64 x 96 (the fixture of the SpatialBN model tests): fp32 inference of the
R-18 and R-18-(2+1)D FPN3D models against the restatement (tests/group_norm_ref.py), hipGraph replay against eager, two clips per
forward against each clip alone, one training forward + backward against autograd, three Trainer steps, and the refusal of
frame-subset forwards."""
import numpy as np
import pytest
import torch

from tests.model_util import fpn3d_kps_cfg, build_product, synthetic_clip, oracle_opts
from tests import group_norm_ref as ref
from tests.test_gpu_parity_full import _check_against_oracle

pytestmark = pytest.mark.gpu
BODY = {'r18': 'FPN3D.add_fpn_ResNet18_conv5_body', 'r18_2plus1d': 'FPN3D.add_fpn_ResNet18_2plus1d_conv5_body'}
T, H, W = 2, 64, 96


def _base(body):
    from oracle.net3d import Net
    from tests.r2plus1d_ref import Net2plus1d
    return Net2plus1d if '2plus1d' in body else Net


def _cfg(body, dtype, pre=300, post=100, **hip):
    c = fpn3d_kps_cfg('18', T=T, dtype=dtype, pre=pre, post=post)
    c['MODEL']['CONV_BODY'] = BODY[body]
    c['HIP'].update(USE_GN=True, **hip)
    return c


@pytest.mark.parametrize('body', sorted(BODY))
def test_fp32_inference_matches_the_restatement(body):
    from detectandtrack_amd.core.config import cfg
    model, ws, weights = build_product(_cfg(body, 'fp32'))
    gn = [op for op in model.net.ops if op.type == 'GroupNorm']
    assert len(gn) == (32 if '2plus1d' in body else 20)
    # (synthetic: no identity scale / bias, so a GroupNorm that skipped them fails)
    assert all(np.all(weights[op.args['scale']] != 1) and np.abs(weights[op.args['bias']]).max() > 0 for op in gn)
    data = synthetic_clip(T, H, W)
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    ws.RunNet(model.net.name)
    net = ref.gn_net(_base(body), float(cfg.HIP.GN_EPSILON), int(cfg.HIP.GN_NUM_GROUPS))(weights, oracle_opts('18', T, 3, 'slice-center', 300, 100))
    net.body(torch.from_numpy(data))
    pyr = net.fpn()
    names = ['pool1'] + sorted(b for b in ws.Blobs() if b.endswith('_sum') and b.startswith(('res', 'fpn_res')))
    assert 'conv1' in ws.blobs          # (the stem runs conv1 unfused, then GN + ReLU, then MaxPool)
    _check_against_oracle(model, ws, weights, net, pyr, im_info, 12, names, True)


def test_bf16_graph_replay_equals_eager():
    """The GroupNorm kernels are captured into the clip's hipGraph like every other launch: replay on new clips gives exactly the eager
    results (the pattern of test_clip_graph_replay_equals_eager)."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.clip_graph import ClipGraph
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.ops import hip_ops
    mode = 'fp16' if hip_ops.H16_DTYPE == torch.float16 else 'bf16'     # (the loaded build's 16-bit mode)
    model, ws, _ = build_product(_cfg('r18_2plus1d', mode))
    cfg.TEST.SCORE_THRESH = 0.0
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    clips = [torch.from_numpy(synthetic_clip(T, H, W, seed=s)).cuda() for s in (3, 4, 5)]

    def eager(data):
        ws.FeedBlob('data', data)
        ws.FeedBlob('im_info', im_info)
        ws.RunNet(model.net.name)
        return engine.read_results_from_device(*engine.enqueue_results_on_device(model, (H, W, 3), 1.0))
    want = [eager(c) for c in clips]
    g = ClipGraph(model, ws, clips[0], im_info, (H, W, 3), stream=torch.cuda.Stream())
    for c, (rb, rk) in zip(clips, want):
        g.launch(c)
        boxes, keyps = g.results()
        np.testing.assert_array_equal(boxes[1], rb[1])
        assert len(keyps[1]) == len(rk[1]) > 0
        for a, b in zip(keyps[1], rk[1]):
            np.testing.assert_array_equal(a, b)
    assert not np.array_equal(want[0][0][1], want[1][0][1])


def test_two_clips_per_forward_give_each_clip_the_results_it_gets_alone():
    """The pattern of test_several_images_per_forward_give_each_image_its_own_results, pass 1: with split-K forced off every conv output
    sums its K axis in the same order whatever the batch size, and the GroupNorm statistics of a clip never see another clip -- so
    proposals, detections and keypoints of a clip in a forward of two EQUAL the ones it gets alone."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.ops import hip_ops
    B = 2
    c = _cfg('r18_2plus1d', 'fp32', pre=400, post=150)
    c['TEST'].update(SCALES=(H,), MAX_SIZE=max(H, W), SCORE_THRESH=0.0, DETECTIONS_PER_IM=20)
    model, ws, _ = build_product(c)
    rs = np.random.RandomState(11)
    ims = [[(rs.randint(0, 255, (H, W, 3)) // (1 + 2 * i)).astype(np.uint8) for _ in range(T)] for i in range(B)]    # (different brightness)
    assert hip_ops.tune_plan(0, 1) == 0
    try:
        singles = []
        for i in range(B):
            cls_boxes, _, cls_keyps = engine.im_detect_all(model, ims[i], None)
            singles.append((cls_boxes, cls_keyps, ws.FetchBlob('rois').copy()))
        batch = engine.im_detect_all_batch(model, ims)
        rois = ws.FetchBlob('rois')
        assert ws.blobs['data'].t.shape[0] == B and ws.blobs['res5_1_sum'].N == B
    finally:
        hip_ops.tune_plan(0, 0)
    for i in range(B):
        rb = rois[rois[:, 0] == i]
        np.testing.assert_array_equal(rb[:, 1:], singles[i][2][:, 1:], err_msg='proposals of clip %d' % i)
        np.testing.assert_array_equal(batch[i][0][1], singles[i][0][1], err_msg='detections of clip %d' % i)
        assert len(batch[i][2][1]) == len(singles[i][1][1]) > 0
        for a, b in zip(batch[i][2][1], singles[i][1][1]):
            np.testing.assert_array_equal(a, b, err_msg='keypoints of clip %d' % i)
    assert not np.array_equal(batch[0][0][1], batch[1][0][1])


def _training_setup(body, dtype):
    from tests.test_gpu_train import _synthetic_training_blobs
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    c = _cfg(body, dtype, pre=100, post=30)
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 100, 'RPN_POST_NMS_TOP_N': 30, 'IMS_PER_BATCH': 1}
    c['NUM_GPUS'] = 1
    reset_cfg()
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    model = model_builder.create(cfg.MODEL.TYPE, train=True)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    weights = net_utils.synthetic_params(model, 3)
    for k, v in weights.items():
        ws.set_param(k, v)
    labels, sampled = _synthetic_training_blobs(T, H, W, np.random.RandomState(7))
    data = synthetic_clip(T, H, W)
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    for k, v in labels.items():
        ws.FeedBlob(k, v)
    ws.train_sampler = lambda rois, info: sampled
    return model, ws, weights, data, im_info, labels, sampled


@pytest.mark.parametrize('body', sorted(BODY))
def test_train_step_matches_autograd(body):
    """One fp32 forward + backward: losses at the rtol of the SpatialBN test, the gradient of every trainable parameter -- every
    `_s` / `_b` of res3-res5 among them -- by the rule of test_train_step_with_batch_statistics_matches_autograd: a parameter may differ
    from the float64 autograd result by the larger of the existing rule (2e-3 of the largest gradient entry; 6e-2 for the keypoint
    head) and 4x the float32-vs-float64 discrepancy of the restatement for the same parameter.  On the CPU at 64 x 96 the float32
    discrepancy exceeds the existing rule for 0 of the 93 (r18) / 0 of the 129 (r18_2plus1d) parameters checked (worst: 0.28 of the rule) (GroupNorm's smallest statistic
    here has 12 cg terms, SpatialBN's 12), so the size stays."""
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.training import TrainExecutor
    model, ws, weights, data, im_info, labels, sampled = _training_setup(body, 'fp32')
    ex = TrainExecutor(ws, model.net)
    ex.run()
    ex.backward()
    got_losses = ex.loss_values()
    scal = dict(num_gpus=1, rpn_batch=cfg.TRAIN.RPN_BATCH_SIZE_PER_IM, ims_per_batch=1, kps_loss_weight=cfg.KRCNN.LOSS_WEIGHT)
    opts = oracle_opts('18', T, 3, 'slice-center', 100, 30)
    eps, mg = float(cfg.HIP.GN_EPSILON), int(cfg.HIP.GN_NUM_GROUPS)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    l64, g64 = ref.autograd_reference(_base(body), weights, opts, data, im_info, labels, sampled, scal, torch.float64, eps, mg)
    l32, g32 = ref.autograd_reference(_base(body), weights, opts, data, im_info, labels, sampled, scal, torch.float32, eps, mg)
    for k in sorted(l64):
        print('%-22s %.6f  (float64 %.6f)' % (k, got_losses[k], l64[k]))
        np.testing.assert_allclose(got_losses[k], l64[k], rtol=2e-4, atol=1e-6)
    trainable = set(model.TrainableParams())
    gn_sb = sorted(n for n in trainable if n.endswith(('_bn_s', '_bn_b')) and n.startswith(('res3', 'res4', 'res5')))
    assert len(gn_sb) >= 2 * 15
    checked, worst, over, failures = 0, 0.0, 0, []
    print('%-38s %10s %10s %10s' % ('parameter', 'gpu-f64', 'f32-f64', 'allowed'))
    for name in sorted(trainable):
        if name.startswith(('conv1', 'res_conv1', 'res2_')):
            assert name not in ex.param_grads, 'gradient for a parameter below StopGradient: ' + name
            continue
        assert name in ex.param_grads, 'no gradient for ' + name
        r64 = g64[name]
        got = ex.param_grads[name].cpu().double().numpy().reshape(r64.shape)
        denom = max(float(np.abs(r64).max()), 1e-8)
        err = float(np.abs(got - r64).max()) / denom
        cpu = float(np.abs(g32[name] - r64).max()) / denom
        rule = 6e-2 if name.startswith(('conv_fcn', 'kps_score')) else 2e-3
        allowed = max(rule, 4 * cpu)
        over += cpu > rule
        print('%-38s %10.3e %10.3e %10.3e' % (name, err, cpu, allowed))
        worst = max(worst, err / allowed)
        if not err < allowed:
            failures.append((name, err, allowed))
        checked += 1
    print('checked gradients of %d parameters (%d GroupNorm scales / biases); float32 restatement over the existing rule: %d; '
          'largest error / allowed %.3f' % (checked, len(gn_sb), over, worst))
    assert all(n in ex.param_grads for n in gn_sb)
    assert not failures, failures
    assert checked > 70


def test_three_bf16_trainer_steps_stay_finite_and_move_scale_and_bias():
    from detectandtrack_amd.training import Trainer
    model, ws, weights, _, _, _, _ = _training_setup('r18_2plus1d', 'bf16')
    trainer = Trainer(model, ws)
    for _ in range(3):
        ex = trainer.step(0.002)
        lv = ex.loss_values()
        assert all(np.isfinite(v) for v in lv.values()), lv
    ws.params_from_device()
    moved = [n for n in model.TrainableParams() if n.endswith(('_bn_s', '_bn_b')) and n.startswith(('res3', 'res4', 'res5'))]
    assert len(moved) >= 30
    for n in moved:
        assert n in trainer.momentum and np.all(np.isfinite(ws.params[n])) and not np.array_equal(ws.params[n], weights[n]), n
    # layers below the StopGradient normalise but get no gradient: their biases (no weight decay) keep their bits, their scales move by
    # the weight decay of three steps only (lr * decay * (1 + 1.9 + 2.71) = 5.6e-6 relative; a gradient would move them by far more)
    below = [n for n in model.params if n.startswith(('conv1', 'res_conv1', 'res2_')) and n.endswith(('_bn_s', '_bn_b'))]
    assert len(below) >= 2 * 5
    for n in below:
        if n.endswith('_b'):
            assert np.array_equal(ws.params[n], weights[n]), n
        else:
            assert float(np.abs(ws.params[n] / weights[n] - 1).max()) < 1e-5, n


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('key,val', [('KEYFRAME_DCE', True), ('FRAME_TRUNK_CACHE', 4)])
def test_frame_subset_forwards_with_a_group_norm_net_are_refused(key, val, train):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import TrainExecutor
    c = _cfg('r18', 'fp32', **{key: val})
    if train:
        c['TRAIN'] = {'IMS_PER_BATCH': 1}
        c['NUM_GPUS'] = 1
    reset_cfg()
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    model = model_builder.create(cfg.MODEL.TYPE, train=train)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    with pytest.raises(ValueError, match=key):
        ws.CreateNet(model.net)
    with pytest.raises(ValueError, match='every frame of the clip'):
        (TrainExecutor if train else workspace.Executor)(ws, model.net)
    reset_cfg()
