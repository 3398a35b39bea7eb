"""SpatialBN (MODEL.USE_BN) in the model on the GPU: test-mode inference against the restatement (tests/spatial_bn_ref.py) and, bit
for bit, against the affine model fed the host-folded pair; one training forward + backward of the R-18 and R-18-(2+1)D graphs against
autograd; three Trainer steps and the checkpoint's running statistics; the refusal of frame-subset forwards."""
import numpy as np
import pytest
import torch

from tests.model_util import fpn3d_kps_cfg, build_product, synthetic_clip, oracle_opts
from tests import spatial_bn_ref as ref
from tests.test_gpu_parity_full import _check_against_oracle

pytestmark = pytest.mark.gpu
BODY = {'r18': 'FPN3D.add_fpn_ResNet18_conv5_body', 'r18_2plus1d': 'FPN3D.add_fpn_ResNet18_2plus1d_conv5_body'}
HEADS = ('kps_score', 'cls_prob', 'bbox_pred')


def _base(body):
    from oracle.net3d import Net
    from tests.r2plus1d_ref import Net2plus1d
    return Net2plus1d if '2plus1d' in body else Net


def _infer(c, weights, data, im_info, n_kp=12):
    model, ws, _ = build_product(c)
    for k, v in weights.items():
        if k in model.params:
            ws.set_param(k, v)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    ws.RunNet(model.net.name)
    ws.FeedBlob('keypoint_rois', ws.FetchBlob('rois')[:n_kp].copy())
    ws.RunNet(model.keypoint_net.name)
    return model, ws, {n: ws.FetchBlob(n).copy() for n in HEADS}


def test_fp32_inference_matches_the_restatement_and_the_folded_affine_model_bit_for_bit():
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.utils import net as net_utils
    from oracle.net3d import Net
    T, H, W = 2, 64, 96
    c = fpn3d_kps_cfg('18', T=T, dtype='fp32', pre=300, post=100)
    c['MODEL']['USE_BN'] = True
    model, ws, weights = build_product(c)
    stats = sorted(model.computed_params)
    assert len(stats) == 40 and all(np.abs(weights[n]).min() > 0 for n in stats)      # (synthetic: no identity statistics)
    eps = float(cfg.MODEL.BN_EPSILON)
    data = synthetic_clip(T, H, W)
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    ws.RunNet(model.net.name)
    net = ref.bn_net(Net, False, eps, 0.9)(weights, oracle_opts('18', T, 3, 'slice-center', 300, 100))
    net.body(torch.from_numpy(data))
    pyr = net.fpn()
    names = ['pool1'] + sorted(b for b in ws.Blobs() if b.endswith('_sum') and b.startswith(('res', 'fpn_res')))
    _check_against_oracle(model, ws, weights, net, pyr, im_info, 12, names, True)
    got = {n: ws.FetchBlob(n).copy() for n in HEADS}
    # the same model without the switch, fed the pair folded on the host
    folded = {k: v for k, v in weights.items() if k not in stats}
    for n in stats:
        if n.endswith('_rm'):
            p = n[:-3]
            folded[p + '_s'], folded[p + '_b'] = net_utils.fold_bn(weights[p + '_s'], weights[p + '_b'], weights[p + '_rm'], weights[p + '_riv'], eps)
    c2 = fpn3d_kps_cfg('18', T=T, dtype='fp32', pre=300, post=100)
    _, _, plain = _infer(c2, folded, data, im_info)
    for n in HEADS:
        assert plain[n].shape == got[n].shape and np.array_equal(plain[n], got[n]), n


@pytest.mark.parametrize('body', sorted(BODY))
def test_train_step_with_batch_statistics_matches_autograd(body):
    """One fp32 forward + backward at T = 2, 64 x 96 (the fixture of test_train_step_gradients_of_the_2plus1d_body_match_autograd):
    losses at that test's rtol, the gradient of every trainable parameter -- every `_s` / `_b` of res3-res5 among them -- and the updated
    `_rm` / `_riv` of ALL layers, conv1 and res2 included.

    Tolerance per parameter: the restatement's autograd runs on the CPU in float64 and in float32; a parameter may differ from the
    float64 result by the larger of the existing rule (2e-3 of the largest gradient entry; 6e-2 for the keypoint head) and 4x the
    float32-vs-float64 discrepancy of the same parameter (fp32 BN over the M = 12 positions of res5 is itself that ill-conditioned).
    On the CPU at 64 x 96 no parameter's float32 discrepancy exceeds the existing rule (0 of 93), so the size stays."""
    from tests.test_gpu_train import _synthetic_training_blobs
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import TrainExecutor
    T, H, W = 2, 64, 96
    c = fpn3d_kps_cfg('18', T=T, dtype='fp32', pre=100, post=30)
    c['MODEL'].update(CONV_BODY=BODY[body], USE_BN=True)
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
    rs = np.random.RandomState(7)
    labels, sampled = _synthetic_training_blobs(T, H, W, rs)
    data = synthetic_clip(T, H, W)
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    for k, v in labels.items():
        ws.FeedBlob(k, v)
    ws.train_sampler = lambda rois, info: sampled
    ex = TrainExecutor(ws, model.net)
    ex.run()
    ex.backward()
    got_losses = ex.loss_values()
    ws.params_from_device(model.computed_params)

    scal = dict(num_gpus=1, rpn_batch=cfg.TRAIN.RPN_BATCH_SIZE_PER_IM, ims_per_batch=1, kps_loss_weight=cfg.KRCNN.LOSS_WEIGHT)
    opts = oracle_opts('18', T, 3, 'slice-center', 100, 30)
    eps, mom = float(cfg.MODEL.BN_EPSILON), float(cfg.MODEL.BN_MOMENTUM)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    l64, g64, s64 = ref.autograd_reference(_base(body), weights, opts, data, im_info, labels, sampled, scal, torch.float64, eps, mom)
    l32, g32, s32 = ref.autograd_reference(_base(body), weights, opts, data, im_info, labels, sampled, scal, torch.float32, eps, mom)
    for k in sorted(l64):
        print('%-22s %.6f  (float64 %.6f)' % (k, got_losses[k], l64[k]))
        np.testing.assert_allclose(got_losses[k], l64[k], rtol=2e-4, atol=1e-6)
    trainable = set(model.TrainableParams())
    bn_sb = sorted(n for n in trainable if n.endswith(('_bn_s', '_bn_b')) and n.startswith(('res3', 'res4', 'res5')))
    assert len(bn_sb) >= 2 * 15 and not trainable & set(model.computed_params)
    checked, worst, failures = 0, 0.0, []
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
        print('%-38s %10.3e %10.3e %10.3e' % (name, err, cpu, allowed))
        worst = max(worst, err / allowed)
        if not err < allowed:
            failures.append((name, err, allowed))
        checked += 1
    print('checked gradients of %d parameters (%d SpatialBN scales / biases); largest error / allowed %.3f' % (checked, len(bn_sb), worst))
    assert not failures, failures
    assert checked > 70
    # the running statistics of every layer -- the layers below the StopGradient normalise with batch statistics too
    assert sorted(s64) == sorted(model.computed_params)
    for n in sorted(s64):
        assert not np.array_equal(ws.params[n], weights[n]), n + ' did not move'
        tol = max(1e-5 * max(1.0, float(np.abs(s64[n]).max())), 4 * float(np.abs(s32[n] - s64[n]).max()))
        assert float(np.abs(ws.params[n] - s64[n]).max()) <= tol, (n, float(np.abs(ws.params[n] - s64[n]).max()), tol)


def test_three_bf16_trainer_steps_and_the_checkpoint_carries_the_statistics(tmp_path):
    from tests.test_gpu_train import _synthetic_training_blobs
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import Trainer
    T, H, W = 2, 64, 96
    c = fpn3d_kps_cfg('18', T=T, dtype='bf16', pre=100, post=30)
    c['MODEL'].update(CONV_BODY=BODY['r18_2plus1d'], USE_BN=True)
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
    trainer = Trainer(model, ws)
    for _ in range(3):
        ex = trainer.step(0.002)
        lv = ex.loss_values()
        assert all(np.isfinite(v) for v in lv.values()), lv
    ws.params_from_device()
    stats = sorted(model.computed_params)
    for n in stats:
        assert np.all(np.isfinite(ws.params[n])) and not np.array_equal(ws.params[n], weights[n]), n
        assert n not in trainer.momentum and n not in trainer.arena
    moved = [n for n in model.TrainableParams() if n.endswith(('_bn_s', '_bn_b')) and n.startswith(('res3', 'res4', 'res5'))]
    assert len(moved) >= 30
    for n in moved:
        assert n in trainer.momentum and not np.array_equal(ws.params[n], weights[n]), n
    path = str(tmp_path / 'bn_model.pkl')
    net_utils.save_model_to_weights_file(path, model, ws, trainer.momentum_blobs())
    blobs = net_utils.load_weights_file(path)
    assert all(np.array_equal(blobs[n], ws.params[n]) for n in stats) and not any(n + '_momentum' in blobs for n in stats)
    trained = {k: np.array(v) for k, v in ws.params.items()}
    # test-mode forward of the trained parameters, and of a fresh inference model that only ever saw the file
    ci = fpn3d_kps_cfg('18', T=T, dtype='bf16', pre=100, post=30)
    ci['MODEL'].update(CONV_BODY=BODY['r18_2plus1d'], USE_BN=True)
    _, _, a = _infer(ci, trained, data, im_info, n_kp=6)
    model2, ws2, _ = build_product(ci)
    ws2.params.clear()
    ws2._dev_params.clear()
    ws2._layers.clear()
    net_utils.initialize_from_weights_file(model2, ws2, path)
    ws2.FeedBlob('data', data)
    ws2.FeedBlob('im_info', im_info)
    ws2.RunNet(model2.net.name)
    ws2.FeedBlob('keypoint_rois', ws2.FetchBlob('rois')[:6].copy())
    ws2.RunNet(model2.keypoint_net.name)
    for n in HEADS:
        b = ws2.FetchBlob(n)
        assert b.shape == a[n].shape and b.size > 0 and np.array_equal(b, a[n]), n


def test_keyframe_dce_with_a_training_mode_bn_graph_is_refused():
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import TrainExecutor
    c = fpn3d_kps_cfg('18', T=2, dtype='fp32')
    c['MODEL']['USE_BN'] = True
    c['HIP']['KEYFRAME_DCE'] = True
    c['TRAIN'] = {'IMS_PER_BATCH': 1}
    c['NUM_GPUS'] = 1
    reset_cfg()
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    model = model_builder.create(cfg.MODEL.TYPE, train=True)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    with pytest.raises(ValueError, match='KEYFRAME_DCE'):
        ws.CreateNet(model.net)
    with pytest.raises(ValueError, match='every frame'):
        TrainExecutor(ws, model.net)
    # the test-mode graph of the same switch has no such op and is accepted
    infer = model_builder.create(cfg.MODEL.TYPE, train=False)
    ws.CreateNet(infer.net)
    reset_cfg()
