"""The C5-dilated keypoint R-CNN (configs/test_r18_c5_dilated_synthetic.yaml: 3D R-18 conv5 body, MODEL.DILATION 2, slice-center,
single-level RPN, 2-MLP box head, keypoint head) on the GPU against the restatement of tests/dilated_ref.py on the oracle graph: the
forward at T = 4, 128 x 160 (fp32: features, RPN head, rois, box head, kps_score; bf16x3: kps_score), a captured clip graph against
eager in bf16, and one fp32 training step against autograd.  The bars are the project's: feature blobs < 1e-3 max(1, |ref|max),
cls_prob 1e-4, bbox_pred 1e-3, kps_score < 1e-3."""
import numpy as np
import pytest
import torch

from tests import dilated_ref as dr
from tests.model_util import build_product, synthetic_clip, oracle_opts

pytestmark = pytest.mark.gpu
T, H, W, PRE, POST = 4, 128, 160, 300, 100


def _opts(T_, pre, post):
    from detectandtrack_amd.core.config import cfg
    return dict(oracle_opts('18', T_, 3, 'slice-center', pre, post), dilation=2, rpn_sizes=tuple(cfg.RPN.SIZES),
                rpn_c4_aspect_ratios=tuple(cfg.RPN.ASPECT_RATIOS))


_REF = {}


def _reference(weights, data, im_info):
    """the restatement's forward, computed once for the fp32 and the bf16x3 test (same weights, same clip) and left unchanged"""
    if 'net' not in _REF:
        torch.set_num_threads(max(1, min(64, torch.get_num_threads())))
        net = dr.NetDilated(weights, _opts(T, PRE, POST))
        feat, rois = dr.forward_2d_heads(net, data, im_info)
        _REF.update(net=net, feat=feat, rois=rois)
    return _REF['net'], _REF['feat'], _REF['rois']


def _forward(dtype):
    model, ws, weights = build_product(dr.c5_dilated_cfg('18', T=T, dilation=2, pre=PRE, post=POST, dtype=dtype))
    data = synthetic_clip(T, H, W)
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    ws.RunNet(model.net.name)
    return model, ws, weights, data, im_info


def _kps_against_the_restatement(model, ws, net, feat, n_kp=8):
    rois = ws.FetchBlob('rois')
    kp_rois = rois[:n_kp].copy()
    ws.FeedBlob('keypoint_rois', kp_rois)
    ws.RunNet(model.keypoint_net.name)
    kps = ws.FetchBlob('kps_score')
    ref = net.kps_head_c4_2d(feat, kp_rois).numpy()
    assert kps.shape == ref.shape == (n_kp, 17, 56, 56)
    err = float(np.abs(kps - ref).max())
    print('C5-dilated kps_score max-abs %.3e (ref max %.2f)' % (err, np.abs(ref).max()))
    assert err < 1e-3
    return rois


def test_fp32_forward_matches_the_restatement():
    from tests.test_gpu_shipped_configs import _close, _rois_found
    model, ws, weights, data, im_info = _forward('fp32')
    net, feat, ref_rois = _reference(weights, data, im_info)
    r4, r5 = ws.FetchBlob('res4_1_sum'), ws.FetchBlob('res5_1_sum')
    assert r5.shape[2:] == r4.shape[2:] == (T, H // 16, W // 16), 'res5 left the 1/16 grid: %r vs res4 %r' % (r5.shape, r4.shape)
    # (the sum of a stage's inner blocks is written in place over `branch2b`'s output: add_stage's inplace_sum)
    for n, ref in (('res4_1_sum', 'res4_1_sum'), ('res5_0_branch2b_bn', 'res5_0_sum'), ('res5_1_sum', 'res5_1_sum')):
        _close(ref, ws.FetchBlob(n), net.blobs[ref])
    A = int(weights['rpn_cls_logits_w'].shape[0])
    head = ws.FetchBlob('rpn_cls_logits+rpn_bbox_pred')                       # (1, 5A, h, w)
    assert head.shape[1] == 5 * A and head.shape[2:] == (H // 16, W // 16)
    np.testing.assert_allclose(1.0 / (1.0 + np.exp(-head[:, :A])), net.blobs['rpn_cls_probs'].numpy(), atol=1e-4)
    np.testing.assert_allclose(head[:, A:], net.blobs['rpn_bbox_pred'].numpy(), atol=1e-3)
    rois = ws.FetchBlob('rois')
    assert rois.shape[1] == 5
    _rois_found(rois, ref_rois)
    cls_prob, bbox_pred = dr.box_head(net, feat, rois)
    np.testing.assert_allclose(ws.FetchBlob('cls_prob'), cls_prob, atol=1e-4)
    np.testing.assert_allclose(ws.FetchBlob('bbox_pred'), bbox_pred, atol=1e-3)
    _kps_against_the_restatement(model, ws, net, feat)


def test_bf16x3_kps_score_meets_the_bar():
    from detectandtrack_amd.ops import hip_ops as ops
    if ops.L.H16 == 'fp16':
        pytest.skip('bf16x3 exists in the bf16 build only')
    model, ws, weights, data, im_info = _forward('bf16x3')
    net, feat, _ = _reference(weights, data, im_info)
    _kps_against_the_restatement(model, ws, net, feat)


def test_bf16_clip_graph_replay_equals_eager():
    """A captured clip graph replayed on a second clip gives exactly the eager results (boxes and keypoints)."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.clip_graph import ClipGraph
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.ops import hip_ops as ops
    mode = 'fp16' if ops.H16_DTYPE == torch.float16 else 'bf16'         # (the loaded build's 16-bit mode)
    model, ws, _ = build_product(dr.c5_dilated_cfg('18', T=T, dilation=2, pre=PRE, post=POST, dtype=mode))
    cfg.TEST.SCORE_THRESH = 0.0
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    clips = [torch.from_numpy(synthetic_clip(T, H, W, seed=s)).cuda() for s in (3, 4)]

    def eager(data):
        ws.FeedBlob('data', data)
        ws.FeedBlob('im_info', im_info)
        ws.RunNet(model.net.name)
        return engine.read_results_from_device(*engine.enqueue_results_on_device(model, (H, W, 3), 1.0))
    prof = ops.ConvProfiler(capacity=4096)
    prof.start()
    ref = [eager(clips[0])]
    tags = [t for t, _, _ in prof.stop()]
    assert sum(1 for t in tags if t % 10 >= 5) == 2, 'dilated launches: %r' % ([t for t in tags if t % 10 >= 5],)   # res5_{0,1}_branch2b
    ref.append(eager(clips[1]))
    g = ClipGraph(model, ws, clips[0], im_info, (H, W, 3), stream=torch.cuda.Stream())
    for c, (rb, rk) in zip(clips, ref):
        g.launch(c)
        boxes, keyps = g.results()
        np.testing.assert_array_equal(boxes[1], rb[1])
        assert len(keyps[1]) == len(rk[1]) > 0
        for a, b in zip(keyps[1], rk[1]):
            np.testing.assert_array_equal(a, b)


def test_train_step_gradients_match_autograd_on_the_restatement():
    """One fp32 forward + backward of configs/train_r18_c5_dilated_synthetic.yaml's graph against torch autograd on
    tests/dilated_ref.training_losses: every loss and the gradient of every trainable parameter, the dilated res5 weights among them."""
    from tests.test_gpu_train import _synthetic_training_blobs
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import TrainExecutor
    Tt, Ht, Wt = 2, 64, 96
    c = dr.c5_dilated_cfg('18', T=Tt, dilation=2, pre=100, post=30, dtype='fp32')
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
    _, sampled = _synthetic_training_blobs(Tt, Ht, Wt, rs)
    # the single-level 'wide' RPN labels (stride 16), wider than the head output like the per-level ones of that helper
    A = int(weights['rpn_cls_logits_w'].shape[0])
    hw, ww = int(np.ceil(Ht / 16.)) + 1, int(np.ceil(Wt / 16.)) + 2
    lab = -np.ones((1, A, hw, ww), dtype=np.int32)
    pick = rs.rand(1, A, hw, ww)
    lab[pick < 0.25] = 0
    lab[pick < 0.05] = 1
    w_in = np.repeat((lab == 1).astype(np.float32), 4, axis=1)
    labels = {'rpn_labels_int32_wide': lab, 'rpn_bbox_targets_wide': (rs.randn(1, 4 * A, hw, ww) * 0.3).astype(np.float32),
              'rpn_bbox_inside_weights_wide': w_in, 'rpn_bbox_outside_weights_wide': w_in / 64.0}
    data = synthetic_clip(Tt, Ht, Wt)
    im_info = np.array([[Ht, Wt, 1.0]], dtype=np.float32)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    for k, v in labels.items():
        ws.FeedBlob(k, v)
    ws.train_sampler = lambda rois, info: sampled
    ex = TrainExecutor(ws, model.net)
    ex.run()
    ex.backward()
    got_losses = ex.loss_values()

    wt = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).requires_grad_(True) for k, v in weights.items()}
    ref_losses = dr.training_losses(wt, _opts(Tt, 100, 30), data, labels, sampled, dict(num_gpus=1, kps_loss_weight=cfg.KRCNN.LOSS_WEIGHT))
    sum(ref_losses.values()).backward()
    assert sorted(ref_losses) == sorted(got_losses), (sorted(ref_losses), sorted(got_losses))
    for k in sorted(ref_losses):
        print('%-22s %.6f  (restatement %.6f)' % (k, got_losses[k], ref_losses[k].item()))
        np.testing.assert_allclose(got_losses[k], ref_losses[k].item(), rtol=2e-4, atol=1e-6)
    trainable = set(model.TrainableParams())
    assert {'res5_0_branch2b_w', 'res5_1_branch2b_w'} <= trainable
    checked, errs = 0, {}
    for name in sorted(trainable):
        if name.startswith(('conv1', 'res_conv1', 'res2_')):
            assert name not in ex.param_grads, 'gradient for a parameter below StopGradient: ' + name
            continue
        assert name in ex.param_grads, 'no gradient for ' + name
        ref = wt[name].grad
        assert ref is not None, name
        got = ex.param_grads[name].cpu()
        denom = max(float(ref.abs().max()), 1e-8)
        err = float((got - ref).abs().max()) / denom
        # (the bars of tests/test_gpu_r2plus1d.py and tests/test_gpu_train.py: the keypoint branch's gradient is sparse, and one
        #  activation within 1e-7 of the ReLU threshold masked differently moves a parameter's gradient by a few 1e-3)
        assert err < (6e-2 if name.startswith(('conv_fcn', 'kps_score')) else 2e-3), '%s: rel err %.3e (|ref|max %.3e)' % (name, err, denom)
        errs[name] = err
        checked += 1
    print('checked gradients of %d parameters, median rel err %.2e, worst %.2e; res5_0_branch2b_w %.2e, res5_1_branch2b_w %.2e' %
          (checked, float(np.median(list(errs.values()))), max(errs.values()), errs['res5_0_branch2b_w'], errs['res5_1_branch2b_w']))
    assert checked > 30 and np.median(list(errs.values())) < 5e-4
