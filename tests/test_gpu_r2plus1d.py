"""FPN3D keypoint R-CNN with ResNet-(2+1)D bodies on the GPU: the forward against the restatement (tests/r2plus1d_ref.py) on the
oracle graph, the north-star bar at the bench shape, graph replay against eager in bf16, and one training step against autograd."""
import numpy as np
import pytest
import torch

from tests.model_util import fpn3d_kps_cfg, build_product, synthetic_clip, oracle_opts
from tests.r2plus1d_ref import Net2plus1d
from tests.test_gpu_parity_full import _check_against_oracle

pytestmark = pytest.mark.gpu
BODY = 'FPN3D.add_fpn_ResNet%s_2plus1d_conv5_body'
TEMPORAL_TAG = 2560351


def _cfg(arch, **kw):
    c = fpn3d_kps_cfg(arch, **kw)
    c['MODEL']['CONV_BODY'] = BODY % arch
    return c


def _forward_against_restatement(arch, T, H, W, dtype, pre, post, names=None):
    model, ws, weights = build_product(_cfg(arch, T=T, dtype=dtype, pre=pre, post=post))
    assert any(k.endswith('_temporal_w') for k in weights)
    data = synthetic_clip(T, H, W)
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    ws.RunNet(model.net.name)
    torch.set_num_threads(max(1, min(64, torch.get_num_threads())))
    net = Net2plus1d(weights, oracle_opts(arch, T, 3, 'slice-center', pre, post))
    net.body(torch.from_numpy(data))
    pyr = net.fpn()
    if names is None:
        names = ['pool1'] + sorted(b for b in ws.Blobs() if b.endswith('_sum') and b.startswith(('res', 'fpn_res')))
    return _check_against_oracle(model, ws, weights, net, pyr, im_info, 12, names, True)


@pytest.mark.parametrize('arch', ['18', '50'])
def test_fp32_2plus1d_forward_matches_the_restatement(arch):
    """Every res*_sum and fpn_* blob, the rois, the box head and kps_score (< 1e-3) at a small clip, fp32 parity mode."""
    _forward_against_restatement(arch, 4, 128, 160, 'fp32', 300, 100)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_r18_2plus1d_at_the_bench_shape_meets_the_kps_bar(dtype):
    """1 x 3 x 8 x 768 x 1344, R-18-(2+1)D FPN3D: kps_score < 1e-3 against the restatement (the config-3 north-star bar)."""
    names = ['pool1', 'res2_1_sum', 'res3_1_sum', 'res4_1_sum', 'res5_1_sum', 'fpn_res5_1_sum', 'fpn_res4_1_sum', 'fpn_res3_1_sum',
             'fpn_res2_1_sum']
    err = _forward_against_restatement('18', 8, 768, 1344, dtype, 1000, 1000, names)
    assert err < 1e-3


def test_bf16_clip_graph_replay_equals_eager_with_the_temporal_kernel():
    """bf16 R-18-(2+1)D on one 8 x 1536 x 2176 clip, large enough for the res4 / res5 temporal convs to take the temporal-tap kernel
    (section 3.7's grid rule): a captured clip graph replayed on new clips gives exactly the eager results."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.clip_graph import ClipGraph
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.ops import hip_ops as ops
    T, H, W = 8, 1536, 2176
    model, ws, _ = build_product(_cfg('18', T=T, dtype='bf16', pre=1000, post=1000))
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
    assert tags.count(TEMPORAL_TAG) == 8, 'the temporal-tap kernel ran %d times' % tags.count(TEMPORAL_TAG)   # res4 + res5: 4 + 4
    ref.append(eager(clips[1]))
    g = ClipGraph(model, ws, clips[0], im_info, (H, W, 3), stream=torch.cuda.Stream())
    for c, (rb, rk) in zip(clips, ref):
        g.launch(c)
        boxes, keyps = g.results()
        np.testing.assert_array_equal(boxes[1], rb[1])
        assert len(keyps[1]) == len(rk[1]) > 0
        for a, b in zip(keyps[1], rk[1]):
            np.testing.assert_array_equal(a, b)


def test_train_step_gradients_of_the_2plus1d_body_match_autograd(monkeypatch):
    """One fp32 forward + backward of the R-18-(2+1)D training graph against torch autograd on the restatement (injected into
    oracle.train_ref): every loss and the gradient of every trainable parameter, every `_spatial` / `_temporal` weight among them."""
    from tests.test_gpu_train import _synthetic_training_blobs
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import TrainExecutor
    from oracle import train_ref
    monkeypatch.setattr(train_ref, 'Net', Net2plus1d)
    T, H, W = 2, 64, 96
    c = _cfg('18', T=T, dtype='fp32', pre=100, post=30)
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

    wt = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).requires_grad_(True) for k, v in weights.items()}
    ref_losses = train_ref.training_losses(
        wt, oracle_opts('18', T, 3, 'slice-center', 100, 30), data, im_info, labels, sampled,
        dict(num_gpus=1, rpn_batch=cfg.TRAIN.RPN_BATCH_SIZE_PER_IM, ims_per_batch=1, kps_loss_weight=cfg.KRCNN.LOSS_WEIGHT))
    sum(ref_losses.values()).backward()
    for k in sorted(ref_losses):
        print('%-22s %.6f  (oracle %.6f)' % (k, got_losses[k], ref_losses[k].item()))
        np.testing.assert_allclose(got_losses[k], ref_losses[k].item(), rtol=2e-4, atol=1e-6)
    trainable = set(model.TrainableParams())
    fact = sorted(n for n in trainable if '_spatial' in n or '_temporal' in n)
    assert len(fact) == 12 * 2, len(fact)           # (the affine parameters are frozen, as in the I3D body)
    checked, errs = 0, []
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
        assert err < (6e-2 if name.startswith(('conv_fcn', 'kps_score')) else 2e-3), '%s: rel err %.3e (|ref|max %.3e)' % (name, err, denom)
        errs.append(err)
        checked += 1
    print('checked gradients of %d parameters, median rel err %.2e, worst %.2e' % (checked, float(np.median(errs)), max(errs)))
    assert checked > 40 and np.median(errs) < 5e-4
