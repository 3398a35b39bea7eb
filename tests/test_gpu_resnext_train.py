"""Training of a ResNeXt body (cfg.HIP.TRAIN_GROUPED_CONV) on the GPU: one fp32 forward + backward of the reduced ResNeXt-50 of
tests/test_gpu_resnext.py against torch autograd on the restatement (tests/grouped_ref.resnext_net injected into oracle.train_ref, as
tests/test_gpu_r2plus1d.py does for its body), and three bf16 Trainer steps after which the re-packed grouped layers equal a fresh
model's built from the updated masters."""
import numpy as np
import pytest
import torch

from tests.grouped_ref import resnext_net
from tests.model_util import fpn3d_kps_cfg, synthetic_clip, oracle_opts

pytestmark = pytest.mark.gpu
GROUPS, WIDTH = 32, 4          # 128 / 256 / 512 / 1024 inner channels in 32 groups of 4 / 8 / 16 / 32
N_GROUPED, N_TRAINABLE_GROUPED = 3 + 4 + 6 + 3, 4 + 6 + 3      # res2 lies below StopGradient


def _cfg(**kw):
    c = fpn3d_kps_cfg('50', **kw)
    c['RESNETS'] = {'NUM_GROUPS': GROUPS, 'WIDTH_PER_GROUP': WIDTH, 'STRIDE_1X1': False}
    c.setdefault('HIP', {})['TRAIN_GROUPED_CONV'] = True
    c['NUM_GPUS'] = 1
    return c


def _create(c):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    reset_cfg()
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    return model_builder.create(cfg.MODEL.TYPE, train=True)


def _count(tags, base):
    return sum(1 for t in tags if t // 10 == base)


def test_fp32_train_step_gradients_of_the_resnext_body_match_autograd(monkeypatch):
    """Every loss (rtol 2e-4) and the gradient of every trainable parameter (max-abs / max-abs < 2e-3; 6e-2 for conv_fcn* / kps_score*;
    median < 5e-4), every res3-res5 `branch2b` weight among them; the grouped kernels ran the forward, the data gradient and the weight
    gradient of each of the 13 trainable grouped layers."""
    from tests.test_gpu_train import _synthetic_training_blobs
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.ops import hip_ops as ops
    from detectandtrack_amd.training import TrainExecutor
    from oracle import train_ref
    monkeypatch.setattr(train_ref, 'Net', resnext_net(GROUPS))
    T, H, W = 2, 64, 96
    c = _cfg(T=T, dtype='fp32', pre=100, post=30)
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 100, 'RPN_POST_NMS_TOP_N': 30, 'IMS_PER_BATCH': 1}
    model = _create(c)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    weights = net_utils.synthetic_params(model, 3)
    assert weights['res3_0_branch2b_w'].shape == (256, 8, 3, 3, 3)
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
    prof = ops.ConvProfiler(capacity=4096)
    prof.start()
    ex.run()
    fwd_tags = [t for t, _, _ in prof.stop()]
    prof.start()
    ex.backward()
    bwd_tags = [t for t, _, _ in prof.stop()]
    assert _count(fwd_tags, 64257) == N_GROUPED and _count(fwd_tags, 64258) == 0, (_count(fwd_tags, 64257), _count(fwd_tags, 64258))
    assert _count(bwd_tags, 64257) == N_TRAINABLE_GROUPED, 'grouped data-gradient launches: %d' % _count(bwd_tags, 64257)
    assert _count(bwd_tags, 64258) == N_TRAINABLE_GROUPED, 'grouped weight-gradient launches: %d' % _count(bwd_tags, 64258)
    got_losses = ex.loss_values()

    torch.set_num_threads(max(1, min(64, torch.get_num_threads())))
    wt = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).requires_grad_(True) for k, v in weights.items()}
    ref_losses = train_ref.training_losses(
        wt, oracle_opts('50', T, 3, 'slice-center', 100, 30), data, im_info, labels, sampled,
        dict(num_gpus=1, rpn_batch=cfg.TRAIN.RPN_BATCH_SIZE_PER_IM, ims_per_batch=1, kps_loss_weight=cfg.KRCNN.LOSS_WEIGHT))
    sum(ref_losses.values()).backward()
    for k in sorted(ref_losses):
        print('%-22s %.6f  (oracle %.6f)' % (k, got_losses[k], ref_losses[k].item()))
        np.testing.assert_allclose(got_losses[k], ref_losses[k].item(), rtol=2e-4, atol=1e-6)
    trainable = set(model.TrainableParams())
    grouped = sorted(n for n in trainable if n.endswith('_branch2b_w') and n.startswith(('res3', 'res4', 'res5')))
    assert len(grouped) == N_TRAINABLE_GROUPED
    checked, errs = set(), []
    for name in sorted(trainable):
        if name.startswith(('conv1', 'res_conv1', 'res2_')):
            assert name not in ex.param_grads, 'gradient for a parameter below StopGradient: ' + name
            continue
        assert name in ex.param_grads, 'no gradient for ' + name
        ref = wt[name].grad
        assert ref is not None, name
        got = ex.param_grads[name].cpu()
        assert got.shape == ref.shape, name
        denom = max(float(ref.abs().max()), 1e-8)
        err = float((got - ref).abs().max()) / denom
        if name in grouped:
            print('%-20s rel err %.3e' % (name, err))
        assert err < (6e-2 if name.startswith(('conv_fcn', 'kps_score')) else 2e-3), '%s: rel err %.3e (|ref|max %.3e)' % (name, err, denom)
        errs.append(err)
        checked.add(name)
    print('checked gradients of %d parameters, median rel err %.2e, worst %.2e' % (len(checked), float(np.median(errs)), max(errs)))
    assert set(grouped) <= checked
    assert len(checked) > 40 and np.median(errs) < 5e-4


def test_bf16_trainer_steps_reduce_the_loss_and_the_grouped_layers_follow_the_masters():
    """Three Trainer.step calls on one clip (deferred weight-gradient finish, gradient arena): the total loss drops; then both packed
    images of every grouped layer (forward and data gradient) are what a fresh pack of the updated master gives, and a forward through
    the re-packed layers equals a forward of a fresh workspace holding the updated masters, bit for bit."""
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.ops import hip_ops as ops
    from detectandtrack_amd.training import Trainer, TrainExecutor
    from detectandtrack_amd.roi_data import rpn as rpn_data, fast_rcnn as frcn_data, synthetic
    T, H, W = 2, 128, 160
    c = _cfg(T=T, dtype='bf16')
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 400, 'RPN_POST_NMS_TOP_N': 200, 'IMS_PER_BATCH': 1, 'MAX_SIZE': 160,
                  'BATCH_SIZE_PER_IM': 64, 'RPN_STRADDLE_THRESH': -1}
    model = _create(c)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    for k, v in net_utils.synthetic_params(model, 3).items():
        ws.set_param(k, v)
    entry = synthetic.synthetic_roidb_entry(H, W, n_persons=3, seed=5)
    data = synthetic_clip(T, H, W)
    rng = np.random.RandomState(0)
    blobs = rpn_data.add_rpn_blobs({}, 1.0, entry, rng)
    fixed = {}

    def sampler(rois, info):
        if not fixed:
            fixed.update(frcn_data.sample_training_blobs(entry, rois, info, rng))
        return fixed

    def feed(w):
        w.FeedBlob('data', data)
        for k, v in blobs.items():
            w.FeedBlob(k, v)
        w.train_sampler = sampler
    feed(ws)
    trainer = Trainer(model, ws)
    w_before = ws.dev_param('res4_1_branch2b_w').clone()
    totals = []
    for it in range(3):
        lv = trainer.step(lr=0.002).loss_values()
        assert all(np.isfinite(v) for v in lv.values()), lv
        totals.append(sum(lv.values()))
    print('total loss per iteration:', ['%.4f' % t for t in totals])
    assert totals[-1] < totals[0], totals
    assert (ws.dev_param('res4_1_branch2b_w') - w_before).abs().max().item() > 0
    # both images of every grouped layer against a fresh pack of the updated master
    n_fwd = n_dgrad = 0
    for key, layer in ws._layers.items():
        lay = layer if isinstance(layer, ops.ConvLayer) else getattr(layer, '_data_layer', None)
        if lay is None or lay.groups == 1:
            continue
        if lay.is_dgrad:
            fresh = ops.ConvLayer(None, None, None, stride=lay.stride, pads=lay.pads, dtype=lay.dtype, cin_stride=lay.cin,
                                  dgrad_of=(lay.w_src.clone(), None if lay.dgrad_scale is None else lay.dgrad_scale.clone()), groups=lay.groups)
            n_dgrad += 1
        else:
            fresh = ops.ConvLayer(lay.w_src.clone(), stride=lay.stride, pads=lay.pads, dtype=lay.dtype, cin_stride=lay.cin, groups=lay.groups)
            n_fwd += 1
        assert torch.equal(fresh.packed, lay.packed), 'packed image of %r does not follow its master' % (key,)
    assert n_fwd == N_GROUPED and n_dgrad == N_TRAINABLE_GROUPED, (n_fwd, n_dgrad)
    # forward through the re-packed layers == forward of a fresh workspace built from the updated masters
    names = ['res3_3_sum', 'res4_5_sum', 'res5_2_sum']
    TrainExecutor(ws, model.net).run()
    mine = {n: ws.blobs[n].t.clone() for n in names}
    ws.params_from_device()
    updated = {k: np.array(v, copy=True) for k, v in ws.params.items()}
    workspace.ResetWorkspace()
    ws2 = workspace.GlobalWorkspace()
    for k, v in updated.items():
        ws2.set_param(k, v)
    feed(ws2)
    TrainExecutor(ws2, model.net).run()
    for n in names:
        assert torch.equal(mine[n].view(torch.int16), ws2.blobs[n].t.view(torch.int16)), n
