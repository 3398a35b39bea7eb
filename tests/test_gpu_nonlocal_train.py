"""Training of the spacetime non-local blocks (HIP.TRAIN_NONLOCAL) on the GPU: one fp32 forward + backward of
the R-18 FPN3D model with blocks behind res3_1 and res4_0 against torch autograd on the restatement (tests/nonlocal_ref.NetNonLocal
injected into oracle.train_ref, as tests/test_gpu_resnext_train.py does for its body); three bf16 Trainer steps from the zero-initialised
closing scale, after which the re-packed layers equal a fresh workspace's built from the updated masters; one step each under HIP.USE_GN
and MODEL.USE_BN."""
import functools

import numpy as np
import pytest
import torch

from tests.model_util import fpn3d_kps_cfg, synthetic_clip, oracle_opts
from tests.nonlocal_ref import NetNonLocal, parse_spec

pytestmark = pytest.mark.gpu

# theta (weights AND bias) is scaled up as in tests/test_gpu_nonlocal_model.py until a query row looks at a handful of keys; the gains are
# those of the 2-frame clip used here (res4_0 has 40 pooled keys there, against 80 in the 4-frame forward test)
THETA_GAIN = {'nonlocal_res3_1': 3.0, 'nonlocal_res4_0': 6.2}

BLOCK_SUFFIXES = ('_theta_w', '_theta_b', '_phi_w', '_phi_b', '_g_w', '_g_b', '_out_w', '_out_bn_s', '_out_bn_b')


def _cfg(spec, **kw):
    c = fpn3d_kps_cfg('18', **kw)
    c['HIP'].update(NONLOCAL=spec, TRAIN_NONLOCAL=True)
    c['NUM_GPUS'] = 1
    return c


def _create(c):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    reset_cfg()
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    return model_builder.create(cfg.MODEL.TYPE, train=True)


def _sharpen(weights):
    for k in weights:
        if k.startswith('nonlocal_') and k.endswith(('_theta_w', '_theta_b')):
            weights[k] = (weights[k] * THETA_GAIN[k[:k.index('_theta')]]).astype(np.float32)
    return weights


def _block_params(spec):
    return ['nonlocal_' + p + s for p in parse_spec(spec) for s in BLOCK_SUFFIXES]


def test_fp32_train_step_gradients_match_autograd_through_the_restatement(monkeypatch):
    """Every loss (rtol 2e-4) and the gradient of every trainable parameter (max-abs / max-abs < 2e-3; 6e-2 for conv_fcn* / kps_score*;
    median < 5e-4), every parameter of both blocks among them with a nonzero reference gradient (`_phi_b` excepted: its gradient is
    zero in exact arithmetic, and both sides are held to rounding noise instead).  The closing scales are set to
    0.3 .. 0.7 and theta is scaled up as in tests/test_gpu_nonlocal_model.py; the restatement's median effective key count must lie in
    [4, L' / 4] (otherwise the block's gradients are zero or those of a mean filter).

    The clip is 2 x 128 x 160, not 2 x 64 x 96: at 64 x 96 the res4 block has L' = 2 x 2 x 3 = 12 pooled keys, and [4, L' / 4] = [4, 3]
    is empty -- no attention can meet the condition there.  128 x 160 is the size of the forward parity test, where L' is 160 / 40."""
    from tests.test_gpu_train import _synthetic_training_blobs
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import TrainExecutor
    from oracle import train_ref
    spec = 'res3_1,res4_0'
    factory, made = functools.partial(NetNonLocal, spec=spec), []

    def net_factory(*a, **k):       # (keeps the instance: its keys_eff is asserted on below)
        made.append(factory(*a, **k))
        return made[-1]
    monkeypatch.setattr(train_ref, 'Net', net_factory)
    T, H, W = 2, 128, 160
    c = _cfg(spec, T=T, dtype='fp32', pre=100, post=30)
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 100, 'RPN_POST_NMS_TOP_N': 30, 'IMS_PER_BATCH': 1}
    model = _create(c)
    assert sum(op.type == 'AffineTrain' for op in model.net.ops) == 2
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    weights = _sharpen(net_utils.synthetic_params(model, 3))
    rs = np.random.RandomState(11)
    for k in weights:
        if k.startswith('nonlocal_') and k.endswith('_out_bn_s'):
            weights[k] = rs.uniform(0.3, 0.7, size=weights[k].shape).astype(np.float32)
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

    torch.set_num_threads(max(1, min(64, torch.get_num_threads())))
    wt = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).requires_grad_(True) for k, v in weights.items()}
    ref_losses = train_ref.training_losses(
        wt, oracle_opts('18', T, 3, 'slice-center', 100, 30), data, im_info, labels, sampled,
        dict(num_gpus=1, rpn_batch=cfg.TRAIN.RPN_BATCH_SIZE_PER_IM, ims_per_batch=1, kps_loss_weight=cfg.KRCNN.LOSS_WEIGHT))
    assert made and made[-1].keys_eff, 'the restatement did not run the blocks'
    for nl in sorted(made[-1].keys_eff):
        eff, tot = made[-1].keys_eff[nl], made[-1].keys_total[nl]
        print('%s: median effective keys %.1f of %d' % (nl, eff, tot))
        assert 4.0 <= eff <= tot / 4.0, 'the attention of %s is degenerate (%.1f of %d keys)' % (nl, eff, tot)
    sum(ref_losses.values()).backward()
    for k in sorted(ref_losses):
        print('%-22s %.6f  (oracle %.6f)' % (k, got_losses[k], ref_losses[k].item()))
        np.testing.assert_allclose(got_losses[k], ref_losses[k].item(), rtol=2e-4, atol=1e-6)
    trainable = set(model.TrainableParams())
    block = _block_params(spec)
    assert set(block) <= trainable
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
        if name in block and name.endswith('_phi_b'):
            # a bias of phi adds <q_i, b> to every score of row i, which the softmax does not see: its gradient is zero in exact
            # arithmetic, so there is no nonzero reference to be relative to -- both sides must be rounding noise against phi_w's
            noise = 1e-5 * float(wt[name[:-2] + '_w'].grad.abs().max())
            print('%-28s |got|max %.3e  |ref|max %.3e  (noise level %.3e)' % (name, float(got.abs().max()), float(ref.abs().max()), noise))
            assert float(got.abs().max()) <= noise and float(ref.abs().max()) <= noise, name
            checked.add(name)
            continue
        denom = max(float(ref.abs().max()), 1e-8)
        err = float((got - ref).abs().max()) / denom
        if name in block:
            print('%-28s rel err %.3e  (|ref|max %.3e)' % (name, err, denom))
            assert float(ref.abs().max()) > 0, 'the reference gradient of %s is zero' % name
        assert err < (6e-2 if name.startswith(('conv_fcn', 'kps_score')) else 2e-3), '%s: rel err %.3e (|ref|max %.3e)' % (name, err, denom)
        errs.append(err)
        checked.add(name)
    print('checked gradients of %d parameters, median rel err %.2e, worst %.2e' % (len(checked), float(np.median(errs)), max(errs)))
    assert set(block) <= checked
    assert len(checked) > 40 and np.median(errs) < 5e-4


def _trainer_setup(c, T, H, W, zero_scale=True):
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.roi_data import rpn as rpn_data, fast_rcnn as frcn_data, synthetic
    model = _create(c)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    weights = net_utils.synthetic_params(model, 3)
    for k in weights:
        if zero_scale and k.startswith('nonlocal_') and k.endswith(('_out_bn_s', '_out_bn_b')):
            weights[k] = np.zeros_like(weights[k])          # what the builder's init spec gives
    for k, v in weights.items():
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
    return model, ws, feed


def test_bf16_trainer_steps_from_the_zero_initialised_scale():
    """Blocks behind res3_1 and res4_1 (both last of their stage; at T = 4 the gradient that reaches res4_1_sum is a frame window), three
    Trainer.step calls on one clip.  Step 1: the closing scale is zero, so its own gradient is finite and nonzero while those of theta,
    phi, g and the out conv are EXACTLY zero; after the first update they are nonzero.  The total loss drops, and a forward through the
    re-packed layers equals a forward of a fresh workspace holding the updated masters, bit for bit."""
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import Trainer, TrainExecutor
    spec = 'res3_1,res4_1'
    T, H, W = 4, 128, 160
    c = _cfg(spec, T=T, dtype='bf16')
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 400, 'RPN_POST_NMS_TOP_N': 200, 'IMS_PER_BATCH': 1, 'MAX_SIZE': 160,
                  'BATCH_SIZE_PER_IM': 64, 'RPN_STRADDLE_THRESH': -1}
    model, ws, feed = _trainer_setup(c, T, H, W)
    trainer = Trainer(model, ws)
    block = _block_params(spec)
    assert set(block) <= set(trainer.trainable)
    inner = [n for n in block if not n.endswith(('_out_bn_s', '_out_bn_b'))]
    totals, grads = [], []
    for it in range(3):
        lv = trainer.step(lr=0.002).loss_values()
        assert all(np.isfinite(v) for v in lv.values()), lv
        totals.append(sum(lv.values()))
        assert bool(torch.isfinite(trainer.flat_g).all())
        grads.append({n: trainer.arena[n].clone() for n in block})
    for nl in ('nonlocal_res3_1', 'nonlocal_res4_1'):
        g = grads[0][nl + '_out_bn_s']
        assert float(g.abs().max()) > 0, 'step 1: the gradient of %s_out_bn_s is zero' % nl
    for n in inner:
        assert float(grads[0][n].abs().max()) == 0.0, 'step 1: %s has a gradient although the closing scale is zero' % n
        assert float(grads[1][n].abs().max()) > 0, 'step 2: the gradient of %s is still zero' % n
    print('total loss per iteration:', ['%.4f' % t for t in totals])
    assert totals[-1] < totals[0], totals
    assert float(ws.dev_param('nonlocal_res4_1_out_bn_s').abs().max()) > 0
    names = ['res3_1_sum', 'res4_1_sum', 'res5_1_sum', 'nonlocal_res4_1_y', 'nonlocal_res3_1_y']
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


@pytest.mark.parametrize('norm', ['gn', 'bn'])
def test_one_step_under_group_norm_and_batch_norm(norm):
    """The closing op is then a trainable GroupNorm / SpatialBN (layers with their own parity tests): the step runs, every gradient is
    finite and the zero-initialised closing scale receives one."""
    from detectandtrack_amd.training import Trainer
    spec = 'res3_1,res4_0'
    T, H, W = 2, 128, 160
    c = _cfg(spec, T=T, dtype='bf16')
    if norm == 'gn':
        c['HIP']['USE_GN'] = True
    else:
        c['MODEL']['USE_BN'] = True
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 400, 'RPN_POST_NMS_TOP_N': 200, 'IMS_PER_BATCH': 1, 'MAX_SIZE': 160,
                  'BATCH_SIZE_PER_IM': 64, 'RPN_STRADDLE_THRESH': -1}
    model, ws, _ = _trainer_setup(c, T, H, W)
    trainer = Trainer(model, ws)
    lv = trainer.step(lr=0.002).loss_values()
    assert all(np.isfinite(v) for v in lv.values()), lv
    assert bool(torch.isfinite(trainer.flat_g).all())
    for nl in ('nonlocal_res3_1', 'nonlocal_res4_0'):
        assert float(trainer.arena[nl + '_out_bn_s'].abs().max()) > 0, nl
