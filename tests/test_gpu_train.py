"""GPU parity of the training-side kernels against torch autograd on the CPU (fp32): weight and data
gradients of the fused conv, ReLU/bias backward, FPN top-down backward, momentum SGD."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import numerics as nm
from tests.wgrad_refs import wgrad_ref64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _ndhwc(x5, cs, dtype):
    """(N, C, T, H, W) fp32 numpy/torch -> CUDA [N*T, H, W, cs]"""
    n, c, t, h, w = x5.shape
    out = torch.zeros((n * t, h, w, cs), dtype=torch.float32)
    out[..., :c] = x5.permute(0, 2, 3, 4, 1).reshape(n * t, h, w, c)
    return out.to(dtype).cuda()


def _from_ndhwc(y, n, c, t):
    f, h, w, cs = y.shape
    return y.float().cpu().view(n, t, h, w, cs)[..., :c].permute(0, 4, 1, 2, 3).contiguous()


CASES = [
    # cin, cout, (kt,kh,kw), stride, (pt,ph,pw), N, T, H, W
    (64, 128, (3, 3, 3), 1, (1, 1, 1), 1, 3, 12, 14),
    (24, 40, (1, 3, 3), 1, (0, 1, 1), 2, 2, 9, 11),
    (64, 128, (3, 3, 3), 2, (1, 1, 1), 1, 3, 12, 16),
    (128, 256, (1, 1, 1), 2, (0, 0, 0), 1, 2, 12, 16),
    (256, 12, (1, 1, 1), 1, (0, 0, 0), 1, 2, 10, 12),
    (130, 70, (3, 3, 3), 1, (1, 1, 1), 1, 4, 8, 10),
]


@pytest.mark.parametrize('dtype_name', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES)
def test_conv_backward_matches_autograd(ops, case, dtype_name):
    cin, cout, k, st, pads, N, T, H, W = case
    dt = ops.F32 if dtype_name == 'fp32' else ops.BF16
    tdt = ops.tdtype(dt)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((N, cin, T, H, W), generator=g)
    w = torch.randn((cout, cin) + k, generator=g) * (2.0 / (cin * k[0] * k[1] * k[2])) ** 0.5
    scale = torch.rand(cout, generator=g) + 0.5
    if dtype_name == 'bf16':   # the reference sees the same rounded operands
        x = nm.q16(x)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    sr = scale.clone().requires_grad_(True)
    z = F.conv3d(xr, wr, None, stride=(1, st, st), padding=pads)
    y = z * sr.view(1, -1, 1, 1, 1)
    gy = torch.randn(y.shape, generator=g)
    if dtype_name == 'bf16':
        gy = nm.q16(gy)
    y.backward(gy)

    cs_x, cs_g = ops.round_up(cin, 64), ops.round_up(cout, 64)
    xd = _ndhwc(x, cs_x, tdt)
    gd = _ndhwc(gy, cs_g, tdt)
    cg = ops.ConvGrad(w.cuda(), scale.cuda(), (st, st), pads, dt, cs_x, cs_g)
    dW, dscale = cg.weight(xd, gd, T, want_dscale=True)
    tol = 2e-4 if dtype_name == 'fp32' else 2e-2
    ref_dw = wr.grad
    err = (dW.cpu() - ref_dw).abs().max() / max(ref_dw.abs().max(), 1e-6)
    assert err < tol, 'dW rel err %.3e' % err
    err = (dscale.cpu() - sr.grad).abs().max() / max(sr.grad.abs().max(), 1e-6)
    assert err < tol, 'dscale rel err %.3e' % err
    dx = cg.data(gd, T, H, W)
    got = _from_ndhwc(dx, N, cin, T)
    err = (got - xr.grad).abs().max() / max(xr.grad.abs().max(), 1e-6)
    assert err < (2e-4 if dtype_name == 'fp32' else 3e-2), 'dx rel err %.3e' % err
    if dtype_name == 'fp32':
        # every element against float64 (tests/numerics.py): fp32 operands, fp32 accumulation, one fp32 rounding of w * scale in the packer
        x64, w64, s64, gy64 = x.double(), w.double(), scale.double().view(1, -1, 1, 1, 1), gy.double()
        dgrad = lambda a, b: torch.nn.grad.conv3d_input(x.shape, a, b, stride=(1, st, st), padding=pads)
        abs_dx = dgrad(w64.abs(), (gy64 * s64).abs())
        nm.assert_elementwise(got, dgrad(w64, gy64 * s64), abs_dx, nm.conv_k(cout, k), 'fp32', 'dx', extra=nm.unit_roundoff('fp32') * abs_dx)
    if dtype_name == 'bf16':
        # per-element bounds against float64 (tests/numerics.py): dW is stored in fp32 after a reduction over every output position
        x64, w64, s64, gy64 = x.double(), w.double(), scale.double().view(1, -1, 1, 1, 1), gy.double()
        st3 = (1, st, st)
        wgrad = lambda a, b: torch.nn.grad.conv3d_weight(a, w.shape, b, stride=st3, padding=pads)
        nm.assert_elementwise(dW.cpu(), wgrad(x64, gy64 * s64), wgrad(x64.abs(), (gy64 * s64).abs()), gy.numel() // cout, 'fp32', 'dW')
        # dx is stored in 16 bits, from weights that dat_conv3d_pack_weights_dgrad packs with the scale folded in (conv_pack.hip
        # pack_tile: w * scale, then ONE rounding to 16 bits): a second rounding, at most u16 * |w * scale| per weight
        dgrad = lambda a, b: torch.nn.grad.conv3d_input(x.shape, a, b, stride=st3, padding=pads)
        abs_dx = dgrad(w64.abs(), (gy64 * s64).abs())
        nm.assert_elementwise(got, dgrad(w64, gy64 * s64), abs_dx, nm.conv_k(cout, k), nm.h16(), 'dx',
                              extra=nm.unit_roundoff(nm.h16()) * abs_dx)
    # accumulate into an existing gradient (a blob with two consumers)
    base = torch.randn(dx.shape, generator=g).to(tdt).cuda()
    base[..., cin:] = 0
    expect = base.float() + dx.float()
    acc = cg.data(gd, T, H, W, accumulate_into=base.clone())
    assert (acc.float() - expect).abs().max() <= (1e-5 if dtype_name == 'fp32' else 0.06 * expect.abs().max())


@pytest.mark.parametrize('dtype_name', ['fp32', 'bf16'])
def test_relu_bias_bwd_and_upsample_bwd(ops, dtype_name):
    dt = ops.F32 if dtype_name == 'fp32' else ops.BF16
    tdt = ops.tdtype(dt)
    g = torch.Generator().manual_seed(2)
    for cs, C in ((64, 64), (256, 200), (2048, 2048)):
        y = torch.relu(torch.randn((3, 6, 8, cs), generator=g)).to(tdt)
        dy = torch.randn((3, 6, 8, cs), generator=g).to(tdt)
        dy2 = torch.randn((3, 6, 8, cs), generator=g).to(tdt)
        dbias = torch.zeros(C, dtype=torch.float32).cuda()
        got = ops.relu_bias_bwd(dy.cuda(), y.cuda(), dt, C, relu=True, dy2=dy2.cuda(), dbias=dbias)
        ref = (dy.float() + dy2.float()) * (y.float() > 0)
        ref[..., C:] = 0
        ref_q = ref.to(tdt).float()
        assert (got.float().cpu() - ref_q).abs().max() <= (0 if dtype_name == 'fp32' else 0.02)
        np.testing.assert_allclose(dbias.cpu().numpy(), ref.reshape(-1, cs).sum(0)[:C].numpy(), rtol=1e-4, atol=1e-3)
    gfine = torch.randn((2, 8, 12, 64), generator=g).to(tdt)
    top = ops.upsample2x_bwd(gfine.cuda(), dt)
    ref = gfine.float().view(2, 4, 2, 6, 2, 64).sum(dim=(2, 4))
    assert (top.float().cpu() - ref).abs().max() <= (1e-6 if dtype_name == 'fp32' else 0.05)
    top2 = ops.upsample2x_bwd(gfine.cuda(), dt, dtop=top.clone())
    assert (top2.float().cpu() - 2 * ref).abs().max() <= (1e-5 if dtype_name == 'fp32' else 0.1)


def test_sgd_momentum_matches_reference_update(ops):
    """model_builder.py:954-985: biases grad*2 no decay; weights grad += wd*w; v = mu*v + lr*g; w -= v."""
    g = torch.Generator().manual_seed(1)
    for is_bias in (0, 1):
        w = torch.randn(1000, generator=g)
        v = torch.randn(1000, generator=g) * 0.1
        grad = torch.randn(1000, generator=g)
        lr, mu, wd = 0.01, 0.9, 1e-4
        gg = 2 * grad if is_bias else grad + wd * w
        nv = mu * v + lr * gg
        nw = w - nv
        wd_, vd, gd = w.clone().cuda(), v.clone().cuda(), grad.clone().cuda()
        ops.sgd_momentum(wd_, vd, gd, lr, mu, wd, is_bias)
        np.testing.assert_allclose(vd.cpu().numpy(), nv.numpy(), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(wd_.cpu().numpy(), nw.numpy(), rtol=1e-6, atol=1e-7)


def test_losses_match_torch(ops):
    g = torch.Generator().manual_seed(9)
    # ---- RPN: sigmoid CE (ignore = -1) + smooth L1 on a fused head tensor, labels "wide" and narrowed by indexing ----
    N, H, W, A, cs = 1, 7, 9, 3, 64
    Hw, Ww = 8, 12
    head = torch.randn((N, H, W, cs), generator=g)
    labels = torch.randint(-1, 2, (N, A, Hw, Ww), generator=g, dtype=torch.int32)
    tgt = torch.randn((N, 4 * A, Hw, Ww), generator=g)
    w_in = (torch.rand((N, 4 * A, Hw, Ww), generator=g) > 0.5).float()
    w_out = w_in * 0.125
    cls_mult, beta, bbox_mult = 1.0 / 256, 1.0 / 9, 0.5
    hr = head.clone().requires_grad_(True)
    logit = hr[..., :A].permute(0, 3, 1, 2)
    lab = labels[:, :, :H, :W]
    valid = lab >= 0
    l_cls = (F.binary_cross_entropy_with_logits(logit, lab.clamp(min=0).float(), reduction='none') * valid).sum() * cls_mult
    d = hr[..., A:5 * A].permute(0, 3, 1, 2)
    v = w_in[:, :, :H, :W] * (d - tgt[:, :, :H, :W])
    l1 = torch.where(v.abs() < beta, 0.5 * v * v / beta, v.abs() - 0.5 * beta)
    l_box = (w_out[:, :, :H, :W] * l1).sum() * bbox_mult
    (l_cls + l_box).backward()
    loss2 = torch.zeros(2).cuda()
    dhead = ops.rpn_loss(head.cuda(), ops.F32, A, 0, A, labels.cuda(), tgt.cuda(), w_in.cuda(), w_out.cuda(), cls_mult, beta,
                         bbox_mult, loss2)
    np.testing.assert_allclose(loss2.cpu().numpy(), [l_cls.item(), l_box.item()], rtol=1e-5)
    np.testing.assert_allclose(dhead.cpu().numpy(), hr.grad.numpy(), atol=1e-7)
    # ---- smooth L1 rows (box head) ----
    R, D, ld = 37, 8, 64
    pred = torch.randn((1, 1, R, ld), generator=g)
    t2, wi2 = torch.randn((R, D), generator=g), (torch.rand((R, D), generator=g) > 0.3).float()
    wo2 = wi2 * 0.01
    pr = pred.clone().requires_grad_(True)
    v = wi2 * (pr[0, 0, :, :D] - t2)
    ref = (wo2 * torch.where(v.abs() < 1.0, 0.5 * v * v, v.abs() - 0.5)).sum() * 0.25
    ref.backward()
    loss = torch.zeros(1).cuda()
    dp = ops.smooth_l1_rows(pred.cuda(), ops.F32, D, t2.cuda(), wi2.cuda(), wo2.cuda(), 1.0, 0.25, loss)
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-5)
    np.testing.assert_allclose(dp.cpu().numpy(), pr.grad.numpy(), atol=1e-7)
    # ---- softmax CE rows: classes (no weights) and spatial 56*56 (weights) ----
    for R, D, ld, weighted in ((50, 2, 64, False), (34, 3136, 3136, True)):
        logits = torch.randn((R, ld), generator=g) * 3
        lab = torch.randint(0, D, (R,), generator=g, dtype=torch.int32)
        w = (torch.rand(R, generator=g) > 0.4).float() if weighted else None
        norm = float(w.sum()) if weighted else float(R)
        lr_ = logits.clone().requires_grad_(True)
        nll = F.cross_entropy(lr_[:, :D], lab.long(), reduction='none')
        ref = ((nll * w).sum() if weighted else nll.sum()) / norm * 0.5
        ref.backward()
        loss = torch.zeros(1).cuda()
        correct = torch.zeros(1, dtype=torch.int32).cuda()
        dl = ops.softmax_ce_rows(logits.cuda(), ops.F32, D, lab.cuda(), None if w is None else w.cuda(), 0.5 / norm, loss, correct)
        np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-5)
        np.testing.assert_allclose(dl.cpu().numpy(), lr_.grad.numpy(), atol=1e-7)
        assert correct.item() == int((logits[:, :D].argmax(1) == lab.long()).sum())


def test_roi_align_and_kps_tail_backward(ops):
    """Adjoint tests: <f(x), u> == <x, f^T(u)> for the two linear ops (RoIAlign over 2 FPN levels, keypoint tail)."""
    g = torch.Generator().manual_seed(4)
    C = 64
    feats = [torch.randn((2, 24, 32, C), generator=g).cuda(), torch.randn((2, 12, 16, C), generator=g).cuda()]
    rois = torch.tensor([[0, 4.3, 5.1, 60.7, 70.2], [1, 10.0, 3.0, 200.0, 150.0], [0, 100.5, 40.2, 127.0, 95.0],
                         [1, -3.0, -2.0, 30.0, 20.0]], dtype=torch.float32).cuda()
    scales = [0.25, 0.125]
    y = ops.roi_align(feats, scales, ops.F32, rois, T=1, Tr=1, t0=0, pooled=7, sampling=2, k_min=2, canon_scale=56., canon_level=3)
    u = torch.randn(y.shape, generator=g).cuda()
    dfeats = [torch.zeros_like(f) for f in feats]
    ops.roi_align_bwd(dfeats, scales, ops.F32, rois, u, T=1, Tr=1, t0=0, pooled=7, sampling=2, k_min=2, canon_scale=56.,
                      canon_level=3)
    lhs = (y * u).sum().item()
    rhs = sum((f * d).sum().item() for f, d in zip(feats, dfeats))
    assert abs(lhs - rhs) < 1e-3 * max(1.0, abs(lhs)), (lhs, rhs)
    assert all(d.abs().sum().item() > 0 for d in dfeats)
    R, Tr, S, cs, K, up = 3, 2, 14, 128, 17, 2
    sub = torch.randn((R * Tr, S, S, cs), generator=g).cuda()
    out = ops.kps_finalize(sub, ops.F32, R, Tr, K, up)
    u = torch.randn(out.shape, generator=g).cuda()
    dsub = ops.kps_finalize_bwd(u, ops.F32, R, Tr, S, cs, K, up)
    lhs = (out * u).sum().item()
    rhs = (sub[..., :4 * K] * dsub[..., :4 * K]).sum().item()
    assert abs(lhs - rhs) < 1e-3 * max(1.0, abs(lhs)), (lhs, rhs)
    assert dsub[..., 4 * K:].abs().max().item() == 0


def _synthetic_training_blobs(T, H, W, rs, n_rois=24, n_kp=4, K=17, M=56):
    """Label blobs in the reference's layouts: 'wide' RPN labels per FPN level and the sampled Fast R-CNN / keypoint blobs."""
    labels = {}
    A = 3
    for lvl in range(2, 7):
        s = 2 ** lvl
        hw, ww = int(np.ceil(H / float(s))) + 1, int(np.ceil(W / float(s))) + 2          # wider than the head output
        lab = -np.ones((1, A, hw, ww), dtype=np.int32)
        pick = rs.rand(1, A, hw, ww)
        lab[pick < 0.25] = 0
        lab[pick < 0.05] = 1
        w_in = np.repeat((lab == 1).astype(np.float32), 4, axis=1)
        labels['rpn_labels_int32_wide_fpn%d' % lvl] = lab
        labels['rpn_bbox_targets_wide_fpn%d' % lvl] = (rs.randn(1, 4 * A, hw, ww) * 0.3).astype(np.float32)
        labels['rpn_bbox_inside_weights_wide_fpn%d' % lvl] = w_in
        labels['rpn_bbox_outside_weights_wide_fpn%d' % lvl] = w_in / 64.0
    x1, y1 = rs.uniform(0, W * 0.6, n_rois), rs.uniform(0, H * 0.6, n_rois)
    bw, bh = rs.uniform(6, W * 0.7, n_rois), rs.uniform(6, H * 0.7, n_rois)
    rois = np.stack([np.zeros(n_rois), x1, y1, np.minimum(x1 + bw, W - 1), np.minimum(y1 + bh, H - 1)], 1).astype(np.float32)
    lab = (rs.rand(n_rois) < 0.4).astype(np.int32)
    tgt = np.zeros((n_rois, 8), np.float32)
    w_in = np.zeros((n_rois, 8), np.float32)
    tgt[lab == 1, 4:] = rs.randn(int(lab.sum()), 4) * 0.5
    w_in[lab == 1, 4:] = 1.0
    kp_rois = rois[np.where(lab == 1)[0][:n_kp]].copy()
    sampled = {
        'rois': rois, 'labels_int32': lab, 'bbox_targets': tgt, 'bbox_inside_weights': w_in,
        'bbox_outside_weights': (w_in > 0).astype(np.float32), 'keypoint_rois': kp_rois,
        'keypoint_locations_int32': rs.randint(0, M * M, (kp_rois.shape[0] * K, 1)).astype(np.int32),
        'keypoint_weights': (rs.rand(kp_rois.shape[0] * K, 1) < 0.7).astype(np.float32),
        'keypoint_loss_normalizer': np.array([1.0], np.float32),
    }
    return labels, sampled


def test_train_step_gradients_match_oracle_autograd(ops):
    """One forward + backward of the FPN3D / 2D-head keypoint R-CNN training graph (fp32 parity mode) against torch autograd
    on the oracle's restatement: every loss value and the gradient of every trainable parameter."""
    from tests.model_util import fpn3d_kps_cfg, synthetic_clip, oracle_opts
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.training import TrainExecutor
    from oracle import train_ref
    T, H, W = 2, 64, 96
    c = fpn3d_kps_cfg('18', T=T, dtype='fp32', pre=100, post=30)
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 100, 'RPN_POST_NMS_TOP_N': 30, 'IMS_PER_BATCH': 1}
    c['NUM_GPUS'] = 1
    from detectandtrack_amd.core.config import cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
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
    frozen_prefix = ('conv1', 'res_conv1', 'res2_')
    checked, errs = 0, []
    for name in sorted(trainable):
        if name.startswith(frozen_prefix):
            assert name not in ex.param_grads, 'gradient for a parameter below StopGradient: ' + name
            continue
        assert name in ex.param_grads, 'no gradient for ' + name
        ref = wt[name].grad
        assert ref is not None, name
        got = ex.param_grads[name].cpu()
        denom = max(float(ref.abs().max()), 1e-8)
        err = float((got - ref).abs().max()) / denom
        # the keypoint branch's gradient is sparse (a few valid keypoints): one activation within 1e-7 of the ReLU threshold that
        # the two fp32 summation orders mask differently moves that layer's gradients by a few 1e-3; the median stays ~1e-5
        assert err < (6e-2 if name.startswith(('conv_fcn', 'kps_score')) else 2e-3), '%s: rel err %.3e (|ref|max %.3e)' % (name, err, denom)
        errs.append(err)
        checked += 1
    print('checked gradients of %d parameters, median rel err %.2e, worst %.2e' % (checked, float(np.median(errs)), max(errs)))
    assert checked > 40 and np.median(errs) < 5e-4


def test_trainer_steps_reduce_the_loss(ops):
    """End to end: synthetic clip + roidb entry -> RPN labels + sampled rois (roi_data) -> Trainer.step x N with momentum SGD
    on the device masters; the same clip is fitted, so the total loss must drop and the packed layers must follow."""
    from tests.model_util import fpn3d_kps_cfg
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import Trainer
    from detectandtrack_amd.roi_data import rpn as rpn_data, fast_rcnn as frcn_data, synthetic
    T, H, W = 2, 128, 160
    c = fpn3d_kps_cfg('18', T=T, dtype='bf16')
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 400, 'RPN_POST_NMS_TOP_N': 200, 'IMS_PER_BATCH': 1, 'MAX_SIZE': 160,
                  'BATCH_SIZE_PER_IM': 64, 'RPN_STRADDLE_THRESH': -1}
    c['NUM_GPUS'] = 1
    reset_cfg()
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    model = model_builder.create(cfg.MODEL.TYPE, train=True)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    for k, v in net_utils.synthetic_params(model, 3).items():
        ws.set_param(k, v)
    entry = synthetic.synthetic_roidb_entry(H, W, n_persons=3, seed=5)
    from tests.model_util import synthetic_clip
    data = synthetic_clip(T, H, W)
    rng = np.random.RandomState(0)
    blobs = rpn_data.add_rpn_blobs({}, 1.0, entry, rng)
    ws.FeedBlob('data', data)
    for k, v in blobs.items():
        ws.FeedBlob(k, v)
    # a fixed sample so that successive iterations optimise the same objective
    fixed = {}

    def sampler(rois, info):
        if not fixed:
            fixed.update(frcn_data.sample_training_blobs(entry, rois, info, rng))
        return fixed
    ws.train_sampler = sampler
    trainer = Trainer(model, ws)
    w_before = ws.dev_param('fc7_w').clone()
    totals = []
    for it in range(6):
        ex = trainer.step(lr=0.002)
        lv = ex.loss_values()
        assert all(np.isfinite(v) for v in lv.values()), lv
        totals.append(sum(lv.values()))
    print('total loss per iteration:', ['%.4f' % t for t in totals])
    assert totals[-1] < totals[0], totals
    assert (ws.dev_param('fc7_w') - w_before).abs().max().item() > 0
    assert 'conv1_w' not in ex.param_grads and 'res2_0_branch2a_w' not in ex.param_grads
    ws.params_from_device()
    assert np.abs(ws.params['fc7_w'] - w_before.cpu().numpy()).max() > 0


def test_deferred_weight_gradient_finish_gives_the_immediate_gradients(ops):
    """cfg.HIP.DEFER_WGRAD_FINISH: the conv weight gradients of one bf16 Trainer step, accumulated in the kernels' [tap][Cout][Cin] order
    and finished by ONE dat_wgrad_finish_batch launch, against the per-layer memset + kernel + finish path (same kernels; the K-split
    atomics make either path's fp32 sums order-dependent, hence a tolerance).  The shared RPN conv (one weight, five FPN levels) goes
    through the accumulator five times."""
    from tests.model_util import fpn3d_kps_cfg, synthetic_clip
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import Trainer
    from detectandtrack_amd.roi_data import rpn as rpn_data, fast_rcnn as frcn_data, synthetic
    T, H, W = 2, 128, 160
    flat = {}
    for defer in (False, True):
        c = fpn3d_kps_cfg('18', T=T, dtype='bf16')
        c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 400, 'RPN_POST_NMS_TOP_N': 200, 'IMS_PER_BATCH': 1, 'MAX_SIZE': 160,
                      'BATCH_SIZE_PER_IM': 64, 'RPN_STRADDLE_THRESH': -1}
        c['NUM_GPUS'] = 1
        c.setdefault('HIP', {})['DEFER_WGRAD_FINISH'] = defer
        reset_cfg()
        cfg_from_cfg(c)
        assert_and_infer_cfg()
        model = model_builder.create(cfg.MODEL.TYPE, train=True)
        workspace.ResetWorkspace()
        ws = workspace.GlobalWorkspace()
        for k, v in net_utils.synthetic_params(model, 3).items():
            ws.set_param(k, v)
        entry = synthetic.synthetic_roidb_entry(H, W, n_persons=3, seed=5)
        rng = np.random.RandomState(0)
        ws.FeedBlob('data', synthetic_clip(T, H, W))
        for k, v in rpn_data.add_rpn_blobs({}, 1.0, entry, rng).items():
            ws.FeedBlob(k, v)
        fixed = {}

        def sampler(rois, info, fixed=fixed, entry=entry, rng=rng):
            if not fixed:
                fixed.update(frcn_data.sample_training_blobs(entry, rois, info, rng))
            return fixed
        ws.train_sampler = sampler
        trainer = Trainer(model, ws)
        assert (trainer.flat_gt is not None) == defer
        ex = trainer.step(lr=0.0)
        torch.cuda.synchronize()
        flat[defer] = {n: trainer.arena[n].detach().clone() for n in trainer.trainable}
        if defer:
            used = [n for n in trainer.gt_arena if float(trainer.gt_arena[n].abs().max()) > 0]
            assert len(used) > 20 and any(n.startswith('conv_rpn') for n in used), used
    # (two bf16 iterations are not bit-reproducible even on ONE path: the fp32 atomics of RoIAlign's backward and of the K-split sums
    #  land in a different order, a bf16 gradient element then rounds the other way and the layers below see it -- a few 1e-3 of a
    #  gradient's maximum on single layers; a wrong transposition or scale in the finish would be O(1) on every deferred layer)
    errs = {}
    for n, ref in flat[False].items():
        got = flat[True][n]
        errs[n] = float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)
    worst = max(errs, key=errs.get)
    print('deferred vs immediate weight-gradient finish: median rel err %.2e, worst %.2e (%s) over %d parameters' % (
        float(np.median(list(errs.values()))), errs[worst], worst, len(errs)))
    assert np.median(list(errs.values())) < 2e-4 and errs[worst] < 2e-2, (worst, errs[worst])


@pytest.mark.parametrize('deconv', ['time_to_batch', 'grouped', 'group_ignored'])
def test_c4_tube_train_step_gradients_match_oracle_autograd(ops, deconv):
    """The shipped 3D configuration (configs/video/3d/04_R-18-3D_*.yaml) in TRAINING mode: tube RPN losses on the per-frame head
    (T-averaged logits), tube RoIAlign, per-RoI res5, T-averaged class scores, regrouped tube deltas, 3D keypoint head: all
    losses and the gradient of every trainable parameter vs autograd on the oracle.  deconv: the shipped time -> batch keypoint deconv
    and the reference default (time -> channels, group = T; model_builder.py:765-767, :848-868) in both readings of `group`."""
    from tests.model_util import c4_tube_kps_cfg, synthetic_clip
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import TrainExecutor
    from detectandtrack_amd.roi_data import rpn as rpn_data, fast_rcnn as frcn_data, synthetic
    from oracle import train_ref
    from oracle.net3d import opts_for
    T, H, W = 3, 96, 128
    c = c4_tube_kps_cfg(T=T, dtype='fp32', pre=200, post=60, deconv=deconv)
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 200, 'RPN_POST_NMS_TOP_N': 60, 'IMS_PER_BATCH': 1, 'MAX_SIZE': 128, 'BATCH_SIZE_PER_IM': 24,
                  'RPN_STRADDLE_THRESH': -1}
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
    entry = synthetic.synthetic_roidb_entry(H, W, n_persons=3, seed=4, T=T)
    rng = np.random.RandomState(0)
    labels = rpn_data.add_rpn_blobs({}, 1.0, entry, rng)
    data = synthetic_clip(T, H, W)
    ws.FeedBlob('data', data)
    for k, v in labels.items():
        ws.FeedBlob(k, v)
    fixed = {}

    def sampler(rois, info):
        if not fixed:
            fixed.update(frcn_data.sample_training_blobs(entry, rois, info, rng))
        return fixed
    ws.train_sampler = sampler
    ex = TrainExecutor(ws, model.net)
    ex.run()
    ex.backward()
    got = ex.loss_values()
    assert fixed['rois'].shape[1] == 4 * T + 1 and fixed['keypoint_locations_int32'].shape[0] == fixed['keypoint_rois'].shape[0] * 17 * T
    wt = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).requires_grad_(True) for k, v in weights.items()}
    ref = train_ref.training_losses_c4_tube(
        wt, opts_for('R18', block_counts=(2, 2, 2), kt_body=3, kt_rpn=3, kt_kps=3, body_head_link='', num_frames_mid=T,
                     kps_time_to_ch=deconv != 'time_to_batch'),
        data, labels, fixed, dict(num_gpus=1, kps_loss_weight=cfg.KRCNN.LOSS_WEIGHT))
    sum(ref.values()).backward()
    for k in sorted(ref):
        print('%-16s %.6f  (oracle %.6f)' % (k, got[k], ref[k].item()))
        np.testing.assert_allclose(got[k], ref[k].item(), rtol=2e-4, atol=1e-6)
    checked, worst, errs = 0, 0.0, []
    for name in sorted(set(model.TrainableParams())):
        if name.startswith(('conv1', 'res_conv1', 'res2_')):
            assert name not in ex.param_grads
            continue
        assert name in ex.param_grads, 'no gradient for ' + name
        r = wt[name].grad
        err = float((ex.param_grads[name].cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-8)
        # the keypoint branch's gradient is sparse (a few valid keypoints x 3 frames): a single activation within 1e-7 of
        # the ReLU threshold masked differently by the two fp32 summation orders moves a parameter's gradient by a few 1e-3
        assert err < (6e-2 if name.startswith(('conv_fcn', 'kps_score')) else 2e-3), '%s: rel err %.3e' % (name, err)
        errs.append((err, name))
        worst = max(worst, err)
        checked += 1
    print('checked gradients of %d parameters, worst rel err %.2e' % (checked, worst))
    print('largest:', ['%s %.1e' % (n, e) for e, n in sorted(errs, reverse=True)[:8]])
    assert checked > 30 and np.median([e for e, _ in errs]) < 1e-3


def _label_cfg(kind, max_size):
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    cfg.MODEL.KEYPOINTS_ON = True
    cfg.MODEL.NUM_CLASSES = 2
    cfg.KRCNN.NUM_KEYPOINTS, cfg.KRCNN.HEATMAP_SIZE = 17, 56
    cfg.TRAIN.MAX_SIZE, cfg.TRAIN.BATCH_SIZE_PER_IM = max_size, 64
    if kind == 'fpn':
        cfg.FPN.FPN_ON = cfg.FPN.MULTILEVEL_RPN = cfg.FPN.MULTILEVEL_ROIS = True
    return cfg


@pytest.mark.parametrize('kind,tube_T,h,w,persons,straddle', [
    ('fpn', 1, 200, 320, 3, 0), ('fpn', 1, 200, 320, 0, 0), ('fpn', 1, 768, 1344, 8, 0), ('fpn', 1, 256, 320, 70, -1),
    ('c4', 2, 200, 320, 4, 0), ('c4', 3, 240, 256, 5, -1)])
def test_device_anchor_labelling_is_bit_identical_to_the_host(ops, kind, tube_T, h, w, persons, straddle):
    """dat_anchor_overlaps (straddle filter + Cython-order IoU + arg-max + best-anchor flags over the whole field, up to
    ~450 k anchors at the bench size) against roi_data.rpn.anchor_overlap_stats — which is pinned to the real reference by
    tests/golden/reference_roi_data.npz — and, downstream, identical dense label blobs from the scatter path."""
    from detectandtrack_amd.core.config import reset_cfg
    from detectandtrack_amd.roi_data import loader, rpn, synthetic
    cfg = _label_cfg(kind, max(h, w))
    cfg.TRAIN.RPN_STRADDLE_THRESH = straddle
    entry = synthetic.synthetic_roidb_entry(h, w, n_persons=max(persons, 1), seed=9, T=tube_T)
    if persons == 0:
        for k in ('boxes', 'gt_classes', 'is_crowd', 'gt_keypoints', 'gt_overlaps', 'box_to_gt_ind_map', 'track_visible'):
            if k in entry:
                entry[k] = entry[k][:0]
    T, foas, names, im_h, im_w, gt, vis, im_info = loader._fields_and_gt(entry, 1.0)
    host = rpn.anchor_overlap_stats(rpn.all_field_anchors(foas), im_h, im_w, gt)
    dev = loader.device_overlap_stats(foas, im_h, im_w, gt, torch.device('cuda', 0))
    print('anchors', rpn.all_field_anchors(foas).shape, 'inside', len(host[0]), 'gts', len(gt), 'best', int(host[3].sum()))
    for name, a, b in zip(('inside', 'a2g_max', 'a2g_arg', 'best'), host, dev):
        np.testing.assert_array_equal(a, b, err_msg=name)
    # the whole minibatch on the device == the host path with the same RNG
    data = np.random.RandomState(1).randn(1, 3, 2, h, w).astype(np.float32)
    sp_h, per_level, _, _ = loader.label_clip_host(entry, 1.0, np.random.RandomState(4))
    sp_d, blobs, names_d = loader.label_clip_device(data, entry, 1.0, np.random.RandomState(4), torch.device('cuda', 0), {})
    assert names == names_d
    np.testing.assert_array_equal(sp_h.idx, sp_d.idx)
    np.testing.assert_array_equal(blobs['data'].cpu().numpy(), data)
    for lvl, suffix in zip(per_level, names):
        for k, v in lvl.items():
            got = blobs[k + suffix].cpu().numpy()
            assert got.dtype == v.dtype and got.shape == v.shape
            np.testing.assert_array_equal(got, v, err_msg=k + suffix)
    reset_cfg()


@pytest.mark.parametrize('device_sampling', [False, True])
def test_training_from_the_prefetching_loader_equals_synchronous_feeding(ops, device_sampling):
    """tools/train_net.py's two input paths: RoIDataLoader minibatches (device labels, worker streams, sparse loss
    normaliser) and the synchronous host rpn.add_rpn_blobs feed give the same losses for the same clips and RNG -- with the roi
    sampling of GenerateProposalLabels on the host (the reference's numpy.random stream) and on the device (cfg.HIP.DEVICE_ROI_SAMPLING:
    its counter-based draw is seeded from the minibatch's RNG on both paths)."""
    from tests.model_util import fpn3d_kps_cfg
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import Trainer
    from detectandtrack_amd.roi_data import rpn as rpn_data, fast_rcnn as frcn_data, synthetic
    from detectandtrack_amd.roi_data.loader import RoIDataLoader
    from tests.model_util import synthetic_clip
    T, H, W = 2, 128, 160
    c = fpn3d_kps_cfg('18', T=T, dtype='fp32')
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 400, 'RPN_POST_NMS_TOP_N': 200, 'IMS_PER_BATCH': 1, 'MAX_SIZE': 160,
                  'BATCH_SIZE_PER_IM': 64, 'RPN_STRADDLE_THRESH': 0}
    c['NUM_GPUS'] = 1
    c['HIP']['DEVICE_ROI_SAMPLING'] = bool(device_sampling)
    reset_cfg()
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    from detectandtrack_amd.roi_data.device_sampler import make_sampler, DeviceRoiSampler

    def source(i):
        return synthetic_clip(T, H, W) + np.float32(i), synthetic.synthetic_roidb_entry(H, W, n_persons=2 + i, seed=5 + i), 1.0

    def run(use_loader):
        model = model_builder.create(cfg.MODEL.TYPE, train=True)
        workspace.ResetWorkspace()
        ws = workspace.GlobalWorkspace()
        for k, v in net_utils.synthetic_params(model, 3).items():
            ws.set_param(k, v)
        trainer = Trainer(model, ws)
        loader = RoIDataLoader(source, num_items=3, num_workers=2, queue_size=2, device=torch.cuda.current_device(), seed=21)
        out = []
        try:
            for it in range(3):
                mb = loader.get_next_minibatch(timeout=120)
                if use_loader:
                    mb.feed(ws)
                else:   # same clip, same RNG seed, labelled synchronously on the host
                    data, entry, _ = source(loader._clip_index(it))
                    rng = np.random.RandomState((21 + 104729 * (it + 1)) % 2 ** 32)
                    ws.FeedBlob('data', data)
                    for k, v in rpn_data.add_rpn_blobs({}, 1.0, entry, rng).items():
                        ws.FeedBlob(k, v)
                    ws.train_sampler = make_sampler(entry, rng, seed=int(rng.randint(0, 2 ** 31 - 1)))
                assert isinstance(ws.train_sampler, DeviceRoiSampler) == bool(device_sampling)
                out.append(trainer.step(lr=0.001).loss_values())
        finally:
            loader.shutdown()
        return out
    a, b = run(True), run(False)
    for it, (la, lb) in enumerate(zip(a, b)):
        assert sorted(la) == sorted(lb)
        print('iteration %d: max |loader - synchronous| = %.3e' % (it, max(abs(la[k] - lb[k]) for k in la)))
        for k in la:
            assert np.isfinite(la[k])
            if it == 0:
                # identical weights, labels and RNG: equal up to the summation order of the fp32 atomics
                assert abs(la[k] - lb[k]) <= 1e-5 * max(1.0, abs(lb[k])), (it, k, la[k], lb[k])
        # later iterations start from weights that differ in the last bits (atomic order in the gradient kernels); a proposal
        # crossing an NMS / fg-bg threshold then changes the sampled rois, so only the RPN losses (fixed labels) stay tight
        if it > 0:
            for k in la:
                if k.startswith('loss_rpn'):
                    assert abs(la[k] - lb[k]) <= 5e-3 * max(1.0, abs(lb[k])), (it, k, la[k], lb[k])
            assert abs(sum(la.values()) - sum(lb.values())) <= 0.25 * abs(sum(lb.values())), (it, la, lb)
    reset_cfg()


def test_fpn_tube_train_step_gradients_match_oracle_autograd(ops):
    """The declared FPN tube-head extension in TRAINING mode: per-level tube RPN losses on heads over
    time-moved-to-channels, tube labels from roi_data, tube RoIAlign on the pyramid, fc6 over T*C*49, 3D keypoint head: every
    loss and the gradient of every trainable parameter vs autograd on the oracle (fp32 parity mode)."""
    from tests.model_util import fpn3d_tube_kps_cfg, synthetic_clip, oracle_opts
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import TrainExecutor
    from detectandtrack_amd.roi_data import rpn as rpn_data, fast_rcnn as frcn_data, synthetic
    from oracle import train_ref
    T, H, W = 2, 96, 128
    c = fpn3d_tube_kps_cfg(T=T, pre=200, post=60)
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 200, 'RPN_POST_NMS_TOP_N': 60, 'IMS_PER_BATCH': 1, 'MAX_SIZE': 128, 'BATCH_SIZE_PER_IM': 24,
                  'RPN_STRADDLE_THRESH': -1}
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
    entry = synthetic.synthetic_roidb_entry(H, W, n_persons=3, seed=4, T=T)
    rng = np.random.RandomState(0)
    labels = rpn_data.add_rpn_blobs({}, 1.0, entry, rng)
    assert labels['rpn_bbox_targets_wide_fpn3'].shape[1] == 3 * 4 * T
    data = synthetic_clip(T, H, W)
    ws.FeedBlob('data', data)
    for k, v in labels.items():
        ws.FeedBlob(k, v)
    fixed = {}

    def sampler(rois, info):
        if not fixed:
            fixed.update(frcn_data.sample_training_blobs(entry, rois, info, rng))
        return fixed
    ws.train_sampler = sampler
    ex = TrainExecutor(ws, model.net)
    ex.run()
    ex.backward()
    got = ex.loss_values()
    assert fixed['rois'].shape[1] == 4 * T + 1 and fixed['bbox_targets'].shape[1] == 2 * 4 * T
    wt = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).requires_grad_(True) for k, v in weights.items()}
    ref = train_ref.training_losses_fpn_tube(
        wt, oracle_opts('18', T, 3, '', 200, 60), data, labels, fixed,
        dict(num_gpus=1, rpn_batch=cfg.TRAIN.RPN_BATCH_SIZE_PER_IM, ims_per_batch=1, kps_loss_weight=cfg.KRCNN.LOSS_WEIGHT))
    sum(ref.values()).backward()
    for k in sorted(ref):
        print('%-22s %.6f  (oracle %.6f)' % (k, got[k], ref[k].item()))
        np.testing.assert_allclose(got[k], ref[k].item(), rtol=2e-4, atol=1e-6)
    checked, errs = 0, []
    for name in sorted(set(model.TrainableParams())):
        if name.startswith(('conv1', 'res_conv1', 'res2_')):
            assert name not in ex.param_grads
            continue
        assert name in ex.param_grads, 'no gradient for ' + name
        r = wt[name].grad
        assert r is not None, name
        err = float((ex.param_grads[name].cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-8)
        assert err < (6e-2 if name.startswith(('conv_fcn', 'kps_score')) else 2e-3), '%s: rel err %.3e' % (name, err)
        errs.append((err, name))
        checked += 1
    print('checked gradients of %d parameters, median rel err %.2e' % (checked, float(np.median([e for e, _ in errs]))))
    print('largest:', ['%s %.1e' % (n, e) for e, n in sorted(errs, reverse=True)[:6]])
    assert checked > 40 and np.median([e for e, _ in errs]) < 1e-3
    reset_cfg()



def test_allreduce_bucket_through_the_c_abi_world1():
    """dat_comm_unique_id / dat_comm_init_rank / dat_allreduce_bucket / dat_comm_destroy (RCCL loaded on first use): a one-rank
    communicator on the test GPU -- the sum over one rank is the identity, bucket by bucket, on the current stream.  (More ranks need
    more GPUs than a test box has; the bucketing protocol itself is covered by the gloo world-2 test on the CPU.)"""
    from detectandtrack_amd.ops import hip_ops as ops
    g = torch.Generator().manual_seed(3)
    flat = torch.randn(1000003, generator=g).cuda()
    want = flat.clone()
    red = ops.BucketAllReduce(0, 1)
    try:
        red.all_reduce(flat, 262144)
        torch.cuda.synchronize()
    finally:
        red.close()
    assert torch.equal(flat, want)


@pytest.mark.parametrize('k,win', [((3, 3, 3), (2, 1)), ((3, 3, 3), (0, 2)), ((1, 1, 1), (1, 2)), ((1, 3, 3), (3, 1))])
def test_direct_weight_gradient_over_a_frame_window(ops, k, win):
    """Round 3: the bf16 direct weight-gradient kernels (transposing LDS reads, no re-pack) with a gradient that is non-zero only in
    frames [t0, t0 + n) of the clip (the key-frame gradient of the FPN post-hoc convs, training.py bwd_Conv): the window launch must
    equal the full launch on the zero-embedded gradient and torch autograd."""
    cin, cout, T, H, W = 128, 192, 4, 17, 22
    pads = (k[0] // 2, k[1] // 2, k[2] // 2)
    g = torch.Generator().manual_seed(11)
    x = torch.randn((1, cin, T, H, W), generator=g).to(nm.h16()).float()
    w = torch.randn((cout, cin) + k, generator=g) * 0.05
    gy = torch.zeros((1, cout, T, H, W))
    t0, n = win
    gy[:, :, t0:t0 + n] = torch.randn((1, cout, n, H, W), generator=g).to(nm.h16()).float()
    wr = w.clone().requires_grad_(True)
    F.conv3d(x, wr, None, stride=1, padding=pads).backward(gy)
    xd, gd = _ndhwc(x, cin, nm.h16()), _ndhwc(gy, cout, nm.h16())
    cg = ops.ConvGrad(w.cuda(), None, (1, 1), pads, ops.BF16, cin, cout)
    full, _ = cg.weight(xd, gd, T)
    part, _ = cg.weight(xd, gd, T, g_frames=(t0, n))
    ref = wr.grad
    scale = float(ref.abs().max())
    assert float((full.cpu() - ref).abs().max()) < 2e-3 * scale
    assert float((part.cpu() - ref).abs().max()) < 2e-3 * scale
    assert float((part - full).abs().max()) < 1e-4 * scale      # (same products; the K split differs, fp32 sums in another order)
    # every element against float64 (tests/wgrad_refs.py): the full launch reduces all T frames (g is zero outside the window: same
    # reference, same |x| |g| sum), the window launch n of them
    ref64, absref, K = wgrad_ref64(x, gy, None, k, 1, pads, window=(t0, n))
    nm.assert_elementwise(full.cpu(), ref64, absref, gy.numel() // cout, 'fp32', 'dW, full launch')
    nm.assert_elementwise(part.cpu(), ref64, absref, K, 'fp32', 'dW, window launch')


@pytest.mark.parametrize('T,n_props,n_persons,jitter', [(1, 2000, 8, 400), (1, 300, 3, 20), (2, 1000, 5, 200), (1, 2000, 8, 0), (1, 0, 4, 0)])
def test_device_roi_sampling_matches_the_reference_semantics(ops, T, n_props, n_persons, jitter):
    """GenerateProposalLabels as one device kernel (dat_sample_rois; roi_data/device_sampler.py) against the host
    restatement that is pinned to the REAL reference (roi_data/fast_rcnn.py, tests/golden/reference_roi_data.npz).  The contract, checked
    piece by piece:  (1) the candidate sets -- foreground, background, keypoint-foreground -- and the counts n_fg / n_bg / n_kp are the
    reference's;  (2) the draw is "the n members of the set with the smallest (roi_key, index)", in that order (the host mirror
    ops.roi_key reproduces every picked row), NOT NumPy's Mersenne-Twister stream;  (3) for the picked rows, rois / labels / box targets /
    weights / keypoint rois / heatmap cells / keypoint weights are what the host code computes for the same rows (targets to float32
    rounding of log, everything else exact);  (4) different iterations draw different subsets of the same sets."""
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.roi_data import fast_rcnn as frcn, synthetic
    from detectandtrack_amd.roi_data.device_sampler import DeviceRoiSampler
    from tests.model_util import fpn3d_kps_cfg
    reset_cfg()
    cfg_from_cfg(fpn3d_kps_cfg('18', T=max(T, 2), dtype='fp32'))
    assert_and_infer_cfg()
    H, W, scale = 720, 1280, 1.0414
    rs = np.random.RandomState(17 + n_props + T)
    entry = synthetic.synthetic_roidb_entry(H, W, n_persons=n_persons, seed=5, T=T)
    # proposals at NETWORK scale: random boxes + jittered copies of the gt boxes (so that some are foreground), tubes repeat the jitter
    x1, y1 = rs.uniform(0, W * 0.8, n_props), rs.uniform(0, H * 0.8, n_props)
    bw, bh = rs.uniform(20, W * 0.5, n_props), rs.uniform(20, H * 0.6, n_props)
    boxes = np.stack([x1, y1, np.minimum(x1 + bw, W - 1), np.minimum(y1 + bh, H - 1)], 1)
    boxes = np.tile(boxes, (1, T))
    for k in range(min(jitter, n_props)):
        g = entry['boxes'][k % n_persons] + np.tile(rs.uniform(-25, 25, 4), T) * (1 + (k % 3))
        boxes[k] = g
    props = np.hstack((np.zeros((n_props, 1)), boxes * scale)).astype(np.float32)
    cap = max(n_props, 1) + 7                                                   # rows past the device count are never read
    props_dev = torch.zeros((cap, 4 * T + 1), dtype=torch.float32, device='cuda')
    props_dev[:n_props] = torch.from_numpy(props).cuda()
    props_dev[n_props:] = 1e6
    n_dev = torch.tensor([n_props], dtype=torch.int32, device='cuda')
    im_info = np.array([[H * scale, W * scale, scale]], np.float32)
    per_im = int(cfg.TRAIN.BATCH_SIZE_PER_IM)
    fg_per_im = int(np.round(cfg.TRAIN.FG_FRACTION * per_im))
    sampler = DeviceRoiSampler(entry, seed=0x1234567890abcdef)
    # ---- host side: the merged entry and the reference's candidate sets
    e = frcn.merge_proposals_into_entry(entry, props[:, 1:] / np.float32(scale))
    mo = e['max_overlaps']
    fg = np.where(mo >= cfg.TRAIN.FG_THRESH)[0]
    bg = np.where((mo < cfg.TRAIN.BG_THRESH_HI) & (mo >= cfg.TRAIN.BG_THRESH_LO))[0]
    kpc = frcn.keypoint_fg_candidates(e)
    n_fg = min(fg_per_im, fg.size)
    n_bg = min(per_im - n_fg, bg.size)
    n_kp = min(fg_per_im, kpc.size) if kpc.size else n_persons
    seen = []
    for it in range(3):
        got = sampler(props_dev, n_dev, im_info, want_picked=True)
        c = sampler.last_counts
        assert (int(c[3]), int(c[4]), int(c[5])) == (fg.size, bg.size, kpc.size), (c, fg.size, bg.size, kpc.size)      # (1) the sets
        assert (int(c[1]), int(c[0]) - int(c[1]), int(c[2])) == (n_fg, n_bg, n_kp)
        picked = got['picked'].cpu().numpy()
        N = e['boxes'].shape[0]

        def draw(cands, n, stream):
            keys = ops.roi_key(0x1234567890abcdef, it, stream, np.arange(N))
            order = sorted(cands.tolist(), key=lambda i: (int(keys[i]), i))
            return np.asarray(order[:n], dtype=np.int64)
        keep = np.append(draw(fg, n_fg, 0), draw(bg, n_bg, 0))
        np.testing.assert_array_equal(picked[:n_fg + n_bg], keep)                                                    # (2) the draw
        kp_keep = draw(kpc, n_kp, 1) if kpc.size else np.arange(n_persons)
        np.testing.assert_array_equal(picked[per_im:per_im + n_kp], kp_keep)
        assert np.all(picked[n_fg + n_bg:per_im] == -1) and np.all(picked[per_im + n_kp:] == -1)
        want = frcn.roi_blobs_for(e, keep, n_fg, scale, 0)                                                           # (3) the rows
        frcn.keypoint_blobs_for(want, e, kp_keep, scale, 0)
        for name in ('rois', 'labels_int32', 'bbox_inside_weights', 'bbox_outside_weights', 'keypoint_rois', 'keypoint_locations_int32',
                     'keypoint_weights'):
            g_ = got[name].cpu().numpy()
            assert g_.shape == want[name].shape, (name, g_.shape, want[name].shape)
            if name.endswith('rois'):
                np.testing.assert_allclose(g_, want[name], rtol=0, atol=1e-4, err_msg=name)     # (p / s) * s in float32 on both sides
            else:
                np.testing.assert_array_equal(g_, want[name], err_msg=name)
        np.testing.assert_allclose(got['bbox_targets'].cpu().numpy(), want['bbox_targets'], rtol=1e-5, atol=2e-6)
        assert got['keypoint_weights_sum'] == float(want['keypoint_weights'].sum())
        if n_fg:
            assert np.all(got['labels_int32'].cpu().numpy()[:n_fg] == 1) and np.all(got['labels_int32'].cpu().numpy()[n_fg:] == 0)
        seen.append(tuple(keep.tolist()))
    if bg.size > n_bg + 5:
        assert len(set(seen)) == 3                                                                                   # (4) a new draw per iteration


def test_device_roi_sampling_is_uniform_without_replacement(ops):
    """The draw key is a hash, not a proven generator: check what the contract promises -- over 400 iterations every one of 40
    foreground candidates is picked with frequency n / |S| = 1 / 4 (5-sigma band of the binomial), no roi twice in one draw."""
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.roi_data import synthetic
    from detectandtrack_amd.roi_data.device_sampler import DeviceRoiSampler
    from tests.model_util import fpn3d_kps_cfg
    c = fpn3d_kps_cfg('18', T=2, dtype='fp32')
    c['TRAIN'] = dict(c.get('TRAIN', {}), BATCH_SIZE_PER_IM=40, FG_FRACTION=0.25)
    reset_cfg()
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    entry = synthetic.synthetic_roidb_entry(720, 1280, n_persons=4, seed=2, T=1)
    rs = np.random.RandomState(0)
    boxes = np.concatenate([entry['boxes'][k % 4][None] + rs.uniform(-6, 6, (1, 4)) for k in range(36)]).astype(np.float32)   # 36 fg proposals + 4 gts
    props = torch.from_numpy(np.hstack((np.zeros((36, 1), np.float32), boxes))).cuda()
    n_dev = torch.tensor([36], dtype=torch.int32, device='cuda')
    sampler = DeviceRoiSampler(entry, seed=99)
    hits = np.zeros(40)
    for it in range(400):
        got = sampler(props, n_dev, np.array([[720, 1280, 1.0]], np.float32), want_picked=True)
        c_ = sampler.last_counts
        assert int(c_[3]) == 40 and int(c_[1]) == 10
        pk = got['picked'].cpu().numpy()[:10]
        assert len(set(pk.tolist())) == 10
        hits[pk] += 1
    p, n = 0.25, 400
    assert np.all(np.abs(hits - n * p) < 5 * np.sqrt(n * p * (1 - p))), hits


def test_training_iteration_with_the_device_roi_sampler_equals_the_host_path_on_the_same_draw(ops):
    """A whole training iteration (forward, 13 losses, backward) with roi_data.device_sampler.DeviceRoiSampler -- the proposals never
    leave the GPU -- against the host path (proposals -> host -> roi_data.fast_rcnn -> uploads) FORCED to the rows the device drew:
    every loss equal to 1e-5, every trainable gradient to the float-atomic noise of the weight-gradient kernels.  Also checks what the
    device path is for: no proposals cross to the host (the sampler is handed device tensors and returns device tensors)."""
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.roi_data import fast_rcnn as frcn, rpn as rpn_data, synthetic
    from detectandtrack_amd.roi_data.device_sampler import DeviceRoiSampler
    from detectandtrack_amd.training import Trainer
    from tests.model_util import synthetic_clip
    T, H, W = 2, 128, 160
    _ddp_model(1)                                       # (the synthetic entry reads cfg: configure first)
    entry = synthetic.synthetic_roidb_entry(H, W, n_persons=3, seed=5)
    data = synthetic_clip(T, H, W, seed=3)

    def run(make_sampler):
        model, ws = _ddp_model(1)
        ws.FeedBlob('data', data)
        for k, v in rpn_data.add_rpn_blobs({}, 1.0, entry, np.random.RandomState(0)).items():
            ws.FeedBlob(k, v)
        ws.train_sampler = make_sampler()
        tr = Trainer(model, ws)
        ex = tr.step(0.0)
        torch.cuda.synchronize()
        return {k: float(v) for k, v in ex.loss_values().items()}, {n: tr.arena[n].clone() for n in tr.trainable}
    record = {}

    class Recording(DeviceRoiSampler):
        def __call__(self, rois_dev, n_dev, im_info, want_picked=False):
            assert rois_dev.is_cuda and n_dev.is_cuda
            out = DeviceRoiSampler.__call__(self, rois_dev, n_dev, im_info, want_picked=True)
            record.update(rois=rois_dev[:int(n_dev.view(-1)[0])].cpu().numpy(), picked=out['picked'].cpu().numpy(), counts=self.last_counts.copy())
            assert all(v.is_cuda for k, v in out.items() if hasattr(v, 'is_cuda'))
            return out
    dev_losses, dev_grads = run(lambda: Recording(entry, seed=7))
    per_im = int(cfg.TRAIN.BATCH_SIZE_PER_IM)

    def forced():
        def sampler(rois, info):
            np.testing.assert_array_equal(rois, record['rois'])           # the same proposals reach the host path
            scale = float(info[0, 2])
            e = frcn.merge_proposals_into_entry(entry, rois[:, 1:] / scale)
            n, n_fg, m = int(record['counts'][0]), int(record['counts'][1]), int(record['counts'][2])
            blobs = frcn.roi_blobs_for(e, record['picked'][:n].astype(np.int64), n_fg, scale, 0)
            frcn.keypoint_blobs_for(blobs, e, record['picked'][per_im:per_im + m].astype(np.int64), scale, 0)
            return blobs
        return sampler
    host_losses, host_grads = run(forced)
    assert sorted(dev_losses) == sorted(host_losses) and len(dev_losses) >= 10
    for k in dev_losses:
        np.testing.assert_allclose(dev_losses[k], host_losses[k], rtol=1e-5, atol=1e-7, err_msg=k)
    live = 0
    for n_, g in dev_grads.items():
        mx = float(host_grads[n_].abs().max())
        if mx == 0.0:
            continue
        live += 1
        assert float((g - host_grads[n_]).abs().max()) <= 2e-4 * mx + 1e-9, n_
    assert live > 40


@pytest.mark.parametrize('cin,cout,T,H,W', [(64, 70, 3, 9, 11), (130, 200, 2, 17, 13), (128, 64, 5, 8, 8)])
def test_nine_tap_weight_gradient_variants_agree(ops, monkeypatch, cin, cout, T, H, W):
    """the default path of the nine-tap weight-gradient kernel -- eight-wave blocks with two K ranges (DAT_WGRAD_SUB=2) --
    against the four-wave variant on shapes that make the sub-ranges UNEQUAL (odd chunk counts), channel counts that are not multiples of 64, a forced two-range split (ks = 2: plain stores, no atomics) and a
    larger forced split: the same gradient to the fp32 summation order, and torch autograd."""
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn((1, cin, T, H, W), generator=g).to(nm.h16()).float()
    w = torch.randn((cout, cin, 3, 3, 3), generator=g) * 0.05
    gy = torch.randn((1, cout, T, H, W), generator=g).to(nm.h16()).float()
    wr = w.clone().requires_grad_(True)
    F.conv3d(x, wr, None, stride=1, padding=1).backward(gy)
    ref = wr.grad
    mx = float(ref.abs().max())
    cs_x, cs_g = ops.round_up(cin, 64), ops.round_up(cout, 64)
    xd, gd = _ndhwc(x, cs_x, nm.h16()), _ndhwc(gy, cs_g, nm.h16())
    outs = {}
    for name, env in (('sub2', {}), ('sub1', {'DAT_WGRAD_SUB': '1'}), ('sub2 ks2', {'DAT_WGRAD_KS': '2'}),
                      ('sub2 ks6', {'DAT_WGRAD_KS': '6'}), ('sub1 ks5', {'DAT_WGRAD_SUB': '1', 'DAT_WGRAD_KS': '5'})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ops.drop_ctx()
        cg = ops.ConvGrad(w.cuda(), None, (1, 1), (1, 1, 1), ops.BF16, cs_x, cs_g)
        outs[name] = cg.weight(xd, gd, T)[0].cpu()
        for k in env:
            monkeypatch.delenv(k)
    ops.drop_ctx()
    ref64, absref, K = wgrad_ref64(x, gy, None, (3, 3, 3), 1, (1, 1, 1))
    for name, o in outs.items():
        assert float((o - ref).abs().max()) < 2e-3 * mx, name
        assert float((o - outs['sub2']).abs().max()) < 2e-5 * mx, name
        nm.assert_elementwise(o, ref64, absref, K, 'fp32', 'dW ' + name)       # every element against float64 (tests/wgrad_refs.py)


@pytest.mark.parametrize('sampling,pooled', [(2, 7), (2, 14), (0, 7)])
def test_roi_align_backward_fold_equals_the_per_sample_scatter(ops, monkeypatch, sampling, pooled):
    """DAT_ROI_BWD_FOLD=1 (a bin's samples folded into one weight per distinct pixel before the atomics, the default) against
    the per-sample scatter (=0) on rois that overlap, leave the map, are smaller than a bin, and -- sampling 0 -- use the adaptive grid
    (bins of more than four samples take the per-sample path inside the folded kernel): the same fp32 maps to the atomic summation order."""
    rs = np.random.RandomState(4)
    R, C = 40, 64
    feats_hw = [(32, 48), (16, 24)]
    rois = np.zeros((R, 5), np.float32)
    x1, y1 = rs.uniform(-20, 150, R), rs.uniform(-20, 100, R)
    rois[:, 1], rois[:, 2] = x1, y1
    rois[:, 3], rois[:, 4] = x1 + rs.uniform(0.5, 160, R), y1 + rs.uniform(0.5, 110, R)
    rois[:5, 3:] = rois[:5, 1:3] + 0.3                                        # smaller than one bin
    dout = torch.from_numpy(rs.randn(R, pooled, pooled, C).astype(np.float32)).cuda()
    outs = []
    for fold in ('1', '0'):
        monkeypatch.setenv('DAT_ROI_BWD_FOLD', fold)
        ops.drop_ctx()
        maps = [torch.zeros((1, h, w, C), dtype=torch.float32, device='cuda') for h, w in feats_hw]
        ops.roi_align_bwd(maps, [0.25, 0.125], ops.F32, torch.from_numpy(rois).cuda(), dout, T=1, Tr=1, t0=0, pooled=pooled, sampling=sampling)
        torch.cuda.synchronize()
        outs.append([m.cpu() for m in maps])
    monkeypatch.delenv('DAT_ROI_BWD_FOLD')
    ops.drop_ctx()
    for a, b in zip(*outs):
        mx = float(b.abs().max())
        assert mx > 0 and float((a - b).abs().max()) < 1e-5 * mx


PW_CASES = [
    # cin, cout, stride, N, T, H, W, window        (the tile shape the launcher picks: 128 x 512 / 256 x 256 / 512 x 128 co x ci)
    (512, 128, 1, 1, 2, 13, 19, None),             # res3 branch2a: one 128 x 512 tile
    (128, 512, 1, 1, 2, 13, 19, None),             # res3 branch2c: one 512 x 128 tile
    (256, 256, 1, 1, 3, 11, 13, (1, 1)),           # P2 lateral shape with a one-frame gradient window
    (1024, 256, 1, 1, 2, 6, 7, None),              # res4 branch2a: 256 x 256 tiles, four ci tiles
    (256, 512, 2, 1, 2, 12, 16, None),             # res3_0 shortcut: stride 2
    (256, 128, 2, 2, 2, 9, 11, None),              # stride 2 on odd map sizes, two clips
    (256, 15, 1, 1, 1, 20, 28, None),              # RPN head: Cout not a multiple of anything
    (200, 70, 1, 1, 2, 7, 9, None),                # both channel counts ragged (strides 256 / 128)
    (64, 8, 1, 1, 1, 1, 37, None),                 # FC geometry: a 1 x R strip, fewer positions than two chunks
    (640, 320, 1, 1, 1, 1, 3, None),               # three positions: every block range shorter than the pipeline depth
]


@pytest.mark.parametrize('acc', [False, True])
@pytest.mark.parametrize('case', PW_CASES)
def test_pointwise_weight_gradient_kernel(ops, monkeypatch, case, acc):
    """Round 5: wgrad_pw_kernel -- the eight-wave, 64 K-accumulator weight-gradient kernel of the pointwise layers
    (1 x 1 x 1 convs, FC; LDS-DMA panels, three stages, transposing LDS reads) -- against torch autograd on bf16-rounded operands, through
    dat_conv3d_wgrad (immediate finish, AffineChannelNd scale folded) and dat_conv3d_wgrad_acc (deferred finish: raw [Cout][Cin] sums
    added into the caller's accumulator), and against the 128 x 128 per-tap kernel it replaces (DAT_WGRAD_PW=0): same products, another
    summation order.  Reference semantics: the ConvGradient of every ConvNd, lib/modeling/model_builder.py:908-951."""
    cin, cout, st, N, T, H, W, win = case
    g = torch.Generator().manual_seed(cin + 3 * cout)
    x = torch.randn((N, cin, T, H, W), generator=g).to(nm.h16()).float()
    w = torch.randn((cout, cin, 1, 1, 1), generator=g) * 0.05
    scale = torch.rand(cout, generator=g) + 0.5
    Ho, Wo = (H - 1) // st + 1, (W - 1) // st + 1
    gy = torch.randn((N, cout, T, Ho, Wo), generator=g).to(nm.h16()).float()
    if win is not None:
        t0, n = win
        keep = torch.zeros_like(gy)
        keep[:, :, t0:t0 + n] = gy[:, :, t0:t0 + n]
        gy = keep
    wr = w.clone().requires_grad_(True)
    (F.conv3d(x, wr, None, stride=(1, st, st)) * scale.view(1, -1, 1, 1, 1)).backward(gy)
    ref = wr.grad
    mx = float(ref.abs().max())
    cs_x, cs_g = ops.round_up(cin, 64), ops.round_up(cout, 64)
    xd, gd = _ndhwc(x, cs_x, nm.h16()), _ndhwc(gy, cs_g, nm.h16())

    def run():
        ops.drop_ctx()                                  # a context made under the current environment
        cg = ops.ConvGrad(w.cuda(), scale.cuda(), (st, st), (0, 0, 0), ops.BF16, cs_x, cs_g)
        if not acc:
            return cg.weight(xd, gd, T, g_frames=win)[0].cpu()
        gt = torch.zeros(cout * cin, dtype=torch.float32, device='cuda')
        assert cg.weight_acc(xd, gd, T, gt, g_frames=win)
        assert cg.weight_acc(xd, gd, T, gt, g_frames=win)              # adds: twice the raw sum
        return (gt.view(cout, cin, 1, 1, 1) * 0.5 * scale.cuda().view(-1, 1, 1, 1, 1)).cpu()
    new = run()
    assert float((new - ref).abs().max()) < 2e-3 * mx, float((new - ref).abs().max()) / mx
    # every element against float64 (tests/wgrad_refs.py).  acc: twice the raw sum, halved (exact) and scaled (one fp32 rounding)
    ref64, absref, K = wgrad_ref64(x, gy, scale, (1, 1, 1), st, (0, 0, 0), window=win)
    nm.assert_elementwise(new, ref64, absref, K, 'fp32', 'dW')
    monkeypatch.setenv('DAT_WGRAD_PW', '0')
    old = run()
    monkeypatch.delenv('DAT_WGRAD_PW')
    assert float((new - old).abs().max()) < 2e-5 * mx + 1e-6
    for forced in ('10', '20', '40'):                   # every tile shape on every layer shape (128 x 512, 256 x 256, 512 x 128)
        monkeypatch.setenv('DAT_WGRAD_PW', forced)
        other = run()
        assert float((other - old).abs().max()) < 2e-5 * mx + 1e-6, forced
    monkeypatch.delenv('DAT_WGRAD_PW')
    ops.drop_ctx()


def test_pointwise_weight_gradient_batch_equals_the_single_launches(ops):
    """dat_conv3d_wgrad_acc_batch: the pointwise layers of PW_CASES (+ one 3 x 3 x 3 layer, which the call runs on its own kernel) queued
    and executed as grouped launches -- both tile classes, stride 1 and 2, a frame window, ragged channel counts, layers shorter than one
    block's pipeline -- must leave in every accumulator what one dat_conv3d_wgrad_acc call per layer leaves (same products; the K ranges
    differ, so fp32 sums in another order), twice in a row (the accumulators add)."""
    jobs, singles, keep, refs = [], [], [], []
    for k, (cin, cout, st, N, T, H, W, win) in enumerate(PW_CASES + [(64, 128, 1, 1, 3, 12, 14, None)]):
        ker = (3, 3, 3) if k == len(PW_CASES) else (1, 1, 1)
        pads = tuple(v // 2 for v in ker)
        g = torch.Generator().manual_seed(100 + k)
        x = torch.randn((N, cin, T, H, W), generator=g).to(nm.h16()).float()
        Ho, Wo = (H + 2 * pads[1] - ker[1]) // st + 1, (W + 2 * pads[2] - ker[2]) // st + 1
        gy = torch.randn((N, cout, T, Ho, Wo), generator=g).to(nm.h16()).float()
        if win is not None:
            keep_ = torch.zeros_like(gy)
            keep_[:, :, win[0]:win[0] + win[1]] = gy[:, :, win[0]:win[0] + win[1]]
            gy = keep_
        cs_x, cs_g = ops.round_up(cin, 64), ops.round_up(cout, 64)
        xd, gd = _ndhwc(x, cs_x, nm.h16()), _ndhwc(gy, cs_g, nm.h16())
        w = torch.zeros((cout, cin) + ker, device='cuda')
        cg = ops.ConvGrad(w, None, (st, st), pads, ops.BF16, cs_x, cs_g)
        assert cg.pointwise == (ker == (1, 1, 1))
        gt_b = torch.zeros(w.numel(), dtype=torch.float32, device='cuda')
        gt_s = torch.zeros_like(gt_b)
        job = cg.weight_acc_job(xd, gd, T, gt_b, g_frames=win)
        assert job is not None
        jobs.append(job)
        singles.append((cg, xd, gd, T, gt_s, win))
        keep.append((gt_b, gt_s))
        refs.append(wgrad_ref64(x, gy, None, ker, st, pads, window=win))
    for rep in range(2):
        ops.wgrad_acc_batch(jobs)
        for cg, xd, gd, T, gt_s, win in singles:
            assert cg.weight_acc(xd, gd, T, gt_s, g_frames=win)
    torch.cuda.synchronize()
    for k, (gt_b, gt_s) in enumerate(keep):
        mx = float(gt_s.abs().max())
        assert mx > 0
        assert float((gt_b - gt_s).abs().max()) < 2e-5 * mx, (k, float((gt_b - gt_s).abs().max()) / mx)
        # every element of both accumulators ([tap][Cout][Cin], two additions of the raw sum) against float64 (tests/wgrad_refs.py)
        ref64, absref, K = refs[k]
        cout, cin = ref64.shape[:2]
        for what, gt in (('grouped', gt_b), ('single', gt_s)):
            got = gt.view(-1, cout, cin).permute(1, 2, 0).reshape(ref64.shape).cpu()
            nm.assert_elementwise(got, 2 * ref64, 2 * absref, K, 'fp32', 'layer %d, %s launches' % (k, what))


# ---- two ranks (VERDICT r3 item 4 / missing #3) ---------------------------------------------------------------------------------------
def _ddp_model(num_gpus, dtype='fp32', T=2, H=128, W=160):
    from tests.model_util import fpn3d_kps_cfg
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    c = fpn3d_kps_cfg('18', T=T, dtype=dtype)
    c['TRAIN'] = {'RPN_PRE_NMS_TOP_N': 400, 'RPN_POST_NMS_TOP_N': 200, 'IMS_PER_BATCH': 1, 'MAX_SIZE': W,
                  'BATCH_SIZE_PER_IM': 64, 'RPN_STRADDLE_THRESH': -1}
    c['NUM_GPUS'] = num_gpus            # the losses carry 1 / NUM_GPUS (reference model_builder.py:484,625,884)
    reset_cfg()
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    model = model_builder.create(cfg.MODEL.TYPE, train=True)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    for k, v in net_utils.synthetic_params(model, 3).items():
        ws.set_param(k, v)
    return model, ws


def _ddp_clip(k, T=2, H=128, W=160):
    """clip k of the job: data, RPN labels and a sampler that fixes its Fast R-CNN sample on first use (both runs then optimise the same objective)"""
    from tests.model_util import synthetic_clip
    from detectandtrack_amd.roi_data import rpn as rpn_data, fast_rcnn as frcn_data, synthetic
    entry = synthetic.synthetic_roidb_entry(H, W, n_persons=3, seed=5 + k)
    rng = np.random.RandomState(k)
    blobs = rpn_data.add_rpn_blobs({}, 1.0, entry, rng)
    fixed = {}

    def sampler(rois, info):
        if not fixed:
            fixed.update(frcn_data.sample_training_blobs(entry, rois, info, rng))
        return fixed
    return synthetic_clip(T, H, W, seed=3 + k), blobs, sampler


def _ddp_feed(ws, clip):
    data, blobs, sampler = clip
    ws.FeedBlob('data', data)
    for k, v in blobs.items():
        ws.FeedBlob(k, v)
    ws.train_sampler = sampler


def _ddp_worker(rank, world, port, out, overlap, backend='gloo', direct=False):
    import os
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch
    import torch.distributed as dist
    # gloo: both ranks share the one GPU of the test box (host-staged buckets); nccl (= RCCL): one device per rank
    torch.cuda.set_device(rank if backend == 'nccl' else 0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.training import Trainer
    model, ws = _ddp_model(world)
    cfg.HIP.OVERLAP_ALLREDUCE = bool(overlap)
    cfg.HIP.RCCL_DIRECT = bool(direct)
    _ddp_feed(ws, _ddp_clip(rank))
    tr = Trainer(model, ws, dist)
    losses = []
    for _ in range(2):
        ex = tr.step(0.01)
        losses.append(sum(ex.loss_values().values()))
    np.savez(out % rank, order=np.array(tr.exchange.order), buckets=np.array([(lo, hi) for lo, hi, _ in tr.buckets]), losses=np.array(losses),
             **{'w_' + n: ws.dev_param(n).cpu().numpy() for n in tr.trainable})
    dist.barrier()
    dist.destroy_process_group()


def _check_two_ranks_against_one(out, min_buckets=2):
    """The assertions of the two-rank tests: both ranks end with identical weights that are (to the float-atomic noise of the
    weight-gradient kernels) those of ONE rank accumulating both clips per iteration with the same 1 / NUM_GPUS scaling."""
    from detectandtrack_amd.training import Trainer
    r0, r1 = np.load(out % 0), np.load(out % 1)
    model, ws = _ddp_model(2)
    clips = [_ddp_clip(0), _ddp_clip(1)]
    tr = Trainer(model, ws)
    ref_losses = []
    for _ in range(2):
        _ddp_feed(ws, clips[0])
        ex0 = tr.step(0.01, update=False)
        _ddp_feed(ws, clips[1])
        ex1 = tr.step(0.01, zero_grad=False)
        ref_losses.append((sum(ex0.loss_values().values()), sum(ex1.loss_values().values())))
    assert len(r0['buckets']) >= min_buckets
    assert list(r0['order']) == list(range(len(r0['buckets']))) == list(r1['order'])
    for it in range(2):
        np.testing.assert_allclose(r0['losses'][it], ref_losses[it][0], rtol=2e-4)
        np.testing.assert_allclose(r1['losses'][it], ref_losses[it][1], rtol=2e-4)
    moved = 0
    for n in tr.trainable:
        a, b, ref = r0['w_' + n], r1['w_' + n], ws.dev_param(n).cpu().numpy()
        np.testing.assert_array_equal(a, b, err_msg=n)
        step = float(np.abs(ref - ws.params[n]).max())
        tol = 0.05 * step + 2e-6 * max(1.0, float(np.abs(ref).max()))      # (see the gloo test below for why 5 % of the update)
        assert float(np.abs(a - ref).max()) <= tol, (n, float(np.abs(a - ref).max()), tol, step)
        moved += int(not n.startswith(('conv1', 'res2')) and step > 0)
    assert moved > 40


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='RCCL needs one device per rank: arms itself on a box with >= 2 GPUs')
@pytest.mark.parametrize('direct', [False, True])
def test_two_ranks_nccl(tmp_path, direct):
    """VERDICT r4 item 8 -- the first evidence of RCCL with N > 1 ranks the moment a multi-GPU node runs this suite: two processes on
    devices 0 / 1, backend `nccl` (= RCCL over xGMI), the overlapped bucket exchange through torch.distributed (direct=False) and
    through the C ABI's dat_allreduce_bucket (cfg.HIP.RCCL_DIRECT), with the assertions of the gloo test below: identical weights on
    both ranks = those of one rank over both clips.  Reference: lib/modeling/model_builder.py:931-942 (NCCLAllreduce / muji.Allreduce
    of every gradient blob).  Skipped on one-GPU boxes (RCCL refuses two ranks on one device)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    port = 29500 + ((os.getpid() + 131 + int(direct)) % 1000)
    out = str(tmp_path / 'rank%d.npz')
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, out, True, 'nccl', direct)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=900)
        assert p.exitcode == 0
    _check_two_ranks_against_one(out)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='arms itself on a box with >= 2 GPUs')
@pytest.mark.parametrize('mode', ['infer', 'train'])
def test_bench_two_gpus_smoke(mode):
    """`python bench.py --gpus 2 --steps 5` as the driver runs it (the script re-executes itself under torch.distributed.run with two
    ranks): one JSON line with n_gpus 2, two distinct devices in ranks_seen, and -- in training mode -- a real RCCL exchange
    (allreduce_ms > 0 over >= 2 buckets)."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    env['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
    cmd = [sys.executable, os.path.join(repo, 'bench.py'), '--gpus', '2', '--steps', '5', '--warmup', '2', '--full', '--no-cpu-baseline',
           '--no-accuracy', '--no-other-configs', '--h2d', '0'] + (['--mode', 'train'] if mode == 'train' else [])
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    line = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert line['n_gpus'] == 2 and len(line['ranks_seen']) == 2 and line['value'] > 0
    assert len({(r.get('device'), r.get('pci')) for r in line['ranks_seen']}) == 2
    if mode == 'train':
        assert line['allreduce']['backend'] == 'nccl' and line['allreduce']['allreduce_ms'] > 0 and line['allreduce']['buckets'] >= 2


@pytest.mark.parametrize('mode', ['infer', 'train'])
def test_bench_two_ranks_control_flow_on_one_gpu(mode):
    """The driver's multi-GPU command line -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N --steps K --warmup W` -- with N = 2 ranks SHARING this box's one GPU over gloo
    (DAT_BENCH_SHARE_GPU=1, a test-only switch: RCCL needs a device per rank): every barrier, the MAX-reduce of the timing, the
    rank-0-only roofline passes, the host-frame leg and (train) the bucketed gradient exchange run with two real processes, rank 0
    prints ONE line with n_gpus 2 that marks itself as a control-flow test.  What only a multi-GPU node can show -- RCCL itself -- is
    test_two_ranks_nccl / test_bench_two_gpus_smoke, which arm themselves there."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(DAT_BENCH_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    port = 29500 + ((os.getpid() + 211 + (mode == 'train')) % 1000)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(repo, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1', '--full', '--no-accuracy'] + (['--mode', 'train'] if mode == 'train' else [])
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith('{')]
    assert len(lines) == 1, lines                      # rank 0 only
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and len(line['ranks_seen']) == 2 and {r['rank'] for r in line['ranks_seen']} == {0, 1}
    assert 'shared_gpu_test' in line and line['value'] > 0 and line['steps'] == 3 and line['scaling'] == 'weak'
    assert 'cpu_baseline' not in line                  # CPU baselines are timed at N = 1 only
    if mode == 'train':
        assert line['allreduce']['buckets'] >= 2 and line['allreduce']['backend'] == 'gloo'
    else:
        assert line['roofline']['frac'] > 0 and line['host_frames']['value_including_upload'] > 0


def test_bench_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: one line with the contract fields and exactly K
    timed steps, none of the --full measurements, and the last step's per-clip boxes / keypoint rows as float32 .npy files -- the same
    arrays from a second run with the same arguments."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    dumps = []
    for run in range(2):
        d = str(tmp_path / ('run%d' % run))
        cmd = [sys.executable, os.path.join(repo, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '2', '--pipeline', '2',
               '--dump-outputs', d]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith('{')]
        assert len(lines) == 1, lines
        line = json.loads(lines[0])
        assert line['steps'] == 3 and line['value'] > 0 and line['ms_per_step'] > 0 and line['higher_is_better'] is True
        assert line['unit'] == 'clips/s' and line['dtype'] == 'bf16' and line['metric'].startswith('clips/sec')
        assert abs(line['value'] - 2 * 1e3 / line['ms_per_step']) <= 1e-3 * line['value']
        for k in ('roofline', 'host_frames', 'accuracy_vs_fp32', 'cpu_baseline', 'other_configs'):
            assert k not in line, k
        names = sorted(os.listdir(d))
        assert names == ['im00_boxes.npy', 'im00_keypoints.npy', 'im01_boxes.npy', 'im01_keypoints.npy'], names
        arrs = {n: np.load(os.path.join(d, n)) for n in names}
        assert all(a.dtype == np.float32 for a in arrs.values())
        assert arrs['im00_boxes.npy'].shape[1] == 5 and arrs['im00_boxes.npy'].shape[0] > 0
        assert arrs['im00_keypoints.npy'].shape[0] == arrs['im00_boxes.npy'].shape[0]
        dumps.append(arrs)
    for n in dumps[0]:
        np.testing.assert_array_equal(dumps[0][n], dumps[1][n])


@pytest.mark.parametrize('mode', ['infer', 'train'])
def test_bench_eight_ranks_control_flow_on_one_gpu(mode):
    """World-8 readiness: the driver's `torch.distributed.run --nproc-per-node 8 ... bench.py --gpus 8` command line with
    EIGHT real ranks sharing this box's one GPU over gloo (DAT_BENCH_SHARE_GPU=1): rendezvous, per-rank contexts, barriers, the MAX-reduce
    of the timing and -- train -- the Trainer's bucketed, overlapped gradient exchange (bucket completion order, seal, deferred finish)
    with eight participants; rank 0 prints ONE line with n_gpus 8 whose value is the sum over the eight ranks.  One clip per forward and
    one forward in flight per rank keep eight model copies inside one device's memory."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(DAT_BENCH_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    port = 29500 + ((os.getpid() + 617 + (mode == 'train')) % 1000)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '8', '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(repo, 'bench.py'), '--gpus', '8', '--steps', '2', '--warmup', '1', '--full', '--no-accuracy', '--no-other-configs', '--h2d', '0'] + (['--mode', 'train'] if mode == 'train' else ['--batch', '1', '--pipeline', '1'])
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith('{')]
    assert len(lines) == 1, lines                      # rank 0 only
    line = json.loads(lines[0])
    assert line['n_gpus'] == 8 and len(line['ranks_seen']) == 8 and {r['rank'] for r in line['ranks_seen']} == set(range(8))
    assert 'shared_gpu_test' in line and line['value'] > 0 and line['steps'] == 2 and line['scaling'] == 'weak'
    assert 'cpu_baseline' not in line
    if mode == 'train':
        assert line['allreduce']['buckets'] >= 2 and line['allreduce']['backend'] == 'gloo'


@pytest.mark.parametrize('overlap', [True, False])
def test_two_ranks_with_one_clip_each_equal_one_rank_over_both_clips(tmp_path, overlap):
    """Data-parallel semantics of the training exchange (reference lib/modeling/model_builder.py:908-951 build_data_parallel_model:
    every GPU runs its own minibatch with losses scaled by 1 / NUM_GPUS (:484, :625, :884), gradients are summed over the GPUs,
    every GPU applies the same update).  Two PROCESSES (ranks 0 / 1, sharing this box's one GPU; gloo with host-staged buckets, RCCL
    needs one device per rank) train clip r each with NUM_GPUS = 2 for two iterations -- with the buckets exchanged as the backward
    pass completes them (cfg.HIP.OVERLAP_ALLREDUCE) or after it -- and must end with the weights of ONE rank that runs both clips
    per iteration with the same 1 / NUM_GPUS scaling (gradients accumulated, one update).  fp32 mode; the weight-gradient kernels
    reduce with float atomics, hence a tolerance of 5 % of each parameter's two-iteration update instead of bit equality (a wrong
    loss scale or a bucket exchanged before it was final moves a parameter by ~100 % of its update)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    port = 29500 + ((os.getpid() + 31 + int(overlap)) % 1000)
    out = str(tmp_path / 'rank%d.npz')
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, out, overlap)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    # 5 % of the update (in _check_two_ranks_against_one).  Measured: < 1 % everywhere except the LAST convs of the keypoint head (conv_fcn7 /
    # conv_fcn8: 1.0-1.5 %), whose weight gradient is a sum over the 56 x 56 map of (softmax - one-hot) x activation -- the per-map gradient
    # sums to ZERO, so the K-split partial sums the kernels combine with float atomics are ~1e4 x larger than their total and the order they
    # arrive in (different between two ranks + all-reduce and one rank accumulating) shows at the 1e-2 level of that small total
    _check_two_ranks_against_one(out)


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('shape', [(64, 128, (3, 3, 3), (1, 1)), (128, 64, (1, 3, 3), (2, 2)), (200, 256, (1, 1, 1), (1, 1))])
def test_relu_mask_in_the_data_gradient_epilogue_is_bit_identical_to_the_separate_pass(ops, dtype_name, shape):
    """ADVICE r3 (training.py FUSE_RELU_BWD): the data-gradient conv that applies the ReLU backward of its INPUT blob in its own
    epilogue (`dat_conv3d_fwd` res_mode 3: dx = x > 0 ? dx : 0) must give bit for bit what the two-launch path gives -- the plain data
    gradient followed by `dat_relu_bias_bwd` masking by x -- including zeros in the padding channels [cin, stride) that every
    consumer of the gradient reads."""
    cin, cout, k, stride = shape
    dt = ops.BF16 if dtype_name == 'bf16' else ops.F32
    tdt = ops.tdtype(dt)
    T, H, W = 4, 14, 18
    g_ = torch.Generator(device='cuda').manual_seed(cin * 7 + cout)
    w = torch.randn((cout, cin) + k, device='cuda', generator=g_) * (2.0 / (cin * k[0] * k[1] * k[2])) ** 0.5
    scale = torch.rand(cout, device='cuda', generator=g_) + 0.5
    pads = (k[0] // 2, k[1] // 2, k[2] // 2)
    cs_in, cs_out = ops.round_up(cin, 64), ops.round_up(cout, 64)
    Ho, Wo = (H + 2 * pads[1] - k[1]) // stride[0] + 1, (W + 2 * pads[2] - k[2]) // stride[1] + 1
    x = torch.relu(torch.randn((T, H, W, cs_in), device='cuda', generator=g_)).to(tdt)       # the forward input: a ReLU output
    x[..., cin:] = 0
    g = torch.randn((T, Ho, Wo, cs_out), device='cuda', generator=g_).to(tdt)
    g[..., cout:] = 0
    cg = ops.ConvGrad(w, scale, stride, pads, dt, cs_in, cs_out)
    plain = cg.data(g, T, H, W)
    two = ops.relu_bias_bwd(plain, x, dt, cin, relu=True)
    fused = cg.data(g, T, H, W, mask=x.contiguous())
    assert fused.shape == two.shape == x.shape
    assert torch.equal(fused, two)
    assert float(fused[..., cin:].abs().max()) == 0.0 if cs_in > cin else True
    assert (fused != 0).any() and ((x == 0) & (plain != 0)).any()            # the mask really removed something


SUM_MASK_SHAPES = [
    # forward conv (cin, cout, kernel, stride), gradient map T, H, W, dtypes -- and the kernel its data gradient takes
    ((64, 128, (3, 3, 3), (1, 1)), (4, 14, 18), ('bf16', 'fp32')),        # generic implicit GEMM (split-K on this small map)
    ((128, 64, (1, 3, 3), (2, 2)), (4, 14, 18), ('bf16', 'fp32')),        # strided: zero-insertion + generic kernel
    ((200, 256, (1, 1, 1), (1, 1)), (4, 14, 18), ('bf16', 'fp32')),       # pointwise on a small map, padded channels [200, 256)
    ((512, 128, (1, 1, 1), (1, 1)), (4, 128, 160), ('bf16',)),            # res3 `branch2a`: 128 -> 512, weights-in-LDS kernel, two passes
    ((1024, 256, (1, 1, 1), (1, 1)), (2, 128, 160), ('bf16',)),           # res4 `branch2a`: 256 -> 1024, weights-in-LDS kernel, four cout parts
    ((2048, 512, (1, 1, 1), (1, 1)), (2, 96, 160), ('bf16',)),            # res5 `branch2a`: 512 -> 2048, K-streaming kernel
]


@pytest.mark.parametrize('inplace', [True, False])
@pytest.mark.parametrize('case', [(s_, m_, d_) for s_, m_, ds in SUM_MASK_SHAPES for d_ in ds],
                         ids=lambda c: '%dto%d_k%d%d%d_s%d_%s' % (c[0][0], c[0][1], c[0][2][0], c[0][2][1], c[0][2][2], c[0][3][0], c[2]))
def test_sum_and_relu_mask_in_the_data_gradient_epilogue_is_bit_identical_to_the_separate_passes(ops, case, inplace):
    """training.py FUSE_RELU_SUM_BWD (round 6): for a blob with two readers -- a residual block's output -- the data-gradient conv of
    the reader that contributes LAST adds the other contribution and applies the ReLU backward of the blob's producer in its own epilogue
    (`dat_conv3d_fwd_sum_mask`, res_mode 4: dx = x > 0 ? conv + other : 0).  It must give bit for bit what the three-launch path gives
    -- the data gradient summed into the other contribution (res_mode 1), then `dat_relu_bias_bwd` masking by x -- in place and into a
    new tensor (the other contribution still read by a queued weight-gradient job), on every kernel that takes such a layer."""
    (cin, cout, k, stride), (T, H, W), dtype_name = case
    dt = ops.BF16 if dtype_name == 'bf16' else ops.F32
    tdt = ops.tdtype(dt)
    g_ = torch.Generator(device='cuda').manual_seed(cin * 7 + cout)
    w = torch.randn((cout, cin) + k, device='cuda', generator=g_) * (2.0 / (cin * k[0] * k[1] * k[2])) ** 0.5
    scale = torch.rand(cout, device='cuda', generator=g_) + 0.5
    pads = (k[0] // 2, k[1] // 2, k[2] // 2)
    cs_in, cs_out = ops.round_up(cin, 64), ops.round_up(cout, 64)
    Ho, Wo = (H + 2 * pads[1] - k[1]) // stride[0] + 1, (W + 2 * pads[2] - k[2]) // stride[1] + 1
    x = torch.relu(torch.randn((T, H, W, cs_in), device='cuda', generator=g_)).to(tdt)       # the block output: a ReLU output
    x[..., cin:] = 0
    g = torch.randn((T, Ho, Wo, cs_out), device='cuda', generator=g_).to(tdt)
    g[..., cout:] = 0
    other = torch.randn((T, H, W, cs_in), device='cuda', generator=g_).to(tdt)               # the shortcut's contribution
    other[..., cin:] = 0
    cg = ops.ConvGrad(w, scale, stride, pads, dt, cs_in, cs_out)
    prof = ops.ConvProfiler(capacity=8)
    summed = cg.data(g, T, H, W, accumulate_into=other.clone())
    three = ops.relu_bias_bwd(summed, x, dt, cin, relu=True)
    into = other.clone()
    prof.start()
    fused = cg.data(g, T, H, W, accumulate_into=into, mask=x.contiguous(), inplace=inplace)
    tags = [t for t, _, _ in prof.stop()]
    assert (fused.data_ptr() == into.data_ptr()) == inplace
    if not inplace:
        assert torch.equal(into, other), 'the contribution a queued job still reads was modified'
    assert torch.equal(fused, three), 'differs in %d elements (kernel tags %r)' % (int((fused != three).sum()), tags)
    assert float(fused[..., cin:].abs().max()) == 0.0 if cs_in > cin else True
    assert (fused != 0).any() and ((x == 0) & (summed != 0)).any()
    if (H, W) == (128, 160) and cin in (512, 1024):
        assert tags == [2560331], tags          # the weights-in-LDS 1x1 kernel
    if cin == 2048:
        assert tags == [2560341], tags          # the K-streaming 1x1 kernel


@pytest.mark.parametrize('dtype,direct', [('fp32', False), ('bf16', False), ('bf16', True)])
def test_overlapped_exchange_over_rccl_with_one_rank_is_the_identity(monkeypatch, dtype, direct):
    """The RCCL side of the overlapped gradient exchange on the one GPU a test box has: a process group of ONE rank (backend nccl =
    RCCL), DAT_FORCE_EXCHANGE=1 so that the Trainer runs its whole multi-rank machinery -- each bucket's deferred weight gradients
    finished and the bucket handed over as the backward pass completes it, the all-reduce on the communication stream behind an event
    of the compute stream, the compute stream waiting before the update; through torch.distributed and through the C ABI's
    dat_allreduce_bucket (cfg.HIP.RCCL_DIRECT).  The sum over one rank is the identity, so the GRADIENTS of an iteration must be those
    of a Trainer without any exchange: within 1 % of each tensor's largest gradient (two identical bf16 runs differ by 0.2 % of it:
    float atomics of the direct weight-gradient kernels, tools/probes/exchange_noise.py; bf16 is the mode in which the per-bucket
    deferred finish runs).  What this cannot show -- several ranks, one device each -- is covered by the gloo two-rank tests."""
    import torch.distributed as dist
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.training import Trainer
    monkeypatch.setenv('MASTER_ADDR', '127.0.0.1')
    monkeypatch.setenv('MASTER_PORT', str(29500 + ((os.getpid() + 77 + int(direct) + 2 * (dtype == 'bf16')) % 1000)))
    monkeypatch.setenv('DAT_FORCE_EXCHANGE', '1')
    monkeypatch.setenv('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    monkeypatch.setattr(Trainer, 'BUCKET_BYTES', 16 << 20)      # several buckets on this small model

    def run(with_dist):
        model, ws = _ddp_model(1, dtype=dtype)
        cfg.HIP.RCCL_DIRECT = bool(direct)
        _ddp_feed(ws, _ddp_clip(0))
        tr = Trainer(model, ws, dist if with_dist else None)
        tr.step(0.0, timing=with_dist)                  # lr 0: forward + backward (+ exchange); the gradients stay in the arena
        torch.cuda.synchronize()
        grads = {n: tr.arena[n].clone() for n in tr.trainable}
        tr.step(0.01, timing=with_dist)                 # and a real update through the same path
        torch.cuda.synchronize()
        return tr, grads
    _, ref = run(False)
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        tr, got = run(True)
        st = tr.last_exchange_stats
    finally:
        dist.destroy_process_group()
    assert tr.exchange is not None and tr.exchange.backend == 'nccl' and tr.exchange.order == list(range(len(tr.buckets)))
    assert len(tr.buckets) >= 4 and st['buckets'] >= 4 and st['allreduce_ms'] > 0 and st['exposed_allreduce_ms'] >= 0
    print('one-rank exchange: %d buckets, %.3f ms of collectives, %.3f ms exposed' % (st['buckets'], st['allreduce_ms'], st['exposed_allreduce_ms']))
    worst, live = (0.0, None), 0
    for n in tr.trainable:
        mx = float(ref[n].abs().max())
        if mx == 0.0:
            assert float(got[n].abs().max()) == 0.0, n         # frozen trunk: no gradient in either run
            continue
        live += 1
        d = float((got[n] - ref[n]).abs().max()) / mx
        worst = max(worst, (d, n))
        assert d <= 0.01, (n, d)
    assert live > 40
    print('largest gradient difference / largest gradient of the tensor: %.2e (%s)' % worst)
