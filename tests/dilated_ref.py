"""References of the dilated convolution (MODEL.DILATION) for tests/test_dilated_cpu.py, tests/test_gpu_dilated_conv.py and
tests/test_gpu_dilated_model.py.

Kernel level.  A 3 x 3 conv dilated by d is the dense (2d + 1) x (2d + 1) conv whose other weights are zero (`inflate`):

    out[h, w] = sum_{kh, kw} x[h + kh * d - pad, w + kw * d - pad] * w[kh, kw],

so the float64 references of the undilated kernels (tests/numerics.conv_ref64, tests/temporal_refs.windowed_conv_ref64) serve as they
are; the zeros add nothing to the sum of absolute products, and the reduction length K of the bound stays Cin x taps.  The gradients
come from torch.nn.grad in float64 with `dilation=`.

Model level.  `NetDilated` restates the C5-dilated body on the oracle graph (`oracle.net3d.Net` with its stage and block functions
overridden, as tests/r2plus1d_ref.py does for the (2+1)D body): in res5 the first block keeps stride 1 -- shortcut included -- and the
3 x 3 conv the reference dilates (`branch2b` of either block function, lib/modeling/ResNet3D.py:40-46, 77-81) gets dilation d and
pads d.  `branch2a` of a basic block is not dilated there and is not here."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.net3d import Net, _t


# ---- kernel level ------------------------------------------------------------------------------------------------------------------------
def inflate(w, d):
    """(Cout, Cin, KT, KH, KW) -> (Cout, Cin, KT, (KH - 1) d + 1, (KW - 1) d + 1): the taps d apart, zeros between (numpy or torch)."""
    d = int(d)
    if d == 1:
        return w
    co, ci, kt, kh, kw = [int(v) for v in w.shape]
    shape = (co, ci, kt, (kh - 1) * d + 1, (kw - 1) * d + 1)
    out = torch.zeros(shape, dtype=w.dtype) if isinstance(w, torch.Tensor) else np.zeros(shape, dtype=w.dtype)
    out[:, :, :, ::d, ::d] = w
    return out


def out_hw(H, W, k, pads, d):
    return H + 2 * pads[1] - d * (k[1] - 1), W + 2 * pads[2] - d * (k[2] - 1)


def _t64(a):
    return a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.float64))


def dgrad_ref64(g, w, scale, pads, d, x_shape, mask=None, base=None):
    """(ref64, absref64) of dL/dx of the stride-1 conv dilated by d (spatially; "same" temporal padding): transpose-conv(g, w * scale)
    (+ base), then `mask > 0 ? v : 0`; absref: the same sum over absolute values, no mask.  numpy (N, Cin, T, H, W)."""
    g, w = _t64(g), _t64(w)
    ws = w if scale is None else w * _t64(scale).view(-1, 1, 1, 1, 1)
    outs = []
    for absolute in (False, True):
        f = (lambda v: v.abs()) if absolute else (lambda v: v)
        y = torch.nn.grad.conv3d_input(tuple(x_shape), f(ws), f(g), stride=1, padding=tuple(pads), dilation=(1, d, d))
        if base is not None:
            y = y + f(_t64(base))
        if mask is not None and not absolute:
            y = torch.where(_t64(mask) > 0, y, torch.zeros_like(y))
        outs.append(y.numpy())
    return outs[0], outs[1]


def wgrad_ref64(x, g, scale, k, pads, d):
    """(ref64, absref64, K) of dW[co][ci][tap] = scale[co] * sum_q g[q][co] * x[q + off(tap)][ci], off = (kt - pt, kh d - p, kw d - p);
    K = the output positions reduced."""
    x, g = _t64(x), _t64(g)
    gs = g if scale is None else g * _t64(scale).view(1, -1, 1, 1, 1)
    shape = (g.shape[1], x.shape[1]) + tuple(k)
    ref = torch.nn.grad.conv3d_weight(x, shape, gs, stride=1, padding=tuple(pads), dilation=(1, d, d))
    absref = torch.nn.grad.conv3d_weight(x.abs(), shape, gs.abs(), stride=1, padding=tuple(pads), dilation=(1, d, d))
    return ref.numpy(), absref.numpy(), int(g.shape[0] * g.shape[2] * g.shape[3] * g.shape[4])


# ---- model level -------------------------------------------------------------------------------------------------------------------------
class NetDilated(Net):
    """opts['dilation'] = MODEL.DILATION: res5 at stride 1 with its `branch2b` 3 x 3 convs dilated; the other stages are the oracle's."""

    def conv_affine_nd_dil(self, x, prefix, kernels, pads, d):
        w = _t(self.w[prefix + '_w'])
        assert list(w.shape[2:]) == list(kernels), (prefix, w.shape, kernels)
        return self.affine(F.conv3d(x, w, None, stride=1, padding=tuple(pads), dilation=(1, d, d)), prefix + '_bn')

    def _basic_dil(self, x, prefix, kt, d):
        y = F.relu(self.conv_affine_nd(x, prefix + '_branch2a', [kt, 3, 3], [1, 1, 1], [kt // 2, 1, 1]))
        return self.conv_affine_nd_dil(y, prefix + '_branch2b', [kt, 3, 3], [kt // 2, d, d], d)

    def _bottleneck_dil(self, x, prefix, kt, d):
        y = F.relu(self.conv_affine_nd(x, prefix + '_branch2a', [1, 1, 1], [1, 1, 1], [0, 0, 0]))
        y = F.relu(self.conv_affine_nd_dil(y, prefix + '_branch2b', [kt, 3, 3], [kt // 2, d, d], d))
        return self.conv_affine_nd(y, prefix + '_branch2c', [1, 1, 1], [1, 1, 1], [0, 0, 0])

    def _stage(self, x, stage_id, prefix, n, dim_in, dim_out, kt, stride_init=2):
        d = int(self.o.get('dilation', 1))
        if stage_id != 4 or d == 1 or prefix != 'res5':
            return Net._stage(self, x, stage_id, prefix, n, dim_in, dim_out, kt, stride_init)
        trans = self._basic_dil if self.o['trans'] == 'basic' else self._bottleneck_dil
        for i in range(n):
            p = '{}_{}'.format(prefix, i)
            tr = trans(x, p, kt, d)
            if dim_in == dim_out:
                sc = x
            else:       # (stride 1 under a dilation: add_bottleneck_block)
                sc = self.affine(self.conv_nd(x, p + '_branch1', [1, 1, 1], [1, 1, 1], [0, 0, 0], bias=False), p + '_branch1_bn')
            x = F.relu(tr + sc)
            self.blobs[p + '_sum'] = x
            dim_in = dim_out
        return x


def c5_dilated_cfg(arch='18', T=4, kt=3, dilation=2, link='slice-center', pre=300, post=100, dtype='fp32', tube=False, body=None):
    """The configuration of configs/test_r18_c5_dilated_synthetic.yaml as a dict: C5 body, MODEL.DILATION, no FPN, single-level RPN,
    2-MLP box head, keypoint head (tube=True: BODY_HEAD_LINK '' with the 3D keypoint head)."""
    from tests.model_util import fpn3d_kps_cfg
    c = fpn3d_kps_cfg(arch, T=T, kt=kt, link='' if tube else link, pre=pre, post=post, dtype=dtype)
    c['MODEL'].update(CONV_BODY=body or 'ResNet3D.add_ResNet%s_conv5_body' % arch, DILATION=dilation)
    c['FPN'] = {'FPN_ON': False, 'MULTILEVEL_ROIS': False, 'MULTILEVEL_RPN': False}
    c['VIDEO']['TIME_KERNEL_DIM'] = {'BODY': kt, 'HEAD_RPN': 1, 'HEAD_KPS': 1, 'HEAD_DET': 1}
    if tube:
        c['KRCNN'].update(ROI_KEYPOINTS_HEAD='keypoint_rcnn_heads.add_roi_pose_head_v1convX_3d', NO_3D_DECONV_TIME_TO_CH=True)
    return c


def forward_2d_heads(net, data, im_info):
    """body -> key frame (slice-center) -> the single-level RPN on the 1/16 map: (feat2d, reference rois).  The RoI heads follow from
    `box_head(net, feat2d, rois)` and `net.kps_head_c4_2d(feat2d, kp_rois)` (RoIAlign at 1/16: oracle/net3d.py)."""
    feat = net.time_link([net.body(torch.from_numpy(data))])[0]
    rois = net.rpn_c4_2d(feat, im_info)[0]
    return feat, rois


def box_head(net, feat2d, rois):
    """RoIAlign 7 x 7 at 1/16 -> the 2-MLP head: (cls_prob, bbox_pred)"""
    from oracle.roi_align import roi_align_2d
    o = net.o
    return net.box_head_2mlp(roi_align_2d(feat2d.numpy(), rois, o['frcn_res'], 1. / 16., o['frcn_sampling']))


def training_losses(weights, opts, data, labels, sampled, cfg_scalars):
    """The training graph of configs/train_r18_c5_dilated_synthetic.yaml with autograd (weights: dict name -> leaf tensors): the
    dilated body, the key frame, the single-level RPN losses (model_builder.py:612-636: SigmoidCrossEntropyLoss normalised by the
    counted anchors, SmoothL1Loss with beta 1/9 per image), the 2-MLP box head and the 2D keypoint head on RoIAlign at 1/16, with
    the loss scaling of oracle/train_ref.py.  Returns dict loss name -> tensor."""
    from oracle import train_ref as tref
    net = NetDilated(weights, opts)
    feat = net.time_link([net.body(torch.from_numpy(data))])[0]       # (1, C, H / 16, W / 16)
    ng = cfg_scalars['num_gpus']
    losses = {}
    h = F.relu(net.conv2d(feat, 'conv_rpn', 3, 1, 1))
    logits, deltas = net.conv2d(h, 'rpn_cls_logits', 1), net.conv2d(h, 'rpn_bbox_pred', 1)
    H, W = logits.shape[2:]
    lab = torch.from_numpy(labels['rpn_labels_int32_wide'][:, :, :H, :W])
    valid = (lab >= 0).float()
    ce = F.binary_cross_entropy_with_logits(logits, lab.clamp(min=0).float(), reduction='none')
    losses['loss_rpn_cls'] = (ce * valid).sum() / max(float(valid.sum()), 1.0) / ng
    t, wi, wo = [torch.from_numpy(labels['rpn_bbox_%s_wide' % k][:, :, :H, :W]) for k in ('targets', 'inside_weights', 'outside_weights')]
    losses['loss_rpn_bbox'] = tref.smooth_l1(deltas, t, wi, wo, 1. / 9.) / logits.shape[0] / ng
    rois = sampled['rois']
    x = tref.roi_align_2d_torch(feat, rois, opts['frcn_res'], 1. / 16., opts['frcn_sampling'])
    x = F.relu(net.fc(x, 'fc6'))
    x = F.relu(net.fc(x, 'fc7'))
    cls_score, bbox_pred = net.fc(x, 'cls_score'), net.fc(x, 'bbox_pred')
    R = rois.shape[0]
    losses['loss_cls'] = F.cross_entropy(cls_score, torch.from_numpy(sampled['labels_int32']).long(), reduction='sum') / R / ng
    losses['loss_bbox'] = tref.smooth_l1(bbox_pred, torch.from_numpy(sampled['bbox_targets']), torch.from_numpy(sampled['bbox_inside_weights']),
                                         torch.from_numpy(sampled['bbox_outside_weights']), 1.0) / R / ng
    kfeat = tref.roi_align_2d_torch(feat, sampled['keypoint_rois'], opts['kps_res'], 1. / 16., opts['kps_sampling'])
    kps = net.kps_head_2d(kfeat)
    Rk, K, M, _ = kps.shape
    w = torch.from_numpy(sampled['keypoint_weights']).reshape(-1)
    nll = F.cross_entropy(kps.reshape(Rk * K, M * M), torch.from_numpy(sampled['keypoint_locations_int32']).reshape(-1).long(), reduction='none')
    losses['loss_kps'] = (nll * w).sum() / w.sum() * cfg_scalars['kps_loss_weight'] / ng
    return losses
