"""Restatements for the per-RoI GroupNorm model tests (tests/test_gpu_gn_roi_model.py), as subclasses of the oracle graph.

1. `gn_kps_head_net(base, ...)`: `tests.group_norm_ref.gn_net(base)` with the keypoint head of HIP.GN_KPS_HEAD -- every `conv_fcn{i}` is a
   conv without bias, `torch.nn.functional.group_norm` on the [R, C, H, W] view (statistics per RoI) with `conv_fcn{i}_gn_s / _b`, ReLU.

2. `c4_tube_net(base)`: the C4 tube graph under the method names `tests.test_gpu_parity_full._check_against_oracle` calls, so that the
   C4 model is held to that function's rules (rois in the oracle set, cls_prob 1e-4, bbox_pred 1e-3, kps_score 1e-3 max-abs): the
   "pyramid" is [res4, res4], the RPN is the tube RPN, the box head the per-RoI res5 stage, the keypoint head the 3D one.  RoI features
   are handed over as (feature map, rois): the oracle's heads pool them themselves.

3. `autograd_reference(loss_fn, base, ...)`: `tests.group_norm_ref.autograd_reference` with the loss function as a parameter (the C4 tube
   training graph has its own, `oracle.train_ref.training_losses_c4_tube`): the same dtype casts, the same GN restatement of `base`.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import group_norm_ref as ref


def gn_kps_head_net(base, eps, max_groups=32):
    class GNKpsHeadNet(ref.gn_net(base, eps, max_groups)):
        def kps_head_2d(self, roi_feat):
            from oracle import net3d           # (`_t` looked up per call: tests.group_norm_ref.autograd_reference patches it)
            x = net3d._t(roi_feat)
            for i in range(self.o['kps_num_convs']):
                name = 'conv_fcn%d' % (i + 1)
                x = F.conv2d(x, net3d._t(self.w[name + '_w']), None, stride=1, padding=1)
                x = F.relu(self.affine(x, name + '_gn'))
            return self.kps_outputs_2d(x)

    return GNKpsHeadNet


def c4_tube_net(base):
    class C4TubeNet(base):
        def time_link(self, pyr):
            return pyr

        def fpn_rpn(self, feats, im_info):
            out = self.rpn_c4_tube(feats[0], im_info)
            return out[0], out[1], None

        def roi_feat_fpn(self, feats, per_level_rois, restore, pooled, sampling):
            return feats[0], np.concatenate(per_level_rois, axis=0)[restore]

        def box_head_2mlp(self, roi_feat):
            return self.box_head_c4_tube(*roi_feat)

        def kps_head_2d(self, roi_feat):
            return self.kps_head_tube(*roi_feat)

    return C4TubeNet


def autograd_reference(loss_fn, base, weights, eps, dtype, max_groups=32):
    """One forward + backward of `loss_fn(weights as tensors)` -- a function that calls one of `oracle.train_ref`'s loss graphs -- on the GN
    restatement of `base`, on the CPU in `dtype`.  -> (losses, gradients), NumPy float64.  As in `ref.autograd_reference`, the oracle's
    float32 casts and its Net class are replaced for the duration of the call only."""
    from oracle import net3d, train_ref
    saved = (net3d._t, train_ref.Net, torch.from_numpy)

    def as_dtype(a):
        t = a if isinstance(a, torch.Tensor) else saved[2](np.ascontiguousarray(a))
        return t.to(dtype) if t.is_floating_point() else t
    wt = {k: saved[2](np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in weights.items()}
    try:
        net3d._t = as_dtype
        train_ref.Net = ref.gn_net(base, eps, max_groups)
        train_ref.torch.from_numpy = as_dtype
        losses = loss_fn(wt)
        sum(losses.values()).backward()
    finally:
        net3d._t, train_ref.Net, torch.from_numpy = saved
    grads = {k: v.grad.detach().double().numpy() for k, v in wt.items() if v.grad is not None}
    return {k: float(v.detach()) for k, v in losses.items()}, grads
