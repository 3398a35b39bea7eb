"""Float64 reference of the grouped conv (ResNeXt `branch2b`) and of the ResNeXt-FPN3D body built from it -- independent of the
kernels and of the builder: a grouped conv is stated as G dense convs, each over its own slice of input channels, concatenated over
the groups (the definition Caffe2's ConvNd `group` argument has, lib/modeling/ResNet3D.py:33-41)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import numerics as nm


def grouped_conv_ref64(x, w, groups, scale=None, bias=None, res=None, stride=(1, 1), pads=(0, 0, 0), relu=False):
    """(ref64, absref64), numpy float64 (N, Cout, T, Ho, Wo): per group g the dense fused conv (tests/numerics.conv_ref64) of input
    channels [g * Cin / G, (g + 1) * Cin / G) with filters [g * Cout / G, (g + 1) * Cout / G), concatenated over g.
    x: (N, Cin, T, H, W); w: (Cout, Cin / G, KT, KH, KW), Caffe2's grouped filter layout."""
    x, w = np.asarray(x), np.asarray(w)
    cin, cout = x.shape[1], w.shape[0]
    assert cin % groups == 0 and cout % groups == 0 and w.shape[1] == cin // groups, (x.shape, w.shape, groups)
    ci, co = cin // groups, cout // groups
    refs, absrefs = [], []
    for g in range(groups):
        so = slice(g * co, (g + 1) * co)
        r, a = nm.conv_ref64(x[:, g * ci:(g + 1) * ci], w[so], None if scale is None else np.asarray(scale)[so],
                             None if bias is None else np.asarray(bias)[so], None if res is None else np.asarray(res)[:, so],
                             stride, pads, relu)
        refs.append(r)
        absrefs.append(a)
    return np.concatenate(refs, axis=1), np.concatenate(absrefs, axis=1)


# ---- the ResNeXt body on the oracle graph ---------------------------------------------------------------------------------------------
def grouped_conv3d(x, w, groups, stride, pads):
    """torch (any float dtype) on (N, C, T, H, W): the same statement -- G dense convs over channel slices, concatenated."""
    ci, co = x.shape[1] // groups, w.shape[0] // groups
    assert w.shape[1] == ci, (tuple(x.shape), tuple(w.shape), groups)
    return torch.cat([F.conv3d(x[:, g * ci:(g + 1) * ci], w[g * co:(g + 1) * co], None, stride=tuple(stride), padding=tuple(pads))
                      for g in range(groups)], dim=1)


def resnext_net(groups):
    """`oracle.net3d.Net` with the ResNeXt bottleneck (lib/modeling/ResNet3D.py:21-55 with RESNETS.NUM_GROUPS = `groups` and
    RESNETS.STRIDE_1X1 False): 1x1x1 -> GROUPED kT x 3 x 3 carrying the spatial stride -> 1x1x1, each + affine, ReLU after the first
    two.  Shortcut, Sum, ReLU, the FPN and the heads are the oracle's."""
    from oracle.net3d import Net, _t

    class NetResNeXt(Net):
        def _bottleneck(self, x, prefix, stride, kt):
            y = F.relu(self.conv_affine_nd(x, prefix + '_branch2a', [1, 1, 1], [1, 1, 1], [0, 0, 0]))
            w = _t(self.w[prefix + '_branch2b_w'])
            assert list(w.shape[2:]) == [kt, 3, 3] and w.shape[1] * groups == y.shape[1], (prefix, tuple(w.shape))
            y = grouped_conv3d(y, w.to(y.dtype), groups, [1, stride, stride], [kt // 2, 1, 1])
            y = F.relu(self.affine(y, prefix + '_branch2b_bn'))
            return self.conv_affine_nd(y, prefix + '_branch2c', [1, 1, 1], [1, 1, 1], [0, 0, 0])
    return NetResNeXt
