"""Reference restatement of the ResNet-(2+1)D body (Tran et al., CVPR 2018) on the oracle graph: `oracle.net3d.Net` with its two
block functions overridden.  Every kT x 3 x 3 conv of a block in a stage with kT > 1 is a 1 x 3 x 3 conv (the spatial stride, pad 1)
+ affine + ReLU, then a kT x 1 x 1 conv (temporal pad kT // 2) + affine, over M = floor(kT * 9 * Nin * Nout / (9 * Nin + kT * Nout))
mid planes; stages with kT = 1 keep the I3D blocks.  Parameter names: `<conv>_spatial_w`, `<conv>_spatial_bn_{s,b}`,
`<conv>_temporal_w`, `<conv>_temporal_bn_{s,b}`.  Shortcut, Sum, ReLU, the FPN and the heads are the oracle's."""
import torch.nn.functional as F

from oracle.net3d import Net


def mid_planes(n_in, n_out, kt):
    return (kt * 9 * n_in * n_out) // (9 * n_in + kt * n_out)


class Net2plus1d(Net):
    def _factorised(self, x, name, kt, stride):
        y = F.relu(self.conv_affine_nd(x, name + '_spatial', [1, 3, 3], [1, stride, stride], [0, 1, 1]))
        return self.conv_affine_nd(y, name + '_temporal', [kt, 1, 1], [1, 1, 1], [kt // 2, 0, 0])

    def _basic(self, x, prefix, stride, kt):
        if kt == 1:
            return Net._basic(self, x, prefix, stride, kt)
        y = F.relu(self._factorised(x, prefix + '_branch2a', kt, stride))
        return self._factorised(y, prefix + '_branch2b', kt, 1)

    def _bottleneck(self, x, prefix, stride, kt):
        if kt == 1:
            return Net._bottleneck(self, x, prefix, stride, kt)
        y = F.relu(self.conv_affine_nd(x, prefix + '_branch2a', [1, 1, 1], [1, stride, stride], [0, 0, 0]))
        y = F.relu(self._factorised(y, prefix + '_branch2b', kt, 1))
        return self.conv_affine_nd(y, prefix + '_branch2c', [1, 1, 1], [1, 1, 1], [0, 0, 0])


def param_shapes(opts):
    """name -> shape of every body parameter the restatement reads (conv1 .. res5), derived from the oracle's options (dims, counts,
    kT): what the builder must create."""
    dims, counts, kt = opts['feat_dims'], opts['block_counts'], opts['kt_body']
    bottleneck = opts['trans'] == 'bottleneck'
    out = {'conv1_w': (dims[0], 3, 1, 7, 7), 'res_conv1_bn_s': (dims[0],), 'res_conv1_bn_b': (dims[0],)}

    def affine(name, c):
        out[name + '_s'] = (c,)
        out[name + '_b'] = (c,)

    def conv(name, co, ci, k):
        out[name + '_w'] = (co, ci) + tuple(k)
        affine(name + '_bn', co)

    def kxk(name, ci, co, k):
        if k == 1:
            conv(name, co, ci, (1, 3, 3))
        else:
            m = mid_planes(ci, co, k)
            conv(name + '_spatial', m, ci, (1, 3, 3))
            conv(name + '_temporal', co, m, (k, 1, 1))

    dim_in = dims[0]
    for s, n in enumerate(counts):
        dim_out = dims[s + 1]
        inner = 64 * 2 ** s
        k = 1 if s == 0 else kt
        for i in range(n):
            p = 'res%d_%d' % (s + 2, i)
            if bottleneck:
                conv(p + '_branch2a', inner, dim_in, (1, 1, 1))
                kxk(p + '_branch2b', inner, inner, k)
                conv(p + '_branch2c', dim_out, inner, (1, 1, 1))
            else:
                kxk(p + '_branch2a', dim_in, dim_out, k)
                kxk(p + '_branch2b', dim_out, dim_out, k)
            if dim_in != dim_out:
                out[p + '_branch1_w'] = (dim_out, dim_in, 1, 1, 1)
                affine(p + '_branch1_bn', dim_out)
            dim_in = dim_out
    return out
