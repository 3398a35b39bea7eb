"""References of the tracker appearance-cost tests: a random state_dict with torchvision's resnet18 names (plain torch, no torchvision),
torchvision's forward restated in float64 on the CPU, and the float64 cosine distance."""
import numpy as np
import torch
import torch.nn.functional as F

# the person keypoints of the PoseTrack annotation files
POSETRACK_KEYPOINTS = ['nose', 'head_bottom', 'head_top', 'left_ear', 'right_ear', 'left_shoulder', 'right_shoulder', 'left_elbow',
                       'right_elbow', 'left_wrist', 'right_wrist', 'left_hip', 'right_hip', 'left_knee', 'right_knee', 'left_ankle',
                       'right_ankle']


class Dataset(object):
    """What the pose cost reads of a roidb entry's `dataset`."""

    def __init__(self, names=POSETRACK_KEYPOINTS):
        self.person_cat_info = {'keypoints': list(names)}


def random_resnet18_state(seed=5, stages=4):
    """A state_dict with torchvision's resnet18 names: He-initialised convs, BatchNorm with non-trivial affine and running statistics."""
    g = torch.Generator().manual_seed(seed)
    state = {}

    def conv(name, cout, cin, k):
        state[name + '.weight'] = torch.randn(cout, cin, k, k, generator=g) * float(np.sqrt(2.0 / (cin * k * k)))

    def bn(name, c):
        state[name + '.weight'] = torch.rand(c, generator=g) * 0.5 + 0.5
        state[name + '.bias'] = torch.randn(c, generator=g) * 0.1
        state[name + '.running_mean'] = torch.randn(c, generator=g) * 0.1
        state[name + '.running_var'] = torch.rand(c, generator=g) + 0.5
        state[name + '.num_batches_tracked'] = torch.tensor(7)
    conv('conv1', 64, 3, 7)
    bn('bn1', 64)
    cin = 64
    for L, c in zip(range(1, stages + 1), (64, 128, 256, 512)):
        for B in range(2):
            p = 'layer%d.%d' % (L, B)
            conv(p + '.conv1', c, cin, 3)
            bn(p + '.bn1', c)
            conv(p + '.conv2', c, c, 3)
            bn(p + '.bn2', c)
            if B == 0 and L > 1:
                conv(p + '.downsample.0', c, cin, 1)
                bn(p + '.downsample.1', c)
            cin = c
    return state


def resnet18_forward64(state, x, layers=(1, 2, 3, 4)):
    """torchvision's ResNet-18 in eval mode on x [n, 3, H, W] (float64): conv 7x7/2 pad 3, batch_norm, relu, max_pool 3/2 pad 1, then
    basic blocks (3x3 conv with the stride, bn, relu, 3x3 conv, bn, + identity or the 1x1 strided downsample + bn, relu).  Returns
    {'layerK': output of layerK} for K in `layers`."""
    d = lambda name: state[name].double()

    def bn(z, p):
        return F.batch_norm(z, d(p + '.running_mean'), d(p + '.running_var'), d(p + '.weight'), d(p + '.bias'), training=False, eps=1e-5)
    z = F.relu(bn(F.conv2d(x.double(), d('conv1.weight'), None, stride=2, padding=3), 'bn1'))
    z = F.max_pool2d(z, 3, 2, 1)
    out = {}
    for L in range(1, max(layers) + 1):
        for B in range(2):
            p = 'layer%d.%d' % (L, B)
            stride = 2 if (L > 1 and B == 0) else 1
            o = F.relu(bn(F.conv2d(z, d(p + '.conv1.weight'), None, stride=stride, padding=1), p + '.bn1'))
            o = bn(F.conv2d(o, d(p + '.conv2.weight'), None, stride=1, padding=1), p + '.bn2')
            idt = z
            if p + '.downsample.0.weight' in state:
                idt = bn(F.conv2d(z, d(p + '.downsample.0.weight'), None, stride=stride), p + '.downsample.1')
            z = F.relu(o + idt)
        if L in layers:
            out['layer%d' % L] = z
    return out


def cosine_cost64(fa, fb):
    """1 - a.b / (|a| |b|) in float64, rows of fa against rows of fb; a row of norm zero is at distance 1 (the project's rule)."""
    fa, fb = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    d = fa @ fb.T
    na, nb = np.sum(fa * fa, axis=1), np.sum(fb * fb, axis=1)
    den = np.sqrt(na[:, None] * nb[None, :])
    live = den > 0
    return np.where(live, 1.0 - d / np.where(live, den, 1.0), 1.0)
