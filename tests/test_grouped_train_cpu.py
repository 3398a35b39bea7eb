"""Training of grouped-conv (ResNeXt) bodies without a GPU: the exported symbols of both library flavours, the opt-in switch
cfg.HIP.TRAIN_GROUPED_CONV at the builder, and the float64 references of tests/grouped_grad_ref.py against torch.autograd."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.grouped_grad_ref import grouped_dgrad_ref64, grouped_wgrad_ref64
from tests.model_util import fpn3d_kps_cfg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dat_conv3d_grouped_pack_weights_dgrad', 'dat_conv3d_grouped_wgrad_acc', 'dat_conv3d_grouped_wgrad',
               'dat_conv3d_grouped_wgrad_workspace_bytes')


def _create_train(switch):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    d = fpn3d_kps_cfg('50', T=4, kt=3)
    d['RESNETS'] = {'NUM_GROUPS': 32, 'WIDTH_PER_GROUP': 8, 'STRIDE_1X1': False}
    reset_cfg()
    cfg_from_cfg(d)
    cfg.TRAIN.DATASET = 'synthetic'
    if switch is not None:
        cfg.HIP.TRAIN_GROUPED_CONV = switch
    assert_and_infer_cfg()
    try:
        return model_builder.create(cfg.MODEL.TYPE, train=True)
    finally:
        reset_cfg()


@pytest.mark.parametrize('lib', ['libdat_hip.so', 'libdat_hip_f16.so'])
def test_both_library_flavours_export_the_grouped_gradient_entry_points(lib):
    h = ctypes.CDLL(os.path.join(REPO, 'detectandtrack_amd', lib))
    for name in NEW_SYMBOLS:
        assert hasattr(h, name), '%s does not export %s' % (lib, name)
    from detectandtrack_amd import libdat
    assert set(NEW_SYMBOLS) <= set(libdat.EXPORTS)


def test_the_switch_builds_the_resnext_training_graph():
    """ResNeXt-50 32x8d with cfg.HIP.TRAIN_GROUPED_CONV: every `branch2b` carries group = 32 and its [C, cg, kT, 3, 3] weight is trainable."""
    model = _create_train(True)
    trainable = set(model.TrainableParams())
    want = {'res2': (256, 8, 1), 'res3': (512, 16, 3), 'res4': (1024, 32, 3), 'res5': (2048, 64, 3)}
    n = 0
    for o in model.net.ops:
        if o.type == 'Conv' and o.args['w'].endswith('_branch2b_w'):
            w = o.args['w']
            c, cg, kt = want[w[:4]]
            assert o.args['group'] == 32, w
            assert tuple(model.param_specs[w]['shape']) == (c, cg, kt, 3, 3), w
            assert w in trainable, w
            n += 1
    assert n == 3 + 4 + 6 + 3
    assert any(o.type in ('SoftmaxLoss', 'KeypointLoss') for o in model.net.ops), 'not a training graph'


@pytest.mark.parametrize('switch', [None, False])
def test_the_default_keeps_refusing_and_names_the_switch(switch):
    from detectandtrack_amd.core.config import cfg_default
    assert cfg_default.HIP.TRAIN_GROUPED_CONV is False
    with pytest.raises(NotImplementedError, match=r'grouped data-gradient and weight-gradient kernels') as e:
        _create_train(switch)
    assert 'TRAIN_GROUPED_CONV' in str(e.value)


def test_convgrad_of_a_grouped_layer_is_never_pointwise_and_counts_the_full_cin():
    """Host bookkeeping only (no launch): cin is the full C, the layer is not pointwise and is never queued into the pointwise batch."""
    from detectandtrack_amd.ops import hip_ops as ops
    cg = ops.ConvGrad(torch.zeros(128, 4, 1, 3, 3), None, (1, 1), (0, 1, 1), ops.F32, 128, 128, groups=32)
    assert (cg.cout, cg.cin, cg.groups) == (128, 128, 32) and not cg.pointwise
    assert cg.weight_acc_job(torch.zeros(1, 8, 8, 128), torch.zeros(1, 8, 8, 128), 1, torch.zeros(128 * 4 * 9)) is None
    assert ops.ConvGrad(torch.zeros(128, 64, 1, 1, 1), None, (1, 1), (0, 0, 0), ops.F32, 64, 128).pointwise


def test_reference_helpers_agree_with_autograd_of_torch_grouped_conv():
    """y = conv3d(x, w, groups = G, stride 2) * scale; L = <y, g>: dL/dx and dL/dw of torch.autograd in float64 against the per-group
    statements of tests/grouped_grad_ref.py, to 1e-11; with the residual add and the mask of the fused epilogue on the data gradient."""
    rs = np.random.RandomState(11)
    N, C, T, H, W, G = 2, 24, 3, 9, 7, 6
    cg = C // G
    x = torch.from_numpy(rs.randn(N, C, T, H, W)).requires_grad_(True)
    w = torch.from_numpy(rs.randn(C, cg, 3, 3, 3)).requires_grad_(True)
    scale = rs.uniform(0.5, 1.5, C)
    y = torch.nn.functional.conv3d(x, w, None, stride=(1, 2, 2), padding=(1, 1, 1), groups=G) * torch.from_numpy(scale).view(1, -1, 1, 1, 1)
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    assert tuple(y.shape) == (N, C, T, Ho, Wo)
    g = rs.randn(N, C, T, Ho, Wo)
    (y * torch.from_numpy(g)).sum().backward()
    ws = w.detach().numpy() * scale.reshape(-1, 1, 1, 1, 1)
    dx, dx_abs = grouped_dgrad_ref64(g, ws, G, 2, (1, 1, 1), H, W)
    assert dx.dtype == np.float64 and dx.shape == (N, C, T, H, W)
    assert np.abs(dx - x.grad.numpy()).max() < 1e-11
    assert (dx_abs >= np.abs(dx) - 1e-11).all()
    add, mask = rs.randn(N, C, T, H, W), rs.randn(N, C, T, H, W)
    dxa, _ = grouped_dgrad_ref64(g, ws, G, 2, (1, 1, 1), H, W, add=add)
    assert np.abs(dxa - (x.grad.numpy() + add)).max() < 1e-11
    dxm, _ = grouped_dgrad_ref64(g, ws, G, 2, (1, 1, 1), H, W, mask=mask)
    assert np.abs(dxm - np.where(mask > 0, x.grad.numpy(), 0.0)).max() < 1e-11
    dw, dw_abs, K = grouped_wgrad_ref64(x.detach().numpy(), g, G, scale, (3, 3, 3), 2, (1, 1, 1))
    assert dw.shape == (C, cg, 3, 3, 3) and K == N * T * Ho * Wo
    assert np.abs(dw - w.grad.numpy()).max() < 1e-11
    assert (dw_abs >= np.abs(dw) - 1e-11).all()
    # a gradient that lives in one frame of a single clip: the window form equals the full form on the zero-extended gradient
    g1 = np.zeros((1, C, T, Ho, Wo))
    g1[:, :, 1] = g[:1, :, 1]
    x1 = x.detach().numpy()[:1]
    a = grouped_wgrad_ref64(x1, g1, G, scale, (3, 3, 3), 2, (1, 1, 1), window=(1, 1))
    b = grouped_wgrad_ref64(x1, g1, G, scale, (3, 3, 3), 2, (1, 1, 1))
    assert np.abs(a[0] - b[0]).max() < 1e-12 and a[2] * T == b[2]
