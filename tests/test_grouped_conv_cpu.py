"""Grouped convs (ResNeXt bodies) without a GPU: what the builder records, the training guard, the exported symbols of both library
flavours, and the float64 reference helper (tests/grouped_ref.py) against torch's own grouped conv."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.grouped_ref import grouped_conv_ref64
from tests.model_util import fpn3d_kps_cfg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dat_conv3d_grouped_packed_weight_bytes', 'dat_conv3d_grouped_pack_weights', 'dat_conv3d_grouped_fwd',
               'dat_conv3d_grouped_flops')


def _resnext_cfg(arch='50', groups=32, width=8, kt=3):
    d = fpn3d_kps_cfg(arch, T=4, kt=kt)
    d['RESNETS'] = {'NUM_GROUPS': groups, 'WIDTH_PER_GROUP': width, 'STRIDE_1X1': False}
    return d


def _create(d, train=False):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    reset_cfg()
    cfg_from_cfg(d)
    if train:
        cfg.TRAIN.DATASET = 'synthetic'
    assert_and_infer_cfg()
    return model_builder.create(cfg.MODEL.TYPE, train=train)


@pytest.mark.parametrize('kt', [1, 3])
def test_builder_records_grouped_branch2b(kt):
    """NUM_GROUPS 32, WIDTH_PER_GROUP 8: every `branch2b` is a grouped conv with the filter shape [dim_inner, dim_inner / 32, kT, 3, 3]
    (kT = 1 in res2) and carries the block's spatial stride (STRIDE_1X1 False); every other conv is ungrouped and records no group."""
    model = _create(_resnext_cfg(kt=kt))
    ops = {o.outputs[0]: o for o in model.net.ops if o.type == 'Conv'}
    by_w = {o.args['w']: o for o in model.net.ops if o.type == 'Conv'}
    op = by_w['res2_0_branch2b_w']
    assert tuple(model.param_specs['res2_0_branch2b_w']['shape']) == (256, 8, 1, 3, 3)
    assert op.args['group'] == 32 and op.args['dim_in'] == op.args['dim_out'] == 256
    want = {'res2': (256, 8, 1), 'res3': (512, 16, kt), 'res4': (1024, 32, kt), 'res5': (2048, 64, kt)}
    n = 0
    for w, o in by_w.items():
        if w.endswith('_branch2b_w'):
            c, cg, k = want[w[:4]]
            assert tuple(model.param_specs[w]['shape']) == (c, cg, k, 3, 3), w
            assert o.args['group'] == 32 and o.args['kernels'] == [k, 3, 3], w
            first_of_strided_stage = w[5] == '0' and w[:4] != 'res2'
            assert o.args['strides'] == ([2, 2] if first_of_strided_stage else [1, 1]), w
            n += 1
        else:
            assert 'group' not in o.args, w
    assert n == 3 + 4 + 6 + 3 and ops
    assert by_w['res3_0_branch2a_w'].args['strides'] == [1, 1]


def test_default_graph_records_no_group():
    model = _create(fpn3d_kps_cfg('50', T=4, kt=3))
    assert all('group' not in o.args for o in model.net.ops if o.type == 'Conv')
    assert tuple(model.param_specs['res2_0_branch2b_w']['shape']) == (64, 64, 1, 3, 3)


def test_group_count_must_divide_both_channel_counts():
    from detectandtrack_amd.modeling.detector import DetectionModelHelper
    m = DetectionModelHelper(train=False, num_classes=2)
    with pytest.raises(AssertionError, match='must divide'):
        m.ConvNd('x', 'y', 96, 128, [1, 3, 3], pads=2 * [0, 1, 1], group=64)
    with pytest.raises(AssertionError, match='must divide'):
        m.ConvNd('x', 'y', 128, 96, [1, 3, 3], pads=2 * [0, 1, 1], group=64)


def test_training_a_grouped_body_is_refused_at_build_time():
    with pytest.raises(NotImplementedError, match=r'grouped data-gradient and weight-gradient kernels'):
        _create(_resnext_cfg(), train=True)


def test_2plus1d_bodies_keep_refusing_groups():
    d = _resnext_cfg()
    d['MODEL']['CONV_BODY'] = 'FPN3D.add_fpn_ResNet50_2plus1d_conv5_body'
    with pytest.raises(AssertionError, match='no groups'):
        _create(d)


@pytest.mark.parametrize('lib', ['libdat_hip.so', 'libdat_hip_f16.so'])
def test_both_library_flavours_export_the_grouped_entry_points(lib):
    h = ctypes.CDLL(os.path.join(REPO, 'detectandtrack_amd', lib))
    for name in NEW_SYMBOLS:
        assert hasattr(h, name), '%s does not export %s' % (lib, name)
    from detectandtrack_amd import libdat
    assert set(NEW_SYMBOLS) <= set(libdat.EXPORTS)


def test_packed_bytes_and_flops_helpers_count_one_group():
    """No GPU needed: the size and FLOPs helpers.  32x8d res5 (2048 channels, 64 per group, 3x3x3): the packed weights hold one
    64-wide slab per output channel -- a 32nd of the dense layer's -- and the FLOPs are 2 * Cout * (Cin / G) * taps * positions."""
    from detectandtrack_amd import libdat as L
    d = L.ConvDesc()
    d.dtype, d.frames, d.T, d.H, d.W, d.Cin, d.Cout, d.out_cstride = L.DAT_BF16, 8, 8, 24, 42, 2048, 2048, 2048
    d.KT, d.KH, d.KW, d.stride_h, d.stride_w, d.pad_t, d.pad_h, d.pad_w = 3, 3, 3, 1, 1, 1, 1, 1
    lib = L.lib()
    dense = lib.dat_conv3d_packed_weight_bytes(ctypes.byref(d))
    assert lib.dat_conv3d_grouped_packed_weight_bytes(ctypes.byref(d), 32) * 32 == dense == 27 * 2048 * 2048 * 2
    assert lib.dat_conv3d_grouped_flops(ctypes.byref(d), 32) == 2.0 * 2048 * 64 * 27 * 8 * 24 * 42
    d.dtype = L.DAT_F32
    assert lib.dat_conv3d_grouped_packed_weight_bytes(ctypes.byref(d), 32) == 27 * 2048 * 64 * 4
    d.dtype = L.DAT_BF16X3
    assert lib.dat_conv3d_grouped_packed_weight_bytes(ctypes.byref(d), 32) == 27 * 2048 * 64 * 3 * 2


def test_reference_helper_agrees_with_torch_grouped_conv():
    """Per-group dense convs concatenated over the groups == torch's conv3d(groups=G) in float64, to 1e-12, fused epilogue included."""
    rs = np.random.RandomState(5)
    N, C, T, H, W, G = 2, 24, 3, 7, 9, 6
    x = rs.randn(N, C, T, H, W)
    w = rs.randn(C, C // G, 3, 3, 3)
    scale, bias = rs.uniform(0.5, 1.5, C), rs.randn(C)
    res = rs.randn(N, C, T, 4, 5)
    ref, absref = grouped_conv_ref64(x, w, G, scale, bias, res, stride=(2, 2), pads=(1, 1, 1), relu=True)
    y = torch.nn.functional.conv3d(torch.from_numpy(x), torch.from_numpy(w), None, stride=(1, 2, 2), padding=(1, 1, 1), groups=G)
    y = torch.relu(y * torch.from_numpy(scale).view(1, -1, 1, 1, 1) + torch.from_numpy(bias).view(1, -1, 1, 1, 1) + torch.from_numpy(res))
    assert ref.dtype == np.float64 and ref.shape == tuple(y.shape) == (N, C, T, 4, 5)
    assert np.abs(ref - y.numpy()).max() < 1e-12
    ya = torch.nn.functional.conv3d(torch.from_numpy(np.abs(x)), torch.from_numpy(np.abs(w)), None, stride=(1, 2, 2), padding=(1, 1, 1),
                                    groups=G)
    ya = ya * torch.from_numpy(scale).view(1, -1, 1, 1, 1) + torch.from_numpy(np.abs(bias)).view(1, -1, 1, 1, 1) + torch.from_numpy(np.abs(res))
    assert np.abs(absref - ya.numpy()).max() < 1e-12
    # a dense conv with the block-diagonal expansion of the same filter is the same function
    wd = np.zeros((C, C, 3, 3, 3))
    cg = C // G
    for co in range(C):
        g = co // cg
        wd[co, g * cg:(g + 1) * cg] = w[co]
    yd = torch.nn.functional.conv3d(torch.from_numpy(x), torch.from_numpy(wd), None, stride=(1, 2, 2), padding=(1, 1, 1))
    ref0, _ = grouped_conv_ref64(x, w, G, stride=(2, 2), pads=(1, 1, 1))
    assert np.abs(ref0 - yd.numpy()).max() < 1e-12


def test_shipped_resnext_config_builds_the_32x8d_body():
    from detectandtrack_amd.core.config import cfg, cfg_from_file, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    reset_cfg()
    cfg_from_file(os.path.join(REPO, 'configs', 'test_x101_32x8d_fpn3d_synthetic.yaml'))
    assert_and_infer_cfg()
    assert cfg.MODEL.CONV_BODY == 'FPN3D.add_fpn_ResNet101_conv5_body'
    assert (cfg.RESNETS.NUM_GROUPS, cfg.RESNETS.WIDTH_PER_GROUP, cfg.RESNETS.STRIDE_1X1) == (32, 8, False)
    model = model_builder.create(cfg.MODEL.TYPE, train=False)
    shp = lambda n: tuple(model.param_specs[n]['shape'])
    assert shp('res4_22_branch2b_w') == (1024, 32, 3, 3, 3) and shp('res5_2_branch2b_w') == (2048, 64, 3, 3, 3)
    assert 'res4_23_branch2b_w' not in model.params


def test_weight_inflation_and_checkpoint_loading_take_grouped_filters(tmp_path):
    """A 2D ResNeXt checkpoint ([out, in / G, k, k] filters) inflates into the 3D body's [out, in / G, kT, k, k] like any other filter."""
    import pickle
    from detectandtrack_amd.utils import net as net_utils

    class WS(object):
        def __init__(self):
            self.params = {}

        def set_param(self, name, v):
            self.params[name] = np.array(v, dtype=np.float32, copy=True)
    model = _create(_resnext_cfg(groups=32, width=4))
    src = net_utils.synthetic_params(model, seed=5)
    flat = {k: (v[:, :, v.shape[2] // 2] if v.ndim == 5 else v) for k, v in src.items()}
    assert flat['res3_0_branch2b_w'].shape == (256, 8, 3, 3)
    path = str(tmp_path / 'x50_2d.pkl')
    with open(path, 'wb') as f:
        pickle.dump({'blobs': flat}, f, protocol=2)
    ws = WS()
    net_utils.initialize_params(model, ws)
    net_utils.initialize_from_weights_file(model, ws, path)
    w = ws.params['res3_0_branch2b_w']
    assert w.shape == (256, 8, 3, 3, 3)
    assert np.array_equal(w[:, :, 1], flat['res3_0_branch2b_w']) and not w[:, :, 0].any() and not w[:, :, 2].any()
