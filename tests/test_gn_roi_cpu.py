"""GroupNorm on per-RoI blobs without a GPU: what the builder records for the C4 res5 head and for HIP.GN_KPS_HEAD, that the switch off
changes nothing, the exports, the shipped configs, and the float64 references on the [R, C, Tr, H, W] view against torch."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

from tests.model_util import fpn3d_kps_cfg, c4_tube_kps_cfg, fpn3d_tube_kps_cfg
from tests import group_norm_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('dat_gn_roi_fwd', 'dat_gn_roi_bwd', 'dat_gn_roi_workspace_bytes')
# (output, input, ReLU folded, residual) of the GroupNorm ops behind RoIFeatureTransform in the C4 R-18 model, in graph order
C4_ROI_OPS = [('res5_0_branch2a_bn', 'res5_0_branch2a', True, None),
              ('res5_0_branch1_bn', 'res5_0_branch1', False, None),
              ('res5_0_branch2b_bn', 'res5_0_branch2b', True, 'res5_0_branch1_bn'),
              ('res5_1_branch2a_bn', 'res5_1_branch2a', True, None),
              ('res5_1_sum', 'res5_1_branch2b', True, 'res5_0_branch2b_bn')]


def _build(c, train):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    if train:
        c['TRAIN'] = {'IMS_PER_BATCH': 1}
        c['NUM_GPUS'] = 1
    reset_cfg()
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    return model_builder.create(cfg.MODEL.TYPE, train=train)


@pytest.fixture(autouse=True)
def _restore_cfg():
    yield
    from detectandtrack_amd.core.config import reset_cfg
    reset_cfg()


def _nets(model, train):
    return [model.net] + ([] if train else [model.conv_body_net, model.keypoint_net])


def _ops(net):
    return [(o.type, list(o.inputs), list(o.outputs), dict(o.args) if isinstance(o.args, dict) else o.args) for o in net.ops]


def _per_roi_group_norms(net):
    """The GroupNorm ops whose input descends from a RoIFeatureTransform."""
    roi = set()
    for op in net.ops:
        if op.type == 'RoIFeatureTransform' or any(i in roi for i in op.inputs):
            roi.update(op.outputs)
    return [op for op in net.ops if op.type == 'GroupNorm' and op.inputs[0] in roi]


def _with_hip(c, **hip):
    c['HIP'].update(hip)
    return c


def test_defaults_leave_the_switch_off():
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    assert cfg.HIP.GN_KPS_HEAD is False and cfg.HIP.USE_GN is False


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('make', [fpn3d_kps_cfg, fpn3d_tube_kps_cfg])
@pytest.mark.parametrize('use_gn', [False, True])
def test_switch_off_records_the_graphs_and_parameters_of_the_defaults(make, train, use_gn):
    plain = _build(_with_hip(make(T=2), USE_GN=use_gn), train)
    off = _build(_with_hip(make(T=2), USE_GN=use_gn, GN_KPS_HEAD=False), train)
    for a, b in zip(_nets(plain, train), _nets(off, train)):
        assert len(a.ops) == len(b.ops)
        for oa, ob in zip(_ops(a), _ops(b)):
            assert oa[:3] == ob[:3] and sorted(oa[3]) == sorted(ob[3])
            assert all(np.array_equal(oa[3][k], ob[3][k]) for k in oa[3]), oa
        assert not any(o.type == 'GroupNorm' and o.outputs[0].startswith('conv_fcn') for o in b.ops)
    assert list(plain.params) == list(off.params) and plain.TrainableParams() == off.TrainableParams()
    assert {n: plain.param_specs[n] for n in plain.params} == {n: off.param_specs[n] for n in off.params}


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('make', [fpn3d_kps_cfg, fpn3d_tube_kps_cfg])
def test_switch_on_normalises_every_layer_of_the_keypoint_head(make, train):
    from detectandtrack_amd.core.config import cfg
    base = _build(_with_hip(make(T=2), USE_GN=True), train)
    gn = _build(_with_hip(make(T=2), USE_GN=True, GN_KPS_HEAD=True), train)
    n = int(cfg.KRCNN.NUM_STACKED_CONVS)
    net = gn.net if train else gn.keypoint_net
    ops = [o for o in net.ops if o.type == 'GroupNorm' and o.outputs[0].startswith('conv_fcn')]
    assert [o.outputs[0] for o in ops] == ['conv_fcn%d_gn' % (i + 1) for i in range(n)] == [o.outputs[0] for o in _per_roi_group_norms(net)
                                                                                             if o.outputs[0].startswith('conv_fcn')]
    trainable = set(gn.TrainableParams())
    for i, o in enumerate(ops):
        name = 'conv_fcn%d' % (i + 1)
        conv = net.producer(o.inputs[0])
        assert conv.type == 'Conv' and conv.outputs == [name] and conv.args['b'] is None and not conv.args['relu']
        assert conv.args['scale'] is None and conv.args['shift'] is None and conv.args['dim_out'] == cfg.KRCNN.CONV_HEAD_DIM
        assert o.inputs == [name] and o.args['relu'] and o.args['residual'] is None
        assert o.args['groups'] == ref.groups_of(cfg.KRCNN.CONV_HEAD_DIM) and o.args['eps'] == 1e-5
        assert (o.args['scale'], o.args['bias']) == (name + '_gn_s', name + '_gn_b')
        assert name + '_gn_s' in gn.weights and name + '_gn_b' in gn.biases and name + '_b' not in gn.params
        assert gn.param_specs[name + '_gn_s']['init'] == ('ConstantFill', {'value': 1.})
        assert gn.param_specs[name + '_gn_b']['init'] == ('ConstantFill', {'value': 0.})
        assert {name + '_w', name + '_gn_s', name + '_gn_b'} <= trainable
    assert not any(o.type == 'Relu' and o.inputs[0].startswith('conv_fcn') for o in net.ops)
    # nothing else moved: the other parameters are the base model's
    drop = {'conv_fcn%d_b' % (i + 1) for i in range(n)}
    add = {'conv_fcn%d_gn_%s' % (i + 1, k) for i in range(n) for k in 'sb'}
    assert set(gn.params) == (set(base.params) - drop) | add
    for a, b in zip(_nets(gn, train), _nets(base, train)):      # (the op behind the head reads conv_fcn<n>_gn: types and outputs compared)
        rest = lambda net: [(o.type, o.outputs) for o in net.ops if not o.outputs[0].startswith('conv_fcn')]
        assert rest(a) == rest(b)


def test_the_switch_needs_use_gn():
    with pytest.raises(ValueError, match='GN_KPS_HEAD needs HIP.USE_GN'):
        _build(_with_hip(fpn3d_kps_cfg(T=2), GN_KPS_HEAD=True), False)
    with pytest.raises(ValueError, match='GN_KPS_HEAD needs HIP.USE_GN'):
        _build(_with_hip(fpn3d_kps_cfg(T=2), GN_KPS_HEAD=True), True)


@pytest.mark.parametrize('train', [True, False])
def test_c4_model_records_exactly_the_five_per_roi_ops(train):
    model = _build(_with_hip(c4_tube_kps_cfg(T=3), USE_GN=True), train)
    assert sum(o.type == 'GroupNorm' for o in model.net.ops) == 20
    got = [(o.outputs[0], o.inputs[0], bool(o.args['relu']), o.args['residual']) for o in _per_roi_group_norms(model.net)]
    assert got == C4_ROI_OPS
    for o in _per_roi_group_norms(model.net):
        assert o.args['groups'] == 32 and model.net.producer(o.inputs[0]).type == 'Conv'
    trainable = set(model.TrainableParams())
    assert all(o.args['scale'] in trainable and o.args['bias'] in trainable for o in _per_roi_group_norms(model.net))
    if not train:
        assert _per_roi_group_norms(model.conv_body_net) == [] and _per_roi_group_norms(model.keypoint_net) == []


def test_the_blob_flag_exists_and_defaults_to_false():
    """(The executor sets it in op_RoIFeatureTransform and carries it with `count`: tests/test_gpu_gn_roi_model.py runs that.)"""
    from detectandtrack_amd.workspace import Blob
    assert 'roi' in Blob.__slots__ and Blob(None, 'fmap').roi is False


@pytest.mark.parametrize('flavour', ['libdat_hip.so', 'libdat_hip_f16.so'])
def test_both_library_flavours_export_the_entry_points(flavour):
    path = os.path.join(REPO, 'detectandtrack_amd', flavour)
    assert os.path.exists(path), path + ' (build() makes it)'
    lib = ctypes.CDLL(path)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), '%s does not export %s' % (flavour, name)
    lib.dat_gn_roi_workspace_bytes.restype = ctypes.c_size_t
    lib.dat_gn_roi_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    assert lib.dat_gn_roi_workspace_bytes(1000, 512) > 0 and lib.dat_gn_roi_workspace_bytes(1000, 512) == lib.dat_gn_roi_workspace_bytes(1, 512)
    assert lib.dat_gn_roi_workspace_bytes(4, 100) == 0 and lib.dat_gn_roi_workspace_bytes(0, 64) == 0
    from detectandtrack_amd import libdat
    assert all(n in libdat._PROTOS for n in ENTRY_POINTS)
    with open(os.path.join(REPO, 'include', 'dat_hip.h')) as f:
        header = f.read()
    assert all(n + '(' in header for n in ENTRY_POINTS)


def test_the_shipped_configs_build_and_name_the_switches():
    from detectandtrack_amd.core.config import cfg, cfg_from_file, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    for fn, train, n_roi in (('train_r18_c4_tube_gn_synthetic.yaml', True, 5), ('test_r18_c4_tube_gn_synthetic.yaml', False, 5),
                             ('train_r18_fpn3d_gn_kps_head_synthetic.yaml', True, 8)):
        with open(os.path.join(REPO, 'configs', fn)) as f:
            c = yaml.safe_load(f)
        assert c['HIP']['USE_GN'] is True and not c['MODEL'].get('USE_BN', False)
        assert bool(c['HIP'].get('GN_KPS_HEAD', False)) == (n_roi == 8)
        reset_cfg()
        cfg_from_file(os.path.join(REPO, 'configs', fn))
        assert_and_infer_cfg()
        model = model_builder.create(cfg.MODEL.TYPE, train=train)
        assert len(_per_roi_group_norms(model.net)) == n_roi


@pytest.mark.parametrize('C,G', [(64, 32), (144, 24), (921, 3)])
def test_references_agree_with_torch_group_norm_on_the_roi_view_with_dead_rois_masked_out(C, G):
    """tests/group_norm_ref.py with N = R is torch.nn.functional.group_norm on [R, C, Tr, H, W], forward and autograd; dead RoIs (their
    output and their upstream gradient masked to zero) contribute nothing to dscale / dbias and get dz = 0."""
    rs = np.random.RandomState(C)
    R, Tr, H, W, eps = 5, 2, 3, 4, 1e-5
    M = Tr * H * W
    z = rs.randn(R, M, C) * rs.uniform(0.5, 3, C) + rs.randn(C) * 2 + np.array([100.0, -50.0, 0.0, 3.0, -7.0])[:, None, None]
    s, b, dy = rs.uniform(0.5, 1.5, C), rs.randn(C) * 0.3, rs.randn(R, M, C)
    live = np.array([True, False, True, True, False])
    ncdhw = lambda a: torch.from_numpy(a.reshape(R, Tr, H, W, C).transpose(0, 4, 1, 2, 3).copy())
    back = lambda t: t.numpy().transpose(0, 2, 3, 4, 1).reshape(R, M, C)
    zt, st, bt = ncdhw(z).requires_grad_(True), torch.from_numpy(s).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    mask = torch.from_numpy(live.astype(np.float64)).view(R, 1, 1, 1, 1)
    y = torch.nn.functional.group_norm(zt, G, st, bt, eps) * mask
    y.backward(ncdhw(dy))
    y64 = ref.forward_ref64(z, G, s, b, eps)[0] * live[:, None, None]
    np.testing.assert_allclose(y64, back(y.detach()), rtol=1e-11, atol=1e-11)
    # the kernel's formulation: per-RoI tables [R, G], sums per (RoI, channel), dz from them; dead RoIs zeroed
    r = ref.stats_ref64(z, G, eps)
    sm = ref.backward_sums_ref64(dy, None, z, r['mu'], r['rstd'], 0, M, False)
    dz = ref.backward_dz_ref64(sm['g'], z, G, s, r['mu'], r['rstd'], sm['S1'], sm['S2'], 0)[0] * live[:, None, None]
    np.testing.assert_allclose(dz, back(zt.grad), rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose((sm['S2'] * live[:, None]).sum(axis=0), st.grad.numpy(), rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose((sm['S1'] * live[:, None]).sum(axis=0), bt.grad.numpy(), rtol=1e-10, atol=1e-11)
    assert np.all(back(zt.grad)[~live] == 0)
    # every RoI alone gives the same tables
    for k in range(R):
        one = ref.stats_ref64(z[k:k + 1], G, eps)
        assert all(np.array_equal(one[key][0], r[key][k]) for key in ('mu', 'rstd'))
