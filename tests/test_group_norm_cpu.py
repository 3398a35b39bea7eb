"""GroupNorm (HIP.USE_GN) without a GPU: the group rule, what the builder records, the parameter sets, the weight file, the float64
restatement against torch, that the bound of the GPU kernel tests tells a cancelling variance from a sound one, and the exports."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

from tests.model_util import fpn3d_kps_cfg
from tests import group_norm_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODIES = ['FPN3D.add_fpn_ResNet18_conv5_body', 'FPN3D.add_fpn_ResNet18_2plus1d_conv5_body']
ENTRY_POINTS = ('dat_gn_workspace_bytes', 'dat_gn_stats', 'dat_gn_apply', 'dat_gn_bwd_reduce', 'dat_gn_bwd_apply')


def _build(body, train, hip=None, **model_kw):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    c = fpn3d_kps_cfg('18', T=2)
    c['MODEL']['CONV_BODY'] = body
    c['MODEL'].update(model_kw)
    c.setdefault('HIP', {}).update(hip or {})
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


def test_group_rule():
    from detectandtrack_amd.modeling.detector import gn_groups
    want = {64: 32, 128: 32, 144: 24, 230: 23, 256: 32, 460: 23, 921: 3, 2048: 32}
    assert {c: gn_groups(c, 32) for c in want} == want
    assert all(ref.groups_of(c) == g for c, g in want.items())
    assert (144 // 24, 230 // 23, 921 // 3) == (6, 10, 307)
    assert gn_groups(64, 8) == 8 and gn_groups(7, 32) == 7 and gn_groups(31, 4) == 1 and gn_groups(1, 32) == 1


def test_defaults_leave_the_switch_off():
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    assert cfg.HIP.USE_GN is False and cfg.HIP.GN_NUM_GROUPS == 32 and cfg.HIP.GN_EPSILON == 1e-5


def _ops(net):
    return [(o.type, list(o.inputs), list(o.outputs), dict(o.args) if isinstance(o.args, dict) else o.args) for o in net.ops]


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('body', BODIES)
def test_graphs_record_one_group_norm_per_affine_site_with_the_folds_of_the_bn_training_graph(body, train):
    aff = _build(body, train)
    gn = _build(body, train, hip={'USE_GN': True})
    bn = _build(body, True, USE_BN=True)            # the BN TRAINING graph: the model of where Sum and ReLU fold
    layers = [p[:-2] for p in aff.params if aff.param_specs[p].get('affine') and p.endswith('_s')]
    assert len(layers) >= 20
    nets = [(gn.net, bn.net)] + ([] if train else [(gn.conv_body_net, None)])
    for gnet, bnet in nets:
        gops = [op for op in gnet.ops if op.type == 'GroupNorm']
        if gnet is gn.net:
            assert sorted(op.args['scale'][:-2] for op in gops) == sorted(layers)
        else:
            assert len(gops) == len(layers)
        for op in gops:
            name = op.args['scale'][:-2]
            C = gn.param_specs[name + '_s']['shape'][0]
            assert op.args['bias'] == name + '_b' and op.args['groups'] == ref.groups_of(C) and op.args['eps'] == 1e-5
            conv = gnet.producer(op.inputs[0])
            assert conv.type == 'Conv' and conv.args['scale'] is None and conv.args['shift'] is None and conv.args['b'] is None
            assert not conv.args['relu'] and conv.args['residual'] is None and conv.args['dim_out'] == C
            assert op.inputs == conv.outputs + ([op.args['residual']] if op.args['residual'] else [])
        if bnet is None:
            continue
        # op for op the BN training graph's body, SpatialBN -> GroupNorm: same blobs, same ReLU and residual folds
        body_g = [o for o in gnet.ops if o.type in ('GroupNorm', 'Conv', 'MaxPool', 'Sum', 'Relu')]
        body_b = [o for o in bnet.ops if o.type in ('SpatialBN', 'Conv', 'MaxPool', 'Sum', 'Relu')]
        n_folded = 0
        bn_by_name = {o.args['scale']: o for o in body_b if o.type == 'SpatialBN'}
        for o in gops:
            b = bn_by_name[o.args['scale']]
            assert (o.inputs, o.outputs, o.args['relu'], o.args['residual']) == (b.inputs, b.outputs, b.args['relu'], b.args['residual'])
            n_folded += bool(o.args['residual'])
        assert n_folded == 8                # one shortcut Sum per basic block of an R-18 body
        assert not any(o.type in ('Sum', 'Relu') for o in body_g if o.outputs[0].startswith('res'))
        if train:
            assert [(o.type.replace('SpatialBN', 'GroupNorm'), o.inputs, o.outputs) for o in bnet.ops] == \
                [(o.type, o.inputs, o.outputs) for o in gnet.ops]
    # parameters: exactly the affine model's, scale a weight and bias a bias, trainable, no computed parameters
    assert list(gn.params) == list(aff.params) and gn.computed_params == []
    trainable = set(gn.TrainableParams())
    for n in layers:
        assert n + '_s' in gn.weights and n + '_b' in gn.biases
        assert not gn.param_specs[n + '_s'].get('affine') and not gn.param_specs[n + '_b'].get('affine')
        assert gn.param_specs[n + '_s']['init'] == ('ConstantFill', {'value': 1.}) and gn.param_specs[n + '_b']['init'] == ('ConstantFill', {'value': 0.})
        assert n + '_s' in trainable and n + '_b' in trainable
    assert set(aff.TrainableParams()) <= trainable


def test_mid_planes_of_the_2plus1d_body_get_their_group_counts():
    gn = _build(BODIES[1], False, hip={'USE_GN': True})
    by_c = {}
    for op in gn.net.ops:
        if op.type == 'GroupNorm':
            by_c[gn.param_specs[op.args['scale']]['shape'][0]] = op.args['groups']
    # (res2 has no temporal extent in this body, so the 144-plane mid layer of a full (2+1)D res2 does not occur; the group rule covers it)
    assert by_c[230] == 23 and by_c[460] == 23 and by_c[921] == 3
    assert by_c[64] == by_c[128] == by_c[256] == by_c[512] == by_c[288] == by_c[576] == by_c[1152] == 32
    few = _build(BODIES[1], False, hip={'USE_GN': True, 'GN_NUM_GROUPS': 8})
    assert {op.args['groups'] for op in few.net.ops if op.type == 'GroupNorm'} <= set(range(1, 9))


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('body', BODIES)
def test_switch_off_records_the_graph_of_the_defaults_op_for_op(body, train):
    plain = _build(body, train)
    off = _build(body, train, hip={'USE_GN': False, 'GN_NUM_GROUPS': 8, 'GN_EPSILON': 1e-3})
    pairs = [(plain.net, off.net)] + ([] if train else [(plain.conv_body_net, off.conv_body_net), (plain.keypoint_net, off.keypoint_net)])
    for a, b in pairs:
        assert len(a.ops) == len(b.ops) and not any(o.type == 'GroupNorm' for o in b.ops)
        for oa, ob in zip(_ops(a), _ops(b)):
            assert oa[:3] == ob[:3] and sorted(oa[3]) == sorted(ob[3])
            assert all(np.array_equal(oa[3][k], ob[3][k]) for k in oa[3]), oa
    assert list(plain.params) == list(off.params) and plain.TrainableParams() == off.TrainableParams()


def test_both_switches_together_raise():
    with pytest.raises(ValueError, match='USE_GN and MODEL.USE_BN'):
        _build(BODIES[0], True, hip={'USE_GN': True}, USE_BN=True)
    with pytest.raises(ValueError, match='USE_GN and MODEL.USE_BN'):
        _build(BODIES[0], False, hip={'USE_GN': True}, USE_BN=True)


def test_share_with_raises_as_for_spatial_bn():
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.modeling.detector import DetectionModelHelper
    reset_cfg()
    cfg.HIP.USE_GN = True
    m = DetectionModelHelper(train=False)
    m.ConvNd('data', 'c', 3, 8, [1, 3, 3], no_bias=1)
    with pytest.raises(NotImplementedError, match='Handle that'):
        m.AffineChannelNd('c', 'c_bn', 8, share_with='other_bn')
    assert m.AffineChannelNd('c', 'c_bn', 8) == 'c_bn'
    op = m.net.ops[-1]
    assert op.type == 'GroupNorm' and op.args['groups'] == 8 and m.Relu('c_bn', 'c_bn') == 'c_bn' and op.args['relu']


def test_a_net_with_group_norm_refuses_frame_subset_forwards():
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.workspace import check_bn_sees_every_frame
    for train in (True, False):
        model = _build(BODIES[0], train, hip={'USE_GN': True})
        check_bn_sees_every_frame(model.net)
        for key, val in (('KEYFRAME_DCE', True), ('FRAME_TRUNK_CACHE', 4)):
            old = cfg.HIP[key]
            cfg.HIP[key] = val
            with pytest.raises(ValueError, match='every frame of the clip'):
                check_bn_sees_every_frame(model.net)
            cfg.HIP[key] = old


class _HostWorkspace(object):
    def __init__(self):
        self.params = {}

    def set_param(self, name, arr):
        self.params[name] = np.asarray(arr, dtype=np.float32)


def test_weight_file_round_trips_scale_and_bias_and_synthetic_values_are_no_identity(tmp_path):
    from detectandtrack_amd.utils import net as net_utils
    gn = _build(BODIES[1], True, hip={'USE_GN': True})
    weights = net_utils.synthetic_params(gn, 3)
    sb = sorted(n for n in gn.params if gn.param_specs[n].get('gn'))
    assert len(sb) == 2 * 32
    for n in sb:
        assert weights[n].std() > 0 and (np.all(weights[n] != 1) if n.endswith('_s') else np.abs(weights[n]).max() > 0), n
    plain = net_utils.synthetic_params(_build(BODIES[1], True), 3)      # the same seed: the same values with and without the switch
    assert sorted(plain) == sorted(weights) and all(np.array_equal(plain[k], weights[k]) for k in plain)
    ws = _HostWorkspace()
    for k, v in weights.items():
        ws.set_param(k, v)
    path = str(tmp_path / 'gn.pkl')
    gn = _build(BODIES[1], True, hip={'USE_GN': True})
    net_utils.save_model_to_weights_file(path, gn, ws, {n: np.full_like(weights[n], 0.25) for n in gn.TrainableParams()})
    blobs = net_utils.load_weights_file(path)
    assert all(np.array_equal(blobs[n], weights[n]) and n + '_momentum' in blobs for n in sb)
    ws2 = _HostWorkspace()
    assert net_utils.initialize_from_weights_file(gn, ws2, path) == []
    assert all(np.array_equal(ws2.params[n], weights[n]) for n in gn.params)


@pytest.mark.parametrize('C,G', [(64, 32), (144, 24), (24, 1), (921, 3)])
def test_restatement_agrees_with_torch_group_norm_and_its_autograd_in_float64(C, G):
    rs = np.random.RandomState(C)
    N, T, H, W, eps = 2, 2, 3, 4, 1e-5
    z = rs.randn(N, T * H * W, C) * rs.uniform(0.5, 3, C) + rs.randn(C) * 2 + np.array([10.0, -5.0])[:, None, None]
    s, b, dy = rs.uniform(0.5, 1.5, C), rs.randn(C) * 0.3, rs.randn(N, T * H * W, C)
    ncdhw = lambda a: torch.from_numpy(a.reshape(N, T, H, W, C).transpose(0, 4, 1, 2, 3).copy())
    back = lambda t: t.numpy().transpose(0, 2, 3, 4, 1).reshape(N, T * H * W, C)
    zt, st, bt = ncdhw(z).requires_grad_(True), torch.from_numpy(s).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    y = torch.nn.functional.group_norm(zt, G, st, bt, eps)
    y.backward(ncdhw(dy))
    y64 = ref.forward_ref64(z, G, s, b, eps)[0]
    np.testing.assert_allclose(y64, back(y.detach()), rtol=1e-11, atol=1e-11)
    dz, ds, db = ref.full_backward_ref64(dy, z, G, s, eps)
    np.testing.assert_allclose(dz, back(zt.grad), rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(ds, st.grad.numpy(), rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-10, atol=1e-11)
    # the tables: a, b' reproduce y
    (mu, rstd, a, bp), _ = ref.table_bounds(z, G, s, b, eps)
    np.testing.assert_allclose(z * a[:, None] + bp[:, None], y64, rtol=1e-9, atol=1e-9)
    # each clip alone gives the same tables
    one = ref.table_bounds(z[1:], G, s, b, eps)[0]
    assert all(np.array_equal(t[0], u[1]) for t, u in zip(one, (mu, rstd, a, bp)))


def test_the_kernel_bound_rejects_a_cancelling_variance_and_accepts_two_pass():
    """The offset case of tests/test_gpu_group_norm.py (z = 100 + 0.5 N(0, 1), 512 positions x 2 channels per group): y from an fp32
    E[x^2] - mu^2 variance falls outside the per-element bound the GPU test holds dat_gn_apply to; y from an fp32 two-pass variance
    is inside it."""
    eps, G = 1e-5, 32
    z = ref.offset_case()
    C = z.shape[2]
    rs = np.random.RandomState(2)
    s, b = rs.uniform(0.5, 1.0, C).astype(np.float32), (rs.randn(C) * 0.1).astype(np.float32)
    zg = ref._grouped(z, G)[0]

    def y_fp32(var_fn):
        stats = [var_fn(zg[g]) for g in range(G)]
        mu = np.repeat(np.array([m for m, _ in stats], np.float32), C // G)
        var = np.repeat(np.array([v for _, v in stats], np.float32), C // G)
        rstd = (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)
        a = s * rstd
        return z * a + (b - mu * a), var
    r = ref.stats_ref64(z, G, eps)
    y2, var2 = y_fp32(ref.two_pass_var_fp32)
    worst = ref.check_forward(y2, z, G, s, b, eps, 'fp32', 'two-pass fp32')
    y1, var1 = y_fp32(ref.naive_var_fp32)
    rel1, rel2 = np.abs(var1 - r['var'][0]) / r['var'][0], np.abs(var2 - r['var'][0]) / r['var'][0]
    print('relative variance error: E[x^2] - mu^2 %.3e (median %.3e), two-pass %.3e; two-pass y err/bound %.3f'
          % (rel1.max(), np.median(rel1), rel2.max(), worst))
    with pytest.raises(AssertionError, match='outside the per-element bound'):
        ref.check_forward(y1, z, G, s, b, eps, 'fp32', 'E[x^2] - mu^2 fp32')
    _, d_var, _ = ref.stats_bounds(z, G, eps)
    assert np.all(np.abs(var2 - r['var'][0]) <= d_var[0] + 2 * ref.U32 * r['var'][0]) and np.any(np.abs(var1 - r['var'][0]) > 10 * d_var[0])


@pytest.mark.parametrize('flavour', ['libdat_hip.so', 'libdat_hip_f16.so'])
def test_both_library_flavours_export_the_entry_points(flavour):
    path = os.path.join(REPO, 'detectandtrack_amd', flavour)
    assert os.path.exists(path), path + ' (build() makes it)'
    lib = ctypes.CDLL(path)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), '%s does not export %s' % (flavour, name)
    lib.dat_gn_workspace_bytes.restype = ctypes.c_size_t
    lib.dat_gn_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int]
    one, three = lib.dat_gn_workspace_bytes(0, 1, 70, 192), lib.dat_gn_workspace_bytes(0, 3, 70, 192)
    assert one > 0 and three == 3 * one and lib.dat_gn_workspace_bytes(0, 1, 70, 100) == 0 and lib.dat_gn_workspace_bytes(0, 0, 70, 64) == 0
    from detectandtrack_amd import libdat
    assert all(n in libdat._PROTOS for n in ENTRY_POINTS)
    with open(os.path.join(REPO, 'include', 'dat_hip.h')) as f:
        header = f.read()
    assert all(n + '(' in header for n in ENTRY_POINTS)


def test_the_shipped_configs_name_the_body_and_the_switch():
    from detectandtrack_amd.core.config import cfg, cfg_from_file, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    for fn, train in (('train_r18_2plus1d_fpn3d_gn_synthetic.yaml', True), ('test_r18_2plus1d_fpn3d_gn_synthetic.yaml', False)):
        with open(os.path.join(REPO, 'configs', fn)) as f:
            c = yaml.safe_load(f)
        assert c['MODEL']['CONV_BODY'] == 'FPN3D.add_fpn_ResNet18_2plus1d_conv5_body' and c['HIP']['USE_GN'] is True
        assert not c['MODEL'].get('USE_BN', False) and c['HIP']['DTYPE'] in ('bf16', 'fp32')
        assert not c['HIP'].get('KEYFRAME_DCE', False) and not c['HIP'].get('FRAME_TRUNK_CACHE', 0)
        reset_cfg()
        cfg_from_file(os.path.join(REPO, 'configs', fn))
        assert_and_infer_cfg()
        model = model_builder.create(cfg.MODEL.TYPE, train=train)
        assert sum(op.type == 'GroupNorm' for op in model.net.ops) == 32
        assert {op.args['groups'] for op in model.net.ops if op.type == 'GroupNorm'} == {32, 23, 3}
