"""Training of the spacetime non-local block (HIP.TRAIN_NONLOCAL) without a GPU: the float64 gradient formulas
against torch autograd in double, the max-pool backward against `F.max_pool2d` autograd on inputs with planted ties, the per-element
bound against a faithful fp32 simulation of the two backward kernels and against every named defect (the bound must hold the first and
refuse the others), the exported signatures, and the builder: the switch, the trainable closing affine, the untouched test-mode graph."""
import numpy as np
import pytest
import torch

from tests import nonlocal_grad_ref as G
from tests import numerics as nm
from tests.model_util import fpn3d_kps_cfg

FORMATS = ('fp32', 'bf16', 'fp16')
SIM_CASES = tuple(n for n in G.GRAD_CASES if n != 'many_tiles') + ('many_tiles',)

_REFS = {}


def _case(name, fmt):
    if (name, fmt) not in _REFS:
        q, k, v, dy, scale, clips = G.make_grad_case(name, fmt)
        ref = G.reference(q, k, v, dy, scale, clips)
        _REFS[(name, fmt)] = (q, k, v, dy, scale, clips, ref, G.bounds(ref, fmt))
    return _REFS[(name, fmt)]


# ---- reference ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ragged', 'clips', 'big', 'growing'])
def test_float64_formulas_equal_autograd_in_double(name):
    q, k, v, dy, scale, clips, ref, _ = _case(name, 'fp32')
    L = q.shape[0] // clips
    tq, tk, tv = (torch.from_numpy(a).double().reshape(clips, -1, a.shape[1]).requires_grad_(True) for a in (q, k, v))
    y = torch.einsum('cij,cjd->cid', torch.softmax(torch.einsum('cid,cjd->cij', tq, tk) * scale, dim=2), tv)
    y.backward(torch.from_numpy(dy).double().reshape(clips, L, -1))
    for n, t in (('dq', tq), ('dk', tk), ('dv', tv)):
        want = t.grad.reshape(-1, t.shape[2]).numpy()
        np.testing.assert_allclose(ref[n], want, rtol=1e-10, atol=1e-12 * np.abs(want).max())
    np.testing.assert_allclose(ref['y'], y.detach().reshape(clips * L, -1).numpy(), rtol=1e-12, atol=1e-13)
    s = (torch.einsum('cid,cjd->cij', tq, tk) * scale).detach()
    np.testing.assert_allclose(ref['lse'], (torch.logsumexp(s, dim=2) * G.LOG2E).reshape(-1).numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('k,stride,pad', [(2, 2, 0), (1, 2, 0), (2, 3, 1)])
def test_pool_backward_equals_max_pool2d_autograd_with_ties_and_odd_maps(k, stride, pad):
    g = torch.Generator().manual_seed(7)
    x = torch.randn((2, 9, 11, 16), generator=g, dtype=torch.float64)
    x[:, 2:4, 4:6, :] = 0.25                        # a window of four equal values
    x[:, 0, 1, ::2] = x[:, 0, 0, ::2] = 7.0         # two equal maxima side by side
    x[:, 5, 6, 1::3] = x[:, 4, 7, 1::3] = 9.0       # ... and on the diagonal
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = torch.nn.functional.max_pool2d(xt, kernel_size=k, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    got = G.maxpool_bwd(x.numpy(), dy.permute(0, 2, 3, 1).numpy(), k, stride, pad)
    assert np.array_equal(got, xt.grad.permute(0, 2, 3, 1).numpy())
    if (k, stride, pad) == (2, 2, 0):
        assert (got[:, 8] == 0).all() and (got[:, :, 10] == 0).all() and (got != 0).any()


# ---- bound against the simulation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('name', SIM_CASES)
def test_faithful_simulation_is_inside_the_bound(name, fmt):
    q, k, v, dy, scale, clips, ref, bnd = _case(name, fmt)
    dq, dk, dv, lse = G.simulate(q, k, v, dy, scale, fmt, clips)
    for n, got in (('dq', dq), ('dk', dk), ('dv', dv)):
        worst = G.check(got, ref, bnd, n, name, fmt)
        assert worst <= 0.8, 'the bound of %s has lost its room: %.3f' % (n, worst)
    assert (np.abs(lse - ref['lse']) <= G.lse_bound(ref)).all()


def _ratios(name, fmt, **kw):
    q, k, v, dy, scale, clips, ref, bnd = _case(name, fmt)
    dq, dk, dv, _ = G.simulate(q, k, v, dy, scale, fmt, clips, **kw)
    return {n: G.worst_ratio(got, ref, bnd, n) for n, got in (('dq', dq), ('dk', dk), ('dv', dv))}


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('defect,name,outs', [('rowmax', 'ragged', ('dq', 'dk', 'dv')), ('rowmax', 'blocks', ('dq', 'dk', 'dv')),
                                              ('no_delta', 'ragged', ('dq', 'dk')), ('no_delta', 'd512', ('dq', 'dk')),
                                              ('no_scale_dq', 'ragged', ('dq',)), ('no_scale_dk', 'ragged', ('dk',)),
                                              ('no_scale_dq', 'd512', ('dq',)), ('no_scale_dk', 'd512', ('dk',)),
                                              ('neighbour_clip', 'clips', ('dq', 'dk', 'dv'))])
def test_named_defects_are_outside_the_bound(defect, name, outs, fmt):
    r = _ratios(name, fmt, defect=defect)
    for n in outs:
        assert r[n] > 2.0, '%s on %s (%s): %s err / bound only %.2f' % (defect, name, fmt, n, r[n])


@pytest.mark.parametrize('fmt', FORMATS)
def test_every_single_dropped_tile_is_outside_the_bound(fmt):
    """ragged (70 queries, 45 keys, tiles of 32): each key tile missing from dq, each query tile missing from dk and dv."""
    q = _case('ragged', fmt)[0]
    k = _case('ragged', fmt)[1]
    for t in range((k.shape[0] + 31) // 32):
        r = _ratios('ragged', fmt, drop_key=t)
        assert r['dq'] > 2.0 and r['dk'] <= 1.0 and r['dv'] <= 1.0, (t, r)
    for t in range((q.shape[0] + 31) // 32):
        r = _ratios('ragged', fmt, drop_query=t)
        assert r['dk'] > 2.0 and r['dv'] > 2.0 and r['dq'] <= 1.0, (t, r)


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
def test_truncated_ds_is_caught_by_the_mean_signed_error(fmt):
    """On the same-sign case every term dS_ij k_jd of dq is positive: a dS rounded to nearest leaves the mean signed error of dq near
    zero, a truncated dS pulls it clearly below -- inside or outside the worst-case bound."""
    q, k, v, dy, scale, clips = G.make_same_sign_case(fmt)
    ref = G.reference(q, k, v, dy, scale, clips)
    c = ref['clips'][0]
    assert ((c['dS'] * c['k'][:, :1].T) > 0).mean() > 0.99, 'the case lost its sign pattern'
    u = nm.unit_roundoff(fmt)
    good = G.truncation_statistic(G.simulate(q, k, v, dy, scale, fmt)[0], ref) / u
    bad = G.truncation_statistic(G.simulate(q, k, v, dy, scale, fmt, defect='truncate_ds')[0], ref) / u
    assert abs(good) <= 0.1, good
    assert bad < -0.3, bad


# ---- exports --------------------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_declared_and_bound():
    from detectandtrack_amd import libdat
    from detectandtrack_amd.ops import hip_ops
    for name in ('dat_nonlocal_attention_lse', 'dat_nonlocal_attention_bwd', 'dat_maxpool_hw_bwd'):
        assert name in libdat.EXPORTS, name
    assert [f[0] for f in libdat.NonLocalBwdDesc._fields_] == ['dtype', 'clips', 'Lq', 'Lk', 'D', 'ldq', 'ldk', 'ldv', 'ldy', 'lddy', 'lddq',
                                                              'lddk', 'lddv', 'scale']
    for f in ('nonlocal_attention_lse', 'nonlocal_attention_bwd', 'maxpool_hw_bwd'):
        assert callable(getattr(hip_ops, f))


# ---- builder --------------------------------------------------------------------------------------------------------------------------------
def _model(arch, spec, train=False, hip=None, model=None):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    d = fpn3d_kps_cfg(arch, T=4)
    d['HIP']['NONLOCAL'] = spec
    d['HIP'].update(hip or {})
    d['MODEL'].update(model or {})
    reset_cfg()
    cfg_from_cfg(d)
    assert_and_infer_cfg()
    return model_builder.create(cfg.MODEL.TYPE, train=train)


@pytest.fixture(autouse=True)
def _reset():
    yield
    from detectandtrack_amd.core.config import reset_cfg
    reset_cfg()


def _graph(net):
    return [(op.type, tuple(op.inputs), tuple(op.outputs), repr(sorted((k, repr(v)) for k, v in op.args.items()))) for op in net.ops]


def test_the_switch_defaults_to_off_and_the_refusal_names_it():
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    assert cfg.HIP.TRAIN_NONLOCAL is False
    with pytest.raises(NotImplementedError, match='backward of the fused attention and of its 2 x 2 max-pool.*HIP.TRAIN_NONLOCAL'):
        _model('18', 'res4_1', train=True)


SPEC = 'res3_1,res4_0'
BLOCK_PARAMS = [nl + s for nl in ('nonlocal_res3_1', 'nonlocal_res4_0')
                for s in ('_theta_w', '_theta_b', '_phi_w', '_phi_b', '_g_w', '_g_b', '_out_w', '_out_bn_s', '_out_bn_b')]


@pytest.mark.parametrize('norm', ['affine', 'bn', 'gn'])
def test_the_training_graph_builds_and_every_block_parameter_trains(norm):
    from detectandtrack_amd.training import param_ready_index
    kw = {'affine': {}, 'bn': {'model': {'USE_BN': True}}, 'gn': {'hip': {'USE_GN': True}}}[norm]
    hip = dict(kw.get('hip', {}), TRAIN_NONLOCAL=True)
    model = _model('18', SPEC, train=True, hip=hip, model=kw.get('model'))
    trainable = set(model.TrainableParams())
    assert not [p for p in BLOCK_PARAMS if p not in trainable]
    ready = param_ready_index(model.net)
    tail_type = {'affine': 'AffineTrain', 'bn': 'SpatialBN', 'gn': 'GroupNorm'}[norm]
    for nl, x, out in (('nonlocal_res3_1', 'res3_1_sum_nl_in', 'res3_1_sum'), ('nonlocal_res4_0', None, 'nonlocal_res4_0_sum')):
        x = x or model.net.producer(nl + '_theta').inputs[0]
        tail = model.net.producer(out)
        assert tail.type == tail_type and tail.inputs == [nl + '_out', x] and tail.args['residual'] == x and not tail.args['relu']
        assert tail.args['scale'] == nl + '_out_bn_s' and tail.args['bias'] == nl + '_out_bn_b'
        assert model.param_specs[nl + '_out_bn_s']['init'] == ('ConstantFill', {'value': 0.})
        assert not model.param_specs[nl + '_out_bn_s'].get('affine')
        conv = model.net.producer(nl + '_out')
        assert conv.type == 'Conv' and conv.args['scale'] is None and conv.args['residual'] is None and conv.inputs == [nl + '_y']
        # the parameters' gradients are final at the op that uses them, above the frozen trunk
        assert ready[nl + '_out_bn_s'] == ready[nl + '_out_bn_b'] == model.net.ops.index(tail) < len(model.net.ops)
        # the block input has four readers: theta, phi, g and the residual
        readers = [op for op in model.net.ops if x in op.inputs]
        assert len(readers) == 4 and tail in readers


@pytest.mark.parametrize('norm', ['affine', 'bn', 'gn'])
def test_test_mode_graphs_do_not_depend_on_the_switch(norm):
    kw = {'affine': {}, 'bn': {'model': {'USE_BN': True}}, 'gn': {'hip': {'USE_GN': True}}}[norm]
    off = _model('18', SPEC, hip=kw.get('hip'), model=kw.get('model'))
    on = _model('18', SPEC, hip=dict(kw.get('hip', {}), TRAIN_NONLOCAL=True), model=kw.get('model'))
    assert _graph(on.net) == _graph(off.net) and on.params == off.params and on.param_specs == off.param_specs
    assert on.TrainableParams() == off.TrainableParams()
    assert not any(op.type == 'AffineTrain' for op in on.net.ops)
    # ... and a graph without the key is the same with and without the switch
    assert _graph(_model('18', '', hip={'TRAIN_NONLOCAL': True}).net) == _graph(_model('18', '').net)


def test_the_shipped_training_config_sets_both_keys():
    import os
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'configs', 'train_r18_fpn3d_nonlocal_synthetic.yaml')) as f:
        new = yaml.safe_load(f)
    with open(os.path.join(root, 'configs', 'train_r18_fpn3d_synthetic.yaml')) as f:
        base = yaml.safe_load(f)
    assert new['HIP'].pop('NONLOCAL') == 'res3_1,res4_1' and new['HIP'].pop('TRAIN_NONLOCAL') is True
    base_hip = base.get('HIP', {})
    assert new.get('HIP', {}) == base_hip or (not new['HIP'] and not base_hip)
    new.pop('HIP', None)
    base.pop('HIP', None)
    assert new == base
