"""The spacetime non-local block (HIP.NONLOCAL) without a GPU: the float64 reference of the fused attention
against an independent statement, the per-element bound against a faithful fp32 simulation of the kernel and against every named defect
(the bound must hold the first and refuse the others), and the builder: ops, parameters, names, refusals."""
import numpy as np
import pytest
import torch

from tests import nonlocal_ref as R
from tests import numerics as nm
from tests.model_util import fpn3d_kps_cfg

FORMATS = ('fp32', 'bf16', 'fp16')


def _operands(name, fmt):
    q, k, v, scale, clips = R.make_case(name, fmt)
    if name == 'res4_bench':
        q = q[R.bench_rows(q.shape[0])]
    return q, k, v, scale, clips


# ---- reference and bound --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ragged', 'clips', 'big'])
def test_reference_against_an_independent_float64_softmax_attention(name):
    q, k, v, scale, clips = _operands(name, 'fp32')
    y, A, s, sabs, p = R.reference(q, k, v, scale, clips)
    L, Lk = q.shape[0] // clips, k.shape[0] // clips
    tq, tk, tv = (torch.from_numpy(a).double().reshape(clips, -1, a.shape[1]) for a in (q, k, v))
    att = torch.softmax(torch.einsum('cid,cjd->cij', tq, tk) * scale, dim=2)
    np.testing.assert_allclose(y, torch.einsum('cij,cjd->cid', att, tv).reshape(clips * L, -1).numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(A, torch.einsum('cij,cjd->cid', att, tv.abs()).reshape(clips * L, -1).numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(p, att.reshape(clips * L, Lk).numpy(), rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(p.sum(axis=1), 1.0, rtol=1e-13)
    assert s.shape == sabs.shape == (clips * L, Lk) and (sabs >= np.abs(s) - 1e-12).all()


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('name', list(R.CASES))
def test_faithful_simulation_is_inside_the_bound(name, fmt):
    q, k, v, scale, clips = _operands(name, fmt)
    ref = R.reference(q, k, v, scale, clips)
    worst = R.check(R.simulate(q, k, v, scale, fmt, clips), ref, q.shape[1], fmt, name)
    assert worst <= 0.7, 'the bound has lost its room: %.3f' % worst           # (0.58 at worst, in bf16 and fp16; 0.05 in fp32)
    if name == 'posv' and fmt != 'fp32':
        for tile in (16, 32, 64, 128):
            stat = R.truncation_statistic(R.simulate(q, k, v, scale, fmt, clips, tile=tile), ref) / nm.unit_roundoff(fmt)
            assert abs(stat) <= 0.05, (tile, stat)


def _outside(name, fmt, **kw):
    q, k, v, scale, clips = _operands(name, fmt)
    ref = R.reference(q, k, v, scale, clips)
    got = R.simulate(q, k, v, scale, fmt, clips, **kw)
    err = np.abs(got - ref[0])
    return float(np.where(np.isfinite(err), err / R.bound_for(ref, q.shape[1], fmt), np.inf).max())


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('tile', [16, 32, 64, 128])
def test_every_single_dropped_key_tile_is_outside_the_bound(tile, fmt):
    """q = 0 (uniform P), a different ramp per channel in V: whichever tile is skipped, the mean of some channel moves."""
    Lk = R.CASES['uniform_ramp'][2]
    assert R.check(R.simulate(*_args('uniform_ramp', fmt), tile=tile), *_ref('uniform_ramp', fmt)) <= 1.0
    for t in range((Lk + tile - 1) // tile):
        ratio = _outside('uniform_ramp', fmt, tile=tile, drop=t)
        assert ratio > 2.0, 'tile %d of width %d dropped: err / bound only %.2f' % (t, tile, ratio)


def _args(name, fmt):
    q, k, v, scale, clips = _operands(name, fmt)
    return q, k, v, scale, fmt, clips


_REFS = {}


def _ref(name, fmt):
    if (name, fmt) not in _REFS:
        q, k, v, scale, clips = _operands(name, fmt)
        _REFS[(name, fmt)] = (R.reference(q, k, v, scale, clips), q.shape[1], fmt, name)
    return _REFS[(name, fmt)]


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('defect,name', [('no_rescale', 'growing'), ('no_scale', 'ragged'), ('no_scale', 'd512'), ('pad_keys', 'ragged'),
                                         ('pad_keys', 'uniform_ramp'), ('neighbour_clip', 'clips')])
def test_named_defects_are_outside_the_bound(defect, name, fmt):
    ratio = _outside(name, fmt, defect=defect)
    assert ratio > 2.0, '%s on %s (%s): err / bound only %.2f' % (defect, name, fmt, ratio)


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
def test_truncated_p_is_caught_by_the_mean_signed_error_only(fmt):
    """A P truncated to 16 bits stays inside the worst-case bound (0.7 - 0.85 of it) -- the statistic of the posv case is what sees it."""
    q, k, v, scale, clips = _operands('posv', fmt)
    ref = R.reference(q, k, v, scale, clips)
    for tile in (16, 32, 64, 128):
        got = R.simulate(q, k, v, scale, fmt, clips, tile=tile, defect='truncate')
        assert R.check(got, ref, q.shape[1], fmt, 'posv') > 0.6
        stat = R.truncation_statistic(got, ref) / nm.unit_roundoff(fmt)
        assert stat < -0.5, (tile, stat)
        assert abs(stat) > 0.1


# ---- builder ----------------------------------------------------------------------------------------------------------------------------
def _model(arch, spec, train=False, hip=None, model=None, body=None):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    d = fpn3d_kps_cfg(arch, T=4)
    d['HIP']['NONLOCAL'] = spec
    d['HIP'].update(hip or {})
    d['MODEL'].update(model or {})
    if body is not None:
        d['MODEL']['CONV_BODY'] = body
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


def _block_ops(model, nl):
    return [op for op in model.net.ops if any(b.startswith(nl + '_') for b in op.outputs) or op.type == 'Conv' and op.args['w'] == nl + '_out_w']


@pytest.mark.parametrize('arch,spec,last', [('18', 'res3_1,res4_0', {'res3_1': True, 'res4_0': False}),
                                            ('50', 'res3_3,res4_5', {'res3_3': True, 'res4_5': True})])
def test_recorded_ops_parameters_and_names(arch, spec, last):
    from oracle.net3d import opts_for
    from detectandtrack_amd.modeling import ResNet3D
    model = _model(arch, spec)
    opts = opts_for('R' + arch)
    want = R.nonlocal_param_shapes(spec, opts)
    got = {n: tuple(model.param_specs[n]['shape']) for n in model.params if n.startswith('nonlocal_')}
    assert got == want
    outputs = set(o for op in model.net.ops for o in op.outputs)
    for p, is_last in last.items():
        nl, C = 'nonlocal_' + p, opts['feat_dims'][int(p[3]) - 1]
        D = C // 2
        assert model.param_specs[nl + '_out_bn_s']['init'] == ('ConstantFill', {'value': 0.})
        assert model.param_specs[nl + '_out_bn_b']['init'] == ('ConstantFill', {'value': 0.})
        x = p + '_sum_nl_in' if is_last else model.net.producer(nl + '_theta').inputs[0]
        assert (p + '_sum_nl_in' in outputs) == is_last
        ops = _block_ops(model, nl)
        assert [op.type for op in ops] == ['Conv', 'Conv', 'Conv', 'MaxPool', 'MaxPool', 'NonLocalAttention', 'Conv']
        for op, b in zip(ops[:3], ('_theta', '_phi', '_g')):
            assert op.inputs == [x] and op.outputs == [nl + b] and op.args['w'] == nl + b + '_w' and op.args['b'] == nl + b + '_b'
            assert op.args['kernels'] == [1, 1, 1] and (op.args['dim_in'], op.args['dim_out']) == (C, D) and not op.args['relu']
        for op, b in zip(ops[3:5], ('_phi', '_g')):
            assert op.inputs == [nl + b] and op.outputs == [nl + b + '_pool'] and (op.args['k'], op.args['stride'], op.args['pad']) == (2, 2, 0)
        att = ops[5]
        assert att.inputs == [nl + '_theta', nl + '_phi_pool', nl + '_g_pool'] and att.outputs == [nl + '_y']
        assert att.args == {'dim': D, 'scale': D ** -0.5}
        tail = ops[6]
        out_name = p + '_sum' if is_last else nl + '_sum'
        assert tail.inputs == [nl + '_y', x] and tail.outputs == [out_name]
        assert tail.args['scale'] == nl + '_out_bn_s' and tail.args['shift'] == nl + '_out_bn_b' and tail.args['b'] is None
        assert tail.args['res_mode'] == 1 and tail.args['residual'] == x and not tail.args['relu']
        assert (tail.args['dim_in'], tail.args['dim_out']) == (D, C)
        if not is_last:       # the next body block reads the block's output
            nxt = '%s_%d' % (p[:4], int(p[5:]) + 1)
            assert model.net.producer(nxt + '_branch2a').inputs[0] == out_name
    # the stage outputs keep their names and the FPN taps them
    info = getattr(ResNet3D, 'stage_info_ResNet%s_conv5' % arch)()
    for blob in info.blobs:
        assert blob in outputs
    for blob in info.blobs[1:]:
        assert model.net.producer('fpn_inner_' + blob).inputs[0] == blob
    assert model.net.producer('fpn_inner_' + info.blobs[0]).inputs[0] == info.blobs[0]


def test_switches_maxpool_and_scale():
    model = _model('18', 'res4_1', hip={'NONLOCAL_MAXPOOL': False, 'NONLOCAL_SCALE': False})
    att = [op for op in model.net.ops if op.type == 'NonLocalAttention']
    assert len(att) == 1 and att[0].inputs == ['nonlocal_res4_1_theta', 'nonlocal_res4_1_phi', 'nonlocal_res4_1_g']
    assert att[0].args == {'dim': 128, 'scale': 1.0}
    assert not any(op.type == 'MaxPool' and 'nonlocal' in op.outputs[0] for op in model.net.ops)


@pytest.mark.parametrize('body', ['FPN3D.add_fpn_ResNet18_2plus1d_conv5_body', 'FPN.add_fpn_ResNet18_conv5_body'])
def test_other_bodies_that_go_through_add_stage_get_the_block(body):
    model = _model('18', 'res3_0,res4_1', body=body, model={} if body.startswith('FPN3D') else {'VIDEO_ON': False})
    assert sum(op.type == 'NonLocalAttention' for op in model.net.ops) == 2
    assert model.net.producer('res4_1_sum').args['w'] == 'nonlocal_res4_1_out_w'


@pytest.mark.parametrize('spec,match', [('res2_0', 'not a block of res3 / res4'), ('res5_1', 'not a block of res3 / res4'),
                                        ('res3', 'not a block of res3 / res4'), ('res4_x', 'not a block of res3 / res4'),
                                        ('res3_2', 'outside its stage'), ('res4_1,res3_0,res4_1', 'listed twice')])
def test_spec_errors(spec, match):
    with pytest.raises(ValueError, match=match):
        _model('18', spec)


def test_odd_channel_count_is_refused():
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.modeling import ResNet3D
    reset_cfg()
    cfg.HIP.NONLOCAL = 'res3_0'
    with pytest.raises(ValueError, match='an odd number'):
        ResNet3D.nonlocal_blocks_of_stage('res3', 2, 129)
    assert ResNet3D.nonlocal_blocks_of_stage('res4', 2, 129) == []
    assert ResNet3D.parse_nonlocal_spec(' res3_1 , res4_0,') == [('res3', 1), ('res4', 0)] and ResNet3D.parse_nonlocal_spec('') == []


def test_training_is_refused():
    with pytest.raises(NotImplementedError, match='backward of the fused attention and of its 2 x 2 max-pool'):
        _model('18', 'res4_1', train=True)


@pytest.mark.parametrize('hip', [{'KEYFRAME_DCE': True}, {'FRAME_TRUNK_CACHE': 8}])
def test_subset_of_frames_forwards_are_refused(hip):
    from detectandtrack_amd import workspace
    model = _model('18', 'res4_1', hip=hip)
    with pytest.raises(ValueError, match='NonLocalAttention ops .* every frame of the clip'):
        workspace.check_bn_sees_every_frame(model.net)
    workspace.check_bn_sees_every_frame(_model('18', '', hip=hip).net)


def test_group_norm_tail_carries_the_residual():
    model = _model('18', 'res3_1,res4_0', hip={'USE_GN': True})
    for nl, x, out in (('nonlocal_res3_1', 'res3_1_sum_nl_in', 'res3_1_sum'), ('nonlocal_res4_0', None, 'nonlocal_res4_0_sum')):
        tail = model.net.producer(out)
        x = x or model.net.producer(nl + '_theta').inputs[0]
        assert tail.type == 'GroupNorm' and tail.inputs == [nl + '_out', x] and tail.args['residual'] == x and not tail.args['relu']
        assert tail.args['scale'] == nl + '_out_bn_s' and model.param_specs[nl + '_out_bn_s']['init'] == ('ConstantFill', {'value': 0.})
        conv = model.net.producer(nl + '_out')
        assert conv.type == 'Conv' and conv.args['scale'] is None and conv.args['residual'] is None and conv.inputs == [nl + '_y']


def test_empty_key_builds_the_graph_of_the_code_before_the_feature(monkeypatch):
    """HIP.NONLOCAL '' (the default): the R-18 FPN3D op list and parameter list equal those built with `add_stage` as it was before the
    feature (restated here), and none of the feature's functions is reached."""
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.modeling import ResNet3D
    assert cfg.HIP.NONLOCAL == '' and cfg.HIP.NONLOCAL_MAXPOOL is True and cfg.HIP.NONLOCAL_SCALE is True
    now = _model('18', '')
    assert not any(op.type == 'NonLocalAttention' for op in now.net.ops) and not any('nonlocal' in p or '_nl_in' in p for p in now.params)

    def add_stage_before(stage_id, model, prefix, blob_in, n, dim_in, dim_out, dim_inner, dilation, stride_init=2, time_kernel_dim=1,
                         time_stride_on=False):
        for i in range(n):
            blob_in = ResNet3D.add_bottleneck_block(stage_id, model, '{}_{}'.format(prefix, i), blob_in, dim_in, dim_out, dim_inner, dilation,
                                                    stride_init, inplace_sum=i < n - 1, time_kernel_dim=time_kernel_dim,
                                                    time_stride_on=time_stride_on)
            dim_in = dim_out
        return blob_in, dim_in

    def unreachable(*a, **k):
        raise AssertionError('a non-local code path was reached with HIP.NONLOCAL empty')
    monkeypatch.setattr(ResNet3D, 'add_stage', add_stage_before)
    for f in ('add_nonlocal_block', 'nonlocal_blocks_of_stage', 'parse_nonlocal_spec'):
        monkeypatch.setattr(ResNet3D, f, unreachable)
    before = _model('18', '')
    assert _graph(now.net) == _graph(before.net) and len(now.net.ops) > 40
    assert now.params == before.params and now.param_specs == before.param_specs
    monkeypatch.undo()
    for f in ('add_nonlocal_block', 'nonlocal_blocks_of_stage', 'parse_nonlocal_spec'):
        monkeypatch.setattr(ResNet3D, f, unreachable)
    again = _model('18', '')
    assert _graph(again.net) == _graph(now.net)
