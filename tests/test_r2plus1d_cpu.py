"""ResNet-(2+1)D bodies without a GPU: the mid-plane rule, the builder against the restatement (tests/r2plus1d_ref.py), kT = 1 stages
against the I3D body, and the checkpoint rules of the factorised parameters."""
import os

import numpy as np
import pytest

from tests.model_util import fpn3d_kps_cfg
from tests.r2plus1d_ref import mid_planes, param_shapes

BODIES = {'18': 'FPN3D.add_fpn_ResNet18_2plus1d_conv5_body', '50': 'FPN3D.add_fpn_ResNet50_2plus1d_conv5_body'}


def _model(arch, kt=3, twoplus1=True, body=None):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    d = fpn3d_kps_cfg(arch, T=4, kt=kt)
    if body is not None:
        d['MODEL']['CONV_BODY'] = body
    elif twoplus1:
        d['MODEL']['CONV_BODY'] = BODIES[arch]
    reset_cfg()
    cfg_from_cfg(d)
    assert_and_infer_cfg()
    return model_builder.create(cfg.MODEL.TYPE, train=False)


def _shapes(model):
    return {n: tuple(model.param_specs[n]['shape']) for n in model.params}


def _graph(net):
    return [(op.type, tuple(op.inputs), tuple(op.outputs), repr(sorted(op.args.items())) if isinstance(op.args, dict) else repr(op.args))
            for op in net.ops]


def test_mid_plane_table():
    from detectandtrack_amd.modeling.ResNet3D import mid_planes_2plus1d
    table = {(64, 128): 230, (128, 128): 288, (128, 256): 460, (256, 256): 576, (256, 512): 921, (512, 512): 1152}
    for (nin, nout), m in table.items():
        assert mid_planes_2plus1d(nin, nout, 3) == m == mid_planes(nin, nout, 3), (nin, nout)


@pytest.mark.parametrize('arch', ['18', '50'])
def test_factorised_blocks_keep_the_i3d_parameter_count_and_flops(arch):
    """Per factorised conv: 9 Nin M + kT M Nout <= kT 9 Nin Nout, short of it by less than one mid plane (9 Nin + kT Nout).  Both
    halves run at the output positions of the conv they replace (the spatial stride sits on the 1 x 3 x 3 conv), so the FLOPs follow."""
    s21, s3d = _shapes(_model(arch)), _shapes(_model(arch, twoplus1=False))
    pairs = 0
    for n, shp in s3d.items():
        if len(shp) != 5 or shp[2:] != (3, 3, 3):
            continue
        if not n.startswith('res'):
            continue
        base = n[:-2]
        sp, tp = s21[base + '_spatial_w'], s21[base + '_temporal_w']
        nout, nin, kt = shp[0], shp[1], shp[2]
        m = sp[0]
        assert sp == (m, nin, 1, 3, 3) and tp == (nout, m, kt, 1, 1)
        p3d, p21 = kt * 9 * nin * nout, int(np.prod(sp)) + int(np.prod(tp))
        assert 0 <= p3d - p21 < 9 * nin + kt * nout, (n, p3d, p21)
        pairs += 1
    assert pairs == (12 if arch == '18' else 13)
    body = lambda s: sum(int(np.prod(v)) for k, v in s.items() if k.startswith('res') and k.endswith('_w'))
    assert abs(body(s21) - body(s3d)) < 0.001 * body(s3d)


@pytest.mark.parametrize('arch', ['18', '50'])
def test_builder_parameters_match_the_restatement(arch):
    from oracle.net3d import opts_for
    want = param_shapes(opts_for('R' + arch, kt_body=3))
    got = {k: v for k, v in _shapes(_model(arch)).items() if k.startswith(('conv1', 'res_conv1', 'res'))}
    assert got == want, (sorted(set(got) ^ set(want)), [k for k in got if k in want and got[k] != want[k]])
    fact = [k for k in got if '_spatial' in k or '_temporal' in k]
    assert len(fact) == (12 if arch == '18' else 13) * 6


@pytest.mark.parametrize('arch', ['18', '50'])
def test_kt1_bodies_build_the_i3d_graph(arch):
    """TIME_KERNEL_DIM 1: every stage has kT = 1, and the (2+1)D body is the I3D body op for op, parameter for parameter."""
    a, b = _model(arch, kt=1), _model(arch, kt=1, twoplus1=False)
    assert _graph(a.net) == _graph(b.net)
    assert _shapes(a) == _shapes(b)
    assert not [k for k in a.params if '_spatial' in k or '_temporal' in k]


def test_res2_and_stage_outputs_are_those_of_the_i3d_body():
    """kT = 3: res2 (kT = 1 always) and the stem are untouched; block outputs, stage outputs and the FPN taps keep their names."""
    a, b = _model('18'), _model('18', twoplus1=False)
    ga, gb = _graph(a.net), _graph(b.net)
    pre = lambda g: [o for o in g if not any(s.startswith(('res3', 'res4', 'res5')) for s in o[1] + o[2])]
    stem = lambda g: [o for o in pre(g) if any(s.startswith(('res2', 'conv1', 'res_conv1', 'pool1', 'data')) for s in o[1] + o[2])]
    assert stem(ga) == stem(gb)
    outs = lambda g: sorted({s for o in g for s in o[2] if s.endswith('_sum') or s.startswith('fpn_')})
    assert outs(ga) == outs(gb)
    sa, sb = _shapes(a), _shapes(b)
    assert {k: v for k, v in sa.items() if not k.startswith(('res3', 'res4', 'res5'))} == \
           {k: v for k, v in sb.items() if not k.startswith(('res3', 'res4', 'res5'))}


class _WS(object):
    def __init__(self):
        self.params = {}

    def set_param(self, name, v):
        self.params[name] = np.array(v, dtype=np.float32, copy=True)


def _save(path, blobs):
    import pickle
    with open(path, 'wb') as f:
        pickle.dump({'blobs': blobs}, f, protocol=2)


@pytest.mark.parametrize('source', ['i3d', '2d'])
def test_i3d_and_2d_checkpoints_leave_factorised_parameters_at_their_fill(tmp_path, source):
    """A checkpoint of the I3D body (5-D weights) or of the 2D network (4-D weights, inflated on load) holds no `_spatial` / `_temporal`
    name: those parameters keep their fill (the missing-parameter path), and no weight of the file is reshaped into them."""
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd.core.config import cfg
    i3d = _model('18', twoplus1=False)
    src = net_utils.synthetic_params(i3d, seed=5)
    if source == '2d':
        src = {k: (v[:, :, 0] if v.ndim == 5 and v.shape[2] == 1 else v[:, :, v.shape[2] // 2] if v.ndim == 5 else v)
               for k, v in src.items()}
    path = str(tmp_path / 'ckpt.pkl')
    _save(path, src)
    model = _model('18')
    fill = _WS()
    net_utils.initialize_params(model, fill)
    ws = _WS()
    net_utils.initialize_params(model, ws)
    kept = net_utils.initialize_from_weights_file(model, ws, path)
    fact = sorted(k for k in model.params if '_spatial' in k or '_temporal' in k)
    assert fact and set(fact) <= set(kept)
    for k in fact:
        assert np.array_equal(ws.params[k], fill.params[k]), k
    for k in model.params:
        if k in src and k not in kept:
            want = src[k] if src[k].shape == tuple(model.param_specs[k]['shape']) else \
                net_utils.inflate_weights(src[k], fill.params[k], k, cfg.VIDEO.WEIGHTS_INFLATE_MODE)
            assert np.array_equal(ws.params[k], want), k
    assert 'res2_0_branch2a_w' not in kept and 'conv1_w' not in kept


def test_a_saved_2plus1d_model_loads_back_bit_identical(tmp_path):
    from detectandtrack_amd.utils import net as net_utils
    model = _model('50')
    ws = _WS()
    for k, v in net_utils.synthetic_params(model, seed=7).items():
        ws.set_param(k, v)
    path = str(tmp_path / 'r50_2plus1d.pkl')
    net_utils.save_model_to_weights_file(path, model, ws)
    ws2 = _WS()
    net_utils.initialize_params(model, ws2)
    kept = net_utils.initialize_from_weights_file(model, ws2, path)
    assert kept == []
    for k in model.params:
        assert ws2.params[k].dtype == np.float32 and np.array_equal(ws2.params[k], ws.params[k]), k


def test_shipped_2plus1d_example_config_names_the_new_body():
    from detectandtrack_amd.core.config import cfg, cfg_from_file, assert_and_infer_cfg, reset_cfg
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    reset_cfg()
    cfg_from_file(os.path.join(repo, 'configs', 'test_r18_2plus1d_fpn3d_synthetic.yaml'))
    assert_and_infer_cfg()
    assert cfg.MODEL.CONV_BODY == 'FPN3D.add_fpn_ResNet18_2plus1d_conv5_body'
    from detectandtrack_amd.modeling import model_builder
    model = model_builder.create(cfg.MODEL.TYPE, train=False)
    assert 'res5_1_branch2b_temporal_w' in model.params
