"""MODEL.DILATION without a GPU: the builder on the C5 bodies (what is recorded, and that an undilated graph records nothing new), the
refusals, the shipped configs, and the zero-inflated reference of tests/dilated_ref.py against torch's dilated conv in float64."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dilated_ref as dr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODIES = {'r18': ('18', 'ResNet3D.add_ResNet18_conv5_body'), 'r50': ('50', 'ResNet3D.add_ResNet50_conv5_body'),
          'r18_2plus1d': ('18', 'ResNet3D.add_ResNet18_2plus1d_conv5_body')}


def _model(body='r18', dilation=2, train=False, tube=False, fpn=False):
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    arch, fn = BODIES[body]
    d = dr.c5_dilated_cfg(arch, T=4, kt=3, dilation=dilation, tube=tube, body=fn)
    if fpn:
        d['MODEL']['CONV_BODY'] = 'FPN3D.add_fpn_ResNet18_conv5_body'
        d['FPN'] = {'FPN_ON': True, 'MULTILEVEL_ROIS': True, 'MULTILEVEL_RPN': True}
    reset_cfg()
    cfg_from_cfg(d)
    assert_and_infer_cfg()
    return model_builder.create(cfg.MODEL.TYPE, train=train)


def _convs(model, prefix):
    """the convs whose WEIGHT is named `<prefix>...` (an output is renamed when the affine that follows is folded in)"""
    nets = [model.net] + [n for n in (model.keypoint_net,) if n is not None]
    return [op for net in nets for op in net.ops if op.type == 'Conv' and str(op.args['w']).startswith(prefix)]


def _body_scales(model):
    """the body's scale as its readers recorded it: the RoI transforms of both heads and the proposal generator"""
    nets = [model.net] + [n for n in (model.keypoint_net,) if n is not None]
    rois = [op for net in nets for op in net.ops if op.type == 'RoIFeatureTransform']
    gen = [op for op in model.net.ops if op.type == 'GenerateProposals']
    assert len(rois) == 2 and len(gen) == 1
    return {float(v) for op in rois for v in op.args['scales']} | {float(op.args['spatial_scale']) for op in gen}


def _spatial_3x3(op):
    return op.args['kernels'][1:] == [3, 3]


@pytest.mark.parametrize('train', [False, True], ids=['test', 'train'])
@pytest.mark.parametrize('tube', [False, True], ids=['2d_heads', 'tube_heads'])
@pytest.mark.parametrize('body', sorted(BODIES))
def test_builder_accepts_dilation_2_on_the_c5_bodies(body, tube, train):
    """Every res5 3 x 3 conv that the reference dilates -- `branch2b` of the basic and the bottleneck block (its 1 x 3 x 3 half in the
    (2+1)D body) -- is recorded with dilation 2, pads 2 and stride 1; every res5 conv has stride 1, the shortcut included; the body's
    scale is 1/16.  `branch2a` of a basic block is a 3 x 3 conv the reference leaves undilated (pads 1), and so does the builder: it
    carries no attribute."""
    model = _model(body, 2, train=train, tube=tube)
    res5 = _convs(model, 'res5_')
    assert res5
    dilated = [op for op in res5 if _spatial_3x3(op) and 'branch2b' in op.args['w']]
    assert len(dilated) == (3 if body == 'r50' else 2), [op.outputs for op in dilated]
    for op in dilated:
        assert op.args.get('dilation') == 2 and op.args['pads'][1:] == [2, 2] and op.args['strides'] == [1, 1], (op.outputs, op.args)
    for op in res5:
        assert op.args['strides'] == [1, 1], (op.outputs, op.args['strides'])
        if op not in dilated:
            assert 'dilation' not in op.args, op.outputs
            if _spatial_3x3(op):
                assert 'branch2a' in op.args['w'] and body != 'r50' and op.args['pads'][1:] == [1, 1]
    short = [op for op in res5 if op.args['w'].startswith('res5_0_branch1')]
    assert len(short) == 1 and short[0].args['strides'] == [1, 1]
    assert _body_scales(model) == {1. / 16.}
    assert not [op for op in _convs(model, 'res') if not op.args['w'].startswith('res5_') and 'dilation' in op.args]


@pytest.mark.parametrize('body', sorted(BODIES))
def test_dilation_1_records_no_new_attribute(body):
    model = _model(body, 1)
    nets = [model.net, model.conv_body_net] + [n for n in (model.keypoint_net,) if n is not None]
    for net in nets:
        for op in net.ops:
            assert not isinstance(op.args, dict) or 'dilation' not in op.args, (op.type, op.outputs)
    res5 = _convs(model, 'res5_0_')
    assert any(op.args['strides'] == [2, 2] for op in res5)
    assert _body_scales(model) == {1. / 32.}


def test_fpn_with_dilation_raises_a_value_error_that_says_why():
    with pytest.raises(ValueError, match='MODEL.DILATION 2 with FPN.FPN_ON.*1/32'):
        _model('r18', 2, fpn=True)


def test_the_helper_refuses_what_is_out_of_scope():
    from detectandtrack_amd.core.config import reset_cfg
    from detectandtrack_amd.modeling.detector import DetectionModelHelper
    reset_cfg()
    m = DetectionModelHelper(train=False, num_classes=2)
    kw = dict(kernels=[1, 3, 3], pads=2 * [0, 2, 2], no_bias=1)
    with pytest.raises(ValueError, match='stride'):
        m.ConvNd('x', 'a', 64, 64, strides=[1, 2, 2], dilations=[1, 2, 2], **kw)
    with pytest.raises(ValueError, match='equal in H and W'):
        m.ConvNd('x', 'b', 64, 64, dilations=[1, 2, 3], **kw)
    with pytest.raises(ValueError, match='grouped'):
        m.ConvNd('x', 'c', 64, 64, dilations=[1, 2, 2], group=2, **kw)
    with pytest.raises(ValueError, match='temporal dilation'):
        m.ConvNd('x', 'd', 64, 64, dilations=[2, 2, 2], **kw)
    op = m.ConvNd('x', 'e', 64, 64, dilations=2, **kw)
    assert m.net.producer('e').args['dilation'] == 2
    # a 1 x 1 kernel has nothing to dilate: recorded as it always was (the reference passes the block's dilation to none of them, the
    # 2D `Conv` wrapper may)
    m.Conv('x', 'f', 64, 64, 1, dilation=2)
    assert 'dilation' not in m.net.producer('f').args


@pytest.mark.parametrize('name', ['test_r18_c5_dilated_synthetic.yaml', 'train_r18_c5_dilated_synthetic.yaml'])
def test_the_shipped_dilated_configs_load_and_build(name):
    from detectandtrack_amd.core.config import cfg, cfg_from_file, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    reset_cfg()
    cfg_from_file(os.path.join(REPO, 'configs', name))
    assert_and_infer_cfg()
    assert cfg.MODEL.DILATION == 2 and cfg.MODEL.CONV_BODY == 'ResNet3D.add_ResNet18_conv5_body' and not cfg.FPN.FPN_ON
    assert cfg.VIDEO.TIME_KERNEL_DIM.BODY == 3 and cfg.VIDEO.BODY_HEAD_LINK == 'slice-center'
    assert cfg.MODEL.ROI_HEAD == 'head_builder.add_roi_2mlp_head'
    assert cfg.KRCNN.ROI_KEYPOINTS_HEAD == 'keypoint_rcnn_heads.add_roi_pose_head_v1convX'
    model = model_builder.create(cfg.MODEL.TYPE, train=name.startswith('train'))
    assert [op.args.get('dilation') for op in _convs(model, 'res5_1_branch2b')] == [2]


@pytest.mark.parametrize('d,pad,k', [(2, 2, (1, 3, 3)), (3, 3, (3, 3, 3)), (4, 4, (1, 3, 3)), (2, 1, (1, 3, 3)), (2, 0, (3, 1, 1))])
def test_the_zero_inflated_reference_is_torchs_dilated_conv_in_float64(d, pad, k):
    """A dilated 3 x 3 is the dense (2d + 1)^2 conv whose other weights are zero: the same sums, term for term (exact in float64 up
    to the order of summation, held to 1e-12 relative), and the same sum of absolute products."""
    rs = np.random.RandomState(d * 10 + pad)
    x = torch.from_numpy(rs.randn(2, 5, 3, 9, 11))
    w = torch.from_numpy(rs.randn(4, 5, *k))
    want = F.conv3d(x, w, None, stride=1, padding=(k[0] // 2, pad, pad), dilation=(1, d, d))
    wi = dr.inflate(w, d)
    assert tuple(wi.shape[3:]) == ((k[1] - 1) * d + 1, (k[2] - 1) * d + 1)
    assert int((wi != 0).sum()) == int((w != 0).sum())
    got = F.conv3d(x, wi, None, stride=1, padding=(k[0] // 2, pad, pad))
    assert got.shape == want.shape and tuple(got.shape[3:]) == dr.out_hw(9, 11, k, (k[0] // 2, pad, pad), d)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    gota = F.conv3d(x.abs(), wi.abs(), None, stride=1, padding=(k[0] // 2, pad, pad))
    wanta = F.conv3d(x.abs(), w.abs(), None, stride=1, padding=(k[0] // 2, pad, pad), dilation=(1, d, d))
    assert float((gota - wanta).abs().max()) <= 1e-12 * float(wanta.abs().max())
    assert np.array_equal(dr.inflate(w.numpy(), d), wi.numpy())


def test_conv_desc_mirrors_the_c_struct():
    """libdat.ConvDesc ends with dil_h, dil_w like dat_conv_desc in include/dat_hip.h; a zero-initialised descriptor is not dilated."""
    import re
    src = open(os.path.join(REPO, 'include', 'dat_hip.h')).read()
    body = src[src.index('typedef struct {\n    int dtype;'):src.index('} dat_conv_desc;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n.strip() for decl in re.findall(r'int ([^;]+);', body) for n in decl.split(',')]
    assert names[-2:] == ['dil_h', 'dil_w']
    from detectandtrack_amd import libdat
    assert [f[0] for f in libdat.ConvDesc._fields_] == names
    d = libdat.ConvDesc()
    d.H, d.W, d.KH, d.KW, d.stride_h, d.stride_w, d.pad_h, d.pad_w = 20, 30, 3, 3, 1, 1, 2, 2
    import ctypes as C
    ho, wo = C.c_int(), C.c_int()
    for dil, want in ((0, (22, 32)), (1, (22, 32)), (2, (20, 30)), (4, (16, 26))):
        d.dil_h = d.dil_w = dil
        assert libdat.lib().dat_conv3d_out_shape(C.byref(d), C.byref(ho), C.byref(wo)) == 0
        assert (ho.value, wo.value) == want, (dil, ho.value, wo.value)
    d.KH = d.KW = 1
    d.pad_h = d.pad_w = 0
    assert libdat.lib().dat_conv3d_out_shape(C.byref(d), C.byref(ho), C.byref(wo)) == 0 and (ho.value, wo.value) == (20, 30)
