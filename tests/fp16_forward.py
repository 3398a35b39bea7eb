"""Helper of tests/test_gpu_fp16.py, run as a script in a process started with DAT_H16=fp16 (the 16-bit format is a property of the loaded
library build): `python tests/fp16_forward.py [MODEL]` runs one model in cfg.HIP.DTYPE 'fp16' on one synthetic clip against the float
restatement (torch-CPU fp32) that the model's own fp32 test uses -- relative error of body / FPN blobs, proposal agreement, kps_score error --
and prints one JSON line.  MODEL (each at the clip size and proposal counts of its fp32 model test):

  r18        the plain R-18 FPN3D keypoint model against the ORACLE graph (the default)
  gn         R-18 FPN3D with GroupNorm (tests/group_norm_ref.gn_net)
  c4_gn_roi  the C4 tube model whose res5 box head normalises per RoI (tests/gn_roi_ref.c4_tube_net on gn_net); the res5 head blobs
             of the device's first RoIs are among the checked blobs
  nonlocal   R-18 FPN3D with non-local blocks behind res3_1 and res4_0 (tests/nonlocal_ref.NetNonLocal, the sharpened theta)
  resnext    the reduced ResNeXt-50 FPN3D model (tests/grouped_ref.resnext_net)
  dilated    the R-18 C5 body with MODEL.DILATION 2 (tests/dilated_ref.NetDilated, single-level RPN, heads at 1/16)"""
import json
import sys

import numpy as np
import torch

MODELS = ('r18', 'gn', 'c4_gn_roi', 'nonlocal', 'resnext', 'dilated')
N_KP = 8


def _sums(ws, prefixes):
    return sorted(b for b in ws.Blobs() if b.endswith('_sum') and b.startswith(prefixes))


def _setup(name):
    """-> (model, ws, net, (T, H, W), names): the product built in 'fp16', the restatement on the same weights, the blobs to compare
    as (product name, restatement name) -- a function to call once the net has run (the workspace lists its blobs then)."""
    from tests.model_util import fpn3d_kps_cfg, build_product, oracle_opts
    from oracle.net3d import Net
    from detectandtrack_amd.core.config import cfg
    if name == 'r18':
        shape = (4, 96, 128)
        model, ws, weights = build_product(fpn3d_kps_cfg('18', T=shape[0], dtype='fp16'))
        net = Net(weights, oracle_opts('18', shape[0], 3, 'slice-center', 300, 100))
        names = lambda: ['pool1', 'res2_1_sum', 'res3_1_sum', 'res4_1_sum', 'res5_1_sum', 'fpn_res5_1_sum', 'fpn_res2_1_sum']
    elif name == 'gn':
        from tests import group_norm_ref as ref
        from tests.test_gpu_group_norm_model import _cfg, T, H, W
        shape = (T, H, W)
        model, ws, weights = build_product(_cfg('r18', 'fp16'))
        net = ref.gn_net(Net, float(cfg.HIP.GN_EPSILON), int(cfg.HIP.GN_NUM_GROUPS))(weights, oracle_opts('18', T, 3, 'slice-center', 300, 100))
        names = lambda: ['pool1'] + _sums(ws, ('res', 'fpn_res'))
    elif name == 'c4_gn_roi':
        from tests import group_norm_ref as ref
        from tests import gn_roi_ref
        from tests.test_gpu_gn_roi_model import _c4_cfg, _c4_opts, T_C4, H, W
        shape = (T_C4, H, W)
        model, ws, weights = build_product(_c4_cfg('fp16', 300, 60))
        net = ref.gn_net(gn_roi_ref.c4_tube_net(Net), float(cfg.HIP.GN_EPSILON), int(cfg.HIP.GN_NUM_GROUPS))(weights, _c4_opts(300, 60))
        names = lambda: ['pool1'] + _sums(ws, ('res2', 'res3', 'res4'))
    elif name == 'nonlocal':
        from tests.nonlocal_ref import NetNonLocal, parse_spec
        from tests.test_gpu_nonlocal_model import _build
        shape, spec = (4, 128, 160), 'res3_1,res4_0'
        model, ws, weights = _build('18', spec, 'fp16')
        net = NetNonLocal(weights, oracle_opts('18', shape[0], 3, 'slice-center', 300, 100), spec)
        names = lambda: ['pool1'] + _sums(ws, ('res', 'fpn_res', 'nonlocal_')) + sorted('nonlocal_' + p + '_y' for p in parse_spec(spec))
    elif name == 'resnext':
        from tests.grouped_ref import resnext_net
        from tests.test_gpu_resnext import _cfg, GROUPS
        shape = (3, 64, 96)
        model, ws, weights = build_product(_cfg(T=shape[0], dtype='fp16', pre=300, post=100))
        net = resnext_net(GROUPS)(weights, oracle_opts('50', shape[0], 3, 'slice-center', 300, 100))
        names = lambda: ['pool1'] + _sums(ws, ('res', 'fpn_res'))
    elif name == 'dilated':
        from tests import dilated_ref as dr
        from tests.test_gpu_dilated_model import _opts, T, H, W, PRE, POST
        shape = (T, H, W)
        model, ws, weights = build_product(dr.c5_dilated_cfg('18', T=T, dilation=2, pre=PRE, post=POST, dtype='fp16'))
        net = dr.NetDilated(weights, _opts(T, PRE, POST))
        # (the sum of a stage's inner blocks is written in place over `branch2b`'s output)
        names = lambda: ['res4_1_sum', ('res5_0_branch2b_bn', 'res5_0_sum'), 'res5_1_sum']
    else:
        raise SystemExit('unknown model %r: one of %s' % (name, ', '.join(MODELS)))
    return model, ws, net, shape, lambda: [n if isinstance(n, tuple) else (n, n) for n in names()]


def _rel(got, ref):
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else ref
    assert got.shape == tuple(ref.shape), (got.shape, tuple(ref.shape))
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def main(name='r18'):
    from tests.model_util import synthetic_clip
    from oracle import proposals as op
    from detectandtrack_amd import libdat
    from detectandtrack_amd.ops import hip_ops as ops
    model, ws, net, (T, H, W), names = _setup(name)
    data = synthetic_clip(T, H, W)
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    ws.RunNet(model.net.name)
    names = names()
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    out = {'model': name, 'h16_format': int(libdat.lib().dat_h16_format()), 'blobs': {},
           'tensor_dtype': str(ws.blobs[[n for n, _ in names if n.endswith('_sum')][0]].t.dtype)}
    if name == 'dilated':
        from tests import dilated_ref as dr
        feat, ref_rois = dr.forward_2d_heads(net, data, im_info)
        kps_ref = lambda kp_rois: net.kps_head_c4_2d(feat, kp_rois).numpy()
    else:
        feat = net.body(torch.from_numpy(data))
        p2d = net.time_link([feat, feat] if name == 'c4_gn_roi' else net.fpn())
        ref_rois = net.fpn_rpn(p2d, im_info)[0]

        def kps_ref(kp_rois):
            _, per_level, restore = op.distribute(kp_rois, 2, 5)
            return net.kps_head_2d(net.roi_feat_fpn(p2d[1:], per_level, restore, 14, 2)).numpy()
    for got_name, ref_name in names:
        out['blobs'][got_name] = _rel(ws.FetchBlob(got_name), net.blobs[ref_name])
    rois = ws.FetchBlob('rois')
    if name == 'c4_gn_roi':
        # the per-RoI res5 head ran on the device's rois: the restatement's head on the first of them (before the keypoint net runs)
        from tests.test_gpu_gn_roi_model import RES5
        nb = min(32, int(ws.blobs['res5_1_sum'].count.item()))
        got5 = {n: ws.FetchBlob(n)[:nb] for n in RES5}
        sub = rois[:nb].copy()
        sub[:, 0] = 0
        _, per_level, restore = op.distribute(sub, 2, 5)
        net.box_head_2mlp(net.roi_feat_fpn(p2d[1:], per_level, restore, 7, 2))
        for n in sorted(RES5):
            out['blobs'][n + ' (%d rois)' % nb] = _rel(got5[n], net.blobs[RES5[n]])
    d = np.abs(rois[:, None, 1:] - ref_rois[None, :, 1:]).max(axis=2).min(axis=1)
    out['rois'] = [int(rois.shape[0]), int(ref_rois.shape[0])]
    out['rois_found_within_1px'] = float((d < 1.0).mean())
    kp_rois = ref_rois[:N_KP].copy()
    ws.FeedBlob('keypoint_rois', kp_rois)
    ws.RunNet(model.keypoint_net.name)
    kps = ws.FetchBlob('kps_score')
    ref = kps_ref(kp_rois)
    assert kps.shape == ref.shape, (kps.shape, ref.shape)
    maps = kps.shape[-2] * kps.shape[-1]
    out['kps_max_abs_err'] = float(np.abs(kps - ref).max())
    out['kps_ref_max_abs'] = float(np.abs(ref).max())
    out['kps_argmax_identical'] = float((kps.reshape(-1, maps).argmax(1) == ref.reshape(-1, maps).argmax(1)).mean())
    # the bf16x3 mode lives in the bf16 build only: the fp16 build must refuse it, loudly
    try:
        ops.split_bf16x2(torch.zeros((4, 64), dtype=torch.float32, device='cuda'))
        out['x3_refused'] = False
    except Exception as e:   # noqa: BLE001
        out['x3_refused'] = 'bf16 build' in str(e)
    print(json.dumps(out))


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:2]))
