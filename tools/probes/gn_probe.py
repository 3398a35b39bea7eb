#!/usr/bin/env python3
"""GroupNorm kernels on the box: achieved TB/s of ALGORITHMIC bytes of the heavy kernels of
csrc/group_norm.hip / csrc/norm_kernels.h on the res2 and res3 blobs of R-18 at 8 x 768 x 1344 (bf16 and fp32, one clip), next to the
same box's copy rate (the measurement of tools/peak_probe.py); one R-18-(2+1)D training iteration with and without HIP.USE_GN; and
inference clips/s of the R-18-(2+1)D model (8 x 768 x 1344, bf16, one captured hipGraph per clip) with and without HIP.USE_GN.

    python tools/probes/gn_probe.py [--no-train] [--no-infer]

Algorithmic bytes (e = element size, n = rows x cstride elements):  stats: n e (one read);  apply: 2 n e (+ n e with a residual);
bwd_reduce: 4 n e (dy, y, z read, g written);  bwd_apply: 3 n e (g, z read, dz written).  Each row is the whole entry point: the heavy
kernel plus its tiny finalize launches (stats: channel merge + group finalize; bwd_reduce: sums + group coefficients).  Times are
device events around `--iters` back-to-back launches after a warm-up; the tables and the partial rows (KB) are not counted."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))


def timeit(f, it):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it


def kernels(iters):
    from detectandtrack_amd.ops import hip_ops as ops
    x = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    y = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    ms = timeit(lambda: y.copy_(x), 10)
    copy = 2.0 * (1 << 30) / ms / 1e9
    print('HBM copy 1 GiB: %.3f ms  %.2f TB/s (read + write)' % (ms, copy))
    del x, y
    # R-18 at 8 x 768 x 1344: res2 = 8 x 192 x 336 x 64, res3 = 8 x 96 x 168 x 128
    for name, shape in (('res2', (8, 192, 336, 64)), ('res3', (8, 96, 168, 128))):
        for dn, dt, td in (('bf16', ops.BF16, ops.H16_DTYPE), ('fp32', ops.F32, torch.float32)):
            C = shape[3]
            z = torch.randn(shape, device='cuda').to(td)
            res, dy = torch.randn(shape, device='cuda').to(td), torch.randn(shape, device='cuda').to(td)
            s, b = torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda')
            G = 32
            st = ops.gn_stats(z, dt, C, G, s, b, 1e-5)
            yy = ops.gn_apply(z, dt, C, st[2], st[3], relu=True, residual=res)
            g, _, coef = ops.gn_bwd_reduce(dy, yy, z, dt, C, G, st[0], st[1], s, relu=True)
            nb = z.numel() * z.element_size()
            rows = [('stats', 1, lambda: ops.gn_stats(z, dt, C, G, s, b, 1e-5)),
                    ('apply', 2, lambda: ops.gn_apply(z, dt, C, st[2], st[3], relu=True)),
                    ('apply+res', 3, lambda: ops.gn_apply(z, dt, C, st[2], st[3], relu=True, residual=res)),
                    ('bwd_reduce', 4, lambda: ops.gn_bwd_reduce(dy, yy, z, dt, C, G, st[0], st[1], s, relu=True)),
                    ('bwd_apply', 3, lambda: ops.gn_bwd_apply(g, z, dt, C, st[0], st[2], coef))]
            for kn, passes, f in rows:
                ms = timeit(f, iters)
                rate = passes * nb / ms / 1e9
                print('%-4s %-4s %-10s %7.3f ms  %5.2f TB/s  (%.0f%% of the copy rate; %d x %.1f MB)' %
                      (name, dn, kn, ms, rate, 100 * rate / copy, passes, nb / 1e6))


def train_iteration(use_gn, iters):
    from detectandtrack_amd.core.config import cfg, cfg_from_file, cfg_from_list, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import Trainer
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    from train_net import synthetic_clip_and_entry, feed_clip       # (tools/train_net.py: the clip and labels its own loop feeds)
    reset_cfg()
    cfg_from_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'configs', 'train_r18_2plus1d_fpn3d_gn_synthetic.yaml'))
    cfg_from_list(['HIP.USE_GN', str(bool(use_gn)), 'TRAIN.MAX_SIZE', '512'])     # (the label blobs are sized by TRAIN.MAX_SIZE)
    assert_and_infer_cfg()
    model = model_builder.create(cfg.MODEL.TYPE, train=True)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    for k, v in net_utils.synthetic_params(model, cfg.RNG_SEED).items():
        ws.set_param(k, v)
    trainer = Trainer(model, ws)
    data, entry = synthetic_clip_and_entry(cfg.VIDEO.NUM_FRAMES, 320, 512, seed=1)
    rng = np.random.RandomState(3)
    feed_clip(ws, data, entry, rng)

    def step():
        trainer.step(0.002)
    for _ in range(3):
        step()
    ms = timeit(step, iters)
    print('R-18-(2+1)D FPN3D training iteration, %d x 320 x 512, bf16, USE_GN %-5s: %.2f ms' % (cfg.VIDEO.NUM_FRAMES, bool(use_gn), ms))


def inference(use_gn, iters):
    from detectandtrack_amd.core.config import cfg, cfg_from_file, cfg_from_list, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.core.clip_graph import ClipGraph
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    reset_cfg()
    cfg_from_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'configs', 'test_r18_2plus1d_fpn3d_gn_synthetic.yaml'))
    cfg_from_list(['HIP.USE_GN', str(bool(use_gn))])
    assert_and_infer_cfg()
    model = model_builder.create(cfg.MODEL.TYPE, train=False)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    for k, v in net_utils.synthetic_params(model, cfg.RNG_SEED).items():
        ws.set_param(k, v)
    for net in (model.net, model.conv_body_net, model.keypoint_net):
        ws.CreateNet(net)
    T, H, W = cfg.VIDEO.NUM_FRAMES, 768, 1344
    rs = np.random.RandomState(3)
    base = rs.uniform(-120, 130, (1, 3, T, H // 8, W // 8)).astype(np.float32)
    data = torch.from_numpy(np.repeat(np.repeat(base, 8, axis=3), 8, axis=4)).cuda()
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    g = ClipGraph(model, ws, data, im_info, (H, W, 3), stream=torch.cuda.Stream())

    def clip():
        g.launch(data)
        g.results()
    for _ in range(3):
        clip()
    ms = timeit(clip, iters)
    print('R-18-(2+1)D FPN3D inference, %d x %d x %d, bf16, one graph replay + read-back per clip, USE_GN %-5s: %.2f ms  %.1f clips/s'
          % (T, H, W, bool(use_gn), ms, 1000.0 / ms))


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--no-train', action='store_true')
    p.add_argument('--no-infer', action='store_true')
    a = p.parse_args()
    assert torch.cuda.is_available(), 'gn_probe needs the GPU'
    kernels(a.iters)
    if not a.no_train:
        for use_gn in (False, True, False, True):       # alternating: the spread of the same configuration is part of the answer
            train_iteration(use_gn, a.iters)
    if not a.no_infer:
        for use_gn in (False, True, False, True):
            inference(use_gn, a.iters)
