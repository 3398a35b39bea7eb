#!/usr/bin/env python3
"""SpatialBN kernels on the box: achieved TB/s of ALGORITHMIC bytes of the four kernels of
csrc/batch_norm.hip on the res2 and res3 blobs of R-18 at 8 x 768 x 1344 (bf16 and fp32), next to the same box's copy rate (the
measurement of tools/peak_probe.py), and one R-18-(2+1)D training iteration with and without MODEL.USE_BN.

    python tools/probes/bn_probe.py [--no-train]

Algorithmic bytes (e = element size, n = rows x cstride elements):  stats: n e (one read);  apply: 2 n e (+ n e with a residual);
bwd_reduce: 4 n e (dy, y, z read, g written);  bwd_apply: 3 n e (g, z read, dz written).  Times are device events around `--iters`
back-to-back launches after a warm-up; the per-channel vectors and the partial rows (KB) are not counted."""
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
            rm, riv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
            st = ops.bn_stats(z, dt, C, s, b, 1e-5, 0.9, rm, riv)
            yy = ops.bn_apply(z, dt, C, st[2], st[3], relu=True, residual=res)
            g, sums = ops.bn_bwd_reduce(dy, yy, z, dt, C, st[0], st[1], relu=True)
            nb = z.numel() * z.element_size()
            rows = [('stats', 1, lambda: ops.bn_stats(z, dt, C, s, b, 1e-5, 0.9, rm, riv)),
                    ('apply', 2, lambda: ops.bn_apply(z, dt, C, st[2], st[3], relu=True)),
                    ('apply+res', 3, lambda: ops.bn_apply(z, dt, C, st[2], st[3], relu=True, residual=res)),
                    ('bwd_reduce', 4, lambda: ops.bn_bwd_reduce(dy, yy, z, dt, C, st[0], st[1], relu=True)),
                    ('bwd_apply', 3, lambda: ops.bn_bwd_apply(g, z, dt, C, st[0], st[1], st[2], sums))]
            for kn, passes, f in rows:
                ms = timeit(f, iters)
                rate = passes * nb / ms / 1e9
                print('%-4s %-4s %-10s %7.3f ms  %5.2f TB/s  (%.0f%% of the copy rate; %d x %.1f MB)' %
                      (name, dn, kn, ms, rate, 100 * rate / copy, passes, nb / 1e6))


def train_iteration(use_bn, iters):
    from detectandtrack_amd.core.config import cfg, cfg_from_file, cfg_from_list, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    from detectandtrack_amd.training import Trainer
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    from train_net import synthetic_clip_and_entry, feed_clip       # (tools/train_net.py: the clip and labels its own loop feeds)
    reset_cfg()
    cfg_from_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'configs', 'train_r18_2plus1d_fpn3d_bn_synthetic.yaml'))
    cfg_from_list(['MODEL.USE_BN', str(bool(use_bn))])
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
    print('R-18-(2+1)D FPN3D training iteration, %d x 320 x 512, bf16, USE_BN %-5s: %.2f ms' % (cfg.VIDEO.NUM_FRAMES, bool(use_bn), ms))


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--no-train', action='store_true')
    a = p.parse_args()
    assert torch.cuda.is_available(), 'bn_probe needs the GPU'
    kernels(a.iters)
    if not a.no_train:
        for use_bn in (False, True, False, True):       # alternating: the spread of the same configuration is part of the answer
            train_iteration(use_bn, a.iters)
