#!/usr/bin/env python3
"""Per-RoI GroupNorm on the box: the fused entry points dat_gn_roi_fwd / dat_gn_roi_bwd against the per-clip
entry points of the same library called with clips = R on the same tensors (dat_gn_stats + dat_gn_apply; dat_gn_bwd_reduce +
dat_gn_bwd_apply), forward (ReLU + residual) and backward (g, dz, dbeta, dgamma), bf16 and fp32.

    python tools/probes/gn_roi_probe.py [--iters 10] [--rounds 5]

Shapes: the C4 R-18 box head (R = 1000 and 4000 RoIs, Tr = 3, 7 x 7, 512 channels) and the keypoint head (R = 104 and 416, Tr = 1 and 8,
14 x 14, 512).  The two paths alternate for `--rounds` rounds of `--iters` back-to-back calls (device events, after a warm-up); the table
holds the median round and the spread (min - max) of each, in microseconds per call."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

SHAPES = [('box head', 1000, 3, 7, 512), ('box head', 4000, 3, 7, 512),
          ('kps head', 104, 1, 14, 512), ('kps head', 416, 1, 14, 512), ('kps head', 104, 8, 14, 512), ('kps head', 416, 8, 14, 512)]


def timeit(f, it):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it * 1e3


def main(iters, rounds):
    from detectandtrack_amd.ops import hip_ops as ops
    G, eps = 32, 1e-5
    print('%-8s %5s %2s %4s %-4s %-3s | %-28s | %-28s | %s' % ('shape', 'R', 'Tr', 'MB', 'fmt', 'dir', 'per-clip, clips = R (us)',
                                                               'per-RoI fused (us)', 'ratio of medians'))
    for name, R, Tr, P, C in SHAPES:
        for dn, dt, td in (('bf16', ops.BF16, ops.H16_DTYPE), ('fp32', ops.F32, torch.float32)):
            shape = (R * Tr, P, P, C)
            z, res, dy = (torch.randn(shape, device='cuda').to(td) for _ in range(3))
            s, b = torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda')
            dbeta, dgamma = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
            st = ops.gn_stats(z, dt, C, G, s, b, eps, clips=R)
            y, mean, rstd = ops.gn_roi_fwd(z, dt, C, G, s, b, eps, R=R, relu=True, residual=res)

            def clip_fwd():
                t = ops.gn_stats(z, dt, C, G, s, b, eps, clips=R)
                return ops.gn_apply(z, dt, C, t[2], t[3], clips=R, relu=True, residual=res)

            def roi_fwd():
                return ops.gn_roi_fwd(z, dt, C, G, s, b, eps, R=R, relu=True, residual=res)

            def clip_bwd():
                g, _, coef = ops.gn_bwd_reduce(dy, y, z, dt, C, G, st[0], st[1], s, clips=R, relu=True, dbeta=dbeta, dgamma=dgamma)
                return ops.gn_bwd_apply(g, z, dt, C, st[0], st[2], coef, clips=R)

            def roi_bwd():
                return ops.gn_roi_bwd(dy, y, z, dt, C, G, mean, rstd, s, R=R, relu=True, dbeta=dbeta, dgamma=dgamma)
            for direction, a, f in (('fwd', clip_fwd, roi_fwd), ('bwd', clip_bwd, roi_bwd)):
                ta, tf = [], []
                for _ in range(rounds):         # alternating: the spread of the same path is part of the answer
                    ta.append(timeit(a, iters))
                    tf.append(timeit(f, iters))
                fmt = lambda t: '%8.1f  (%8.1f - %8.1f)' % (float(np.median(t)), min(t), max(t))
                print('%-8s %5d %2d %4.0f %-4s %-3s | %s | %s | %.2f' % (name, R, Tr, z.numel() * z.element_size() / 1e6, dn, direction,
                                                                        fmt(ta), fmt(tf), float(np.median(ta) / np.median(tf))))
            del z, res, dy, y, st
            torch.cuda.empty_cache()


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=10)
    p.add_argument('--rounds', type=int, default=5)
    a = p.parse_args()
    assert torch.cuda.is_available(), 'gn_roi_probe needs the GPU'
    main(a.iters, a.rounds)
