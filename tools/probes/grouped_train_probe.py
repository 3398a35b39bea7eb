"""The grouped backward on the `branch2b` layers of ResNeXt-101 32x8d at 8 x 768 x 1344 (one clip, bf16): the
grouped data-gradient layer and wgrad_grouped_kernel next to the only alternative the library has -- the dense data-gradient conv and
the dense dat_conv3d_wgrad on the block-diagonal expansion of the same weights (C x C x taps, zeros outside the groups).

    python tools/probes/grouped_train_probe.py [stage ...]

Per layer: five interleaved rounds of the four launches, each round the mean of 10 back-to-back launches; medians (minima) in
microseconds.  `dx` = hip_ops.ConvGrad.data (stride 2: the zero-insert pass included on both sides), `dW` = ConvGrad.weight (memset +
kernel + finish on both sides).  A grouped time above the dense one is a finding, printed like any other row."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

GROUPS = 32
# stage, channels, H, W of the layer's INPUT at 768 x 1344, stride (see grouped_probe.py)
SHAPES = [('res2_x', 256, 192, 336, 1), ('res3_x', 512, 96, 168, 1), ('res4_x', 1024, 48, 84, 1), ('res5_x', 2048, 24, 42, 1),
          ('res3_0', 512, 192, 336, 2), ('res4_0', 1024, 96, 168, 2), ('res5_0', 2048, 48, 84, 2)]


def _timed(fn, iters=10):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main(only=(), rounds=5):
    import torch
    from detectandtrack_amd.ops import hip_ops as ops
    gen = torch.Generator().manual_seed(1)
    T = 8
    med = lambda v: sorted(v)[len(v) // 2]
    print('%-7s %5s %3s %2s | %19s %19s %6s | %19s %19s %6s | %s' % ('layer', 'C', 'cg', 's', 'dx grouped us', 'dx dense us', 'speed',
                                                                     'dW grouped us', 'dW dense us', 'speed', 'max rel |grouped - dense| dx, dW'))
    for name, c, h, w, s in SHAPES:
        if only and name not in only:
            continue
        kt = 1 if name.startswith('res2') else 3
        cg = c // GROUPS
        wt = (torch.randn((c, cg, kt, 3, 3), generator=gen) * (2.0 / (cg * kt * 9)) ** 0.5).cuda()
        dense = torch.zeros((c, c, kt, 3, 3), device='cuda')
        for grp in range(GROUPS):
            dense[grp * cg:(grp + 1) * cg, grp * cg:(grp + 1) * cg] = wt[grp * cg:(grp + 1) * cg]
        scale = (torch.rand(c, generator=gen) + 0.5).cuda()
        pads = (kt // 2, 1, 1)
        gg = ops.ConvGrad(wt, scale, (s, s), pads, ops.BF16, c, c, groups=GROUPS)
        gd = ops.ConvGrad(dense, scale, (s, s), pads, ops.BF16, c, c)
        ho, wo = (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1
        x = torch.randn((T, h, w, c), generator=gen).to(ops.H16_DTYPE).cuda()
        g = torch.randn((T, ho, wo, c), generator=gen).to(ops.H16_DTYPE).cuda()
        runs = [lambda: gg.data(g, T, h, w), lambda: gd.data(g, T, h, w), lambda: gg.weight(x, g, T), lambda: gd.weight(x, g, T)]
        dxg, dxd = runs[0]().float(), runs[1]().float()
        ddx = float((dxg - dxd).abs().max() / dxd.abs().max())
        del dxg, dxd
        dwg, dwd = runs[2]()[0], runs[3]()[0]
        blocks = torch.stack([dwd[grp * cg:(grp + 1) * cg, grp * cg:(grp + 1) * cg] for grp in range(GROUPS)]).reshape(dwg.shape)
        ddw = float((dwg - blocks).abs().max() / blocks.abs().max())
        del dwd, blocks, dwg
        t = [[], [], [], []]
        for _ in range(rounds):
            for i, fn in enumerate(runs):
                t[i].append(_timed(fn))
        print('%-7s %5d %3d %2d | %9.1f (%7.1f) %9.1f (%7.1f) %5.2fx | %9.1f (%7.1f) %9.1f (%7.1f) %5.2fx | %.2e %.2e' % (
            name, c, cg, s, med(t[0]), min(t[0]), med(t[1]), min(t[1]), med(t[1]) / med(t[0]),
            med(t[2]), min(t[2]), med(t[3]), min(t[3]), med(t[3]) / med(t[2]), ddx, ddw))
        sys.stdout.flush()
        del gg, gd, x, g, dense, runs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main(tuple(sys.argv[1:]))
