"""The grouped conv kernel (conv3d_grouped_kernel) on the four 3 x 3 x 3 `branch2b` layers of ResNeXt-101 32x8d
at 8 x 768 x 1344 (one clip, bf16), next to the only alternative the library had before it: the dense kernel on a block-diagonal
expansion of the same weights (C x C x taps, zeros outside the groups).

    python tools/probes/grouped_probe.py

Per layer: five interleaved rounds of both sides, each round the mean of 20 back-to-back launches; medians (minima) are printed with the
achieved TFLOP/s on the grouped layer's own algorithmic FLOPs, 2 * C * (C / 32) * 27 * positions, for both sides."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

GROUPS = 32
# stage, channels, H, W of the layer's INPUT at 768 x 1344, stride: the stride-1 blocks of res2 .. res5 (1/4 .. 1/32), then the first
# block of res3 .. res5, whose 3 x 3 carries the stride (STRIDE_1X1 False)
SHAPES = [('res2_x', 256, 192, 336, 1), ('res3_x', 512, 96, 168, 1), ('res4_x', 1024, 48, 84, 1), ('res5_x', 2048, 24, 42, 1),
          ('res3_0', 512, 192, 336, 2), ('res4_0', 1024, 96, 168, 2), ('res5_0', 2048, 48, 84, 2)]


def _timed(fn, iters=20):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main(rounds=5):
    import torch
    from detectandtrack_amd.ops import hip_ops as ops
    g = torch.Generator().manual_seed(1)
    T = 8
    print('%-7s %5s %3s %6s | %17s %8s | %17s %8s | %6s | %s' % ('layer', 'C', 'cg', 'stride', 'grouped us', 'TFLOP/s', 'dense us', 'TFLOP/s',
                                                               'speed', 'max |grouped - dense|'))
    for name, c, h, w, s in SHAPES:
        kt = 1 if name.startswith('res2') else 3
        cg = c // GROUPS
        wt = (torch.randn((c, cg, kt, 3, 3), generator=g) * (2.0 / (cg * kt * 9)) ** 0.5).cuda()
        dense = torch.zeros((c, c, kt, 3, 3), device='cuda')
        for grp in range(GROUPS):
            dense[grp * cg:(grp + 1) * cg, grp * cg:(grp + 1) * cg] = wt[grp * cg:(grp + 1) * cg]
        kw = dict(stride=(s, s), pads=(kt // 2, 1, 1), relu=True, dtype=ops.BF16)
        one, zero = torch.ones(c).cuda(), torch.zeros(c).cuda()
        lg = ops.ConvLayer(wt, one, zero, groups=GROUPS, **kw)
        ld = ops.ConvLayer(dense, one, zero, **kw)
        del dense
        x = torch.randn((T, h, w, c), generator=g).to(ops.H16_DTYPE).cuda()
        diff = float((lg(x, T=T).float() - ld(x, T=T).float()).abs().max())
        tg, td = [], []
        for _ in range(rounds):
            tg.append(_timed(lambda: lg(x, T=T)))
            td.append(_timed(lambda: ld(x, T=T)))
        med = lambda v: sorted(v)[len(v) // 2]
        fl = lg.flops(T, h, w)
        print('%-7s %5d %3d %6d | %8.1f (%6.1f) %8.1f | %8.1f (%6.1f) %8.1f | %5.2fx | %.3g' % (
            name, c, cg, s, med(tg), min(tg), fl / med(tg) / 1e6, med(td), min(td), fl / med(td) / 1e6, med(td) / med(tg), diff))
        del lg, ld, x
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
