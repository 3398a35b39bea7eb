"""The dilated res5 3 x 3 convs of the C5-dilated bodies (MODEL.DILATION 2; R-18 and R-50 share the shape: 512 -> 512, kT x 3 x 3 on
the 48 x 84 map of one 8 x 768 x 1344 clip) next to the same layer undilated (d = 1, pad 1): same shape, same FLOPs, same box.

    python tools/probes/dilated_probe.py            the table of DESIGN.md section 3.14
    python tools/probes/dilated_probe.py once       one launch per case (for a kernel trace: which variant each case takes)

Per case: the median and minimum of 5 alternating rounds, each round the mean of 30 back-to-back launches between two HIP events after
3 warm-up launches; the ratio d = 2 / d = 1; the patch-size ratio (tile + 2 d)^2 / (tile + 2)^2 of a 16 x 16 tile it should be compared
with (what the block stages per channel chunk; the MFMA work is the same); the profiler tag of each (last digit 5-7: the generic kernel
on a dilated layer)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

# name, Cin, Cout, kT, frames, H, W
SHAPES = [('res5_branch2b kT3', 512, 512, 3, 8, 48, 84), ('res5_branch2b kT1', 512, 512, 1, 8, 48, 84)]
MODES = ('bf16', 'bf16x3', 'fp32')


def _timed(fn, iters=30):
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


def main(once=False, rounds=5):
    import torch
    from detectandtrack_amd.ops import hip_ops as ops
    g = torch.Generator().manual_seed(1)
    print('%-18s %-7s | %17s %8s | %17s %8s | %6s %6s | %s' % ('layer', 'mode', 'd=1 us (min)', 'TFLOP/s', 'd=2 us (min)', 'TFLOP/s', 'ratio',
                                                             'patch', 'tags d=1 / d=2'))
    for name, cin, cout, kt, frames, h, w in SHAPES:
        for mode in MODES:
            if mode == 'bf16x3' and ops.L.H16 == 'fp16':
                continue
            dtype, x3 = (ops.BF16, False) if mode == 'bf16' else (ops.F32, mode == 'bf16x3')
            wt = (torch.randn((cout, cin, kt, 3, 3), generator=g) * (2.0 / (9 * kt * cin)) ** 0.5).cuda()
            x = torch.randn((frames, h, w, cin), generator=g).to(ops.tdtype(dtype)).cuda()
            layers, tags, times = {}, {}, {1: [], 2: []}
            for d in (1, 2):
                layers[d] = ops.ConvLayer(wt, torch.ones(cout).cuda(), torch.zeros(cout).cuda(), pads=(kt // 2, d, d), relu=True, dtype=dtype,
                                          x3=x3, dilation=d)
                prof = ops.ConvProfiler(capacity=4)
                prof.start()
                layers[d](x, T=frames)
                tags[d] = prof.stop()[0][0]
            if once:
                print('%-18s %-7s tags %d / %d' % (name, mode, tags[1], tags[2]))
                continue
            for _ in range(rounds):
                for d in (1, 2):
                    times[d].append(_timed(lambda: layers[d](x, T=frames)))
            med = lambda v: sorted(v)[len(v) // 2]
            fl = layers[1].flops(frames, h, w)
            assert fl == layers[2].flops(frames, h, w)
            print('%-18s %-7s | %9.1f (%5.1f) %8.0f | %9.1f (%5.1f) %8.0f | %5.2fx %5.2fx | %d / %d' % (
                name, mode, med(times[1]), min(times[1]), fl / med(times[1]) / 1e6, med(times[2]), min(times[2]), fl / med(times[2]) / 1e6,
                med(times[2]) / med(times[1]), (16 + 4) ** 2 / float((16 + 2) ** 2), tags[1], tags[2]))


if __name__ == '__main__':
    main(once='once' in sys.argv[1:])
