"""The fused attention of the spacetime non-local block (dat_nonlocal_attention) at the shapes of the benched
clip (8 x 768 x 1344), in the build's 16-bit format, at 1 and 4 clips per launch:

    res4   L = 8 x 48 x 84 = 32 256 queries,  L' = 8 x 24 x 42 =  8 064 pooled keys, D = 128
    res3   L = 8 x 96 x 168 = 129 024 queries, L' = 8 x 48 x 84 = 32 256 pooled keys, D = 64

    python tools/probes/nonlocal_probe.py

Per case: the kernel time (median of 5 rounds of back-to-back calls between two HIP events after 2 warm-up calls) and the
algorithmic rate 4 L L' D / time as a fraction of the 2.5 PFLOP/s bf16 MFMA peak.  At the res4 shape, where the scores fit in memory
(0.5 GB per clip in 16 bits), also the time of the unfused composition -- torch bmm, softmax, bmm -- on the same operands; the res3
scores (16.6 GB per clip in fp32) are never materialised, so there is nothing to compare with."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

PEAK = 2.5e15
SHAPES = (('res4', 8 * 48 * 84, 8 * 24 * 42, 128), ('res3', 8 * 96 * 168, 8 * 48 * 84, 64))


def _timed(fn, iters, rounds=5):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return float(np.median(out))


def main():
    import torch
    from detectandtrack_amd.ops import hip_ops as ops
    td = ops.H16_DTYPE
    print('format %s' % str(td).replace('torch.', ''))
    g = torch.Generator(device='cuda').manual_seed(1)
    for name, L, Lk, D in SHAPES:
        for clips in (1, 4):
            q = torch.randn((clips * L, D), generator=g, device='cuda').to(td)
            k = torch.randn((clips * Lk, D), generator=g, device='cuda').to(td)
            v = torch.randn((clips * Lk, D), generator=g, device='cuda').to(td)
            y = torch.empty((clips * L, D), dtype=td, device='cuda')
            scale = D ** -0.5
            ms = _timed(lambda: ops.nonlocal_attention(q, k, v, ops.BF16, clips, D, scale, out=y), iters=3 if name == 'res3' else 10)
            flops = 4.0 * clips * L * Lk * D
            line = '%s x %d clips: fused %8.3f ms  %6.1f TFLOP/s  %.1f %% of 2.5 PFLOP/s' % (name, clips, ms, flops / ms * 1e-9,
                                                                                           100 * flops / (ms * 1e-3) / PEAK)
            if name == 'res4':
                q3, k3, v3 = q.view(clips, L, D), k.view(clips, Lk, D), v.view(clips, Lk, D)

                def unfused():
                    s = torch.bmm(q3, k3.transpose(1, 2))
                    s.mul_(scale)
                    return torch.bmm(torch.softmax(s, dim=2), v3)
                ms_u = _timed(unfused, iters=5)
                err = float((unfused().view(-1, D).float() - y.float()).abs().max())
                line += '   unfused (bmm, softmax, bmm) %8.3f ms  (fused / unfused %.2f, max |difference| %.3g)' % (ms_u, ms / ms_u, err)
            print(line, flush=True)
            del q, k, v, y


if __name__ == '__main__':
    main()
