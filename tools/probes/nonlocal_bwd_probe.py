"""The backward of the fused attention of the spacetime non-local block (dat_nonlocal_attention_bwd) at the
shapes of the benched clip (8 x 768 x 1344), in the build's 16-bit format, one clip:

    res4   L = 8 x 48 x 84 = 32 256 queries,  L' = 8 x 24 x 42 =  8 064 pooled keys, D = 128
    res3   L = 8 x 96 x 168 = 129 024 queries, L' = 8 x 48 x 84 = 32 256 pooled keys, D = 64

    python tools/probes/nonlocal_bwd_probe.py [res4|res3 ...]

Per shape: the time of the forward that stores the row statistic and of the backward (all three launches: delta, dq, dk / dv), each the
median of 5 rounds of back-to-back calls between two HIP events after 2 warm-up calls; the ratio backward / forward (by arithmetic
14 L L' D against 4 L L' D = 3.5); the algorithmic rate of the backward against the 2.5 PFLOP/s MFMA peak.  At res4, where the scores
fit in memory, also torch's autograd of bmm / softmax / bmm on the same operands (forward + backward and backward alone) and the largest
difference of the three gradients; the res3 scores (16.6 GB per clip in fp32) are never materialised."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

PEAK = 2.5e15
SHAPES = {'res4': (8 * 48 * 84, 8 * 24 * 42, 128), 'res3': (8 * 96 * 168, 8 * 48 * 84, 64)}


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
    for name in (sys.argv[1:] or ['res4', 'res3']):
        L, Lk, D = SHAPES[name]
        q = torch.randn((L, D), generator=g, device='cuda').to(td)
        k = torch.randn((Lk, D), generator=g, device='cuda').to(td)
        v = torch.randn((Lk, D), generator=g, device='cuda').to(td)
        dy = torch.randn((L, D), generator=g, device='cuda').to(td)
        scale = D ** -0.5
        y, lse = ops.nonlocal_attention_lse(q, k, v, ops.BF16, 1, D, scale)
        dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
        iters = 2 if name == 'res3' else 5
        ms_f = _timed(lambda: ops.nonlocal_attention_lse(q, k, v, ops.BF16, 1, D, scale, out=y), iters)
        ms_b = _timed(lambda: ops.nonlocal_attention_bwd(q, k, v, y, dy, lse, ops.BF16, 1, D, scale, dq=dq, dk=dk, dv=dv), iters)
        flops = 14.0 * L * Lk * D
        line = '%s: forward (lse) %8.3f ms   backward %8.3f ms   backward / forward %.2f   %6.1f TFLOP/s  %.1f %% of 2.5 PFLOP/s' % (
            name, ms_f, ms_b, ms_b / ms_f, flops / ms_b * 1e-9, 100 * flops / (ms_b * 1e-3) / PEAK)
        if name == 'res4':
            q3, k3, v3 = (t.view(1, -1, D).clone().requires_grad_(True) for t in (q, k, v))

            def fwd():
                s = torch.bmm(q3, k3.transpose(1, 2)) * scale
                return torch.bmm(torch.softmax(s, dim=2), v3)

            def fwd_bwd():
                for t in (q3, k3, v3):
                    t.grad = None
                fwd().backward(dy.view(1, -1, D))
            with torch.no_grad():
                ms_uf = _timed(fwd, iters=5)
            ms_ufb = _timed(fwd_bwd, iters=5)
            fwd_bwd()
            err = max(float((a.grad.view(-1, D).float() - b.float()).abs().max()) for a, b in ((q3, dq), (k3, dk), (v3, dv)))
            line += '\n      torch autograd of bmm / softmax / bmm: forward + backward %8.3f ms, backward alone about %8.3f ms  ' \
                    '(fused backward / that %.2f, max |gradient difference| %.3g)' % (ms_ufb, ms_ufb - ms_uf, ms_b / (ms_ufb - ms_uf), err)
        print(line, flush=True)
        del q, k, v, dy, y, lse, dq, dk, dv


if __name__ == '__main__':
    main()
