"""dat_oks_nms (KRCNN.NMS_OKS on the device) per launch: 104 live rows per image (DETECTIONS_PER_IM 100 + the spare
rows), T = 1 and T = 3, 1 and 4 images per call.

    python tools/probes/oks_nms_probe.py

Two inputs per case: `clustered` (the seeded clusters of tests/oks_nms_ref.py: about half of the rows are removed) and `all kept` (poses
far apart: nothing is removed, the greedy loop runs its longest, one round per row).  Medians of 5 rounds of 20 back-to-back launches
between two HIP events after 2 warm-up launches, in microseconds; the outputs are allocated once, outside the timed region."""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

CAP = 104


def _timed(fn, iters=20, rounds=5):
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
        out.append(e0.elapsed_time(e1) / iters * 1e3)
    return float(np.median(out))


def main():
    import torch
    from detectandtrack_amd.ops import hip_ops as ops
    from tests import oks_nms_ref as R
    print('%-10s %2s %6s | %8s %10s' % ('input', 'T', 'images', 'kept', 'launch us'))
    for T in (1, 3):
        for ni in (1, 4):
            for name in ('clustered', 'all kept'):
                kps, dets = zip(*[R.clustered_poses(CAP, T, R.seed_for(CAP, T) + i) for i in range(ni)])
                kps, dets = np.concatenate(kps), np.concatenate(dets)
                if name == 'all kept':
                    kps[:, 0] += (np.arange(ni * CAP, dtype=np.float32) * 5000)[:, None]
                kps_d, dets_d = torch.from_numpy(kps).cuda(), torch.from_numpy(dets).cuda()
                n_rows = torch.full((ni,), CAP, dtype=torch.int32, device='cuda')
                d_out, k_out = torch.empty_like(dets_d), torch.empty_like(kps_d)
                keep = torch.empty((ni, CAP), dtype=torch.int32, device='cuda')
                n_keep = torch.empty((ni,), dtype=torch.int32, device='cuda')
                ctx, args = ops.ctx(), (ops._ptr(kps_d), ops._ptr(dets_d), int(dets_d.shape[1]), ops._ptr(n_rows), 1, CAP, ni, T, R.K,
                                        C.c_double(R.THRESH), ops._ptr(keep), ops._ptr(n_keep), ops._ptr(d_out), ops._ptr(k_out))
                us = _timed(lambda: ctx.call('dat_oks_nms', ops._stream(), *args))
                print('%-10s %2d %6d | %8s %10.1f' % (name, T, ni, '/'.join(str(int(v)) for v in n_keep.cpu().numpy()), us))


if __name__ == '__main__':
    main()
