"""The tracker's appearance cost (TRACKING.DISTANCE_METRICS 'cnn-cosdist') per frame: 8, 32 and 100 boxes of one
720 x 1280 frame, features of `layer3`, bf16 and fp32, random He-initialised ResNet-18 weights.

    python tools/probes/track_cost_probe.py            the table of DESIGN.md section 3.15
    python tools/probes/track_cost_probe.py layers     additionally, per conv launch of one forward: blob, profiler tag, ms

Per case, medians of 5 rounds of 10 back-to-back calls between two HIP events after 2 warm-up calls: `upload` (the uint8 frame, host to
device), `crop` (dat_crop_resize_patches), `trunk` (one forward of the body with N = boxes), `cosine` (dat_cosine_cost, boxes x boxes);
`frame wall` is the host wall-clock of one uncached `embed` + one `cosine` with a synchronisation at the end (what the tracker waits for
per frame), and `launches` the number of conv launches of the forward."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

BOXES = (8, 32, 100)
MODES = ('bf16', 'fp32')


def _timed(fn, iters=10, rounds=5):
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


def main(layers=False):
    import torch
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.core.track_features import TrackFeatureExtractor
    from detectandtrack_amd.ops import hip_ops as ops
    from detectandtrack_amd.utils import image as iu
    rs = np.random.RandomState(0)
    frame = rs.randint(0, 256, (720, 1280, 3)).astype(np.uint8)
    from tests.track_costs_ref import random_resnet18_state
    state = random_resnet18_state(seed=9)
    print('%-5s %5s | %9s %9s %9s %9s | %12s %9s' % ('mode', 'boxes', 'upload ms', 'crop ms', 'trunk ms', 'cosine ms', 'frame wall ms', 'launches'))
    for mode in MODES:
        if mode == 'bf16' and ops.L.H16 == 'fp16':
            mode = 'fp16'
        reset_cfg()
        cfg.HIP.DTYPE = mode
        ex = TrackFeatureExtractor(state=state, layer='layer3')
        for n in BOXES:
            ctr = rs.uniform([100, 100], [1180, 620], (n, 2))
            size = rs.uniform(60, 220, (n, 2))
            boxes = np.hstack([ctr - size / 2, ctr + size / 2, np.ones((n, 1))]).astype(np.float32)
            ranges = iu.crop_ranges(boxes[:, :4], 720, 1280)
            host = torch.from_numpy(frame)
            dev = host.cuda()
            data = ops.crop_resize_patches(dev, ranges, 224, iu.TRACK_CNN_MEAN, iu.TRACK_CNN_STD)
            feat, D, dt = ex.forward(data)
            feat = feat.clone()
            t_up = _timed(lambda: host.cuda())
            t_crop = _timed(lambda: ops.crop_resize_patches(dev, ranges, 224, iu.TRACK_CNN_MEAN, iu.TRACK_CNN_STD, out=data))
            t_trunk = _timed(lambda: ex.forward(data))
            t_cos = _timed(lambda: ops.cosine_cost(feat, feat, D, dt))
            ex.ws.conv_log = []
            prof = ops.ConvProfiler(capacity=64)
            prof.start()
            ex.forward(data)
            torch.cuda.synchronize()
            recs, names = prof.stop(), [r[0] for r in ex.ws.conv_log]
            ex.ws.conv_log = None
            walls = []
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f2, _, _ = ex.embed(frame, boxes)
                ops.cosine_cost(feat, f2, D, dt)
                torch.cuda.synchronize()
                walls.append((time.perf_counter() - t0) * 1e3)
            print('%-5s %5d | %9.3f %9.3f %9.3f %9.3f | %12.3f %9d' % (mode, n, t_up, t_crop, t_trunk, t_cos, float(np.median(walls[2:])), len(recs)))
            if layers:
                for name, (tag, _, ms) in zip(names, recs):
                    print('        %-22s tag %-8d %.4f ms' % (name, tag, ms))
    reset_cfg()


if __name__ == '__main__':
    main(layers='layers' in sys.argv[1:])
