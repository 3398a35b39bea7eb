"""Soft-NMS / box voting on the device: what they cost.

    python tools/probes/soft_nms_ab.py [rois per image] [images per launch] [frames per tube]
        (frames per tube > 1: tube detections, HIP.TUBE_SOFT_NMS; soft_nms_kernel / box_vote_kernel for every T)
        ops.box_results (select + decode, NMS or Soft-NMS, voting, limit + emit) with each Soft-NMS method and with voting against
        hard NMS on the same clustered synthetic proposals: hip events, median of 50 launches after 10 warm-up launches.
    python tools/probes/soft_nms_ab.py e2e <tree> [cfg opts ...]
        end-to-end clips/s of core/test_engine.test_net (what tools/test_net.py --synthetic runs) on the bench network, four clips per
        forward, from the checkout at <tree> (this commit: `.`; a checkout of the parent commit with its library built: the host path
        when TEST.SOFT_NMS.ENABLED True is among the opts).  Wall time of 52 clips minus wall time of 4 clips -- model build, weight
        packing and graph capture are in both -- best of two each."""
import os
import sys

import numpy as np
import torch

E2E = len(sys.argv) > 2 and sys.argv[1] == 'e2e'
sys.path.insert(0, os.path.abspath(sys.argv[2]) if E2E else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from detectandtrack_amd.ops import hip_ops as ops  # noqa: E402


def e2e(root, opts):
    import json
    import tempfile
    import time
    from detectandtrack_amd.core.config import cfg_from_file, cfg_from_list, assert_and_infer_cfg
    from detectandtrack_amd.core import test_engine
    cfg_from_file(os.path.join(root, 'configs', 'test_r18_fpn3d_synthetic.yaml'))
    # (--synthetic clips carry no frame ids, which the per-frame trunk cache needs; four clips per forward as bench.py)
    cfg_from_list(['HIP.FRAME_TRUNK_CACHE', '0', 'HIP.IMS_PER_FORWARD', '4'] + list(opts))
    assert_and_infer_cfg()
    test_engine.SYNTHETIC_WEIGHTS = True
    rs = np.random.RandomState(3)
    roidb = [{'image': [rs.randint(0, 255, (720, 1280, 3)).astype(np.uint8) for _ in range(8)], 'height': 720, 'width': 1280}
             for _ in range(52)]
    out = tempfile.mkdtemp()

    def run(n):
        torch.cuda.synchronize()
        t = time.time()
        test_engine.test_net(roidb[:n], None, out)
        torch.cuda.synchronize()
        return time.time() - t
    run(4)
    small = min(run(4), run(4))
    big = min(run(52), run(52))
    st = getattr(test_engine.test_net, 'last_stats', None)
    print(json.dumps({'tree': root, 'opts': list(opts), 'clips_per_s': round(48.0 / (big - small), 2), 'seconds_4_clips': round(small, 3),
                      'seconds_52_clips': round(big, 3), 'pipelined_engine': st is not None,
                      'steady_clips_per_s': st.get('steady_clips_per_s') if st else None}))


def inputs(seed, R, K, H=720, W=1280, T=1):
    rs = np.random.RandomState(seed)
    centres = np.stack([rs.uniform(100, W - 300, 12), rs.uniform(100, H - 300, 12)], axis=1)
    xy = centres[rs.randint(0, 12, R)] + rs.uniform(-40, 40, (R, 2))
    wh = rs.uniform(60, 260, (R, 2))
    rois = np.zeros((R, 4 * T + 1), np.float32)
    rois[:, 1:3], rois[:, 3:5] = xy, xy + wh
    for t in range(1, T):                          # (the frames of a tube: the first frame's box moved by up to 4 pixels)
        jit = rs.uniform(-4, 4, (R, 2))
        rois[:, 1 + 4 * t:3 + 4 * t], rois[:, 3 + 4 * t:5 + 4 * t] = xy + jit, xy + jit + wh
    logits = rs.randn(R, K).astype(np.float32) * 2
    prob = (np.exp(logits) / np.exp(logits).sum(axis=1, keepdims=True)).astype(np.float32)
    pred = (rs.randn(R, K * 4 * T) * 0.5).astype(np.float32)
    return rois, prob, pred


def main():
    if E2E:
        return e2e(os.path.abspath(sys.argv[2]), sys.argv[3:])
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    ni = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    K = 2
    per = [inputs(i, R, K, T=T) for i in range(ni)]
    rois, prob, pred = (torch.from_numpy(np.concatenate([p[c] for p in per])).cuda() for c in range(3))
    n_rois = torch.tensor([R] * ni, dtype=torch.int32).cuda()
    modes = [('hard NMS', None, None), ('soft hard', 'hard', None), ('soft linear', 'linear', None), ('soft gaussian', 'gaussian', None),
             ('hard NMS + vote', None, 0.8), ('soft linear + vote', 'linear', 0.8)]
    for thr in (0.05, 0.0):
        for name, soft, vote in modes:
            def run():
                return ops.box_results(rois, n_rois, prob, pred, K, T, 1.0, (720, 1280, 3), (10., 10., 5., 5.), float(np.float32(np.log(1000. / 16.))),
                                       thr, 0.5, 100, 104, n_images=ni,
                                       soft_nms=dict(method=soft, sigma=0.5, score_thresh=0.0001) if soft else None, bbox_vote=vote,
                                       tubes=T > 1)
            for _ in range(10):
                out = run()
            ts = []
            for _ in range(50):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = run()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            print('%d rois x %d images, T %d, SCORE_THRESH %.2f  %-20s %8.1f us   (rows kept %s)' % (
                R, ni, T, thr, name, float(np.median(ts)), out[2].cpu().numpy().reshape(-1, 2)[:, 1].tolist()))


if __name__ == '__main__':
    main()
