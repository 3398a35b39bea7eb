"""FPN3D keypoint R-CNN with a ResNeXt body (grouped `branch2b` convs, spatial stride on the 3 x 3) on the GPU: the fp32 forward against
the restatement (tests/grouped_ref.py: per-group dense convs on the oracle graph), graph replay against eager in bf16, and the shipped
ResNeXt-101 32x8d config through tools/test_net.py and the pipelined engine."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.grouped_ref import resnext_net
from tests.model_util import fpn3d_kps_cfg, build_product, synthetic_clip, oracle_opts
from tests.test_gpu_parity_full import _check_against_oracle

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS, WIDTH = 32, 4          # the reduced model: 128 / 256 / 512 / 1024 inner channels in 32 groups of 4 / 8 / 16 / 32


def _cfg(**kw):
    c = fpn3d_kps_cfg('50', **kw)
    c['RESNETS'] = {'NUM_GROUPS': GROUPS, 'WIDTH_PER_GROUP': WIDTH, 'STRIDE_1X1': False}
    return c


def _grouped_tags(tags):
    return [t for t in tags if t // 10 == 64257]


def test_fp32_resnext_forward_matches_the_restatement():
    """One 3 x 64 x 96 clip of T = 3, synthetic weights, fp32: pool1, every res*_sum and fpn_res*_sum blob within 1e-3 * max(1, |ref|max), the rois, the box
    head and kps_score (< 1e-3 max-abs); all 16 `branch2b` convs ran on the grouped kernel."""
    from detectandtrack_amd.ops import hip_ops as ops
    T, H, W = 3, 64, 96
    model, ws, weights = build_product(_cfg(T=T, dtype='fp32', pre=300, post=100))
    assert weights['res3_0_branch2b_w'].shape == (256, 8, 3, 3, 3)
    data = synthetic_clip(T, H, W)
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    prof = ops.ConvProfiler(capacity=4096)
    prof.start()
    ws.RunNet(model.net.name)
    tags = [t for t, _, _ in prof.stop()]
    assert len(_grouped_tags(tags)) == 3 + 4 + 6 + 3, 'grouped kernel launches: %d' % len(_grouped_tags(tags))
    torch.set_num_threads(max(1, min(64, torch.get_num_threads())))
    net = resnext_net(GROUPS)(weights, oracle_opts('50', T, 3, 'slice-center', 300, 100))
    net.body(torch.from_numpy(data))
    pyr = net.fpn()
    names = ['pool1'] + sorted(b for b in ws.Blobs() if b.endswith('_sum') and b.startswith(('res', 'fpn_res')))
    # (the Sum of every block but a stage's last is folded in place into its `branch2c` conv: the stage outputs are the `_sum` blobs)
    assert [n for n in names if n.startswith('res')] == ['res2_2_sum', 'res3_3_sum', 'res4_5_sum', 'res5_2_sum']
    _check_against_oracle(model, ws, weights, net, pyr, im_info, 12, names, True)


def test_bf16_clip_graph_replay_equals_eager():
    """bf16: a captured clip graph replayed on new clips gives exactly the eager results (the grouped launches are capturable)."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.clip_graph import ClipGraph
    from detectandtrack_amd.core.config import cfg
    from detectandtrack_amd.ops import hip_ops
    T, H, W = 3, 128, 160
    mode = 'fp16' if hip_ops.H16_DTYPE == torch.float16 else 'bf16'     # (the loaded build's 16-bit mode)
    model, ws, _ = build_product(_cfg(T=T, dtype=mode, pre=300, post=100))
    cfg.TEST.SCORE_THRESH = 0.0
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    clips = [torch.from_numpy(synthetic_clip(T, H, W, seed=s)).cuda() for s in (3, 4)]

    def eager(data):
        ws.FeedBlob('data', data)
        ws.FeedBlob('im_info', im_info)
        ws.RunNet(model.net.name)
        return engine.read_results_from_device(*engine.enqueue_results_on_device(model, (H, W, 3), 1.0))
    ref = [eager(c) for c in clips]
    g = ClipGraph(model, ws, clips[0], im_info, (H, W, 3), stream=torch.cuda.Stream())
    for c, (rb, rk) in zip(clips, ref):
        g.launch(c)
        boxes, keyps = g.results()
        np.testing.assert_array_equal(boxes[1], rb[1])
        assert len(keyps[1]) == len(rk[1]) > 0
        for a, b in zip(keyps[1], rk[1]):
            np.testing.assert_array_equal(a, b)


def test_shipped_resnext101_config_runs_through_test_net(tmp_path):
    """configs/test_x101_32x8d_fpn3d_synthetic.yaml, four synthetic clips, through the pipelined engine.  (`--synthetic` clips carry no
    frame ids, and with the config's per-frame trunk cache on the engine runs such clips one at a time through the eager loop: the
    cache is switched off on the command line, as for any run on unrelated clips.)"""
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'test_net.py'), '--cfg',
                        os.path.join(REPO, 'configs', 'test_x101_32x8d_fpn3d_synthetic.yaml'), '--synthetic', '4', '--synthetic-weights',
                        'OUTPUT_DIR', str(tmp_path), 'HIP.FRAME_TRUNK_CACHE', '0'], env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    stats = [json.loads(ln)['test_net'] for ln in p.stdout.decode().splitlines() if ln.startswith('{"test_net"')]
    assert stats and stats[0]['clips'] == 4, p.stdout.decode()[-2000:]
