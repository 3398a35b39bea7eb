"""FPN3D keypoint R-CNN with spacetime non-local blocks (HIP.NONLOCAL) on the GPU: the forward against the
restatement on the oracle graph (tests/nonlocal_ref.NetNonLocal) in fp32 and bf16x3, R-18 (D 64 / 128) and R-50 (D 256 / 512); the
identity a zeroed last affine gives; and, in the 16-bit mode, graph replay and two clips per forward against the eager one-clip loop."""
import numpy as np
import pytest
import torch

from tests.model_util import fpn3d_kps_cfg, build_product, synthetic_clip, oracle_opts
from tests.nonlocal_ref import NetNonLocal, parse_spec
from tests.test_gpu_parity_full import _check_against_oracle

pytestmark = pytest.mark.gpu

# `synthetic_params` gives theta / phi outputs of O(1), so the scores are small and the softmax nearly uniform -- a mean filter, which
# would pass a kernel that ignores q.  Each block's theta is scaled up (weights AND bias) until a query row looks at a handful of keys;
# the tests assert that condition on the restatement: 4 <= median exp(entropy) <= L' / 4.
THETA_GAIN = {'nonlocal_res3_1': 3.0, 'nonlocal_res4_0': 3.0, 'nonlocal_res3_3': 5.0, 'nonlocal_res4_5': 3.0}


def _cfg(arch, spec, **kw):
    c = fpn3d_kps_cfg(arch, **kw)
    c['HIP']['NONLOCAL'] = spec
    return c


def _sharpen(weights):
    for k in weights:
        if k.startswith('nonlocal_') and k.endswith(('_theta_w', '_theta_b')):
            weights[k] = (weights[k] * THETA_GAIN[k[:k.index('_theta')]]).astype(np.float32)
    return weights


def _build(arch, spec, dtype, mutate=None):
    model, ws, weights = build_product(_cfg(arch, spec, T=4, dtype=dtype, pre=300, post=100))
    _sharpen(weights)
    if mutate is not None:
        mutate(weights)
    for k, v in weights.items():
        ws.set_param(k, v)
    return model, ws, weights


def _forward_against_restatement(arch, spec, dtype):
    T, H, W = 4, 128, 160
    model, ws, weights = _build(arch, spec, dtype)
    assert sum(op.type == 'NonLocalAttention' for op in model.net.ops) == len(parse_spec(spec))
    data = synthetic_clip(T, H, W)
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    ws.RunNet(model.net.name)
    torch.set_num_threads(max(1, min(64, torch.get_num_threads())))
    net = NetNonLocal(weights, oracle_opts(arch, T, 3, 'slice-center', 300, 100), spec)
    net.body(torch.from_numpy(data))
    pyr = net.fpn()
    for nl in sorted(net.keys_eff):
        print('%s: median effective keys %.1f of %d' % (nl, net.keys_eff[nl], net.keys_total[nl]))
        assert 4.0 <= net.keys_eff[nl] <= net.keys_total[nl] / 4.0, 'the attention of %s is degenerate (%.1f of %d keys)' % (
            nl, net.keys_eff[nl], net.keys_total[nl])
    names = ['pool1'] + sorted(b for b in ws.Blobs() if b.endswith('_sum') and b.startswith(('res', 'fpn_res', 'nonlocal_')))
    assert all('nonlocal_' + p + '_y' in ws.Blobs() for p in parse_spec(spec))
    names += sorted('nonlocal_' + p + '_y' for p in parse_spec(spec))
    return _check_against_oracle(model, ws, weights, net, pyr, im_info, 12, names, True)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_r18_forward_matches_the_restatement(dtype):
    """R-18 FPN3D, 4 x 128 x 160, blocks behind res3_1 (last of its stage, D 64) and res4_0 (mid-stage, D 128): every res*_sum,
    nonlocal_*_sum and fpn_* blob, the rois, the box head and kps_score (< 1e-3)."""
    _forward_against_restatement('18', 'res3_1,res4_0', dtype)


def test_r50_forward_matches_the_restatement():
    """R-50 FPN3D, the same clip, fp32: D 256 behind res3_3 and D 512 (the sliced-value path) behind res4_5, both last of their stage."""
    _forward_against_restatement('50', 'res3_3,res4_5', 'fp32')


def test_zeroed_last_affine_is_the_base_network_bit_for_bit():
    """`_out_bn_s` = `_out_bn_b` = 0 (what a checkpoint without the block's blobs gets): every blob the two graphs share equals that of
    the plain model fed the same named weights."""
    T, H, W = 4, 128, 160
    spec = 'res3_1,res4_0'
    data = synthetic_clip(T, H, W)
    im_info = np.array([[H, W, 1.0]], dtype=np.float32)

    def zero(weights):
        for k in weights:
            if k.endswith(('_out_bn_s', '_out_bn_b')):
                weights[k] = np.zeros_like(weights[k])
    model, ws, weights = _build('18', spec, 'fp32', zero)
    ws.FeedBlob('data', data)
    ws.FeedBlob('im_info', im_info)
    ws.RunNet(model.net.name)
    shared = ['pool1', 'res2_1_sum', 'res3_1_sum', 'res4_1_sum', 'res5_1_sum', 'fpn_res5_1_sum', 'fpn_res4_1_sum', 'fpn_res3_1_sum',
              'fpn_res2_1_sum', 'rois', 'cls_prob', 'bbox_pred']
    with_blocks = {n: ws.FetchBlob(n).copy() for n in shared}
    np.testing.assert_array_equal(ws.FetchBlob('res3_1_sum'), ws.FetchBlob('res3_1_sum_nl_in'))
    assert float(np.abs(ws.FetchBlob('nonlocal_res4_0_y')).max()) > 0.1        # the branch did run
    plain, ws2, w2 = build_product(fpn3d_kps_cfg('18', T=T, dtype='fp32', pre=300, post=100))
    assert not any(k.startswith('nonlocal_') for k in w2) and set(w2) < set(weights)
    for k in w2:
        ws2.set_param(k, weights[k])
    ws2.FeedBlob('data', data)
    ws2.FeedBlob('im_info', im_info)
    ws2.RunNet(plain.net.name)
    for n in shared:
        np.testing.assert_array_equal(with_blocks[n], ws2.FetchBlob(n), err_msg=n)


@pytest.fixture(scope='module')
def engine_runs(tmp_path_factory):
    """The placement of configs/test_r18_fpn3d_nonlocal_synthetic.yaml (res3_1, res4_1) in the 16-bit mode through core/test_engine on
    five clips: the eager one-clip loop, the pipelined engine with captured clip graphs, and the same with two clips per forward."""
    from detectandtrack_amd.core import test_engine
    from detectandtrack_amd.core.config import cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.ops import hip_ops
    from detectandtrack_amd import workspace
    T, H, W = 4, 96, 128
    rs = np.random.RandomState(5)
    roidb = [{'image': [rs.randint(0, 255, (H, W, 3)).astype(np.uint8) for _ in range(T)], 'height': H, 'width': W} for _ in range(5)]
    mode = 'fp16' if hip_ops.H16_DTYPE == torch.float16 else 'bf16'

    def run(depth, per, graph, name):
        c = _cfg('18', 'res3_1,res4_1', T=T, dtype=mode, pre=300, post=100)
        c['TEST'].update(SCALES=(H,), MAX_SIZE=max(H, W), SCORE_THRESH=0.0, DETECTIONS_PER_IM=15)
        c['HIP'].update(PIPELINE_DEPTH=depth, IMS_PER_FORWARD=per, CLIP_GRAPH=graph)
        c['RNG_SEED'] = 3
        reset_cfg()
        cfg_from_cfg(c)
        assert_and_infer_cfg()
        workspace.ResetWorkspace()
        res = test_engine.test_net(roidb, None, str(tmp_path_factory.mktemp(name)))
        return res, test_engine.test_net.last_stats
    runs = {'eager': run(0, 1, False, 'eager'), 'graph': run(3, 1, True, 'graph'), 'two': run(2, 2, True, 'two')}
    reset_cfg()
    return runs


def test_16_bit_graph_replay_equals_eager_and_two_clips_per_forward_keep_their_boxes(engine_runs):
    """Captured clip graphs replayed on five clips write the detections of the eager one-clip loop bit for bit, boxes and keypoints
    (the attention is captured like a conv); with HIP.IMS_PER_FORWARD 2 every clip's boxes equal, bit for bit, those it gets alone."""
    eager = engine_runs['eager'][0]
    got, st = engine_runs['graph']
    assert st['clips'] == 5 and st['per_forward'] == 1
    for i in range(5):
        np.testing.assert_array_equal(got['all_boxes'][1][i], eager['all_boxes'][1][i])
        assert len(got['all_keyps'][1][i]) == len(eager['all_keyps'][1][i]) >= 15
        for a, b in zip(got['all_keyps'][1][i], eager['all_keyps'][1][i]):
            np.testing.assert_array_equal(a, b)
    got, st = engine_runs['two']
    assert st['per_forward'] == 2
    for i in range(5):
        assert got['all_boxes'][1][i].shape[0] >= 15
        np.testing.assert_array_equal(got['all_boxes'][1][i], eager['all_boxes'][1][i])


def test_16_bit_two_clips_per_forward_keep_the_keypoints_of_a_clip_alone(engine_runs):
    """With HIP.IMS_PER_FORWARD 2 every clip's keypoints equal, bit for bit, those it gets alone.

    The keypoint head runs once per forward over the RoI rows of all its clips.  Its convs take the split-K factor the planner picks
    for ONE clip's rows (dat_conv_desc.plan_frames, workspace.op_Conv), so the fp32 partial sums of a heat map are added in the order
    they are added when the clip runs alone.  Planned from the whole grid (the factor then differs between one clip's rows and two
    clips') the heat maps differed in their last bits and, with random weights, their maxima moved: up to 37.5 px in bf16 with the
    blocks, up to 124 px without them."""
    eager, got = engine_runs['eager'][0], engine_runs['two'][0]
    worst = []
    for i in range(5):
        ka, kb = got['all_keyps'][1][i], eager['all_keyps'][1][i]
        assert len(ka) == len(kb)
        worst.append(max(float(np.abs(a - b).max()) for a, b in zip(ka, kb)))
    print('largest keypoint difference per clip, two per forward against alone: %s' % ', '.join('%.4g' % w for w in worst))
    for i in range(5):
        for a, b in zip(got['all_keyps'][1][i], eager['all_keyps'][1][i]):
            np.testing.assert_array_equal(a, b)
