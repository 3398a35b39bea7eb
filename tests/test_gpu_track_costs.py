"""The tracker's appearance cost on the device: dat_crop_resize_patches bit for bit against its host
restatement, dat_cosine_cost per element against float64, the ResNet-18 feature extractor against a float64 restatement of
torchvision's forward, and the tracker end to end on frames whose people swap places."""

import numpy as np
import pytest
import torch

from tests import numerics as nm
from tests.track_costs_ref import Dataset, POSETRACK_KEYPOINTS, cosine_cost64, random_resnet18_state, resnet18_forward64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# Largest deviation of the layer3 cost matrix of `test_extractor_16_bit_mode_stays_near_fp32` from the fp32-mode matrix, measured on the
# MI355X, per 16-bit build format; the test allows twice that for box-to-box differences.
H16_COST_DEV = {'bf16': 1.485e-4, 'fp16': 9.0e-6}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


@pytest.fixture
def cfg():
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    yield cfg
    reset_cfg()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _refused(ops, fn, match):
    from detectandtrack_amd.libdat import DatError
    prof = ops.ConvProfiler(capacity=8)
    prof.start()
    try:
        with pytest.raises(DatError, match=match) as e:
            fn()
    finally:
        launched = prof.stop()
    assert '(code -1)' in str(e.value), str(e.value)       # DAT_ERR_ARG
    assert launched == [], 'a refused call launched %r' % (launched,)


# ---- crop kernel -------------------------------------------------------------------------------------------------------------------------
def _frame(seed=0, h=96, w=128):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _crop_boxes(out):
    """x1, y1, x2, y2 on a 96 x 128 frame.  (A crop of exactly 224 x 224 does not fit the frame: at out = 224 that row is one more
    crop clipped at two borders, at out = 7 it is the identity resize.)"""
    return np.array([[10.3, 8.7, 70.2, 60.9],              # ordinary, fractional
                     [20, 5, 21, 50],                      # 1 pixel wide
                     [5, 30, 100, 31],                     # 1 pixel high
                     [0, 0, 128, 96],                      # the whole frame
                     [10, 10, 10 + out, 10 + out],         # exactly out-sized
                     [30, 30, 30, 40],                     # empty: x2 == x1
                     [50, 50, 40, 60],                     # empty: x2 < x1
                     [-0.5, 10, 30, 40],                   # left border (int() truncates towards zero)
                     [10, -0.9, 40, 30],                   # top border
                     [100, 10, 140.5, 50],                 # right border: clipped
                     [10, 80, 50, 120],                    # bottom border: clipped
                     [-20, -10, 128, 96],                  # negative starts count from the far border
                     [126, 94, 500, 500]],                 # the last 2 x 2 pixels
                    dtype=np.float32)


@pytest.mark.parametrize('out', [224, 7])
def test_crop_kernel_is_bit_identical_to_the_host_restatement(ops, out):
    from detectandtrack_amd.utils import image as iu
    frame = _frame()
    ranges = iu.crop_ranges(_crop_boxes(out), 96, 128)
    want = torch.from_numpy(iu.crop_resize_patches(frame, ranges, out))
    got = ops.crop_resize_patches(torch.from_numpy(frame).cuda(), ranges, out, iu.TRACK_CNN_MEAN, iu.TRACK_CNN_STD)
    assert tuple(got.shape) == (len(ranges), 3, 1, out, out) and got.dtype == torch.float32
    got = got.cpu().view(len(ranges), 3, out, out)
    for i in range(len(ranges)):
        assert torch.equal(_bits(got[i]), _bits(want[i])), 'box %d %r: %d of %d elements differ, max |diff| %.3g' % (
            i, ranges[i].tolist(), int((_bits(got[i]) != _bits(want[i])).sum()), want[i].numel(), float((got[i] - want[i]).abs().max()))
    # the empty crops are the normalised zero image, not zeros
    assert float(want[5].abs().min()) > 1.0


def test_crop_kernel_more_boxes_than_one_launch_holds(ops):
    """More than 128 boxes take a second launch of the same kernel: every box still lands in its own slot."""
    from detectandtrack_amd.utils import image as iu
    rs = np.random.RandomState(4)
    frame = _frame(1)
    xy = rs.uniform(0, 90, (131, 2))
    boxes = np.hstack([xy, xy + rs.uniform(1, 40, (131, 2))]).astype(np.float32)
    ranges = iu.crop_ranges(boxes, 96, 128)
    want = torch.from_numpy(iu.crop_resize_patches(frame, ranges, 5))
    got = ops.crop_resize_patches(torch.from_numpy(frame).cuda(), ranges, 5, iu.TRACK_CNN_MEAN, iu.TRACK_CNN_STD).cpu().view(131, 3, 5, 5)
    assert torch.equal(_bits(got), _bits(want))


def test_crop_kernel_no_boxes_and_refusals(ops):
    from detectandtrack_amd.utils import image as iu
    dev = torch.from_numpy(_frame()).cuda()
    mean, std = iu.TRACK_CNN_MEAN, iu.TRACK_CNN_STD
    empty = ops.crop_resize_patches(dev, np.zeros((0, 4), np.int32), 7, mean, std)
    assert tuple(empty.shape) == (0, 3, 1, 7, 7)
    sentinel = torch.full((2, 3, 1, 7, 7), 123.0, device='cuda')
    for bad in ([[0, 129, 0, 10], [0, 5, 0, 5]], [[0, 5, 0, 5], [3, 9, -1, 10]], [[0, 5, 0, 97], [0, 5, 0, 5]], [[-2, 5, 0, 9], [0, 5, 0, 5]]):
        _refused(ops, lambda: ops.crop_resize_patches(dev, np.array(bad, np.int32), 7, mean, std, out=sentinel), 'outside the 128 x 96 frame')
    _refused(ops, lambda: ops.crop_resize_patches(dev, np.array([[0, 5, 0, 5]], np.int32), 0, mean, std, out=sentinel[:0]), 'output size 0')
    import ctypes as C
    d3 = (C.c_double * 3)(*mean)
    _refused(ops, lambda: ops.ctx().call('dat_crop_resize_patches', ops._stream(), ops._ptr(dev), 96, 128, None, -1, 7, d3, d3,
                                         ops._ptr(sentinel)), '-1 boxes')
    torch.cuda.synchronize()
    assert bool((sentinel == 123.0).all()), 'a refused call wrote to its output'


# ---- cosine kernel -----------------------------------------------------------------------------------------------------------------------
# (n, m, D, ld, zero rows): one 16 x 16 tile; a partial k step and zero rows; many chunks (layer3's D); all four waves of a block;
# poisoned tail columns behind D; rows that are not 16-byte aligned (element-wise operand loads); more than one 128-row tile and a
# partial last chunk
COS_CASES = [(1, 1, 64, 64, False), (3, 5, 200, 200, True), (17, 9, 50176, 50176, False), (100, 100, 4096, 4096, False),
             (5, 7, 200, 264, True), (3, 5, 200, 203, False), (130, 3, 1000, 1000, False)]
_COS = {}


def _cos_operands(case, mode):
    """fp32 numpy operands [n, ld] / [m, ld] (ReLU-like, as the trunk's features are), rounded to the build's 16-bit format in the 16-bit
    mode; columns behind D hold NaN.  Made once per (case, mode) and left unchanged."""
    key = (case, mode)
    if key not in _COS:
        n, m, D, ld, zero = case
        rs = np.random.RandomState(n * 1000 + m * 10 + D % 97)
        fa = np.maximum(rs.randn(n, ld) + 0.3, 0).astype(np.float32)
        fb = np.maximum(rs.randn(m, ld) + 0.3, 0).astype(np.float32)
        fb[: min(n, m)] += 0.5 * fa[: min(n, m)]                 # some pairs are close, some far
        if zero:
            fa[0] = 0
            fb[m - 1] = 0
        if mode == 'bf16':
            fa, fb = nm.q16(fa), nm.q16(fb)
        fa[:, D:] = np.nan
        fb[:, D:] = np.nan
        _COS[key] = (fa, fb)
    return _COS[key]


def _cos_bound(fa, fb):
    """Per-element bound on |cost - ref| of a kernel that sums d = a.b, A = |a|^2, B = |b|^2 in fp32 and finishes 1 - d / sqrt(A * B) in fp32.

    Each sum carries nm.sum_bound: |dd| <= ed = C sqrt(D) 2^-24 sum|a_k b_k|, and A' = A (1 + alpha), B' = B (1 + beta) with
    |alpha| <= ea / A =: a, |beta| <= eb / B =: b (ea = C sqrt(D) 2^-24 A: the terms of a squared norm are positive).
    With r = d / sqrt(A B) and s = 1 / sqrt((1 + alpha)(1 + beta)),  |s - 1| <= g := 1 / sqrt((1 - a)(1 - b)) - 1  (the worst case, both
    norms too small), the exactly finished quotient is  r' = (d + dd) s / sqrt(A B),  so
        |r' - r| <= (|d| g + ed (1 + g)) / sqrt(A B) =: e1.
    The fp32 finish rounds the product A' B' (u), its root (u / 2 inherited + u), the division (u): (1 + theta), |theta| <= 5 u covers them
    with their second-order terms; the subtraction adds u |1 - r'|.  Total: e1 + 5 u (|r| + e1) + u (|1 - r| + e1) + the smallest half-ulp."""
    D = fa.shape[1]
    a64, b64 = fa.astype(np.float64), fb.astype(np.float64)
    d = a64 @ b64.T
    A, B = np.sum(a64 * a64, axis=1), np.sum(b64 * b64, axis=1)
    ed = np.vectorize(lambda v: nm.sum_bound(v, D))(np.abs(a64) @ np.abs(b64).T)
    live = (A[:, None] > 0) & (B[None, :] > 0)
    ra = np.array([nm.sum_bound(v, D) / v if v > 0 else 0.0 for v in A])
    rb = np.array([nm.sum_bound(v, D) / v if v > 0 else 0.0 for v in B])
    assert ra.max() < 0.5 and rb.max() < 0.5
    g = 1.0 / np.sqrt((1 - ra[:, None]) * (1 - rb[None, :])) - 1.0
    den = np.where(live, np.sqrt(A[:, None] * B[None, :]), 1.0)
    r = d / den
    e1 = (np.abs(d) * g + ed * (1 + g)) / den
    bound = e1 + 5 * U * (np.abs(r) + e1) + U * (np.abs(1 - r) + e1) + 2.0 ** -150
    return np.where(live, bound, 0.0)       # a zero row: exactly 1


@pytest.mark.parametrize('mode', ['bf16', 'fp32'])
@pytest.mark.parametrize('case', COS_CASES, ids=lambda c: 'n%d_m%d_D%d_ld%d' % c[:4])
def test_cosine_kernel_within_the_propagated_bound(ops, case, mode):
    n, m, D, ld, zero = case
    dt = ops.BF16 if mode == 'bf16' else ops.F32
    fa, fb = _cos_operands(case, mode)
    ta, tb = torch.from_numpy(fa).cuda().to(ops.tdtype(dt)), torch.from_numpy(fb).cuda().to(ops.tdtype(dt))
    got = ops.cosine_cost(ta, tb, D, dt)
    again = ops.cosine_cost(ta, tb, D, dt)
    assert torch.equal(_bits(got), _bits(again)), 'two runs differ'
    got = got.cpu().numpy().astype(np.float64)
    ref = cosine_cost64(fa[:, :D], fb[:, :D])
    bound = _cos_bound(fa[:, :D], fb[:, :D])
    err = np.abs(got - ref)
    print('%s %s: max |err| %.3g, max err / bound %.3g' % (case, mode, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    bad = ~(err <= bound)
    assert not bad.any(), '%d of %d elements outside the bound; worst: |err| %.3g > %.3g at %r' % (
        bad.sum(), bad.size, err[bad].max(), bound[bad][np.argmax(err[bad])], np.argwhere(bad)[0].tolist())
    if zero:
        assert np.all(got[0] == 1.0) and np.all(got[:, m - 1] == 1.0)


def test_cosine_kernel_empty_sets_and_refusals(ops):
    fa, fb = torch.zeros(0, 64, device='cuda'), torch.ones(4, 64, device='cuda')
    assert tuple(ops.cosine_cost(fa, fb, 64, ops.F32).shape) == (0, 4)
    assert tuple(ops.cosine_cost(fb, fa, 64, ops.F32).shape) == (4, 0)
    big = torch.ones(1025, 8, device='cuda')
    sentinel = torch.full((1025, 4), 7.0, device='cuda')
    _refused(ops, lambda: ops.cosine_cost(big, torch.ones(4, 8, device='cuda'), 8, ops.F32, out=sentinel), 'at most 1024')
    _refused(ops, lambda: ops.cosine_cost(fb, fb, 65, ops.F32), '65 features at row stride 64')
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())


# ---- extractor ---------------------------------------------------------------------------------------------------------------------------
EX_BOXES = np.array([[10.2, 8.1, 70.9, 80.5, 0.99], [60, 20, 120, 90, 0.98], [0, 0, 128, 96, 0.97], [100, 50, 160, 120, 0.96],
                     [30, 40, 31, 90, 0.95]], dtype=np.float32)       # ordinary x2, the whole frame, clipped, 1 pixel wide


@pytest.fixture(scope='module')
def extractor_ref():
    """The float64 restatement of torchvision's forward on the HOST crops of a 96 x 128 frame, computed once."""
    from detectandtrack_amd.utils import image as iu
    torch.manual_seed(0)
    state = random_resnet18_state(seed=9)
    frame = _frame(7)
    crops = iu.crop_resize_patches(frame, iu.crop_ranges(EX_BOXES[:, :4], 96, 128), 224)
    feats = resnet18_forward64(state, torch.from_numpy(crops).double(), layers=(1, 3, 4))
    return state, frame, {k: v.numpy() for k, v in feats.items()}


def _h16_mode(ops):
    return 'fp16' if ops.L.H16 == 'fp16' else 'bf16'


@pytest.mark.parametrize('layer', ['layer1', 'layer3', 'layer4'])
def test_extractor_fp32_against_float64_torchvision_forward(ops, cfg, extractor_ref, layer):
    from detectandtrack_amd.core.track_features import TrackFeatureExtractor
    state, frame, ref = extractor_ref
    cfg.HIP.DTYPE = 'fp32'
    cfg.MODEL.USE_BN, cfg.MODEL.DILATION = True, 2          # the detector's switches must not reach the trunk
    ex = TrackFeatureExtractor(state=state, layer=layer)
    assert cfg.MODEL.USE_BN is True and cfg.MODEL.DILATION == 2
    feat, D, dt = ex.embed(frame, EX_BOXES)
    want = ref[layer]
    assert dt == ops.F32 and D == want[0].size and tuple(feat.shape) == (5, D)
    got = ex.ws.FetchBlob(ex.blob)[:, :, 0]
    err = float(np.abs(got - want).max())
    print('%s: max |err| %.3g, max |ref| %.3g' % (layer, err, np.abs(want).max()))
    assert got.shape == want.shape and err <= 1e-3 * float(np.abs(want).max())
    C = ex.cost(frame, EX_BOXES[:3], frame, EX_BOXES[2:])
    flat = want.reshape(5, -1)
    refC = cosine_cost64(flat[:3], flat[2:])
    print('%s: cost max |err| %.3g' % (layer, np.abs(C - refC).max()))
    assert C.dtype == np.float64 and C.shape == (3, 3) and np.abs(C - refC).max() <= 1e-3
    assert C[2, 0] <= 1e-3                                 # the same crop on both sides
    assert ex.cost(frame, EX_BOXES[:0], frame, EX_BOXES).shape == (0, 5) and not ex.cost(frame, EX_BOXES, frame, EX_BOXES[:0]).size


def test_extractor_16_bit_mode_stays_near_fp32(ops, cfg, extractor_ref):
    """The build's 16-bit mode against the fp32 mode on the same five crops (layer3): the deviation of the cost matrix measured on the
    MI355X is recorded in H16_COST_DEV / DESIGN.md section 3.15; twice that is allowed for box-to-box differences."""
    from detectandtrack_amd.core.track_features import TrackFeatureExtractor
    state, frame, _ = extractor_ref
    mats = {}
    for mode in ('fp32', _h16_mode(ops)):
        cfg.HIP.DTYPE = mode
        mats[mode] = TrackFeatureExtractor(state=state, layer='layer3').cost(frame, EX_BOXES, frame, EX_BOXES)
    dev = float(np.abs(mats[_h16_mode(ops)] - mats['fp32']).max())
    print('%s cost matrix: max deviation from fp32 %.4g (largest cost %.4g)' % (_h16_mode(ops), dev, mats['fp32'].max()))
    assert dev <= 2 * H16_COST_DEV[_h16_mode(ops)]


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
LEFT, RIGHT = [16, 24, 72, 96], [88, 24, 144, 96]           # x1, y1, x2, y2: mirror images of each other in a 160-wide frame


def _write_swap_video(tmp_path):
    """Three 120 x 160 PNG frames: texture A (coarse random blocks) and its inverse B sit in two symmetric boxes; between frame 0 and
    frame 1 they swap places, frame 2 repeats frame 1.  Returns (json_data, dets) with both boxes detected in every frame, left first;
    the pose of a detection is tied to its TEXTURE (and does not move), so poses swap with the textures."""
    from PIL import Image
    rs = np.random.RandomState(12)
    h, w = LEFT[3] - LEFT[1], LEFT[2] - LEFT[0]
    tex_a = np.kron(rs.randint(0, 2, (h // 8, w // 8, 3)) * 255, np.ones((8, 8, 1))).astype(np.uint8)
    tex_b = 255 - tex_a
    K = len(POSETRACK_KEYPOINTS)
    pose_a, pose_b = np.zeros((4, K), np.float32), np.zeros((4, K), np.float32)
    pose_a[:2] = rs.uniform(20, 70, (2, K))
    pose_b[:2] = pose_a[:2] + np.float32([[72.0], [0.0]])           # 72 pixels = 12 head sizes to the right
    top, bottom = POSETRACK_KEYPOINTS.index('head_top'), POSETRACK_KEYPOINTS.index('head_bottom')
    for p in (pose_a, pose_b):
        p[:2, bottom] = p[:2, top] + np.float32([3.0, 4.0])        # head size 6: 0.25 pixels of drift match, the other pose does not
    pose_a[2:], pose_b[2:] = 1.0, 1.0
    json_data, boxes, keyps = [], [], []
    for f in range(3):
        img = np.full((120, 160, 3), 128, dtype=np.uint8)
        left_tex, right_tex = (tex_a, tex_b) if f == 0 else (tex_b, tex_a)
        img[LEFT[1]:LEFT[3], LEFT[0]:LEFT[2]] = left_tex
        img[RIGHT[1]:RIGHT[3], RIGHT[0]:RIGHT[2]] = right_tex
        path = str(tmp_path / ('%03d.png' % f))
        Image.fromarray(img[:, :, ::-1].copy()).save(path)          # (the arrays are BGR)
        json_data.append({'image': path, 'height': 120, 'width': 160, 'dataset': Dataset()})
        boxes.append(np.array([LEFT + [0.99], RIGHT + [0.98]], dtype=np.float32))
        keyps.append([pose_a + 0.25 * f, pose_b + 0.25 * f] if f == 0 else [pose_b + 0.25 * f, pose_a + 0.25 * f])
    return json_data, {'all_boxes': [[], boxes], 'all_keyps': [[], keyps]}


@pytest.mark.parametrize('weights, tracks', [((1.0, 0.0, 0.0), [[0, 1], [0, 1], [0, 1]]),      # IoU alone: ids stay with the position
                                             ((1.0, 10.0, 0.0), [[0, 1], [1, 0], [1, 0]]),     # appearance: ids follow the texture
                                             ((1.0, 0.0, 10.0), [[0, 1], [1, 0], [1, 0]])],    # poses: ids follow the poses
                         ids=['iou', 'cnn-cosdist', 'pose-pck'])
def test_tracks_follow_texture_and_pose_when_their_costs_are_on(ops, cfg, tmp_path, weights, tracks):
    import copy
    from detectandtrack_amd.core import tracking_engine as te
    json_data, dets = _write_swap_video(tmp_path)
    wfile = str(tmp_path / 'resnet18_random.pth')
    torch.save(random_resnet18_state(seed=9), wfile)
    cfg.HIP.DTYPE = _h16_mode(ops)
    cfg.HIP.TRACK_CNN_WEIGHTS = wfile
    cfg.TRACKING.CNN_MATCHING_LAYER = 'layer1'
    cfg.TRACKING.DISTANCE_METRIC_WTS = weights
    if weights[1]:
        from detectandtrack_amd.core.track_features import TrackFeatureExtractor
        C = TrackFeatureExtractor().cost(json_data[0]['image'], dets['all_boxes'][1][0], json_data[1]['image'], dets['all_boxes'][1][1])
        print('appearance cost frame 0 -> 1:\n%r' % (C,))
        assert C[0, 1] < 0.01 and C[1, 0] < 0.01, 'the same crop content must be at distance ~ 0'
    first = te.compute_matches_tracks(json_data, copy.deepcopy(dets))['all_tracks'][1]
    second = te.compute_matches_tracks(json_data, copy.deepcopy(dets))['all_tracks'][1]
    assert first == second, 'two runs gave different tracks'
    assert [[int(t) for t in fr] for fr in first] == tracks
