"""CPU tests of the tracker's appearance and pose costs: the pose distance against the reference's own code,
the 8-bit resize and the crop rule of the patch kernel's host restatement, the torchvision -> blob converter, and the tracker wiring.

`pose-pck` is pinned by tests/golden/reference_track_costs.json, which tests/golden/make_golden_track_costs.py produced by running the
REAL reference's `pck_distance` and `_compute_distance_matrix`.  `cnn-cosdist` cannot be run from the reference in this environment
(it needs torchvision, cv2 and CUDA, all absent): its pieces are pinned to their written definitions here and to float64 restatements
on the GPU (tests/test_gpu_track_costs.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.track_costs_ref import Dataset, random_resnet18_state

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('dat_crop_resize_patches', 'dat_cosine_cost', 'dat_cosine_cost_workspace_bytes')


@pytest.fixture(scope='module')
def golden_costs():
    with open(os.path.join(REPO, 'tests', 'golden', 'reference_track_costs.json')) as f:
        g = json.load(f)
    g['prev_poses'] = [np.asarray(p, dtype=np.float32) for p in g['prev_poses']]
    g['cur_poses'] = [np.asarray(p, dtype=np.float32) for p in g['cur_poses']]
    g['prev_boxes'] = np.asarray(g['prev_boxes'], dtype=np.float32)
    g['cur_boxes'] = np.asarray(g['cur_boxes'], dtype=np.float32)
    return g


@pytest.fixture
def default_cfg():
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    yield cfg
    reset_cfg()


# ---- pose-pck against the reference ------------------------------------------------------------------------------------------------------
def test_pck_distance_matrix_equals_the_reference(golden_costs):
    """Equality, not closeness: the values are 1 - k / 17, and the seeded poses hold a head of length zero and keypoints exactly at
    the threshold (strict `<`: no match)."""
    from detectandtrack_amd.utils import keypoints as kps
    g = golden_costs
    ref = np.asarray(g['pck'], dtype=np.float64)
    got = kps.pck_distance_matrix(g['prev_poses'], g['cur_poses'], g['keypoints'])
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.array_equal(got, ref), np.abs(got - ref).max()
    scalar = np.array([[kps.pck_distance(a, b, g['keypoints']) for b in g['cur_poses']] for a in g['prev_poses']])
    assert np.array_equal(scalar, ref)
    k17 = np.rint((1 - ref) * 17)
    assert np.array_equal(ref, 1.0 - k17 / 17.0)
    assert kps.compute_head_size(g['prev_poses'][0], g['keypoints']) == 1.0          # zero head length
    assert kps.compute_head_size(g['prev_poses'][1], g['keypoints']) == 6.0
    assert kps.pck_distance_matrix([], g['cur_poses'], g['keypoints']).shape == (0, len(g['cur_poses']))


def test_iou_plus_pose_cost_matches_the_reference_matrix(golden_costs, default_cfg):
    from detectandtrack_amd.core import tracking_engine as te
    g = golden_costs
    entry = {'dataset': Dataset(g['keypoints']), 'image': '/data/vid00/00000.jpg'}
    got = te._compute_distance_matrix(g['prev_boxes'], g['cur_boxes'], tuple(g['cost_types']), tuple(g['cost_weights']),
                                      prev_poses=g['prev_poses'], cur_poses=g['cur_poses'], prev_entry=entry, cur_entry=entry)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, np.asarray(g['combined'], dtype=np.float64), rtol=0, atol=1e-12)


# ---- resize_bilinear_u8 --------------------------------------------------------------------------------------------------------------------
def test_resize_u8_identity_constant_and_single_pixel():
    from detectandtrack_amd.utils.image import resize_bilinear_u8
    rs = np.random.RandomState(0)
    im = rs.randint(0, 256, (13, 17, 3)).astype(np.uint8)
    out = resize_bilinear_u8(im, 17, 13)
    assert out.dtype == np.uint8 and np.array_equal(out, im)
    for v in (0, 1, 127, 254, 255):
        const = np.full((9, 5, 3), v, dtype=np.uint8)
        for ow, oh in ((224, 224), (7, 7), (3, 20)):
            assert np.array_equal(resize_bilinear_u8(const, ow, oh), np.full((oh, ow, 3), v, dtype=np.uint8)), (v, ow, oh)
    one = np.array([[[3, 200, 255]]], dtype=np.uint8)
    assert np.array_equal(resize_bilinear_u8(one, 6, 4), np.broadcast_to(one, (4, 6, 3)))
    grey = rs.randint(0, 256, (5, 4)).astype(np.uint8)
    assert resize_bilinear_u8(grey, 8, 3).shape == (3, 8)


def test_resize_u8_hand_worked_2x2_to_4x4():
    """2 -> 4 along an axis reads source coordinates -0.25, 0.25, 0.75, 1.25.  x snaps at the borders (weights 2048 / 0), the inner
    two columns take weights (1536, 512) and (512, 1536); y keeps the weights of -0.25 = floor -1 + 0.75, i.e. (512, 1536) on the
    clamped rows (0, 0), and of 1.25 = 1 + 0.25, i.e. (1536, 512) on rows (1, 1): the border rows are copies too.
    Row 0 of [[0, 100], [200, 40]]: (0, 25, 75, 100); row 1 (200, 160, 80, 40); the blends 3:1 / 1:3 of those rows:
    (50, 58.75, 76.25, 85) -> 59 / 76 and (150, 126.25, 78.75, 55) -> 126 / 79 after (.. + 2^21) >> 22."""
    from detectandtrack_amd.utils.image import resize_bilinear_u8
    src = np.array([[0, 100], [200, 40]], dtype=np.uint8)
    want = np.array([[0, 25, 75, 100], [50, 59, 76, 85], [150, 126, 79, 55], [200, 160, 80, 40]], dtype=np.uint8)
    assert np.array_equal(resize_bilinear_u8(src, 4, 4), want)


def test_resize_u8_stays_close_to_the_float_resize():
    """A sanity check, not a pin: the same sampling positions with 11-bit weights and one final rounding.  Each rounded weight is off by
    at most 2^-12, so a blended value moves by at most 4 * 255 * 2^-12 = 0.25 grey levels before the final rounding adds its half:
    the 8-bit image differs from the rounded float32 resize by at most one grey level."""
    from detectandtrack_amd.utils.image import resize_bilinear, resize_bilinear_u8
    rs = np.random.RandomState(1)
    for (h, w), (oh, ow) in (((31, 47), (224, 224)), ((300, 260), (224, 224)), ((9, 12), (7, 7)), ((50, 20), (16, 33))):
        im = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        got = resize_bilinear_u8(im, ow, oh).astype(np.int32)
        ref = resize_bilinear(im.astype(np.float32), out_w=ow, out_h=oh)
        assert np.abs(got - ref).max() <= 0.25 + 0.5 + 1e-3, np.abs(got - ref).max()
        assert np.abs(got - np.rint(ref).astype(np.int32)).max() <= 1


# ---- crop rule -------------------------------------------------------------------------------------------------------------------------------
def test_crop_ranges_are_numpy_slices():
    from detectandtrack_amd.utils.image import crop_ranges
    rs = np.random.RandomState(2)
    frame = rs.randint(0, 256, (40, 60, 3)).astype(np.uint8)
    boxes = np.array([[5, 6, 30, 28, 0.9],             # ordinary
                      [5.9, 6.99, 30.2, 28.7, 0.9],    # fractional: truncation
                      [-4.5, -3.2, 20, 15, 0.9],       # negative start: counts from the far border (mostly an empty slice)
                      [-0.5, -0.9, 20, 15, 0.9],       # int() truncates towards zero: start 0, not -1
                      [50, 30, 75.5, 44, 0.9],         # past the border: clipped
                      [-100, -100, 500, 500, 0.9],     # everything
                      [30, 10, 30, 20, 0.9],           # x2 == x1
                      [30, 10, 12, 20, 0.9]],          # x2 < x1
                     dtype=np.float32)
    r = crop_ranges(boxes, 40, 60)
    assert r.dtype == np.int32 and r.shape == (len(boxes), 4)
    for b, (x0, x1, y0, y1) in zip(boxes, r.tolist()):
        literal = frame[int(b[1]):int(b[3]), int(b[0]):int(b[2]), :]
        mine = frame[y0:y1, x0:x1, :] if (x1 > x0 and y1 > y0) else frame[0:0, 0:0, :]
        assert literal.size == mine.size and np.array_equal(literal.reshape(-1), mine.reshape(-1)), (b, (x0, x1, y0, y1))
        assert 0 <= x0 <= 60 and 0 <= x1 <= 60 and 0 <= y0 <= 40 and 0 <= y1 <= 40
    assert r[3].tolist() == [0, 20, 0, 15] and r[2].tolist() == [56, 20, 37, 15]


def test_host_patches_follow_the_written_steps():
    from detectandtrack_amd.utils import image as iu
    rs = np.random.RandomState(3)
    frame = rs.randint(0, 256, (30, 44, 3)).astype(np.uint8)
    boxes = np.array([[4, 3, 29, 25], [10, 10, 10, 20]], dtype=np.float32)
    out = iu.crop_resize_patches(frame, iu.crop_ranges(boxes, 30, 44), 16)
    assert out.dtype == np.float32 and out.shape == (2, 3, 16, 16)
    rgb = iu.resize_bilinear_u8(frame[3:25, 4:29, ::-1], 16, 16).transpose(2, 0, 1).astype(np.float64)
    mean, std = np.array([0.485, 0.456, 0.406]).reshape(3, 1, 1), np.array([0.229, 0.224, 0.224]).reshape(3, 1, 1)
    assert np.array_equal(out[0], ((rgb / 255.0 - mean) / std).astype(np.float32))
    assert np.array_equal(out[1], np.broadcast_to(((0.0 - mean) / std).astype(np.float32), (3, 16, 16)))       # the empty crop


# ---- torchvision state_dict -> blobs -------------------------------------------------------------------------------------------------------
def test_resnet18_state_to_blobs_folds_batch_norm_in_float64():
    import torch
    import torch.nn.functional as F
    from detectandtrack_amd.utils.net import resnet18_state_to_blobs
    state = random_resnet18_state()
    state['fc.weight'], state['fc.bias'] = torch.zeros(1000, 512), torch.zeros(1000)        # a full resnet18 carries them: dropped
    blobs = resnet18_state_to_blobs(state, stages=4)
    assert 'res5_1_branch2b_w' in blobs and 'res5_0_branch1_bn_s' in blobs and 'res2_0_branch1_w' not in blobs
    assert not [k for k in resnet18_state_to_blobs(state, stages=3) if k.startswith('res5')]
    assert blobs['conv1_w'].shape == (64, 3, 1, 7, 7) and blobs['conv1_w'].dtype == np.float32
    rs = np.random.RandomState(6)
    for tv, bnp, blob, stride, pad, cin in (('conv1', 'bn1', 'conv1', 2, 3, 3), ('layer3.0.conv1', 'layer3.0.bn1', 'res4_0_branch2a', 2, 1, 128),
                                            ('layer2.0.downsample.0', 'layer2.0.downsample.1', 'res3_0_branch1', 2, 0, 64),
                                            ('layer1.1.conv2', 'layer1.1.bn2', 'res2_1_branch2b', 1, 1, 64)):
        x = torch.from_numpy(rs.randn(2, cin, 12, 11))
        z = F.conv2d(x, state[tv + '.weight'].double(), None, stride=stride, padding=pad)
        ref = F.batch_norm(z, state[bnp + '.running_mean'].double(), state[bnp + '.running_var'].double(), state[bnp + '.weight'].double(),
                           state[bnp + '.bias'].double(), training=False, eps=1e-5)
        aff = blob + '_bn' if blob != 'conv1' else 'res_conv1_bn'
        w = torch.from_numpy(blobs[blob + '_w'][:, :, 0]).double()
        got = F.conv2d(x, w, None, stride=stride, padding=pad) * torch.from_numpy(blobs[aff + '_s']).double().view(1, -1, 1, 1) \
            + torch.from_numpy(blobs[aff + '_b']).double().view(1, -1, 1, 1)
        # the folded pair is stored in float32: two roundings of 2^-24 on values of the size of the output
        assert float((got - ref).abs().max()) <= 4 * 2.0 ** -24 * float(ref.abs().max() + z.abs().max()), tv


def test_resnet18_state_to_blobs_names_missing_and_unknown_tensors():
    from detectandtrack_amd.utils.net import resnet18_state_to_blobs
    state = random_resnet18_state(stages=3)
    resnet18_state_to_blobs(state, stages=3)
    with pytest.raises(KeyError, match='layer4.0.conv1.weight'):
        resnet18_state_to_blobs(state, stages=4)
    broken = dict(state)
    del broken['layer2.0.bn1.running_var']
    with pytest.raises(KeyError, match='layer2.0.bn1.running_var'):
        resnet18_state_to_blobs(broken, stages=3)
    extra = dict(state)
    extra['layer1.0.conv3.weight'] = state['conv1.weight']
    with pytest.raises(KeyError, match='layer1.0.conv3.weight'):
        resnet18_state_to_blobs(extra, stages=3)


def test_weight_file_formats(tmp_path):
    import pickle
    import torch
    from detectandtrack_amd.utils.net import load_resnet18_state, resnet18_state_to_blobs
    state = random_resnet18_state(stages=3)
    p1, p2 = str(tmp_path / 'r18.pth'), str(tmp_path / 'r18.pkl')
    torch.save(state, p1)
    with open(p2, 'wb') as f:
        pickle.dump({k: v.numpy() for k, v in state.items()}, f)
    a = resnet18_state_to_blobs(load_resnet18_state(p1), 3)
    b = resnet18_state_to_blobs(load_resnet18_state(p2), 3)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


# ---- tracker wiring ----------------------------------------------------------------------------------------------------------------------------
class _FakeFeatures(object):
    def __init__(self, C):
        self.C, self.calls = C, []

    def cost(self, prev_frame, prev_boxes, cur_frame, cur_boxes):
        self.calls.append((prev_frame, cur_frame, len(prev_boxes), len(cur_boxes)))
        return self.C


def _wiring_case(golden_costs):
    g = golden_costs
    entry_a = {'dataset': Dataset(g['keypoints']), 'image': ['/v/0.jpg', '/v/1.jpg', '/v/2.jpg']}     # a clip: named by its centre frame
    entry_b = {'dataset': Dataset(g['keypoints']), 'image': '/v/2.jpg'}
    return g, entry_a, entry_b


def test_costs_are_weighted_and_summed_in_order_in_float64(golden_costs, default_cfg):
    from detectandtrack_amd.core import tracking_engine as te
    from detectandtrack_amd.utils import keypoints as kps
    g, ea, eb = _wiring_case(golden_costs)
    rs = np.random.RandomState(8)
    Cf = rs.uniform(0, 1, (len(g['prev_boxes']), len(g['cur_boxes']))).astype(np.float32)
    fake = _FakeFeatures(Cf)
    types, wts = ('bbox-overlap', 'cnn-cosdist', 'pose-pck'), (1.0, 0.3, 0.7)
    kw = dict(prev_poses=g['prev_poses'], cur_poses=g['cur_poses'], prev_entry=ea, cur_entry=eb)
    got = te._compute_distance_matrix(g['prev_boxes'], g['cur_boxes'], types, wts, features=fake, **kw)
    parts = [(1 - te._compute_pairwise_iou(g['prev_boxes'], g['cur_boxes'])) * 1.0, Cf.astype(np.float64) * 0.3,
             kps.pck_distance_matrix(g['prev_poses'], g['cur_poses'], g['keypoints']) * 0.7]
    assert got.dtype == np.float64 and np.array_equal(got, np.sum(np.stack(parts, axis=0), axis=0))
    assert fake.calls == [('/v/1.jpg', '/v/2.jpg', len(g['prev_boxes']), len(g['cur_boxes']))]
    # a factory instead of an extractor is called on first use
    made = []
    te._compute_distance_matrix(g['prev_boxes'], g['cur_boxes'], types, wts, features=lambda: made.append(1) or fake, **kw)
    assert made == [1]
    m = te._compute_matches(g['prev_boxes'], g['cur_boxes'], types, wts, 'hungarian', features=fake, **kw)
    assert m.shape == (len(g['cur_boxes']),)
    assert np.array_equal(te._compute_matches(None, None, None, None, 'hungarian', C=got), m)


def test_a_zero_weight_touches_nothing(golden_costs, default_cfg):
    from detectandtrack_amd.core import tracking_engine as te
    g, ea, eb = _wiring_case(golden_costs)

    def boom():
        raise AssertionError('the extractor was constructed for a weight of 0')
    types = ('bbox-overlap', 'cnn-cosdist', 'pose-pck')
    got = te._compute_distance_matrix(g['prev_boxes'], g['cur_boxes'], types, (1.0, 0.0, 0.0), features=boom)
    assert np.array_equal(got, 1 - te._compute_pairwise_iou(g['prev_boxes'], g['cur_boxes']))
    # the whole tracker on the default weights: no poses, files or device needed, as before
    json_data, dets = te.synthetic_detections(2, 5, 4, seed=1)
    del dets['all_keyps']
    out = te.compute_matches_tracks(json_data, dets)
    assert len(out['all_tracks'][1]) == len(json_data)


def test_cnn_cosdist_without_weights_names_the_config_key(default_cfg):
    from detectandtrack_amd.core import tracking_engine as te
    cfg = default_cfg
    cfg.TRACKING.DISTANCE_METRIC_WTS = (1.0, 0.5, 0.0)
    assert cfg.HIP.TRACK_CNN_WEIGHTS == ''
    json_data, dets = te.synthetic_detections(1, 3, 3, seed=1)
    with pytest.raises(ValueError, match='HIP.TRACK_CNN_WEIGHTS'):
        te.compute_matches_tracks(json_data, dets)


def test_unknown_matching_layer_names_the_supported_ones(default_cfg):
    from detectandtrack_amd.core.track_features import TrackFeatureExtractor
    with pytest.raises(ValueError, match='layer1, layer2, layer3 and layer4'):
        TrackFeatureExtractor(state={}, layer='avgpool')


@pytest.mark.parametrize('kind', ['cnn-cosdist', 'pose-pck'])
def test_tube_rows_are_refused_for_the_box_indexed_costs(golden_costs, default_cfg, kind):
    from detectandtrack_amd.core import tracking_engine as te
    g, ea, eb = _wiring_case(golden_costs)
    tubes = np.hstack([g['prev_boxes'][:, :4]] * 3 + [g['prev_boxes'][:, 4:]])
    with pytest.raises(ValueError, match='TRACKING.KEEP_CENTER_DETS_ONLY'):
        te._compute_distance_matrix(tubes, tubes, ('bbox-overlap', kind), (1.0, 1.0), prev_poses=g['prev_poses'], cur_poses=g['prev_poses'],
                                    prev_entry=ea, cur_entry=eb, features=_FakeFeatures(None))
    with pytest.raises(NotImplementedError):
        te._compute_distance_matrix(tubes, tubes, ('bbox-overlap', 'lstm'), (1.0, 1.0))


def test_trunk_graph_ignores_the_detector_configuration(default_cfg):
    """The appearance trunk is torchvision's ResNet-18 whatever the detector was configured with, and the configuration is put back."""
    from detectandtrack_amd.core import track_features as tf
    cfg = default_cfg
    cfg.MODEL.USE_BN = True
    cfg.MODEL.DILATION = 2
    cfg.RESNETS.NUM_GROUPS = 32
    cfg.VIDEO.TIME_KERNEL_DIM.BODY = 3
    plain = [repr(op) + repr(sorted(op.args.items())) for op in tf._build_trunk(4).net.ops]
    assert cfg.MODEL.USE_BN is True and cfg.MODEL.DILATION == 2 and cfg.RESNETS.NUM_GROUPS == 32 and cfg.VIDEO.TIME_KERNEL_DIM.BODY == 3
    from detectandtrack_amd.core.config import reset_cfg
    reset_cfg()
    assert plain == [repr(op) + repr(sorted(op.args.items())) for op in tf._build_trunk(4).net.ops]
    assert all(op.args['kernels'][0] == 1 and 'group' not in op.args and 'dilation' not in op.args and not op.args.get('rm')
               for op in tf._build_trunk(4).net.ops if op.type == 'Conv')


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lib', ['libdat_hip.so', 'libdat_hip_f16.so'])
def test_both_library_flavours_export_the_track_cost_entry_points(lib):
    h = ctypes.CDLL(os.path.join(REPO, 'detectandtrack_amd', lib))
    for name in NEW_SYMBOLS:
        assert hasattr(h, name), '%s does not export %s' % (lib, name)
    from detectandtrack_amd import libdat
    assert set(NEW_SYMBOLS) <= set(libdat.EXPORTS)
    f = h.dat_cosine_cost_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
    assert f(0, 4, 64) == 0 and f(1025, 4, 64) == 0 and f(3, 5, 0) == 0
    assert f(3, 5, 200) == 4 * (3 * 5 + 3 + 5)                      # one chunk
    assert 0 < f(1024, 1024, 200704) <= (40 << 20)                  # the slabs of the largest case stay bounded
