"""Appearance features of the tracker's `cnn-cosdist` cost on the device.

The reference (lib/core/tracking_engine.py:132-155, lib/utils/pytorch_cnn_features.py) crops every box out of the frame, resizes the crop to
224 x 224, runs an ImageNet ResNet-18 up to TRACKING.CNN_MATCHING_LAYER one crop at a time -- every frame twice, once as "previous" and
once as "current" -- and takes scipy's cosine distances of the flattened features.  Here a frame is uploaded once, ONE launch cuts and
normalises all its boxes (dat_crop_resize_patches), ONE forward of the project's own 2D ResNet-18 body embeds them with N = boxes, the
features stay on the device (cached per frame, so a frame is embedded once), and dat_cosine_cost compares two frames' features.  The
Hungarian solve that consumes the matrix stays on the host.
"""
import collections
import copy

import numpy as np
import torch

from detectandtrack_amd.core import config as config_mod
from detectandtrack_amd.core.config import cfg
from detectandtrack_amd.ops import hip_ops as ops
from detectandtrack_amd.utils import image as image_utils
from detectandtrack_amd.utils import net as net_utils

# CNN_MATCHING_LAYER -> (output blob of the stage's last block, stages the body needs)
_LAYERS = {'layer1': ('res2_1_sum', 3), 'layer2': ('res3_1_sum', 3), 'layer3': ('res4_1_sum', 3), 'layer4': ('res5_1_sum', 4)}
PATCH_SIZE = 224


def _build_trunk(stages):
    """The body graph under the DEFAULT configuration (the global cfg is saved and put back): the trunk is torchvision's ResNet-18
    whatever MODEL.USE_BN / HIP.USE_GN / MODEL.DILATION / RESNETS.NUM_GROUPS / VIDEO.TIME_KERNEL_DIM the detector was built with."""
    from detectandtrack_amd.modeling import ResNet3D
    from detectandtrack_amd.modeling.detector import DetectionModelHelper
    saved = copy.deepcopy(dict(cfg))
    config_mod.reset_cfg()
    try:
        model = DetectionModelHelper(name='track_cnn', train=False, num_classes=2)
        body = ResNet3D.add_ResNet18_conv5_body if stages == 4 else ResNet3D.add_ResNet18_conv4_body
        body(model)
    finally:
        for k in list(cfg.keys()):
            del cfg[k]
        for k, v in saved.items():
            cfg[k] = v
    return model


class TrackFeatureExtractor(object):
    """ResNet-18 features of the boxes of a frame, and the cosine cost of two frames' boxes."""

    def __init__(self, weights=None, layer=None, state=None, device=None, cache_frames=2):
        from detectandtrack_amd.workspace import Workspace
        layer = cfg.TRACKING.CNN_MATCHING_LAYER if layer is None else layer
        if layer not in _LAYERS:
            raise ValueError('TRACKING.CNN_MATCHING_LAYER %r: supported are layer1, layer2, layer3 and layer4' % (layer,))
        self.layer = layer
        self.blob, stages = _LAYERS[layer]
        if state is None:
            path = cfg.HIP.TRACK_CNN_WEIGHTS if weights is None else weights
            if not path:
                raise ValueError('the cnn-cosdist cost needs ResNet-18 weights: set HIP.TRACK_CNN_WEIGHTS to a torchvision resnet18 '
                                 'state_dict (torch.save) or a pickle of name -> ndarray')
            state = net_utils.load_resnet18_state(path)
        blobs = net_utils.resnet18_state_to_blobs(state, stages)
        model = _build_trunk(stages)
        last = max(i for i, op in enumerate(model.net.ops) if self.blob in op.outputs)
        model.net.ops = model.net.ops[:last + 1]        # (layer1 / layer2: the stages behind the matching layer never run)
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.ws = Workspace(self.device, dtype=cfg.HIP.DTYPE)     # an inference path: 'bf16x3' is allowed
        for name in model.params:
            self.ws.set_param(name, blobs[name])
        self.ws.CreateNet(model.net)
        self.net_name = model.net.name
        self.cache_frames = int(cache_frames)
        self._cache = collections.OrderedDict()         # (frame path, boxes) -> (features [n, ld] on the device, D, dtype tag)

    # ---- one frame ---------------------------------------------------------------------------------------------------------------
    def patches(self, frame, boxes):
        """frame: (h, w, 3) uint8 BGR -> the `data` blob fp32 [n, 3, 1, 224, 224] on the device (upload + one crop launch)."""
        frame = np.asarray(frame)
        assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3, (frame.dtype, frame.shape)
        ranges = image_utils.crop_ranges(np.asarray(boxes)[:, :4], frame.shape[0], frame.shape[1])
        dev = torch.from_numpy(np.array(frame, dtype=np.uint8, order='C')).to(self.ws.device)
        return ops.crop_resize_patches(dev, ranges, PATCH_SIZE, image_utils.TRACK_CNN_MEAN, image_utils.TRACK_CNN_STD)

    def forward(self, data):
        """`data` [n, 3, 1, s, s] -> (features [n, ld] on the device in the working dtype, D, dtype tag): one trunk forward, N = boxes."""
        n = int(data.shape[0])
        self.ws.FeedBlob('data', data)
        self.ws.RunNet(self.net_name)
        b = self.ws.blobs[self.blob]
        assert b.kind == 'fmap' and b.t.shape[0] == n, (b.kind, tuple(b.t.shape), n)
        # the channel stride equals the channel count for every ResNet-18 stage: no (possibly unwritten) padding channels in a row
        assert int(b.t.shape[3]) == int(b.C), 'feature blob %s: %d channels at stride %d' % (self.blob, b.C, b.t.shape[3])
        feat = b.t.reshape(n, -1)
        return feat, int(feat.shape[1]), b.dt

    def embed(self, frame, boxes):
        """Features of the boxes (rows whose first four columns are x1, y1, x2, y2) of one frame; `frame` is an image path (decoded with
        read_frame and cached per (path, boxes), least recently used dropped) or a BGR uint8 array (not cached).  None for no boxes."""
        boxes = np.asarray(boxes)
        if len(boxes) == 0:
            return None
        key = None
        if isinstance(frame, str):
            key = (frame, boxes.shape, np.ascontiguousarray(boxes).tobytes())
            hit = self._cache.get(key)
            if hit is not None:
                self._cache.move_to_end(key)
                return hit
            from detectandtrack_amd.core.test_engine import read_frame
            frame = read_frame(frame)
        out = self.forward(self.patches(frame, boxes))
        if key is not None:
            self._cache[key] = out
            while len(self._cache) > self.cache_frames:
                self._cache.popitem(last=False)
        return out

    # ---- two frames ----------------------------------------------------------------------------------------------------------------
    def cost(self, prev_frame, prev_boxes, cur_frame, cur_boxes):
        """float64 ndarray [len(prev_boxes), len(cur_boxes)] of cosine distances; zeros when either set is empty (reference :152-153).  A
        feature row of norm zero is at distance 1 from everything (the reference would hand NaN to the solver)."""
        n, m = len(prev_boxes), len(cur_boxes)
        if n == 0 or m == 0:
            return np.zeros((n, m))
        fa, D, dt = self.embed(prev_frame, prev_boxes)
        fb, _, _ = self.embed(cur_frame, cur_boxes)
        return ops.cosine_cost(fa, fb, D, dt).cpu().numpy().astype(np.float64)
