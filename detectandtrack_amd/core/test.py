"""Inference driver — mirror of reference lib/core/test.py (single-scale path; TTA variants are
COMPETITION_MODE-only and out of the hot-path scope).

Call order and blob names are the reference's (:158-252 im_detect_bbox, :584-627 im_detect_keypoints, :750-806
box_results_with_nms_and_limit, :865-894 keypoint_results, :897-957 im_detect_all): feed `data`/`im_info`, run
`model.net`, fetch `rois`/`cls_prob`/`bbox_pred`; per-class NMS + top-100 on the host glue (NMS itself on the
device through core.nms_wrapper); feed `keypoint_rois`, run `model.keypoint_net`, fetch `kps_score`.
"""
from collections import defaultdict

import numpy as np

from detectandtrack_amd.core.config import cfg
from detectandtrack_amd.core.nms_wrapper import nms, soft_nms
from detectandtrack_amd.ops.hip_ops import SOFT_NMS_MAX_BOXES      # the device Soft-NMS keeps a class's rows in LDS
from detectandtrack_amd.ops.hip_ops import OKS_NMS_MAX_ROWS        # the device OKS-NMS keeps an image's keys, order and flags in LDS
from detectandtrack_amd.utils.timer import Timer
from detectandtrack_amd import workspace
import detectandtrack_amd.utils.blob as blob_utils
import detectandtrack_amd.utils.boxes as box_utils
import detectandtrack_amd.utils.keypoints as keypoint_utils


def _get_image_blob(im, num_frames=None):
    """im: list of BGR frames (len 1 for images) -> (data blob, scale factors) (:43-75); num_frames: frames per clip of the
    blob when it is not cfg.VIDEO.NUM_FRAMES (the new frames of a sliding-window clip, im_detect_bbox)."""
    per_frame, scales = [], []
    for frame in im:
        ims, sc = blob_utils.prep_im_for_blob(frame, cfg.PIXEL_MEANS, cfg.TEST.SCALES, cfg.TEST.MAX_SIZE)
        per_frame.append(ims)
        scales.append(sc)
    for s in scales:
        assert scales[0] == s
    processed = [frames[i] for i in range(len(per_frame[0])) for frames in per_frame]
    return blob_utils.im_list_to_blob(processed, num_frames), np.array(scales[0])


def _project_im_rois(im_rois, scales):
    """(:95-123) single scale: every roi at pyramid level 0."""
    im_rois = im_rois.astype(np.float64, copy=False)
    if len(scales) > 1:
        w = im_rois[:, 2] - im_rois[:, 0] + 1
        h = im_rois[:, 3] - im_rois[:, 1] + 1
        areas = (w * h)[:, np.newaxis] * (scales[np.newaxis, :] ** 2)
        levels = np.abs(areas - 224 * 224).argmin(axis=1)[:, np.newaxis]
    else:
        levels = np.zeros((im_rois.shape[0], 1), dtype=np.int64)
    return im_rois * scales[levels], levels


def _get_rois_blob(im_rois, im_scale_factors):
    """R x (4T) boxes in image coordinates -> R x (4T+1) [level, boxes * scale] fp32 (:78-92)."""
    rois, levels = _project_im_rois(im_rois, im_scale_factors)
    return np.hstack((levels, rois)).astype(np.float32, copy=False)


def _get_blobs(im, rois, num_frames=None):
    """(:146-157)"""
    blobs = {}
    blobs['data'], im_scale_factors = _get_image_blob(im, num_frames)
    if cfg.MODEL.FASTER_RCNN and rois is None:
        blobs['im_info'] = np.array([[blobs['data'].shape[-2], blobs['data'].shape[-1], im_scale_factors[0]]],
                                    dtype=np.float32)
    if rois is not None:
        blobs['rois'] = _get_rois_blob(rois, im_scale_factors)
    return blobs, im_scale_factors


def im_detect_bbox(model, im, boxes=None, frame_ids=None, fetch=True):
    """(:158-252) returns scores (R x K), pred_boxes (R x 4TK), im_scales.

    frame_ids (one hashable id per frame of the clip, e.g. (video, frame index)) with cfg.HIP.FRAME_TRUNK_CACHE > 0: only the
    frames whose per-frame trunk output (conv1 / pool1 / res2) is not cached are pre-processed, uploaded and run through
    the trunk; consecutive clips of a sliding window share T-1 of T frames.  Results are identical to the plain path."""
    ws = workspace.GlobalWorkspace()
    if frame_ids is not None and cfg.HIP.FRAME_TRUNK_CACHE > 0 and boxes is None and cfg.MODEL.VIDEO_ON:
        assert len(frame_ids) == len(im), (len(frame_ids), len(im))
        new_ids = ws.trunk_missing(frame_ids)
        first = {}
        for j, fid in enumerate(frame_ids):
            first.setdefault(fid, j)
        # (a clip with nothing new still needs one pre-processed frame for the blob geometry)
        sub = [im[first[fid]] for fid in (new_ids or list(frame_ids)[:1])]
        inputs, im_scales = _get_blobs(sub, None, num_frames=len(sub))
        if not new_ids:
            inputs.pop('data')
        for k, v in inputs.items():
            workspace.FeedBlob(k, v)
        ws.trunk_request = (list(frame_ids), new_ids)
        workspace.RunNet(model.net.Proto().name)
        return _read_bbox_outputs(im, im_scales) if fetch else im_scales
    inputs, im_scales = _get_blobs(im, boxes)
    for k, v in inputs.items():
        workspace.FeedBlob(k, v)
    workspace.RunNet(model.net.Proto().name)
    return _read_bbox_outputs(im, im_scales) if fetch else im_scales    # fetch=False: nothing read back (device post-processing)


def _read_bbox_outputs(im, im_scales, image=None):
    """image: with several images per forward, the index of the ONE image whose rows are read (rois col 0 == image)."""
    assert cfg.MODEL.FASTER_RCNN and len(im_scales) == 1, 'Only single-image / single-scale batch implemented'
    rois = workspace.FetchBlob('rois')
    sel = slice(None) if image is None else np.where(rois[:, 0] == image)[0]
    rois = rois[sel]
    # float32 / float32(scale): what the reference environment's NumPy 1.14 value-based casting computes (NumPy 2 would promote)
    boxes = rois[:, 1:] / np.float32(im_scales[0])
    scores = workspace.FetchBlob('cls_prob')
    scores = scores.reshape([-1, scores.shape[-1]])[sel]
    time_dim = boxes.shape[-1] // 4
    if cfg.TEST.BBOX_REG:
        box_deltas = workspace.FetchBlob('bbox_pred')
        box_deltas = box_deltas.reshape([-1, box_deltas.shape[-1]])[sel]
        if cfg.MODEL.CLS_AGNOSTIC_BBOX_REG:
            box_deltas = box_deltas[:, -4 * time_dim:]
        pred_boxes = box_utils.bbox_transform(boxes, box_deltas, cfg.MODEL.BBOX_REG_WEIGHTS)
        pred_boxes = box_utils.clip_tiled_boxes(pred_boxes, im[0].shape)
        if cfg.MODEL.CLS_AGNOSTIC_BBOX_REG:
            pred_boxes = np.tile(pred_boxes, (1, scores.shape[1]))
    else:
        pred_boxes = np.tile(boxes, (1, scores.shape[1]))
    return scores, pred_boxes, im_scales


def box_results_with_nms_and_limit(scores, boxes):
    """Score threshold, per-class NMS, keep the DETECTIONS_PER_IM best over all classes (:750-806)."""
    num_classes = cfg.MODEL.NUM_CLASSES
    time_dim = boxes.shape[-1] // (num_classes * 4)
    cls_boxes = [[] for _ in range(num_classes)]
    for j in range(1, num_classes):
        inds = np.where(scores[:, j] > cfg.TEST.SCORE_THRESH)[0]
        dets_j = np.hstack((boxes[inds, j * 4 * time_dim:(j + 1) * 4 * time_dim],
                            scores[inds, j][:, np.newaxis])).astype(np.float32, copy=False)
        if cfg.TEST.SOFT_NMS.ENABLED:    # (:766-772; for time_dim > 1 only with cfg.HIP.TUBE_SOFT_NMS, as voting of all 4T columns)
            nms_dets, _ = soft_nms(dets_j, sigma=cfg.TEST.SOFT_NMS.SIGMA, overlap_thresh=cfg.TEST.NMS, score_thresh=0.0001,
                                   method=cfg.TEST.SOFT_NMS.METHOD)
        else:
            keep = nms(dets_j, cfg.TEST.NMS)
            nms_dets = dets_j[keep, :]
        if cfg.TEST.BBOX_VOTE.ENABLED:   # refine the post-NMS boxes using bounding-box voting (:776-779)
            nms_dets = box_utils.box_voting(nms_dets, dets_j, cfg.TEST.BBOX_VOTE.VOTE_TH)
        cls_boxes[j] = nms_dets
    if cfg.TEST.DETECTIONS_PER_IM > 0:
        image_scores = np.hstack([cls_boxes[j][:, -1] for j in range(1, num_classes)])
        if len(image_scores) > cfg.TEST.DETECTIONS_PER_IM:
            thresh = np.sort(image_scores)[-cfg.TEST.DETECTIONS_PER_IM]
            for j in range(1, num_classes):
                cls_boxes[j] = cls_boxes[j][np.where(cls_boxes[j][:, -1] >= thresh)[0], :]
    im_results = np.vstack([cls_boxes[j] for j in range(1, num_classes)])
    return im_results[:, -1], im_results[:, :-1], cls_boxes


def im_detect_keypoints(model, im_scales, boxes):
    """(:584-627) returns R x (17 T) x M x M heatmap logits."""
    assert len(im_scales) == 1, 'Only single-image / single-scale batch implemented'
    time_dim = boxes.shape[-1] // 4
    M = cfg.KRCNN.HEATMAP_SIZE
    if boxes.shape[0] == 0:
        return np.zeros((0, time_dim * cfg.KRCNN.NUM_KEYPOINTS, M, M), np.float32)
    workspace.FeedBlob('keypoint_rois', _get_rois_blob(boxes, im_scales))
    workspace.RunNet(model.keypoint_net.Proto().name)
    heat = workspace.FetchBlob('kps_score')
    if heat.ndim == 3:
        heat = np.expand_dims(heat, axis=0)
    return heat


def keypoint_results_on_device(model, cls_boxes, ref_boxes, im_scales, image=0):
    """im_detect_keypoints (:584-627) + keypoint_results (:865-894) without the heatmaps ever leaving the GPU
    (SURVEY.md §8 f-2): run the keypoint net on `ref_boxes`, decode `kps_score` with dat_heatmaps_to_keypoints and
    fetch only the R x 4 x (17 T) rows.  Same return value as keypoint_results.  image: the batch index of the image the boxes
    belong to (several images per forward)."""
    from detectandtrack_amd.ops import hip_ops as ops
    import torch
    num_classes = cfg.MODEL.NUM_CLASSES
    K = cfg.KRCNN.NUM_KEYPOINTS
    cls_keyps = [[] for _ in range(num_classes)]
    person = keypoint_utils.get_person_class_index()
    assert len(im_scales) == 1, 'Only single-image / single-scale batch implemented'
    time_dim = ref_boxes.shape[-1] // 4
    kp_rois = _get_rois_blob(ref_boxes, im_scales)
    kp_rois[:, 0] = image                               # (column 0 = the image's index in the batch: what RoIAlign reads)
    workspace.FeedBlob('keypoint_rois', kp_rois)
    workspace.RunNet(model.keypoint_net.Proto().name)
    ws = workspace.GlobalWorkspace()
    heat = ws.blobs['kps_score'].t                      # fp32 [R, 17 T, M, M] on the device
    assert heat.shape[1] == K * time_dim, 'Heatmaps must be 17xT'
    boxes = torch.from_numpy(np.ascontiguousarray(ref_boxes, dtype=np.float32)).to(heat.device)
    xy = ops.heatmaps_to_keypoints(heat.contiguous(), boxes, time_dim, K, cfg.KRCNN.INFERENCE_MIN_SIZE).cpu().numpy()
    if cfg.KRCNN.NMS_OKS:
        xy = _nms_oks_on_host(xy, ref_boxes, cls_boxes, person)
    cls_keyps[person] = [xy[i] for i in range(xy.shape[0])]
    return cls_keyps


def _nms_oks_on_host(xy, ref_boxes, cls_boxes, person):
    """KRCNN.NMS_OKS (:883-890, the statements behind the reference's unconditional raise): greedy NMS of the poses on their OKS; the
    keypoint rows are returned re-indexed by the keep list and cls_boxes[person] is re-indexed in place, as the reference does.  Tubes:
    the reference's NotImplementedError unless cfg.HIP.TUBE_NMS_OKS defines the overlap (utils/keypoints.compute_oks_tubes)."""
    if ref_boxes.shape[-1] // 4 > 1 and not cfg.HIP.TUBE_NMS_OKS:
        raise NotImplementedError('Handle tubes')
    keypoint_utils.check_nms_oks_config()
    keep = np.asarray(keypoint_utils.nms_oks(xy, ref_boxes, cfg.HIP.NMS_OKS_THRESH), dtype=np.int64)
    cls_boxes[person] = cls_boxes[person][keep, :]
    return xy[keep, :, :]


def _tube_detections():
    """The detections are tubes (T > 1) when a 3D body feeds 3D heads (modeling/head_builder.py)."""
    return bool(cfg.MODEL.VIDEO_ON and cfg.VIDEO.BODY_HEAD_LINK == '' and cfg.VIDEO.NUM_FRAMES_MID > 1)




def _soft_nms_capacity():
    """Rows per class the device Soft-NMS holds in LDS for this config's detections: SOFT_NMS_MAX_BOXES for boxes, and for tubes what
    their 4T coordinates leave of a workgroup's LDS (2048 up to T = 4, falling beyond)."""
    if not _tube_detections():
        return SOFT_NMS_MAX_BOXES
    from detectandtrack_amd.ops.hip_ops import soft_nms_tubes_max_boxes
    return soft_nms_tubes_max_boxes(cfg.VIDEO.NUM_FRAMES_MID)


def _device_out_cap():
    """Rows per image of the device detection buffers (enqueue_results_on_device without out_cap)."""
    D = int(cfg.TEST.DETECTIONS_PER_IM)
    return D + max(0, int(cfg.HIP.get('DET_SPARE_ROWS', 4))) if D > 0 else int(cfg.TEST.RPN_POST_NMS_TOP_N) * (cfg.MODEL.NUM_CLASSES - 1)


def _nms_oks_on_device():
    """KRCNN.NMS_OKS runs in the device post-processing (dat_oks_nms) for box detections, and for tubes with HIP.TUBE_NMS_OKS, when person
    is the only foreground class, the poses have the 17 COCO keypoints and an image's rows fit the kernel.  Anything else takes the host
    path, which raises what the config deserves (_nms_oks_on_host) or runs the host loop."""
    return bool((not _tube_detections() or cfg.HIP.TUBE_NMS_OKS) and cfg.MODEL.NUM_CLASSES == 2 and cfg.KRCNN.NUM_KEYPOINTS == 17 and
                _device_out_cap() <= OKS_NMS_MAX_ROWS)


def device_results_supported():
    """The device post-processing covers FASTER_RCNN with hard NMS, and TEST.SOFT_NMS / TEST.BBOX_VOTE (:766-779) for box detections
    and, with HIP.TUBE_SOFT_NMS, for tube detections, and KRCNN.NMS_OKS under the conditions of _nms_oks_on_device.  Without that switch tubes with either one stay on the host path, where Soft-NMS
    is the loud error the reference raises (nms_wrapper.py:34-35); so does Soft-NMS over more rois per image
    (TEST.RPN_POST_NMS_TOP_N, the capacity of the `rois` blob) than the device kernel holds for the clip's T: the host loop has no
    capacity."""
    return bool(cfg.HIP.DEVICE_BOX_RESULTS and cfg.MODEL.FASTER_RCNN and cfg.TEST.BBOX_REG and
                not ((cfg.TEST.SOFT_NMS.ENABLED or cfg.TEST.BBOX_VOTE.ENABLED) and _tube_detections() and not cfg.HIP.TUBE_SOFT_NMS) and
                not (cfg.TEST.SOFT_NMS.ENABLED and cfg.TEST.RPN_POST_NMS_TOP_N > _soft_nms_capacity()) and
                not cfg.TEST.SVM and not (cfg.KRCNN.NMS_OKS and cfg.MODEL.KEYPOINTS_ON and not _nms_oks_on_device()) and
                (cfg.HIP.DEVICE_KPS_DECODE or not cfg.MODEL.KEYPOINTS_ON))


def rerun_rows_supported(need):
    """The tie-overflow re-run of the device glue with `need` rows per image: dat_oks_nms holds at most OKS_NMS_MAX_ROWS (more: the host
    path for that image)."""
    return not (cfg.KRCNN.NMS_OKS and cfg.MODEL.KEYPOINTS_ON) or int(need) <= OKS_NMS_MAX_ROWS


def enqueue_results_on_device(model, im_shape, im_scale, out_cap=None, image=None):
    """Everything between `model.net` and the final read-back, enqueued on the current HIP stream WITHOUT a host sync:
    dat_box_results (test.py:215-252 decode + clip, :750-806 score threshold / per-class NMS or Soft-NMS / voting / DETECTIONS_PER_IM, :78-123 keypoint
    rois), then -- with MODEL.KEYPOINTS_ON -- `model.keypoint_net` on the device-resident rois and the heatmap decode
    (:584-627, :865-894).  Returns device tensors (dets [cap, 4T+2], n_out int32[2], keypoint rows [cap, 4, 17T] | None).
    With KRCNN.NMS_OKS (and keypoints) dat_oks_nms follows the decode: dets and keypoint rows are then the rows it keeps, in its
    visiting order with zero rows behind them, and a fourth value is returned, n_keep int32[n_images] -- n_out stays what
    dat_box_results wrote, since n_out[1] > n_out[0] is the tie-overflow signal of the read-back.

    Several images per forward (the `rois` blob carries one count per image): `im_shape` / `im_scale` may be per-image sequences;
    dets / keypoint rows then hold `cap` rows per image and n_out is int32[n_images, 2] (read_batch_results_from_device)."""
    from detectandtrack_amd.ops import hip_ops as ops
    ws = workspace.GlobalWorkspace()
    rois = ws.blobs['rois']
    assert rois.kind == 'rois' and rois.count is not None, 'device post-processing expects the on-device proposal blob'
    ni = int(rois.count.numel())
    prob = workspace.blob_as_matrix(ws.blobs['cls_prob'])
    pred = workspace.blob_as_matrix(ws.blobs['bbox_pred'])
    rois_t, rois_n = rois.t if rois.t.dim() == 2 else rois.t.view(-1, rois.t.shape[-1]), rois.count
    if image is not None:
        # ONE image of a forward of `ni` (the tie-overflow re-run of core/pipeline.py: only the image that overflowed pays for it): its
        # row segment of the batch blobs; `im_shape` / `im_scale` are that image's; the keypoint rois keep the image's batch index
        seg = int(rois_t.shape[0]) // ni
        lo = int(image) * seg
        rois_t, rois_n = rois_t[lo:lo + seg], rois.count.view(-1)[int(image):int(image) + 1]
        prob, pred = prob[lo:lo + seg], pred[lo:lo + seg]
        ni = 1
    cols = int(rois_t.shape[1])
    T = (cols - 1) // 4
    D = int(cfg.TEST.DETECTIONS_PER_IM)
    # rows per image: the limit rule keeps EVERY score tied with the D-th best (test.py:795-800), so D rows are not always enough --
    # frequent with bf16 logits; a few spare rows (cfg.HIP.DET_SPARE_ROWS, default 4: ties at the cut are pairs, and every spare row is a
    # row of keypoint-head work) make the overflow (host path for that image) rare.  No limit: every roi may survive in every class.
    # out_cap (optional): rows per image the caller wants -- the pipelined engine re-runs the glue with exactly as many rows as the
    # limit rule keeps when an image overflowed the default (core/pipeline.py)
    if out_cap is None:
        out_cap = _device_out_cap() if D > 0 else (int(rois_t.shape[0]) // ni) * (cfg.MODEL.NUM_CLASSES - 1)
    dets, kp_rois, n_out = ops.box_results(
        rois_t, rois_n, prob, pred, cfg.MODEL.NUM_CLASSES, T, im_scale, im_shape, cfg.MODEL.BBOX_REG_WEIGHTS,
        float(np.float32(cfg.BBOX_XFORM_CLIP)), cfg.TEST.SCORE_THRESH, cfg.TEST.NMS, D, out_cap,
        cls_agnostic=cfg.MODEL.CLS_AGNOSTIC_BBOX_REG, n_images=ni,
        # (:766-779) the reference's arguments: overlap_thresh = TEST.NMS, score_thresh = 0.0001
        soft_nms=dict(method=cfg.TEST.SOFT_NMS.METHOD, sigma=cfg.TEST.SOFT_NMS.SIGMA, score_thresh=0.0001)
        if cfg.TEST.SOFT_NMS.ENABLED else None,
        bbox_vote=cfg.TEST.BBOX_VOTE.VOTE_TH if cfg.TEST.BBOX_VOTE.ENABLED else None,
        tubes=bool(cfg.HIP.TUBE_SOFT_NMS))
    xy = None
    if cfg.MODEL.KEYPOINTS_ON:
        if image is not None:
            kp_rois[:, 0] = float(image)        # (RoIAlign reads the image's frames of the batch's feature maps)
        b = workspace.Blob(kp_rois, 'mat')
        b.count = n_out[0:1] if ni == 1 else n_out[:, 0]
        ws.blobs['keypoint_rois'] = b
        workspace.RunNet(model.keypoint_net.Proto().name)
        heat = ws.blobs['kps_score'].t                       # fp32 [cap, 17 T, M, M] on the device
        assert heat.shape[1] == cfg.KRCNN.NUM_KEYPOINTS * T, 'Heatmaps must be 17xT'
        xy = ops.heatmaps_to_keypoints(heat.contiguous(), dets, T, cfg.KRCNN.NUM_KEYPOINTS,     # (box columns of the detection rows, in place)
                                       cfg.KRCNN.INFERENCE_MIN_SIZE)
        if cfg.KRCNN.NMS_OKS:
            keypoint_utils.check_nms_oks_config()
            dets, xy, _, n_keep = ops.oks_nms(xy, dets, b.count, ni, T, cfg.KRCNN.NUM_KEYPOINTS, cfg.HIP.NMS_OKS_THRESH)
            return dets, n_out, xy, n_keep
    return dets, n_out, xy


def _split_results(d, keyps, num_classes):
    cls_boxes = [[] for _ in range(num_classes)]
    cls_keyps = [[] for _ in range(num_classes)] if keyps is not None else None
    for j in range(1, num_classes):
        sel = np.where(d[:, -1] == j)[0]
        cls_boxes[j] = d[sel, :-1]
        if keyps is not None and j == keypoint_utils.get_person_class_index():
            cls_keyps[j] = [keyps[i] for i in sel]
    return cls_boxes, cls_keyps


def read_results_from_device(dets, n_out, xy, n_keep=None):
    """The ONE device -> host transfer of a clip: (cls_boxes, cls_keyps) in the reference's layout, or None when exact score ties
    at the DETECTIONS_PER_IM cut keep more rows than the device buffers hold (the caller then takes the host path).  n_keep (KRCNN.NMS_OKS):
    the rows dat_oks_nms kept, the result's row count in place of n_out[0]."""
    n = n_out.cpu().numpy()
    assert n.ndim == 1, 'several images per forward: read_batch_results_from_device'
    if int(n[1]) > int(n[0]):
        return None
    k = int(n[0]) if n_keep is None else int(n_keep.cpu().numpy().reshape(-1)[0])
    d = dets[:k].cpu().numpy()
    keyps = xy[:k].cpu().numpy() if xy is not None else None
    return _split_results(d, keyps, cfg.MODEL.NUM_CLASSES)


def read_batch_results_from_device(dets, n_out, xy, n_keep=None):
    """Several images per forward: the list of per-image (cls_boxes, cls_keyps) -- or None for an image with the exact-tie
    overflow -- from ONE read-back of the batch (dets / keypoint rows hold `cap` rows per image)."""
    n = n_out.cpu().numpy().reshape(-1, 2)
    ni = n.shape[0]
    cap = int(dets.shape[0]) // ni
    d_all = dets.cpu().numpy()
    k_all = xy.cpu().numpy() if xy is not None else None
    kept = n_keep.cpu().numpy().reshape(-1) if n_keep is not None else n[:, 0]     # (KRCNN.NMS_OKS: the rows dat_oks_nms kept)
    out = []
    for i in range(ni):
        if int(n[i, 1]) > int(n[i, 0]):
            out.append(None)
            continue
        k = int(kept[i])
        d = d_all[i * cap:i * cap + k]
        keyps = k_all[i * cap:i * cap + k] if k_all is not None else None
        out.append(_split_results(d, keyps, cfg.MODEL.NUM_CLASSES))
    return out


def im_detect_all_batch(model, ims, timers=None):
    """Several independent images (2D models) or clips (3D models) in ONE forward: `ims` is a list of B entries, each what
    im_detect_all takes (a list of T frames).  The reference runs its inference one image per forward (lib/core/test.py:212-214,
    `assert len(im_scales) == 1`); here the batch shares every kernel launch -- the N axis of the NC[T]HW blobs -- and each image
    keeps exactly the proposals / detections / keypoints it gets alone (per-image proposal NMS and top-N, per-image detection NMS
    and limit).  Returns a list of B (cls_boxes, cls_segms, cls_keyps) tuples in input order.  All entries must pre-process to
    the same blob size (same frame size and scale), as the frames of one video do."""
    if timers is None:
        timers = defaultdict(Timer)
    assert device_results_supported() and not cfg.MODEL.MASK_ON and not cfg.TEST.COMPETITION_MODE, \
        'batched inference runs the device post-processing path (cfg.HIP.DEVICE_BOX_RESULTS)'
    B = len(ims)
    if B == 1:
        return [im_detect_all(model, ims[0], None, timers)]
    timers['im_detect_bbox'].tic()
    frames = [f for clip in ims for f in clip]
    T = len(ims[0])
    assert all(len(clip) == T for clip in ims)
    data, im_scales = _get_image_blob(frames, num_frames=T if cfg.MODEL.VIDEO_ON else None)
    assert data.shape[0] == B, (data.shape, B)
    im_info = np.tile(np.array([[data.shape[-2], data.shape[-1], im_scales[0]]], dtype=np.float32), (B, 1))
    workspace.FeedBlob('data', data)
    workspace.FeedBlob('im_info', im_info)
    workspace.RunNet(model.net.Proto().name)
    dev = enqueue_results_on_device(model, [clip[0].shape for clip in ims], [im_scales[0]] * B)
    res = read_batch_results_from_device(*dev)
    timers['im_detect_bbox'].toc()
    out = []
    for i, r in enumerate(res):
        if r is None:        # exact ties at the detection limit: this image alone through the reference's host path
            out.append(im_detect_all(model, ims[i], None, timers))
            continue
        cls_boxes, cls_keyps = r
        if cfg.MODEL.KEYPOINTS_ON and sum(len(b) for b in cls_boxes[1:]) == 0:
            cls_keyps = None
        out.append((cls_boxes, None, cls_keyps))
    return out


def keypoint_results(cls_boxes, pred_heatmaps, ref_boxes):
    """(:865-894) per-frame heatmap decoding, concatenated along the keypoint axis for tubes."""
    num_classes = cfg.MODEL.NUM_CLASSES
    K = cfg.KRCNN.NUM_KEYPOINTS
    cls_keyps = [[] for _ in range(num_classes)]
    person = keypoint_utils.get_person_class_index()
    assert pred_heatmaps.shape[1] % K == 0, 'Heatmaps must be 17xT'
    time_dim = pred_heatmaps.shape[1] // K
    assert time_dim == ref_boxes.shape[-1] // 4, 'Same T for boxes and keypoints'
    per_t = [keypoint_utils.heatmaps_to_keypoints(pred_heatmaps[:, t * K:(t + 1) * K], ref_boxes[:, t * 4:(t + 1) * 4])
             for t in range(time_dim)]
    xy = np.concatenate(per_t, axis=-1)
    if cfg.KRCNN.NMS_OKS:
        xy = _nms_oks_on_host(xy, ref_boxes, cls_boxes, person)
    cls_keyps[person] = [xy[i] for i in range(xy.shape[0])]
    return cls_keyps


def im_detect_all(model, im, box_proposals, timers=None, frame_ids=None):
    """(:897-957); frame_ids: see im_detect_bbox."""
    if timers is None:
        timers = defaultdict(Timer)
    if cfg.TEST.COMPETITION_MODE:
        raise NotImplementedError('test-time augmentation (COMPETITION_MODE) is out of the hot-path scope; the '
                                  'shipped configs set TEST.COMPETITION_MODE False')
    if device_results_supported() and box_proposals is None and not cfg.MODEL.MASK_ON:
        # the whole clip is enqueued without a host synchronisation; one read-back at the end
        timers['im_detect_bbox'].tic()
        im_scales = im_detect_bbox(model, im, None, frame_ids=frame_ids, fetch=False)
        dev = enqueue_results_on_device(model, im[0].shape, im_scales[0])
        res = read_results_from_device(*dev)
        if res is None:
            # exact score ties at the DETECTIONS_PER_IM cut beyond the spare rows: the device glue again with as many rows as the limit rule
            # keeps (n_out[1]) -- the same kernels, every tied row, no host post-processing (the pipelined engine does the same)
            need = int(dev[1].cpu().numpy().reshape(-1)[1])
            if rerun_rows_supported(need):
                res = read_results_from_device(*enqueue_results_on_device(model, im[0].shape, im_scales[0], out_cap=need))
        timers['im_detect_bbox'].toc()
        if res is not None:
            cls_boxes, cls_keyps = res
            if cfg.MODEL.KEYPOINTS_ON and sum(len(b) for b in cls_boxes[1:]) == 0:
                cls_keyps = None
            return cls_boxes, None, cls_keyps
        scores, boxes, im_scales = _read_bbox_outputs(im, im_scales)      # ties at the cut: the reference's host path
    else:
        timers['im_detect_bbox'].tic()
        scores, boxes, im_scales = im_detect_bbox(model, im, box_proposals, frame_ids=frame_ids)
        timers['im_detect_bbox'].toc()
    timers['misc_bbox'].tic()
    scores, boxes, cls_boxes = box_results_with_nms_and_limit(scores, boxes)
    timers['misc_bbox'].toc()
    if cfg.MODEL.MASK_ON and boxes.shape[0] > 0:
        raise NotImplementedError('Handle tubes..')
    cls_segms = None
    if cfg.MODEL.KEYPOINTS_ON and boxes.shape[0] > 0 and cfg.HIP.DEVICE_KPS_DECODE:
        timers['im_detect_keypoints'].tic()
        cls_keyps = keypoint_results_on_device(model, cls_boxes, boxes, im_scales)
        timers['im_detect_keypoints'].toc()
    elif cfg.MODEL.KEYPOINTS_ON and boxes.shape[0] > 0:
        timers['im_detect_keypoints'].tic()
        heatmaps = im_detect_keypoints(model, im_scales, boxes)
        timers['im_detect_keypoints'].toc()
        timers['misc_keypoints'].tic()
        cls_keyps = keypoint_results(cls_boxes, heatmaps, boxes)
        timers['misc_keypoints'].toc()
    else:
        cls_keyps = None
    return cls_boxes, cls_segms, cls_keyps
