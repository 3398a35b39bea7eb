"""Keypoint utilities — mirror of reference lib/utils/keypoints.py (heatmap decoding :94-149, :210-216)."""
import numpy as np

from detectandtrack_amd.core.config import cfg
import detectandtrack_amd.utils.image as image_utils


def get_keypoints():
    """COCO person keypoints and the left/right flip map (reference :23-60)."""
    names = ['nose', 'left_eye', 'right_eye', 'left_ear', 'right_ear', 'left_shoulder', 'right_shoulder',
             'left_elbow', 'right_elbow', 'left_wrist', 'right_wrist', 'left_hip', 'right_hip', 'left_knee',
             'right_knee', 'left_ankle', 'right_ankle']
    flip = {n: n.replace('left', 'right') for n in names if n.startswith('left')}
    return names, flip


def get_person_class_index():
    return 1


def scores_to_probs(scores):
    """Spatial softmax per channel of a CxHxW score map (:210-216)."""
    for c in range(scores.shape[0]):
        t = scores[c]
        e = np.exp(t - t.max())
        scores[c] = e / np.sum(e)
    return scores


def heatmaps_to_keypoints(maps, rois):
    """(#rois, K, M, M) heatmaps + (#rois, 4) boxes -> (#rois, 4, K) rows (x, y, logit, prob) (:94-149): each map
    is bicubically resized to the RoI's (ceil) size, the argmax cell centre is mapped back to image coordinates."""
    off_x, off_y = rois[:, 0], rois[:, 1]
    widths = np.maximum(rois[:, 2] - rois[:, 0], 1)
    heights = np.maximum(rois[:, 3] - rois[:, 1], 1)
    wc, hc = np.ceil(widths), np.ceil(heights)
    maps = np.transpose(maps, [0, 2, 3, 1])
    min_size = cfg.KRCNN.INFERENCE_MIN_SIZE
    K = cfg.KRCNN.NUM_KEYPOINTS
    xy = np.zeros((len(rois), 4, K), dtype=np.float32)
    for i in range(len(rois)):
        mw = int(np.maximum(wc[i], min_size)) if min_size > 0 else int(wc[i])
        mh = int(np.maximum(hc[i], min_size)) if min_size > 0 else int(hc[i])
        w_corr, h_corr = widths[i] / mw, heights[i] / mh
        roi_map = np.transpose(image_utils.resize_bicubic(maps[i], mw, mh), [2, 0, 1])
        probs = scores_to_probs(roi_map.copy())
        w = roi_map.shape[2]
        for k in range(K):
            pos = roi_map[k].argmax()
            x_int = pos % w
            y_int = (pos - x_int) // w
            xy[i, 0, k] = (x_int + 0.5) * w_corr + off_x[i]
            xy[i, 1, k] = (y_int + 0.5) * h_corr + off_y[i]
            xy[i, 2, k] = roi_map[k, y_int, x_int]
            xy[i, 3, k] = probs[k, y_int, x_int]
    return xy


# ---- greedy NMS of poses on object keypoint similarity, KRCNN.NMS_OKS (reference :221-263) ----------------------
OKS_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


def compute_oks(src_keypoints, src_roi, dst_keypoints, dst_roi):
    """OKS of N poses against one (:240-263).  src_keypoints 4 x K, src_roi (4,), dst_keypoints N x 4 x K, dst_roi N x 4 (never read, as in
    the reference: the area is the SOURCE box's, with the + 1 convention).  float32 inputs: differences, squares and the area in float32,
    the division chain and the exponentials in float64, as NumPy evaluates the reference's statements.  float64 [N]."""
    src_keypoints, dst_keypoints = np.asarray(src_keypoints, dtype=np.float32), np.asarray(dst_keypoints, dtype=np.float32)
    src_roi = np.asarray(src_roi, dtype=np.float32)
    vars = (OKS_SIGMAS * 2) ** 2
    src_area = (src_roi[2] - src_roi[0] + np.float32(1)) * (src_roi[3] - src_roi[1] + np.float32(1))
    dx = dst_keypoints[:, 0, :] - src_keypoints[0, :]
    dy = dst_keypoints[:, 1, :] - src_keypoints[1, :]
    e = (dx * dx + dy * dy).astype(np.float64) / vars / (np.float64(src_area) + np.spacing(1)) / 2
    return np.sum(np.exp(-e), axis=1) / e.shape[1]


def compute_oks_tubes(src_keypoints, src_roi, dst_keypoints, dst_roi):
    """The tube form (cfg.HIP.TUBE_NMS_OKS; the reference defines none): src_keypoints 4 x (K T), src_roi (4 T,), dst_keypoints
    N x 4 x (K T), dst_roi N x 4T -> the T per-frame compute_oks values, each with frame t's box of the source as the area, summed in
    float64 in frame order from 0 and divided by T.  At T = 1 it is compute_oks bit for bit (0 + x and x / 1 are exact)."""
    src_keypoints, dst_keypoints = np.asarray(src_keypoints), np.asarray(dst_keypoints)
    src_roi, dst_roi = np.asarray(src_roi), np.asarray(dst_roi)
    T = src_roi.shape[-1] // 4
    K = src_keypoints.shape[-1] // T
    total = np.zeros(dst_keypoints.shape[0], dtype=np.float64)
    for t in range(T):
        total = total + compute_oks(src_keypoints[:, t * K:(t + 1) * K], src_roi[4 * t:4 * t + 4],
                                    dst_keypoints[:, :, t * K:(t + 1) * K], dst_roi[:, 4 * t:4 * t + 4])
    return total / T


def nms_oks(kp_predictions, rois, thresh):
    """Greedy NMS on OKS (:221-237): kp_predictions N x 4 x (K T), rois N x 4T -> the kept rows in visiting order.  The score is the mean
    logit; rows are visited in descending score order and a visited row removes every later row whose OKS with it is not <= thresh.
    Score ties: the reference's argsort()[::-1] leaves them undefined; here the sort is stable, so among equal scores the LATER row
    comes first (a definition).  Rows of more than 4 box columns are tubes (compute_oks_tubes; the callers gate them)."""
    kp_predictions, rois = np.asarray(kp_predictions), np.asarray(rois)
    oks = compute_oks if rois.shape[-1] == 4 else compute_oks_tubes
    scores = np.mean(kp_predictions[:, 2, :], axis=1)
    order = np.argsort(scores, kind='stable')[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(i)
        ovr = oks(kp_predictions[i], rois[i], kp_predictions[order[1:]], rois[order[1:]])
        inds = np.where(ovr <= thresh)[0]
        order = order[inds + 1]
    return keep


def check_nms_oks_config():
    """What KRCNN.NMS_OKS needs of a config, host and device path alike: re-indexing cls_boxes[person] by the poses' keep list
    (lib/core/test.py:886-890) is only right when person is the one foreground class, and the sigma table has 17 entries."""
    if cfg.MODEL.NUM_CLASSES != 2:
        raise ValueError('KRCNN.NMS_OKS re-indexes the person boxes by the kept poses: MODEL.NUM_CLASSES must be 2, not %d' % cfg.MODEL.NUM_CLASSES)
    if cfg.KRCNN.NUM_KEYPOINTS != 17:
        raise ValueError('KRCNN.NMS_OKS uses the 17 COCO keypoint sigmas: KRCNN.NUM_KEYPOINTS must be 17, not %d' % cfg.KRCNN.NUM_KEYPOINTS)


# ---- pose distance of the tracker,TRACKING.DISTANCE_METRICS 'pose-pck' (reference :266-291) ------------------------------------
def compute_head_size(kps, kpt_names):
    """|head_top - head_bottom| + 1 of a 3 x K / 4 x K pose (:266-274; the + 1 keeps a degenerate head from dividing by zero)."""
    kps = np.asarray(kps, dtype=np.float64)
    top = kps[:2, kpt_names.index('head_top')]
    bottom = kps[:2, kpt_names.index('head_bottom')]
    return np.linalg.norm(top - bottom) + 1


def pck_distance(kps_a, kps_b, kpt_names, dist_thresh=0.5):
    """1 - PCK of two poses (:277-291): a keypoint matches when its distance, divided by the head size of `kps_a`, is strictly below
    `dist_thresh`; every keypoint counts, labelled or not.  float64."""
    a, b = np.asarray(kps_a, dtype=np.float64), np.asarray(kps_b, dtype=np.float64)
    normed = np.linalg.norm(a[:2] - b[:2], axis=0) / compute_head_size(a, kpt_names)
    match = normed < dist_thresh
    return 1.0 - np.sum(match) / match.size


def pck_distance_matrix(poses_a, poses_b, kpt_names, dist_thresh=0.5):
    """C[i, j] = pck_distance(poses_a[i], poses_b[j]) for two lists of poses, vectorised (tracking_engine.py:114-129): the head size is
    that of the ROW pose (the previous frame's).  float64 [len(a), len(b)]; zeros((n, m)) when either list is empty."""
    n, m = len(poses_a), len(poses_b)
    if n == 0 or m == 0:
        return np.zeros((n, m))
    a = np.stack([np.asarray(p, dtype=np.float64)[:2] for p in poses_a])          # (n, 2, K)
    b = np.stack([np.asarray(p, dtype=np.float64)[:2] for p in poses_b])          # (m, 2, K)
    d = a[:, None] - b[None]                                                      # (n, m, 2, K)
    # np.linalg.norm over an axis is sqrt(sum(|x|^2)): the same two squares, one sum and one root per keypoint as the scalar function
    dist = np.sqrt(np.sum(d * d, axis=2))
    head = a[:, :, kpt_names.index('head_top')] - a[:, :, kpt_names.index('head_bottom')]
    head = np.sqrt(np.sum(head * head, axis=1)) + 1
    match = dist / head[:, None, None] < dist_thresh
    return 1.0 - np.sum(match, axis=2) / float(match.shape[2])
