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


# ---- pose distance of the tracker, TRACKING.DISTANCE_METRICS 'pose-pck' (reference :266-291) ------------------------------------
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
