"""Host image helpers (no OpenCV in this environment): `cv2.resize` INTER_LINEAR / INTER_CUBIC for float32 images, and
the B*T -> T-axis move of reference lib/utils/image.py:82-93.

Resampling follows OpenCV's float32 path (the reference environment pins opencv 3.4.1): destination index d reads source
coordinate f = float32((d + 0.5) * step - 0.5), step = 1 / inv_scale in double, inv_scale = the caller's fx/fy when the scale
is given (lib/utils/blob.py:86-87) or dst/src when the size is given (lib/utils/keypoints.py:129-131); the horizontal pass runs
first, then the vertical one; cubic weights are the Keys kernel with a = -0.75 and replicated borders.  Checked against the
independent restatement in oracle/resize.py (tests/test_host_cpu.py)."""
import numpy as np


def _src_coords(n_dst, inv_scale):
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * (1.0 / inv_scale) - 0.5).astype(np.float32)
    i0 = np.floor(f)
    return i0.astype(np.int64), f - i0.astype(np.float32)


def _sizes(im, out_w, out_h, fx, fy):
    h, w = im.shape[:2]
    if out_w is None:
        return int(np.rint(w * fx)), int(np.rint(h * fy)), float(fx), float(fy)      # cvRound: half to even
    return int(out_w), int(out_h), float(out_w) / w, float(out_h) / h


def resize_bilinear(im, out_w=None, out_h=None, fx=None, fy=None):
    """im (H, W[, C]) float32 -> (out_h, out_w[, C]); cv2.INTER_LINEAR.  Either the output size or the scale factors.
    One horizontal pass over every SOURCE row, then the vertical blend of the gathered rows."""
    im = np.asarray(im, dtype=np.float32)
    h, w = im.shape[:2]
    out_w, out_h, isx, isy = _sizes(im, out_w, out_h, fx, fy)
    x0, tx = _src_coords(out_w, isx)
    y0, ty = _src_coords(out_h, isy)
    # columns outside the image snap onto the border pixel (weights 1, 0); rows keep their weights and clamp the indices
    tx = np.where((x0 < 0) | (x0 >= w - 1), np.float32(0), tx).astype(np.float32)
    x0 = np.clip(x0, 0, w - 1)
    x1 = np.minimum(x0 + 1, w - 1)
    y1 = np.clip(y0 + 1, 0, h - 1)
    y0 = np.clip(y0, 0, h - 1)
    tail = (1,) * (im.ndim - 2)
    tx = tx.reshape((1, -1) + tail)
    ty = ty.reshape((-1, 1) + tail)
    rows = np.take(im, x0, axis=1)
    rows *= (np.float32(1) - tx)
    right = np.take(im, x1, axis=1)
    right *= tx
    rows += right                                   # (h, out_w[, C])
    out = np.take(rows, y0, axis=0)
    out *= (np.float32(1) - ty)
    below = np.take(rows, y1, axis=0)
    below *= ty
    out += below
    return out


def _u8_axis(n_src, n_dst, snap):
    """Per destination index of an axis resized n_src -> n_dst: the two source indices and their weights in 11 fractional bits, as
    cv::resize builds them for 8-bit INTER_LINEAR -- `_src_coords` and the border rules of `resize_bilinear` (snap: positions outside
    the image read the border pixel with weights (1, 0); else weights kept, indices clamped), each weight rounded on its own, half to
    even (saturate_cast<short>(w * 2048))."""
    i0, t = _src_coords(n_dst, float(n_dst) / n_src)
    if snap:
        t = np.where((i0 < 0) | (i0 >= n_src - 1), np.float32(0), t).astype(np.float32)
        i0 = np.clip(i0, 0, n_src - 1)
        i1 = np.minimum(i0 + 1, n_src - 1)
    else:
        i1 = np.clip(i0 + 1, 0, n_src - 1)
        i0 = np.clip(i0, 0, n_src - 1)
    w0 = np.rint((np.float32(1) - t) * np.float32(2048)).astype(np.int32)
    w1 = np.rint(t * np.float32(2048)).astype(np.int32)
    return i0, i1, w0, w1


def resize_bilinear_u8(im, out_w, out_h):
    """im (H, W[, C]) uint8 -> (out_h, out_w[, C]) uint8: cv2.resize(im, (out_w, out_h)) with INTER_LINEAR on 8-bit data, as OpenCV's
    scalar fixed-point path: weights in 11 fractional bits, the horizontal pass in int32, then the vertical pass
    (b0 * r0 + b1 * r1 + 2^21) >> 22, saturated.  Integer arithmetic throughout (the tracker's patch kernel repeats it bit for bit).
    Not pinned against cv2 (absent here); DESIGN.md section 4 lists the known differences of OpenCV builds."""
    im = np.asarray(im)
    assert im.dtype == np.uint8 and im.ndim in (2, 3) and im.shape[0] >= 1 and im.shape[1] >= 1, (im.dtype, im.shape)
    h, w = im.shape[:2]
    x0, x1, ax0, ax1 = _u8_axis(w, int(out_w), True)
    y0, y1, by0, by1 = _u8_axis(h, int(out_h), False)
    tail = (1,) * (im.ndim - 2)
    src = im.astype(np.int32)
    rows = np.take(src, x0, axis=1) * ax0.reshape((1, -1) + tail) + np.take(src, x1, axis=1) * ax1.reshape((1, -1) + tail)
    out = np.take(rows, y0, axis=0) * by0.reshape((-1, 1) + tail) + np.take(rows, y1, axis=0) * by1.reshape((-1, 1) + tail)
    return np.clip((out + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def crop_ranges(boxes, h, w):
    """The slices of `I[int(y1):int(y2), int(x1):int(x2)]` (reference tracking_engine.py:143) resolved against an h x w frame with
    NumPy's own rule (slice.indices: int() truncates towards zero, a negative start counts from the far border, ends are clipped):
    int32 [n, 4] = x0, x1, y0, y1 with the crop = rows [y0, y1) x columns [x0, x1); x1 <= x0 or y1 <= y0 is an empty crop."""
    boxes = np.asarray(boxes)
    out = np.zeros((len(boxes), 4), dtype=np.int32)
    for i, b in enumerate(boxes):
        xs = slice(int(b[0]), int(b[2])).indices(int(w))
        ys = slice(int(b[1]), int(b[3])).indices(int(h))
        out[i] = (xs[0], xs[1], ys[0], ys[1])
    return out


# ImageNet normalisation of the reference's feature extractor (lib/utils/pytorch_cnn_features.py): its third std is 0.224
TRACK_CNN_MEAN = (0.485, 0.456, 0.406)
TRACK_CNN_STD = (0.229, 0.224, 0.224)


def crop_resize_patches(frame, ranges, out_size, mean=TRACK_CNN_MEAN, std=TRACK_CNN_STD):
    """Host restatement of dat_crop_resize_patches: frame (h, w, 3) uint8 BGR, ranges from `crop_ranges` -> fp32 [n, 3, out, out]: the
    crop, BGR -> RGB, 8-bit bilinear resize (an empty crop: an all-zero image), HWC -> CHW, (v / 255 - mean) / std in float64, rounded
    to float32."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    s = int(out_size)
    mean64 = np.asarray(mean, dtype=np.float64).reshape(3, 1, 1)
    std64 = np.asarray(std, dtype=np.float64).reshape(3, 1, 1)
    out = np.zeros((len(ranges), 3, s, s), dtype=np.float32)
    for i, (x0, x1, y0, y1) in enumerate(np.asarray(ranges).tolist()):
        patch = frame[y0:y1, x0:x1, ::-1] if (x1 > x0 and y1 > y0) else None
        small = resize_bilinear_u8(patch, s, s) if patch is not None else np.zeros((s, s, 3), dtype=np.uint8)
        chw = small.transpose(2, 0, 1).astype(np.float64)
        out[i] = ((chw / 255.0 - mean64) / std64).astype(np.float32)
    return out


def _keys_weights(t):
    """Four weights of the a = -0.75 bicubic kernel at fractional offset t (distances t+1, t, 1-t, 2-t)."""
    a = np.float32(-0.75)
    one = np.float32(1)
    p, q = t + one, one - t
    w0 = ((a * p - np.float32(5) * a) * p + np.float32(8) * a) * p - np.float32(4) * a
    w1 = ((a + np.float32(2)) * t - (a + np.float32(3))) * t * t + one
    w2 = ((a + np.float32(2)) * q - (a + np.float32(3))) * q * q + one
    return [w0, w1, w2, one - w0 - w1 - w2]


def resize_bicubic(im, out_w, out_h):
    """im (H, W[, C]) float32 -> (out_h, out_w[, C]); cv2.INTER_CUBIC (a = -0.75, replicated borders)."""
    im = np.asarray(im, dtype=np.float32)
    h, w = im.shape[:2]
    x0, tx = _src_coords(out_w, float(out_w) / w)
    y0, ty = _src_coords(out_h, float(out_h) / h)
    tail = (1,) * (im.ndim - 2)
    wx, wy = _keys_weights(tx), _keys_weights(ty)
    rows = np.take(im, np.clip(x0 - 1, 0, w - 1), axis=1) * wx[0].reshape((1, -1) + tail)
    for k in range(1, 4):
        rows += np.take(im, np.clip(x0 - 1 + k, 0, w - 1), axis=1) * wx[k].reshape((1, -1) + tail)
    out = np.take(rows, np.clip(y0 - 1, 0, h - 1), axis=0) * wy[0].reshape((-1, 1) + tail)
    for k in range(1, 4):
        out += np.take(rows, np.clip(y0 - 1 + k, 0, h - 1), axis=0) * wy[k].reshape((-1, 1) + tail)
    return out


def move_batch_to_time(blob, num_frames):
    """(B*T, C, H, W) -> (B, C, T, H, W) (reference :82-93)."""
    bt, c, h, w = blob.shape
    assert bt % num_frames == 0
    return np.ascontiguousarray(blob.reshape(bt // num_frames, num_frames, c, h, w).transpose(0, 2, 1, 3, 4))
