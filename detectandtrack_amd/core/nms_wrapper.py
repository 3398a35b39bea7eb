"""NMS dispatch -- mirror of reference lib/core/nms_wrapper.py:29-70, backed by libdat_hip.

Boxes (5 columns) use the cython_nms semantics (suppress at IoU >= thresh, ascending original indices); tubes use
py_cpu_nms_tubes semantics (mean IoU over frames, keep while <= thresh, score order) -- both on the device.  Soft-NMS
(lib/utils/cython_nms.pyx:98-203) for host arrays runs the reference's loop in the same C float arithmetic (`dat_soft_nms_host`);
callers that hold device tensors use ops.hip_ops.soft_nms / box_results(soft_nms=...), the device twin the engine runs.  `nms(..., soft_nms=True)` is rejected loudly: the reference's dispatcher accepts the flag and silently ignores it.  Soft-NMS of
tube rows is the reference's NotImplementedError unless cfg.HIP.TUBE_SOFT_NMS is on (`dat_soft_nms_tubes_host`)."""
import ctypes as C

import numpy as np
import torch

from detectandtrack_amd import libdat as L
from detectandtrack_amd.ops import hip_ops as ops

_METHODS = {'hard': 0, 'linear': 1, 'gaussian': 2}


def nms(dets, thresh, soft_nms=False):
    if soft_nms:
        raise ValueError('nms(soft_nms=True): the reference ignores this flag (nms_wrapper.py:49-57); call soft_nms() instead')
    if dets.shape[0] == 0:
        return []
    d = torch.from_numpy(np.ascontiguousarray(dets, dtype=np.float32)).cuda()
    return ops.nms(d, float(thresh)).cpu().numpy().astype(np.int64)


def tube_nms(dets, thresh):
    return nms(dets, thresh)


def soft_nms(dets, sigma=0.5, overlap_thresh=0.3, score_thresh=0.001, method='linear'):
    """(:29-46) returns what the Cython function returns: (re-scored dets [m, 5], indices into the input [m]).  The reference's
    test.py:766-772 stores that tuple as the class's detections and breaks on the next line; core/test.py unpacks it."""
    if dets.shape[0] == 0:
        return dets, np.zeros((0,), dtype=np.int64)
    if dets.shape[1] > 5:
        from detectandtrack_amd.core.config import cfg
        if not cfg.HIP.TUBE_SOFT_NMS:
            raise NotImplementedError('Need to handle tubes..')
        return _soft_nms_tubes(dets, sigma, overlap_thresh, score_thresh, method)
    assert method in _METHODS, 'Unknown soft_nms method: {}'.format(method)
    src = np.ascontiguousarray(dets, dtype=np.float32)
    n = src.shape[0]
    out = np.empty((n, 5), dtype=np.float32)
    inds = np.empty((n,), dtype=np.int32)
    m = C.c_int(0)
    rc = L.lib().dat_soft_nms_host(src.ctypes.data_as(C.POINTER(C.c_float)), n, np.float32(sigma), np.float32(overlap_thresh),
                                   np.float32(score_thresh), _METHODS[method], out.ctypes.data_as(C.POINTER(C.c_float)),
                                   inds.ctypes.data_as(C.POINTER(C.c_int)), C.byref(m))
    if rc != L.DAT_OK:
        raise L.DatError('dat_soft_nms_host failed with %d' % rc)
    return out[:m.value], inds[:m.value].astype(np.int64)


def _soft_nms_tubes(dets, sigma, overlap_thresh, score_thresh, method):
    """Rows [n, 4T+1] with cfg.HIP.TUBE_SOFT_NMS: the same loop with the mean per-frame IoU as the overlap (`dat_soft_nms_tubes_host`,
    DESIGN.md section 3.13; the reference defines none)."""
    assert method in _METHODS, 'Unknown soft_nms method: {}'.format(method)
    assert (dets.shape[1] - 1) % 4 == 0, 'Invalid tube dimensions {}'.format(dets.shape)
    T = (dets.shape[1] - 1) // 4
    src = np.ascontiguousarray(dets, dtype=np.float32)
    n = src.shape[0]
    out = np.empty((n, 4 * T + 1), dtype=np.float32)
    inds = np.empty((n,), dtype=np.int32)
    m = C.c_int(0)
    rc = L.lib().dat_soft_nms_tubes_host(src.ctypes.data_as(C.POINTER(C.c_float)), n, T, np.float32(sigma), np.float32(overlap_thresh),
                                         np.float32(score_thresh), _METHODS[method], out.ctypes.data_as(C.POINTER(C.c_float)),
                                         inds.ctypes.data_as(C.POINTER(C.c_int)), C.byref(m))
    if rc != L.DAT_OK:
        raise L.DatError('dat_soft_nms_tubes_host failed with %d (T = %d)' % (rc, T))
    return out[:m.value], inds[:m.value].astype(np.int64)
