"""NMS dispatch -- mirror of reference lib/core/nms_wrapper.py:29-70, backed by libdat_hip.

Boxes (5 columns) use the cython_nms semantics (suppress at IoU >= thresh, ascending original indices); tubes use
py_cpu_nms_tubes semantics (mean IoU over frames, keep while <= thresh, score order) -- both on the device.  Soft-NMS
(lib/utils/cython_nms.pyx:98-203) for host arrays runs the reference's loop in the same C float arithmetic (`dat_soft_nms_host`);
callers that hold device tensors use ops.hip_ops.soft_nms / box_results(soft_nms=...), the device twin the engine runs.  `nms(..., soft_nms=True)` is rejected loudly: the reference's dispatcher accepts the flag and silently ignores it.  Soft-NMS of
tube rows is the reference's NotImplementedError unless cfg.HIP.TUBE_SOFT_NMS is on (`dat_soft_nms_tubes_host`, of which
`dat_soft_nms_host` is the five-column case)."""
import ctypes as C

import numpy as np
import torch

from detectandtrack_amd import libdat as L
from detectandtrack_amd.ops import hip_ops as ops


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
    test.py:766-772 stores that tuple as the class's detections and breaks on the next line; core/test.py unpacks it.
    Rows [n, 4T+1] with cfg.HIP.TUBE_SOFT_NMS: the same loop with the mean per-frame IoU as the overlap (the
    reference defines none)."""
    if dets.shape[0] == 0:
        return dets, np.zeros((0,), dtype=np.int64)
    cols = dets.shape[1]
    if cols > 5:
        from detectandtrack_amd.core.config import cfg
        if not cfg.HIP.TUBE_SOFT_NMS:
            raise NotImplementedError('Need to handle tubes..')
        assert (cols - 1) % 4 == 0, 'Invalid tube dimensions {}'.format(dets.shape)
    assert method in ops.SOFT_NMS_METHODS, 'Unknown soft_nms method: {}'.format(method)
    entry, extra = ('dat_soft_nms_tubes_host', ((cols - 1) // 4,)) if cols > 5 else ('dat_soft_nms_host', ())
    src = np.ascontiguousarray(dets, dtype=np.float32)
    n = src.shape[0]
    out = np.empty((n, cols), dtype=np.float32)
    inds = np.empty((n,), dtype=np.int32)
    m = C.c_int(0)
    rc = getattr(L.lib(), entry)(src.ctypes.data_as(C.POINTER(C.c_float)), n, *extra, np.float32(sigma), np.float32(overlap_thresh),
                                 np.float32(score_thresh), ops.SOFT_NMS_METHODS[method], out.ctypes.data_as(C.POINTER(C.c_float)),
                                 inds.ctypes.data_as(C.POINTER(C.c_int)), C.byref(m))
    if rc != L.DAT_OK:
        raise L.DatError('%s failed with %d (rows of %d columns)' % (entry, rc, cols))
    return out[:m.value], inds[:m.value].astype(np.int64)
