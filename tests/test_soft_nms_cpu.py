"""CPU tests of the Soft-NMS specification the device kernel (csrc/detections.hip soft_nms_kernel) is written from."""
import numpy as np
import pytest

from tests import soft_nms_cases as sc


def _cases():
    yield 'golden', sc.golden_dets()
    for n in sc.TIE_SIZES:
        yield 'ties_n%d' % n, sc.tie_dets(n, 1000 + n)


@pytest.mark.parametrize('method', sc.METHODS)
def test_reweight_all_then_fill_holes_from_the_tail_equals_the_serial_loop(method):
    """Per iteration of lib/utils/cython_nms.pyx:98-203 -- re-score every later position at once, keep the survivors below the new N
    where they are and fill the holes below it (ascending) with the surviving tail rows (descending) -- leaves the rows exactly where
    the reference's serial swap-with-last walk (dat_soft_nms_host) leaves them: row for row and index for index, for the golden
    inputs and for random boxes whose scores take 8 values, so that positions decide ties in nearly every iteration."""
    saw_removal = False
    for name, dets in _cases():
        ref_d, ref_i = sc.host_soft_nms(dets, method)
        got_d, got_i = sc.parallel_soft_nms(dets, method)
        np.testing.assert_array_equal(got_i, ref_i, err_msg=name)
        np.testing.assert_array_equal(got_d, ref_d, err_msg=name)
        saw_removal |= 0 < len(ref_i) < len(dets)
    assert saw_removal or method == 'gaussian'       # (the compaction was exercised)


def test_the_gaussian_inputs_of_the_device_comparison_qualify():
    """The device's double exp is accurate to 1 ulp, not correctly rounded, so a gaussian score may differ from the reference's by
    one float ulp per re-scoring: k * 2^-23 relative after k re-scorings, the allowance the device comparison was designed with
    (tests/test_gpu_soft_nms.py measured zero and asserts bit-identity).  Identical indices in
    identical order can only be demanded of inputs on which no decision of the reference run is closer than that: every arg-max
    winner leads every other candidate by more than the two rows' allowances together, and every re-scored score is further from
    the threshold than its own.  All generated cases must qualify (a case that did not would get another seed here, not a skip)."""
    assert max(n for n, _ in sc.GAUSSIAN_CASES) == sc.CAPACITY
    qualified = 0
    for n, seed in sc.GAUSSIAN_CASES:
        dets = sc.smooth_dets(n, seed)
        audit = {}
        d, i, k = sc.parallel_soft_nms(dets, 'gaussian', count_rescorings=True, audit=audit)
        ref_d, ref_i = sc.host_soft_nms(dets, 'gaussian')
        np.testing.assert_array_equal(i, ref_i)
        np.testing.assert_array_equal(d, ref_d)
        # the issue's statement of the condition: consecutive selected scores of the reference differ by more than the tolerance
        s = ref_d[:, 4].astype(np.float64)
        consecutive = np.all(s[:-1] - s[1:] > (k[:-1] + k[1:]) * sc.ULP * s[:-1]) if len(s) > 1 else True
        qualified += bool(audit.get('slack', np.inf) > 0 and consecutive)
    assert qualified == len(sc.GAUSSIAN_CASES)


def test_device_results_predicate_with_soft_nms_and_voting():
    """core/test.device_results_supported: TEST.SOFT_NMS / TEST.BBOX_VOTE no longer leave the device path for box detections; tube
    detections with either switch do, and so does Soft-NMS over more rois per image than the device kernel holds in LDS (the host
    loop has no capacity, so such a config keeps working as before)."""
    from detectandtrack_amd.core import test as engine
    from detectandtrack_amd.core.config import cfg, reset_cfg
    reset_cfg()
    try:
        cfg.MODEL.FASTER_RCNN = True
        assert engine.device_results_supported()
        cfg.TEST.SOFT_NMS.ENABLED = True
        assert cfg.TEST.RPN_POST_NMS_TOP_N <= engine.SOFT_NMS_MAX_BOXES == sc.CAPACITY
        assert engine.device_results_supported()
        cfg.TEST.RPN_POST_NMS_TOP_N = sc.CAPACITY + 1
        assert not engine.device_results_supported()
        cfg.TEST.SOFT_NMS.ENABLED, cfg.TEST.BBOX_VOTE.ENABLED = False, True        # (voting has no capacity: global-memory reads)
        assert engine.device_results_supported()
        cfg.TEST.RPN_POST_NMS_TOP_N = 1000
        cfg.MODEL.VIDEO_ON, cfg.VIDEO.BODY_HEAD_LINK, cfg.VIDEO.NUM_FRAMES_MID = True, '', 3      # tube detections
        assert not engine.device_results_supported()
        cfg.TEST.BBOX_VOTE.ENABLED = False
        assert engine.device_results_supported()
        cfg.TEST.SOFT_NMS.ENABLED = True
        assert not engine.device_results_supported()
        cfg.VIDEO.BODY_HEAD_LINK = 'slice-center'                                  # 3D body, 2D heads: boxes
        assert engine.device_results_supported()
    finally:
        reset_cfg()
