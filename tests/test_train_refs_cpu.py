"""The float64 references of tests/train_refs.py against the operators they restate, and the scalar-loss bound of tests/numerics.py
against a correctly and an incorrectly summed loss -- on the CPU, so that tests/test_gpu_train_kernels.py holds the kernels to
references that are themselves right."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import numerics as nm
from tests import train_refs as tr
from oracle import roi_align as ora


def _rois(rs, R, Tr, n_batch, img_h, img_w):
    r = np.zeros((R, 4 * Tr + 1), np.float32)
    r[:, 0] = rs.randint(0, n_batch, R)
    for t in range(Tr):
        x1, y1 = rs.uniform(-20, img_w - 10, R), rs.uniform(-20, img_h - 10, R)
        r[:, 1 + 4 * t], r[:, 2 + 4 * t] = x1, y1
        r[:, 3 + 4 * t], r[:, 4 + 4 * t] = x1 + rs.uniform(0.3, 90, R), y1 + rs.uniform(0.3, 70, R)
    return r


@pytest.mark.parametrize('Tr,T,t0,sampling,pooled', [(1, 1, 0, 2, 7), (1, 3, 2, 0, 7), (2, 2, 0, 2, 5), (3, 3, 0, 0, 4)])
def test_roi_align_bwd_ref_is_the_adjoint_of_the_oracle(Tr, T, t0, sampling, pooled):
    """<RoIAlign(x), u> == <x, RoIAlign^T(u)> with the forward of oracle/roi_align.py (2D rois on frame n*T + t0, tube rois through
    roi_align_tube) and the transpose restated in tests/train_refs.py."""
    rs = np.random.RandomState(7 + Tr + sampling)
    N, C, H, W, sc = 2, 5, 12, 15, 0.25
    x = rs.randn(N * T, H, W, C).astype(np.float32)
    rois = _rois(rs, 9, Tr, N, H / sc, W / sc)
    rois[0, 3:5] = rois[0, 1:3] + 0.2                       # smaller than a bin
    if Tr == 1:
        rb = rois.copy()
        rb[:, 0] = rb[:, 0] * T + t0
        y = ora.roi_align_2d(x.transpose(0, 3, 1, 2), rb, pooled, sc, sampling)                  # (R, C, P, P)
        y = y.transpose(0, 2, 3, 1)
    else:
        x5 = x.reshape(N, T, H, W, C).transpose(0, 4, 1, 2, 3)
        y = ora.roi_align_tube(x5, rois, pooled, sc, sampling)                                    # (R, C, T, P, P)
        y = y.transpose(0, 2, 3, 4, 1).reshape(-1, pooled, pooled, C)
    u = rs.randn(*y.shape)
    ref, ab, ex, K = tr.roi_align_bwd_ref([(N * T, H, W)], [sc], rois, u, T, Tr, t0, pooled, sampling)
    lhs = float((y.astype(np.float64) * u).sum())
    rhs = float((x.astype(np.float64) * ref[0]).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((np.abs(y) * np.abs(u)).sum()), (lhs, rhs)
    assert np.all(ab[0] >= np.abs(ref[0])) and np.all(ex[0] >= 0) and K >= 1


def test_roi_levels_follow_the_oracle_fpn_mapping():
    """The per-roi level of the reference (mean tube area, FPN.py:349-360) == oracle.proposals.map_rois_to_fpn_levels for 2D rois,
    including rois whose side sits exactly on a level boundary (56, 112, 224, 448 at canonical scale 224, level 4)."""
    from oracle.proposals import map_rois_to_fpn_levels
    rs = np.random.RandomState(3)
    rois = _rois(rs, 60, 1, 1, 800, 800)
    for i, s in enumerate((56, 112, 224, 448, 55, 111, 223, 447)):
        rois[i, 1:3] = (10.25, 20.5)
        rois[i, 3:5] = rois[i, 1:3] + s - 1
    got = tr.roi_levels(rois, 1, 4, 2, 224., 4)
    exp = map_rois_to_fpn_levels(rois[:, 1:5], 2, 5) - 2
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(got[:8], [0, 1, 2, 3, 0, 0, 1, 2])


@pytest.mark.parametrize('up,Tr,S', [(2, 1, 14), (2, 2, 7), (4, 1, 5), (4, 2, 6)])
def test_kps_finalize_bwd_ref_is_the_transpose_of_the_tail(up, Tr, S):
    """kps_finalize_ref is the bilinear ConvTranspose of oracle.net3d.kps_outputs_2d (as test_kps_tail writes it) on the sub-pixel
    channels unfolded by their definition, and kps_finalize_bwd_ref is its transpose."""
    from oracle.net3d import bilinear_kernel
    rs = np.random.RandomState(up * 10 + Tr)
    R, K, cs = 2, 3, 16
    sub = rs.randn(R * Tr, S, S, cs)
    low = np.zeros((R * Tr, K, 2 * S, 2 * S))
    for Y in range(2 * S):
        for X in range(2 * S):
            low[:, :, Y, X] = sub[:, Y >> 1, X >> 1, ((Y & 1) * 2 + (X & 1)) * K:((Y & 1) * 2 + (X & 1) + 1) * K]
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    exp = F.conv_transpose2d(t64(low), t64(bilinear_kernel(K, up)), None, stride=up, padding=up // 2).numpy()
    out = tr.kps_finalize_ref(sub, R, Tr, K, up)
    np.testing.assert_allclose(out.reshape(exp.shape), exp, rtol=1e-12, atol=1e-12)
    u = rs.randn(*out.shape)
    dsub = tr.kps_finalize_bwd_ref(u, R, Tr, S, cs, K, up)
    assert dsub.shape == sub.shape and np.all(dsub[..., 4 * K:] == 0)
    lhs, rhs = float((out * u).sum()), float((sub * dsub).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((np.abs(out) * np.abs(u)).sum()), (lhs, rhs)


def _rpn_cls_terms():
    """The RPN classification loss on random logits: the float64 reference, and the per-term fp32 values a kernel thread computes."""
    rs = np.random.RandomState(11)
    N, T, H, W, A = 2, 3, 16, 16, 4
    head = (rs.randn(N * T, H, W, A + 4 * A) * 3).astype(np.float32)
    labels = rs.randint(0, 2, (N, A, H, W)).astype(np.int32)
    z = np.zeros((N, 4 * T * A, H, W), np.float32)
    ref = tr.rpn_loss_ref(head, labels, z, z, z, A, 0, A, T, 1, 1.0, 1.0 / 9, 1.0)
    lg = head[..., :A].reshape(N, T, H, W, A)
    v = lg[:, 0]
    for t in range(1, T):
        v = v + lg[:, t]
    v = v / np.float32(T)
    lab = labels.transpose(0, 2, 3, 1).astype(np.float32)
    terms = (np.maximum(v, np.float32(0)) - v * lab + np.log1p(np.exp(-np.abs(v)))).astype(np.float32).reshape(-1)
    return ref, terms


def _kernel_order_sum(terms, fmt=np.float32):
    """Per-block sums over 256 terms (an LDS tree), then one add per block in launch order -- in `fmt`."""
    torch_fmt = {np.float32: torch.float32, 'bf16': torch.bfloat16}[fmt]
    t = torch.from_numpy(terms).to(torch_fmt)
    n = (len(terms) + 255) // 256 * 256
    t = torch.cat([t, torch.zeros(n - len(terms), dtype=torch_fmt)]).view(-1, 256)
    while t.shape[1] > 1:
        t = t[:, : t.shape[1] // 2] + t[:, t.shape[1] // 2:]
    acc = torch.zeros((), dtype=torch_fmt)
    for b in t[:, 0]:
        acc = acc + b
    return float(acc)


def test_scalar_loss_bound_accepts_fp32_and_rejects_a_dropped_term_and_bf16_accumulation():
    ref, terms = _rpn_cls_terms()
    n = ref['n'][0]
    assert n == len(terms)
    good = _kernel_order_sum(terms)
    nm.assert_sum(good, ref['loss'][0], ref['loss_abs'][0], n, 'fp32 sum', extra=ref['loss_extra'][0])
    dropped = _kernel_order_sum(np.delete(terms, len(terms) // 2))
    assert float(terms[len(terms) // 2]) > 0.05
    with pytest.raises(AssertionError):
        nm.assert_sum(dropped, ref['loss'][0], ref['loss_abs'][0], n, 'one term dropped', extra=ref['loss_extra'][0])
    bf = _kernel_order_sum(terms, 'bf16')
    with pytest.raises(AssertionError):
        nm.assert_sum(bf, ref['loss'][0], ref['loss_abs'][0], n, 'bf16 accumulation', extra=ref['loss_extra'][0])
