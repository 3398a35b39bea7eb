"""Float64 references of the grouped conv's backward (ResNeXt `branch2b`), independent of the kernels: both gradients are stated as G
dense problems, each over its own slice of channels, concatenated over the groups -- the definition tests/grouped_ref.py gives the
forward.  tests/test_grouped_train_cpu.py holds both against torch.autograd on F.conv3d(groups=G)."""
import numpy as np

from tests import numerics as nm
from tests import wgrad_refs as wr


def dgrad_filter(w, groups):
    """The filter of the data-gradient conv in the grouped layout, from the (already scaled and quantised) forward filter
    w [C, cg, KT, KH, KW]: W'[ci][co_local] = flip(w[co][ci_local]) inside every group -- flipped over the taps, transposed per group."""
    w = np.asarray(w)
    C, cg = w.shape[0], w.shape[1]
    assert C == cg * groups, (w.shape, groups)
    out = np.empty_like(w)
    for g in range(groups):
        blk = w[g * cg:(g + 1) * cg]                                   # [co_local, ci_local, taps...]
        out[g * cg:(g + 1) * cg] = np.transpose(blk, (1, 0, 2, 3, 4))[:, :, ::-1, ::-1, ::-1]
    return out


def zero_insert2x(g, H, W):
    """g (N, C, T, Ho, Wo) -> (N, C, T, H, W) with g at the even positions (the stride-2 layer's gradient as a stride-1 problem)."""
    g = np.asarray(g)
    out = np.zeros(g.shape[:3] + (H, W), dtype=g.dtype)
    out[..., 0:2 * g.shape[3]:2, 0:2 * g.shape[4]:2] = g
    return out


def grouped_dgrad_ref64(g, w_scaled, groups, stride, pads, H, W, add=None, mask=None):
    """(ref64, absref64) of dL/dx (N, C, T, H, W): per group the dense stride-1 conv (tests/numerics.conv_ref64) of the group's slice of
    the (zero-inserted) gradient with the group's flipped, transposed filter; `add` is summed in (res_mode 1), `mask > 0 ? v : 0` applied
    last (res_mode 3).  g: (N, C, T, Ho, Wo); w_scaled: the forward filter times its AffineChannelNd scale, as the kernel sees it."""
    g, w_scaled = np.asarray(g), np.asarray(w_scaled)
    C, cg, kt = w_scaled.shape[0], w_scaled.shape[1], w_scaled.shape[2]
    assert tuple(w_scaled.shape[3:]) == (3, 3) and tuple(pads[1:]) == (1, 1)
    gz = zero_insert2x(g, H, W) if stride == 2 else g
    assert gz.shape[3:] == (H, W), (gz.shape, H, W)
    wd = dgrad_filter(w_scaled, groups)
    refs, absrefs = [], []
    for k in range(groups):
        sl = slice(k * cg, (k + 1) * cg)
        r, a = nm.conv_ref64(gz[:, sl], wd[sl], None, None, None if add is None else np.asarray(add)[:, sl], (1, 1),
                             (kt - 1 - pads[0], 1, 1), False, None if mask is None else np.asarray(mask)[:, sl])
        refs.append(r)
        absrefs.append(a)
    return np.concatenate(refs, axis=1), np.concatenate(absrefs, axis=1)


def grouped_wgrad_ref64(x, g, groups, scale, k, stride, pads, window=None):
    """(ref, absref, K): dW (C, cg, KT, KH, KW) -- per group tests/wgrad_refs.wgrad_ref64 of the group's slices of x and g, concatenated
    over the output channels; K = the number of output positions reduced."""
    x, g = np.asarray(x), np.asarray(g)
    C = x.shape[1]
    cg = C // groups
    refs, absrefs, K = [], [], 0
    for j in range(groups):
        sl = slice(j * cg, (j + 1) * cg)
        r, a, K = wr.wgrad_ref64(x[:, sl], g[:, sl], None if scale is None else np.asarray(scale)[sl], k, stride, pads, window)
        refs.append(r)
        absrefs.append(a)
    return np.concatenate(refs, axis=0), np.concatenate(absrefs, axis=0), K
