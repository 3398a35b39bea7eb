"""Inputs of tests/test_gpu_proposals.py, built on the host (NumPy only) so that tests/test_proposals_ref_cpu.py can check them and
the reference (tests/proposals_ref.py) on a machine without a GPU: every head array [frames, H, W, cstride] the GPU tests upload,
with the level geometry and the call's arguments, and the inputs of the collect and detection tests.

Scores are built to meet the selection kernels where uniform random scores do not: clustered in one histogram bin, tied in groups
that the cut divides, tied across index 65536 and across K0's chunks of 32768 anchors, exactly zero.  Unused head channels hold 7.0,
so a kernel reading a wrong channel offset decodes visibly wrong boxes.
"""
import functools

import numpy as np

from oracle.anchors import generate_anchors
from tests import numerics as nm
from tests import proposals_ref as pr

F32 = np.float32
S = (105, 105)      # x A = 3: 33 075 anchors, a second, nearly empty K0 chunk
M = (150, 148)      # x A = 3: 66 600 anchors, three K0 chunks, indices above 65 535
NO_NMS = 2.0        # IoU <= 1 < nms_thresh: the call returns K3's sorted, filtered list itself
RATIOS3 = (0.5, 1, 2)


class Case(object):
    """One dat_rpn_proposals(_batch) call: levels = [(head float32 array, proposals_ref.Level)], dtype 0 (fp32 head) or 1 (16-bit
    head; the array already holds values of the 16-bit format `fmt`)."""

    def __init__(self, levels, im_info, pre_nms, post_nms=None, nms_thresh=NO_NMS, min_size=0., dtype=0, batch_idx=0., n_images=1,
                 frame_stride=0, bites=()):
        self.levels = levels
        self.im_info = np.asarray(im_info, F32).reshape(-1, 3)
        self.pre_nms, self.post_nms = int(pre_nms), int(pre_nms if post_nms is None else post_nms)
        self.nms_thresh, self.min_size, self.dtype, self.batch_idx = float(nms_thresh), float(min_size), int(dtype), float(batch_idx)
        self.n_images, self.frame_stride = int(n_images), int(frame_stride)
        self.bites = tuple(bites)     # which wrong selection rules must change the expected output: 'tie', 'cut'
        assert self.im_info.shape[0] == self.n_images

    def deltas(self):
        """Every delta value a decode of this case may read (the arguments of exp among them)."""
        out = []
        for head, spec in self.levels:
            n = 4 * spec.A * (1 if spec.per_frame else spec.T)
            out.append(head[..., spec.delta_off:spec.delta_off + n].reshape(-1))
        return np.concatenate(out)

    def reference(self, select_fn=pr.select):
        """[image][level] -> (rois, probs, flat indices) of proposals_ref.proposals."""
        return [[pr.proposals(head, spec.at_frame(spec.frame + i * self.frame_stride), self.im_info[i], self.pre_nms, self.post_nms,
                              self.nms_thresh, self.min_size, self.batch_idx + i, select_fn) for head, spec in self.levels]
                for i in range(self.n_images)]


def _anchors(stride, size, ratios=RATIOS3, T=1):
    return generate_anchors(float(stride), (size,), ratios, time_dim=T).astype(F32)


def _level(rs, shape, A, scores, fmt, stride=4, size=16, frames=1, frame=0, logit_off=0, T=1, per_frame=False, apply_sigmoid=False,
           sigma=0.5, ratios=RATIOS3):
    """scores [frames, N] (flat (h, w, a) order) -> (head, Level).  Deltas randn * sigma; channels: logit_off junk, A logits, one
    junk channel, the deltas, junk up to a multiple of 8."""
    H, W = shape
    scores = np.asarray(scores, F32).reshape(frames, H, W, A)
    nd = 4 * A * (1 if per_frame else T)
    delta_off = logit_off + A + 1
    cs = (delta_off + nd + 1 + 7) // 8 * 8
    head = np.full((frames, H, W, cs), 7.0, F32)
    head[..., logit_off:logit_off + A] = scores
    head[..., delta_off:delta_off + nd] = (rs.randn(frames, H, W, nd) * sigma).astype(F32)
    if fmt != 'fp32':
        head = nm.q16(head, fmt)
    spec = pr.Level(H, W, A, T, stride, cs, logit_off, delta_off, frame, _anchors(stride, size, ratios, T), apply_sigmoid, per_frame)
    return head, spec


def _im(shape, stride, scale=1.0):
    return [[shape[0] * stride, shape[1] * stride, scale]]


# ---- selection ------------------------------------------------------------------------------------------------------------------
def one_bin_distinct(fmt):
    """All keys distinct inside ONE histogram bin (0x3F00): n_gt = 0, the whole level is the boundary list."""
    rs = np.random.RandomState(1)
    n = S[0] * S[1] * 3
    scores = (F32(0.5) + rs.permutation(n).astype(F32) * F32(2.0 ** -24)).astype(F32)
    assert np.unique(scores).size == n and (scores.view(np.uint32) >> 16 == 0x3F00).all()
    return Case([_level(rs, S, 3, scores, fmt)], _im(S, 4), 700, bites=('cut',))


def tie_cut(v, pre, fmt):
    """Level M, scores in {0.75, v, 0.25}; pre // 3 anchors score 0.75 and the cut falls inside the v group, whose members lie below
    index 65536 in K0's chunks 0 and 1 (half of the members taken) and above it in chunk 2 (the other half, the cut, 100 left out)."""
    rs = np.random.RandomState(1000 + pre)
    n = M[0] * M[1] * 3
    n_top = pre // 3
    need = pre - n_top
    n_low = need // 2
    n_high = need - n_low + 100
    low = rs.choice(65536, n_low + n_top, replace=False)
    high = 65536 + rs.choice(n - 65536, n_high, replace=False)
    scores = np.full(n, 0.25, F32)
    scores[low[:n_low]] = v
    scores[low[n_low:]] = 0.75
    scores[high] = v
    return Case([_level(rs, M, 3, scores, fmt)], _im(M, 4), pre, bites=('tie', 'cut'))


def full_chunk_one_bin(fmt):
    """All-equal scores on M, pre_nms 16384: K0's chunks 0 and 1 put 32768 keys into one packed 16-bit counter, and K3 sorts 16384."""
    rs = np.random.RandomState(3)
    return Case([_level(rs, M, 3, np.full(M[0] * M[1] * 3, 0.5, F32), fmt)], _im(M, 4), 16384, bites=('tie', 'cut'))


def whole_boundary_bin(fmt):
    """200 anchors above the boundary bin and exactly 500 in it (fifty values of ten ties each), pre_nms 700: need == n_bnd, the
    branch that skips the radix select (thr48 = 0)."""
    rs = np.random.RandomState(4)
    n = S[0] * S[1] * 3
    at = rs.choice(n, 700, replace=False)
    scores = np.full(n, 0.25, F32)
    scores[at[:200]] = 0.75
    scores[at[200:]] = F32(0.5) + (np.arange(500) % 50).astype(F32) * F32(2.0 ** -24)
    return Case([_level(rs, S, 3, scores, fmt)], _im(S, 4), 700, bites=('tie',))


def k_eff_n(fmt):
    """pre_nms 1000 above both levels' anchor counts (1 and 700): k_eff = N."""
    rs = np.random.RandomState(5)
    one = _level(rs, (1, 1), 1, [0.625], fmt, stride=32, size=64, ratios=(1,))
    many = _level(rs, (10, 14), 5, np.round(rs.uniform(0.01, 0.99, 700) * 64) / 64, fmt, stride=16, size=64, ratios=(0.25, 0.5, 1, 2, 4))
    return Case([one, many], _im((10, 14), 16), 1000, bites=('tie',))


def exact_zeros(fmt):
    """16000 positive scores, 17075 exact zeros, pre_nms 16384: the cut falls in bin 0, whose composites have a zero score half like
    K3's sort padding."""
    rs = np.random.RandomState(6)
    n = S[0] * S[1] * 3
    scores = np.zeros(n, F32)
    scores[rs.choice(n, 16000, replace=False)] = rs.uniform(0.01, 0.99, 16000).astype(F32)
    return Case([_level(rs, S, 3, scores, fmt)], _im(S, 4), 16384, bites=('tie', 'cut'))


# ---- head formats and layouts ---------------------------------------------------------------------------------------------------
def head16(fmt):
    """A 16-bit head: continuous random probabilities rounded to the format.  Equal keys by the hundred (bf16) or handful (fp16), and
    the low 16 key bits are zero in bf16: the select inside the boundary bin is decided by the index digits alone."""
    assert fmt in ('bf16', 'fp16')
    rs = np.random.RandomState(7)
    return Case([_level(rs, S, 3, rs.uniform(0.001, 0.999, S[0] * S[1] * 3), fmt)], _im(S, 4), 700, dtype=1, bites=('tie', 'cut'))


SIGMOID_GRID = np.arange(-384, 385).astype(F32) / F32(64)      # neighbouring probabilities differ by >= 2^-16 relative


def sigmoid_path(pre, fmt):
    """Logits through the kernel's sigmoid: -100 (probability exactly 0), {18, 24, 30} (exactly 1.0 in float32: expf(-18) < 2^-25),
    and a grid of step 1/64 on [-6, 6] whose order no expf can change.  300 ones, 4200 grid values, 1500 zeros: pre_nms 700 cuts
    inside the grid, 5000 among the zeros."""
    rs = np.random.RandomState(8)
    shape, n = (40, 50), 6000
    logits = SIGMOID_GRID[rs.randint(0, SIGMOID_GRID.size, n)]
    at = rs.choice(n, 1800, replace=False)
    logits[at[:300]] = np.asarray([18, 24, 30], F32)[rs.randint(0, 3, 300)]
    logits[at[300:]] = -100
    return Case([_level(rs, shape, 3, logits, fmt, stride=16, size=64, apply_sigmoid=True)], _im(shape, 16), pre, bites=('tie', 'cut'))


TUBE = dict(shape=(40, 30), A=2, T=3, stride=16, size=64, ratios=(0.5, 2))


def _tube_logits(rs, frames, n):
    """Forty base values; the last frame's logit is 0..3 float32 ulps above: sums that tie and sums that differ in the last bit."""
    base = rs.uniform(0.3, 0.7, 40).astype(F32)[rs.randint(0, 40, n)]
    out = np.tile(base, (frames, 1))
    out[-1] = (out[-1].view(np.uint32) + rs.randint(0, 4, n).astype(np.uint32)).view(F32)
    return out


def tubes(per_frame, fmt):
    """T = 3 tubes: per_frame 0 (one frame holds the logit and the (a, t, xywh) deltas) or 1 (frames 1..3 of a 5-frame head: the
    logits averaged, the deltas of tube frame t read from head frame 1 + t)."""
    rs = np.random.RandomState(9 + per_frame)
    t = TUBE
    n = t['shape'][0] * t['shape'][1] * t['A']
    if per_frame:
        scores = np.zeros((5, n), F32)
        scores[0] = scores[4] = 0.9          # frames outside the tube: a kernel averaging a wrong frame selects other anchors
        scores[1:4] = _tube_logits(rs, 3, n)
        lvl = _level(rs, t['shape'], t['A'], scores, fmt, t['stride'], t['size'], frames=5, frame=1, logit_off=1, T=3, per_frame=True,
                     ratios=t['ratios'])
    else:
        lvl = _level(rs, t['shape'], t['A'], _tube_logits(rs, 1, n), fmt, t['stride'], t['size'], logit_off=1, T=3, ratios=t['ratios'])
    return Case([lvl], _im(t['shape'], t['stride']), 500, bites=('tie', 'cut'))


# ---- filter, emit, NMS on -------------------------------------------------------------------------------------------------------
def min_size_filter(min_size, fmt):
    """2700 anchors of size 32, pre_nms 2048 (K3 owns two entries per thread), im_info scale 1.3: min_size 16 -> 20.8 (float32) drops
    about a third of the selected rows, all through the order; 0 keeps every row; 1000 drops every row."""
    rs = np.random.RandomState(11)
    shape = (30, 30)
    return Case([_level(rs, shape, 3, rs.uniform(0.01, 0.99, 2700), fmt, stride=8, size=32)], _im(shape, 8, 1.3), 2048, min_size=min_size)


def min_size_largest_sort(fmt):
    """The same filter behind the largest sort: pre_nms 16384 on S, sixteen entries per K3 thread, about a third of them dropped."""
    rs = np.random.RandomState(15)
    return Case([_level(rs, S, 3, rs.uniform(0.01, 0.99, S[0] * S[1] * 3), fmt)], _im(S, 4, 1.3), 16384, min_size=8.)


def nms_on(post, fmt):
    """NMS at 0.7 over 600 selected rows with tied scores (multiples of 1/256); post_nms below (50) and above (600) the survivors."""
    rs = np.random.RandomState(12)
    shape = (20, 25)
    scores = np.round(rs.uniform(0.01, 0.99, 1500) * 256) / 256
    return Case([_level(rs, shape, 3, scores, fmt, stride=16, size=64, sigma=0.3)], _im(shape, 16), 600, post, nms_thresh=0.7)


# ---- batch and reuse ------------------------------------------------------------------------------------------------------------
def batch3(fmt):
    """Three images in one launch: frames 1, 3, 5 of 6-frame heads (frame 1, frame_stride 2), two levels, batch_idx 4, and three
    im_info rows that differ in height, width and scale (clip bounds and min_size * scale per image)."""
    rs = np.random.RandomState(13)
    lv = [_level(rs, (20, 24), 3, np.round(rs.uniform(0.01, 0.99, (6, 1440)) * 512) / 512, fmt, stride=8, size=32, frames=6, frame=1),
          _level(rs, (10, 12), 3, np.round(rs.uniform(0.01, 0.99, (6, 360)) * 512) / 512, fmt, stride=16, size=64, frames=6, frame=1)]
    im_info = [[160., 192., 1.0], [150., 180., 1.2], [120., 192., 0.9]]
    return Case(lv, im_info, 300, min_size=16., batch_idx=4., n_images=3, frame_stride=2)


def mixed_levels(fmt):
    """A three-chunk level and a 700-anchor level in one launch: K0's blocks past the small level's end leave at once, and the small
    level's k_eff is its anchor count."""
    return Case([tie_cut(0.5, 700, fmt).levels[0], small700(fmt).levels[0]], _im(M, 4), 700, bites=('tie', 'cut'))


def small700(fmt):
    rs = np.random.RandomState(14)
    return Case([_level(rs, (10, 14), 5, np.round(rs.uniform(0.01, 0.99, 700) * 64) / 64, fmt, stride=16, size=32,
                        ratios=(0.25, 0.5, 1, 2, 4))], _im((10, 14), 16), 300, bites=('tie', 'cut'))


TIE_PRE = (1, 700, 1024, 1025)
TIE_V = {'even_bin': 0.5, 'odd_bin': 0.50390625}      # bins 0x3F00 and 0x3F01: the two halves of K0's packed counters
CASES = {
    'one_bin_distinct': one_bin_distinct,
    'full_chunk_one_bin': full_chunk_one_bin,
    'whole_boundary_bin': whole_boundary_bin,
    'k_eff_n': k_eff_n,
    'exact_zeros': exact_zeros,
    'sigmoid_path': functools.partial(sigmoid_path, 700),
    'sigmoid_zeros': functools.partial(sigmoid_path, 5000),
    'tubes_per_frame0': functools.partial(tubes, 0),
    'tubes_per_frame1': functools.partial(tubes, 1),
    'min_size_16': functools.partial(min_size_filter, 16.),
    'min_size_0': functools.partial(min_size_filter, 0.),
    'min_size_1000': functools.partial(min_size_filter, 1000.),
    'min_size_largest_sort': min_size_largest_sort,
    'mixed_levels': mixed_levels,
    'nms_post_50': functools.partial(nms_on, 50),
    'nms_post_600': functools.partial(nms_on, 600),
    'batch3': batch3,
    'small700': small700,
}
for _b, _v in TIE_V.items():
    for _p in TIE_PRE:
        CASES['tie_cut_%s_%d' % (_b, _p)] = functools.partial(tie_cut, _v, _p)
FP32_CASES = sorted(CASES)
CASES['head16'] = head16


@functools.lru_cache(maxsize=None)
def build(name, fmt='fp32'):
    """The case `name` (heads rounded to `fmt` where a case has a 16-bit head) -- built once, shared and never modified."""
    case = CASES[name](fmt)
    for head, _ in case.levels:
        head.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def reference(name, fmt='fp32'):
    return build(name, fmt).reference()


# ---- collect --------------------------------------------------------------------------------------------------------------------
def collect_inputs(counts, cap=40, cols=5, seed=21):
    """Per-level outputs as rpn_emit_kernel leaves them: counts [n_images, 5]; probabilities descending per level and drawn from
    sixteen values, so that levels share them; rows past a level's count hold junk that must not be read."""
    rs = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int32).reshape(-1, 5)
    ni = counts.shape[0]
    rois = rs.uniform(0, 300, (ni, 5, cap, cols)).astype(F32)
    probs = np.full((ni, 5, cap), 2.0, F32)            # junk above every real probability
    for i in range(ni):
        for l in range(5):
            c = counts[i, l]
            probs[i, l, :c] = -np.sort(-(rs.randint(1, 17, c) / 16.0)).astype(F32)
    return rois, probs, counts


# ---- detection select and limit --------------------------------------------------------------------------------------------------
DET_H, DET_W = 720, 1280
DET_WEIGHTS = (10., 10., 5., 5.)
DET_THRESH = F32(0.05)


def det_clustered(seed, R, cap, K, scale):
    """Proposals around twelve centres, softmax scores, zero size deltas (the decode has no exp: NumPy states it bit for bit)."""
    rs = np.random.RandomState(seed)
    centres = np.stack([rs.uniform(100, DET_W * scale - 300, 12), rs.uniform(100, DET_H * scale - 300, 12)], axis=1)
    xy = centres[rs.randint(0, 12, cap)] + rs.uniform(-40, 40, (cap, 2))
    wh = rs.uniform(60, 260, (cap, 2))
    rois = np.zeros((cap, 5), F32)
    rois[:, 1:3] = xy
    rois[:, 3:5] = xy + wh
    logits = rs.randn(cap, K).astype(F32) * 2
    prob = (np.exp(logits) / np.exp(logits).sum(axis=1, keepdims=True)).astype(F32)
    pred = (rs.randn(cap, K * 4) * np.tile([1.0, 1.0, 0.0, 0.0], K)).astype(F32)
    return rois, prob, pred


def det_grid(R, cap, K, seed=31):
    """R boxes of 4 pixels on a grid of pitch 8 (no two overlap, so the NMS keeps every selected row), zero size deltas; scores
    uniform in (0.1, 0.9) for every class.  Callers overwrite scores."""
    rs = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(cap)))
    assert side * 8 < DET_H
    i = np.arange(cap)
    rois = np.zeros((cap, 5), F32)
    rois[:, 1], rois[:, 2] = 8 * (i % side), 8 * (i // side)
    rois[:, 3], rois[:, 4] = rois[:, 1] + 3, rois[:, 2] + 3
    prob = rs.uniform(0.1, 0.9, (cap, K)).astype(F32)
    pred = (rs.randn(cap, K * 4) * np.tile([1.0, 1.0, 0.0, 0.0], K)).astype(F32)
    return rois, prob, pred


def det_reference(rois, prob, pred, K, D, scale, image=0):
    """oracle.box_results on the host: (dets [n, 6] = box, score, class in class-major order, keypoint rois [n, 5])."""
    from oracle import box_results as obr
    scores, boxes = obr.read_bbox_outputs(rois, prob, pred, scale, (DET_H, DET_W, 3), DET_WEIGHTS)
    s, b, cls = obr.box_results_with_nms_and_limit(scores, boxes, K, DET_THRESH, 0.5, D)
    col = np.concatenate([np.full((len(cls[j]),), j, F32) for j in range(1, K)])
    dets = np.hstack((b, s[:, None], col[:, None])).astype(F32)
    kp = obr.get_rois_blob(b, scale)
    kp[:, 0] = image
    return dets, kp
