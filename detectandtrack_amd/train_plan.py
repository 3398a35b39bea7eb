"""What the training backward decides before it launches: the gradient ledger (who contributed which gradient to which blob) and the
plan of one conv op's backward (`plan_conv_bwd`: every decision of `TrainExecutor.bwd_Conv` as a pure function of plain facts).
Nothing here launches a kernel; tests/test_conv_bwd_plan_cpu.py holds both to the rules they replaced.
"""
import collections

import torch

from detectandtrack_amd.ops import hip_ops as ops

# One gradient contribution to a blob: `t` covers frames [lo, lo + t.shape[0]) of the blob (everything else is exactly zero); masked: the
# ReLU backward of the blob's producer is already applied to `t` (fused into the data-gradient conv that made it) -- the flag travels
# WITH the entry, not in a side table keyed by id(tensor); roi_acc: the fp32 accumulator of the RoIAlign backward.
Entry = collections.namedtuple('Entry', 't lo masked roi_acc')


def check_one_clip(ok, what='frame-window gradients assume', hint=False):
    """A gradient that covers a window of frames (or a head over time moved to channels) presumes ONE clip per forward."""
    assert ok, '%s one clip per forward%s' % (what, ' (TRAIN.IMS_PER_BATCH 1)' if hint else '')


def sealed_error(name):
    return RuntimeError('gradient contribution to %r after its bucket was handed to the all-reduce (static completion index '
                        'of the parameter is wrong)' % name)


class GradLedger(object):
    """The gradient contributions that wait for each blob during one backward pass.

    A gradient of a T-frame feature map may cover only a WINDOW of frames [lo, lo + n): with BODY_HEAD_LINK 'slice-center' the heads read
    one frame, so the FPN post-hoc convs (60 % of the forward FLOPs) receive a 1-frame gradient and hand a 3-frame gradient down; each
    kT = 3 conv widens the window by its temporal reach."""

    def __init__(self):
        self._entries = {}      # blob name -> [Entry]
        self._count = {}        # blob name -> contributions received so far (an entry may be the sum of several)

    def add(self, name, t, lo=0, masked=False):
        self._entries.setdefault(name, []).append(Entry(t, lo, bool(masked), False))
        self._count[name] = self._count.get(name, 0) + 1

    def waiting(self, name):
        """The entries that wait for `name` (a copy: read only)."""
        return tuple(self._entries.get(name, ()))

    def contributions(self, name):
        return self._count.get(name, 0)

    def summed_into(self, name, result, masked):
        """A data-gradient epilogue added its contribution to the ONE entry that waited for `name`: `result` is that entry's tensor
        (summed in place) or the new tensor that now holds the sum; masked: the epilogue also applied the producer's ReLU backward."""
        (e,) = self._entries[name]
        self._entries[name] = [Entry(result, e.lo, bool(masked), False)]
        self._count[name] = self._count.get(name, 0) + 1

    def move(self, src, dst):
        """The entries of `src` now wait for `dst` (Alias, TimeToBatch, BatchToTime: views of the same values).  They are not counted as
        contributions of `dst`: the count is what the conv fusions compare with the blob's readers, and a view is not one of them."""
        if src in self._entries:
            self._entries.setdefault(dst, []).extend(self._entries.pop(src))
        self._count.pop(src, None)

    def roi_accumulator(self, name, shape, device):
        """The fp32 accumulator the RoIAlign backward adds into for feature map `name`: the one that already waits, or a new zeroed one."""
        acc = None
        for e in self._entries.get(name, ()):
            if e.roi_acc and e.t.dtype == torch.float32:
                acc = e.t
        if acc is None:
            acc = torch.zeros(shape, dtype=torch.float32, device=device)
            self._entries.setdefault(name, []).append(Entry(acc, 0, False, True))
            self._count[name] = self._count.get(name, 0) + 1
        return acc

    def clear(self):
        self._entries.clear()
        self._count.clear()

    def take(self, name, dtype):
        """-> (dy, lo, masked): dy in the activation dtype covering frames [lo, lo + dy.shape[0]), or (None, 0, False).  masked: the
        gradient already carries the ReLU mask of `name`'s producer (a single, masked contribution)."""
        lst = self._entries.pop(name, None)
        self._count.pop(name, None)
        if not lst:
            return None, 0, False
        tdt = ops.tdtype(dtype)
        assert not any(e.masked for e in lst) or len(lst) == 1, 'a masked gradient must be the only contribution to %r' % name
        if len(lst) == 1:
            e = lst[0]
            return (e.t if e.t.dtype == tdt else e.t.to(tdt)), e.lo, e.masked
        lo = min(e.lo for e in lst)
        hi = max(e.lo + e.t.shape[0] for e in lst)
        # the sum starts as ONE out-of-place add of two full-window contributions (no clone + add pair).  (Adding the fp32 accumulators of
        # the RoIAlign backward without the .to() pass -- a mixed-dtype in-place add -- measured slower: ATen's casting kernel is not vectorised.)
        full = [e for e in lst if e.t.shape[0] == hi - lo and not e.roi_acc]
        first = next((e for e in full if e.t.dtype == tdt), None)
        acc = None
        if first is not None:
            second = next((e for e in full if e is not first and e.t.shape == first.t.shape), None)
            if second is not None:
                acc = torch.add(first.t, second.t) if second.t.dtype == tdt else torch.add(first.t, second.t).to(tdt)
                lst = [e for e in lst if e is not first and e is not second]
            else:
                acc = first.t.clone()
                lst = [e for e in lst if e is not first]
        if acc is None:
            acc = torch.zeros((hi - lo,) + tuple(lst[0].t.shape[1:]), dtype=tdt, device=lst[0].t.device)
        for e in lst:
            acc[e.lo - lo:e.lo - lo + e.t.shape[0]] += e.t if e.t.dtype == tdt else e.t.to(tdt)
        return acc, lo, False


def bytes_overlap(a, b):
    """Do the memory extents of two (dense) tensors intersect?"""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


# ---- the backward of one conv op ---------------------------------------------------------------------------------------------------
# The facts `plan_conv_bwd` decides from (plain values and live tensors it only inspects):
#   args            the op's args (relu, b, w, residual, res_mode, pads, dim_out)
#   train_w/train_b the parameter is trainable;  w_in_arena/b_in_arena: it has a view in the gradient arena;  w_in_gt_arena: the weight has
#                   a deferred-finish accumulator;  w_sealed: its bucket is being exchanged
#   pw_batch        TrainExecutor._pw_batch (0: pointwise layers are not queued)
#   dy, lo, masked  the taken gradient, its first frame and its masked flag
#   y_frames, y_dt, y_keyframe      of the output blob
#   src, x          the input blob's name and tensor;  x_N, x_T, x_t2c, x_keyframe: the blob's fields
#   waiting, ncontrib, readers      the ledger's entries / contribution count of the input blob, and how many ops read it
#   producer        (type, relu) of the op that made the input blob, or None
#   in_no_grad      no gradient is computed for the input blob
#   fuse_relu, fuse_relu_sum, sum_env      cfg.HIP.FUSE_RELU_BWD, cfg.HIP.FUSE_RELU_SUM_BWD, DAT_FUSE_RELU_SUM_BWD
#   pointwise, groups, cin          of the layer's ConvGrad;  acc_direct: its `takes_acc` (asked only when the answer decides)
#   queued          the (x, g) operands of the pointwise weight-gradient jobs that wait for their grouped launch
ConvBwdFacts = collections.namedtuple('ConvBwdFacts', (
    'args train_w train_b w_in_arena b_in_arena w_in_gt_arena w_sealed pw_batch dy lo masked y_frames y_dt y_keyframe '
    'src x x_N x_T x_t2c x_keyframe waiting ncontrib readers producer in_no_grad fuse_relu fuse_relu_sum sum_env '
    'pointwise groups cin acc_direct queued'))

# relu_pass: the ReLU mask is still to be applied (relu_bias_bwd);  bias: where the bias reduction goes ('arena' view, 'temp', None);
# zero_pad: g aliases dy and its padding channels must be zeroed;  residual: None, 'same' (g itself) or 'upsample' (upsample2x_bwd);
# (ilo, ihi): the input frames the window reaches;  embed: g is embedded in zeros over them;  Tw, g_frames: what the kernels are told;
# wgrad: 'none', 'queue', 'acc', 'immediate';  dgrad: 'none', 'plain', 'sum', 'mask', 'sum_mask';  inplace: the sum may overwrite the
# waiting contribution
ConvBwdPlan = collections.namedtuple('ConvBwdPlan', 'relu_pass bias zero_pad residual ilo ihi embed Tw g_frames wgrad dgrad inplace')


def plan_conv_bwd(f):
    a, lo, n, x = f.args, f.lo, f.dy.shape[0], f.x
    assert not f.x_t2c and f.y_keyframe is None, 'training with time->channel heads / key-frame DCE is not supported'
    # (the residual's contribution is added while the plan is carried out: what waits for the input is judged as it is now)
    assert not a['residual'] or a['residual'] != f.src, 'a conv whose residual is its own input (%r): no model builds one' % (f.src,)
    check_one_clip((lo == 0 and n == f.y_frames) or f.x_N == 1, hint=True)
    cout = a['dim_out']
    # the kernel ACCUMULATES the bias reduction: straight into the (zeroed) arena view when there is one
    bias = ('arena' if f.b_in_arena else 'temp') if (a['b'] and f.train_b) else None
    # (the mask may already be in dy: the data-gradient conv of this blob's only reader applied it in its epilogue)
    relu_pass = bool(a['relu']) and not f.masked
    # without a pre-pass g ALIASES dy (no ReLU to mask by, no trainable bias to reduce into -- the shortcut convs: AffineChannelNd has no
    # gradient; it may also be queued as the residual's gradient): everything downstream reads whole channel strides, so the padding
    # channels [cout, stride) must be zero -- they are when dy came out of a conv epilogue or relu_bias_bwd of a layer with
    # cout == stride; make it so otherwise instead of trusting the producer
    zero_pad = not relu_pass and bias is None and cout != f.dy.shape[3]
    residual = None if not a['residual'] else ('upsample' if a['res_mode'] == 2 else 'same')
    # frames of the input this gradient window reaches through the temporal taps
    pt = a['pads'][0]
    one = f.x_N == 1
    ilo, ihi = (max(0, lo - pt), min(f.x_T, lo + n + pt)) if one else (0, x.shape[0])
    Tw = (ihi - ilo) if one else f.x_T
    g_frames = (lo - ilo, n) if one else None
    embed = (ilo, ihi) != (lo, lo + n)
    wgrad = 'none'
    if f.train_w:
        if f.w_sealed:
            raise sealed_error(a['w'])      # the bucket of this weight is already being exchanged
        frames, H, W, _ = x.shape
        if not (f.w_in_arena and f.w_in_gt_arena):
            wgrad = 'immediate'
        elif f.groups > 1:      # the grouped accumulating kernel takes every grouped layer; never queued into the pointwise batch
            wgrad = 'acc'
        elif not f.acc_direct(ihi - ilo, Tw, H, W, g_frames):
            wgrad = 'immediate'
        else:
            # pointwise layers: queued, and run as ONE grouped launch per gradient bucket / per `WGRAD_PW_BATCH` layers (a layer launched
            # alone is split over all CUs and adds 64 MB of partial tiles with float atomics; a shared grid a tenth of that)
            wgrad = 'queue' if (f.pointwise and f.pw_batch > 0) else 'acc'
    dgrad, inplace = 'none', True
    if not f.in_no_grad:
        _, H, W, _ = x.shape
        x_win = x[ilo:ihi]
        dense = x.shape[3] == ops.round_up(f.cin, 64)
        relu_conv = f.producer is not None and f.producer[0] == 'Conv' and bool(f.producer[1])
        # a gradient of the same frame window that already waits for this input (the block's shortcut): the data-gradient conv
        # adds into it in its epilogue instead of producing a second tensor for an ATen add
        into = None
        if len(f.waiting) == 1:
            e = f.waiting[0]
            assert not e.masked, 'a ReLU-masked gradient is the ONLY contribution of its blob (one reader): nothing may be added into it'
            if e.lo == ilo and e.t.shape[0] == ihi - ilo and e.t.dtype == ops.tdtype(f.y_dt) and tuple(e.t.shape[1:3]) == (H, W) and \
                    e.t.is_contiguous() and not e.roi_acc and e.t.shape[3] == ops.round_up(f.cin, 64):
                into = e.t
        # ReLU backward of the input blob fused into this launch's epilogue: x = relu(...) is read by this conv only, its
        # gradient has this one contribution, and its producer is a conv this executor differentiates
        mask = (into is None and f.fuse_relu and relu_conv and f.readers == 1 and not f.waiting and f.x_keyframe is None and
                not f.x_t2c and dense and x_win.is_contiguous())
        # a queued pointwise weight gradient may still have to READ the tensor the sum would be written into (the block output's gradient
        # is both branch2c's `g` and the shortcut contribution of the block input): then the sum goes to a new tensor
        # (byte-range overlap with BOTH operands of every queued job -- an offset view or the x operand would have slipped past
        #  an equality test of the g operand's start pointer)
        # By the time the data gradient runs this layer's own job is queued too, or its arrival has flushed the queue.  Of its operands
        # only dy (g without a ReLU pass or embedding may be dy itself) and the input window can be a tensor that waits already.
        queued = list(f.queued)
        if wgrad == 'queue':
            own = (x_win if x_win.is_contiguous() else None, f.dy if not (relu_pass or embed) else None)
            queued = [] if len(queued) + 1 >= f.pw_batch else queued + [own]
        if into is not None:
            inplace = not any(bytes_overlap(into, t) for job in queued for t in job if t is not None)
        # ... and when this conv is the LAST of the blob's readers to contribute (a residual block's output: read by the next block's
        # first conv and by its shortcut), the same epilogue applies the ReLU backward of the blob's producer to the finished sum
        # (dat_conv3d_fwd_sum_mask, round 6): that producer's elementwise mask pass (three passes over the block output) goes
        # (grouped layers have no sum + mask instantiation; a `branch2b` input has one reader, so the case does not arise for them)
        if (into is not None and f.groups == 1 and f.fuse_relu and f.fuse_relu_sum and f.sum_env and relu_conv and f.readers == 2 and
                f.ncontrib == 1 and f.x_keyframe is None and not f.x_t2c and x_win.is_contiguous() and
                tuple(x_win.shape) == tuple(into.shape) and x_win.dtype == into.dtype):
            mask = True
        dgrad = ('sum_mask' if mask else 'sum') if into is not None else ('mask' if mask else 'plain')
    return ConvBwdPlan(relu_pass, bias, zero_pad, residual, ilo, ihi, embed, Tw, g_frames, wgrad, dgrad, inplace)
