"""The rules `detectandtrack_amd/train_plan.py` replaced, restated from the text of `TrainExecutor._take_grad` and
`TrainExecutor.bwd_Conv` as they stood before the split (NOT from the new plan), and the facts tests/test_conv_bwd_plan_cpu.py
enumerates.  CPU tensors of the smallest legal shapes stand for the blobs.
"""
import itertools

import torch

from detectandtrack_amd.ops import hip_ops as ops
from detectandtrack_amd.train_plan import ConvBwdFacts, Entry


# ---- the parent's _take_grad ---------------------------------------------------------------------------------------------------------
def parent_take_grad(lst, dtype):
    """lst: [(tensor, first frame, masked)], a RoIAlign accumulator marked by `t._roi_acc = True` -> (dy, lo, last_masked)."""
    last_masked = False
    if not lst:
        return None, 0, last_masked
    tdt = ops.tdtype(dtype)
    last_masked = len(lst) == 1 and lst[0][2]
    assert not any(m for _, _, m in lst) or len(lst) == 1, 'a masked gradient must be the only contribution to %r' % 'x'
    lo = min(l for _, l, _ in lst)
    hi = max(l + t.shape[0] for t, l, _ in lst)
    if len(lst) == 1:
        t, l, _ = lst[0]
        return (t if t.dtype == tdt else t.to(tdt)), l, last_masked
    full = [e for e in lst if e[0].shape[0] == hi - lo and not getattr(e[0], '_roi_acc', False)]
    first = next((e for e in full if e[0].dtype == tdt), None)
    acc = None
    if first is not None:
        second = next((e for e in full if e is not first and e[0].shape == first[0].shape), None)
        if second is not None:
            acc = torch.add(first[0], second[0]) if second[0].dtype == tdt else torch.add(first[0], second[0]).to(tdt)
            lst = [e for e in lst if e is not first and e is not second]
        else:
            acc = first[0].clone()
            lst = [e for e in lst if e is not first]
    if acc is None:
        acc = torch.zeros((hi - lo,) + tuple(lst[0][0].shape[1:]), dtype=tdt, device=lst[0][0].device)
    for t, l, _ in lst:
        acc[l - lo:l - lo + t.shape[0]] += t if t.dtype == tdt else t.to(tdt)
    return acc, lo, last_masked


def take_branch(lst, dtype):
    """Which branch of the rule a contribution list exercises (the test requires every one)."""
    tdt = ops.tdtype(dtype)
    if len(lst) == 1:
        return 'single' if lst[0][0].dtype == tdt else 'single cast'
    lo = min(l for _, l, _ in lst)
    hi = max(l + t.shape[0] for t, l, _ in lst)
    full = [e for e in lst if e[0].shape[0] == hi - lo and not getattr(e[0], '_roi_acc', False)]
    first = next((e for e in full if e[0].dtype == tdt), None)
    if first is None:
        return 'zero start, union' if all(e[0].shape[0] < hi - lo for e in lst) else 'zero start'
    return 'pair' if any(e is not first and e[0].shape == first[0].shape for e in full) else 'clone start'


# ---- the parent's bwd_Conv ------------------------------------------------------------------------------------------------------------
def _overlap(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


FRESH = None        # stands for a tensor a launch of the step allocates: it cannot overlap one that is alive already


def parent_conv_bwd(f):
    """The parent's body, launches replaced by what they return (FRESH or the tensor they pass through) -> the decision tuple
    (need_relu, bias target, zero padding, residual route, ilo, ihi, embedded, Tw, g_frames, weight route, data route, inplace)."""
    a, dy, lo = f.args, f.dy, f.lo
    assert not f.x_t2c and f.y_keyframe is None, 'training with time->channel heads / key-frame DCE is not supported'
    n = dy.shape[0]
    full = (lo == 0 and n == f.y_frames)
    assert full or f.x_N == 1, 'frame-window gradients assume one clip per forward (TRAIN.IMS_PER_BATCH 1)'
    cout = a['dim_out']
    train_b = a['b'] if (a['b'] and f.train_b) else None
    dbias = None
    if train_b:
        dbias = 'arena' if f.b_in_arena else 'temp'
    need_relu = bool(a['relu']) and not f.masked
    zero_pad = False
    if need_relu or dbias is not None:
        # relu_bias_bwd: only the bias reduction runs, and the gradient tensor is dy itself, when there is nothing to mask and no padding
        g = dy if (not need_relu and cout == dy.shape[-1] and dy.is_contiguous()) else FRESH
    else:
        g = dy
        if cout != dy.shape[3]:
            zero_pad = True
    residual = None
    if a['residual']:
        residual = 'upsample' if a['res_mode'] == 2 else 'same'
    pt = a['pads'][0]
    T = f.x_T if f.x_N == 1 else f.x.shape[0]
    ilo, ihi = (max(0, lo - pt), min(T, lo + n + pt)) if f.x_N == 1 else (0, f.x.shape[0])
    x_win = f.x[ilo:ihi]
    embedded = (ilo, ihi) != (lo, lo + n)
    g_emb = FRESH if embedded else g
    Tw = (ihi - ilo) if f.x_N == 1 else f.x_T
    gfr = (lo - ilo, n) if f.x_N == 1 else None
    pending = list(f.queued)
    wroute = 'none'
    if f.train_w:
        gt = (f.w_in_gt_arena and f.w_in_arena) or None
        if f.w_sealed:
            raise RuntimeError('gradient contribution to %r after its bucket was handed to the all-reduce (static completion index '
                               'of the parameter is wrong)' % a['w'])
        frames, H, W, _ = x_win.shape
        job = None
        if gt is not None and f.pointwise and f.pw_batch > 0:
            if f.groups == 1 and f.acc_direct(frames, Tw, H, W, gfr):        # weight_acc_job
                job = (x_win if x_win.is_contiguous() else FRESH, g_emb)
        if job is not None:
            wroute = 'queue'
            pending.append(job)
            if len(pending) >= f.pw_batch:
                pending = []
        elif gt is not None and (f.groups > 1 or f.acc_direct(frames, Tw, H, W, gfr)):       # weight_acc
            wroute = 'acc'
        else:
            wroute = 'immediate'
    droute, inplace = 'none', True
    if not f.in_no_grad:
        _, H, W, _ = f.x.shape
        into = None
        pend = list(f.waiting)
        if pend and len(pend) == 1:
            t0, l0, m0, roi0 = pend[0]
            assert not m0, 'a ReLU-masked gradient is the ONLY contribution of its blob (one reader): nothing may be added into it'
            if l0 == ilo and t0.shape[0] == ihi - ilo and t0.dtype == ops.tdtype(f.y_dt) and tuple(t0.shape[1:3]) == (H, W) and \
                    t0.is_contiguous() and not roi0 and t0.shape[3] == ops.round_up(f.cin, 64):
                into = t0
        mask = None
        prod = f.producer
        if (into is None and f.fuse_relu and prod is not None and prod[0] == 'Conv' and prod[1] and f.readers == 1 and
                not pend and f.x_keyframe is None and not f.x_t2c and f.x.shape[3] == ops.round_up(f.cin, 64)):
            mask = x_win if x_win.is_contiguous() else None
        held = into is not None and any((j[0] is not FRESH and _overlap(into, j[0])) or (j[1] is not FRESH and _overlap(into, j[1]))
                                        for j in pending)
        if (into is not None and f.groups == 1 and f.fuse_relu and f.fuse_relu_sum and f.sum_env and prod is not None and
                prod[0] == 'Conv' and prod[1] and f.readers == 2 and f.ncontrib == 1 and f.x_keyframe is None and not f.x_t2c and
                x_win.is_contiguous() and tuple(x_win.shape) == tuple(into.shape) and x_win.dtype == into.dtype):
            mask = x_win
        inplace = not held
        if into is None:
            droute = 'mask' if mask is not None else 'plain'
        else:
            droute = 'sum_mask' if mask is not None else 'sum'
    return (need_relu, dbias, zero_pad, residual, ilo, ihi, embedded, Tw, gfr, wroute, droute, inplace)


# ---- the facts the plan test enumerates ------------------------------------------------------------------------------------------------
T, HW = 4, 2
TDT = ops.tdtype(ops.BF16)

KERNELS = (     # (kT, kHW, stride, temporal pad)
    (1, 1, 1, 0), (1, 1, 2, 0), (1, 3, 1, 0), (1, 3, 2, 0), (3, 3, 1, 1), (3, 3, 1, 0))
AXES = dict(
    kernel=KERNELS, groups=(1, 32), window=('full', 'partial'), N=(1, 2), readers=(1, 2, 4), ncontrib=(0, 1, 2),
    producer=(('Conv', True), ('Conv', False), ('SpatialBN', True), None),
    waiting=('empty', 'match', 'window', 'dtype', 'hw', 'cstride', 'noncontig', 'roi', 'two'), held=(False, True),
    fuse_relu=(True, False), fuse_relu_sum=(True, False), sum_env=(True, False), train_w=(True, False), train_b=(True, False),
    arena=(True, False), gt_arena=(True, False), pw_batch=(0, 16), sealed=(False, True), in_no_grad=(False, True),
    cout_is_stride=(True, False), cin_is_stride=(True, False), relu=(True, False), masked=(False, True),
    residual=(None, 'same', 'upsample'), acc_direct=(True, False), queue_len=(0, 15))
NAMES = tuple(AXES)
_x_cache = {}


def _x(frames, cs):
    if (frames, cs) not in _x_cache:
        _x_cache[(frames, cs)] = torch.zeros(frames, HW, HW, cs, dtype=TDT)
    return _x_cache[(frames, cs)]


def facts(c):
    """One point of the product (a dict over AXES) -> ConvBwdFacts."""
    kt, k, stride, pt = c['kernel']
    cin = 64 if c['cin_is_stride'] else 24
    cout = 64 if c['cout_is_stride'] else 60
    x = _x(c['N'] * T, 64 if c['cin_is_stride'] else 24)
    Ty = T + 2 * pt - (kt - 1)
    y_frames = c['N'] * Ty
    lo, n = (0, y_frames) if c['window'] == 'full' else (1, 1)
    ho = HW // stride
    dy = torch.zeros(n, ho, ho, 64, dtype=TDT)
    if c['N'] == 1:
        ilo, ihi = max(0, lo - pt), min(T, lo + n + pt)
    else:
        ilo, ihi = 0, x.shape[0]
    cs = ops.round_up(cin, 64)
    shape = (ihi - ilo, HW, HW, cs)
    w = c['waiting']
    match = torch.zeros(shape, dtype=TDT)
    waiting = {
        'empty': (), 'match': (Entry(match, ilo, False, False),), 'window': (Entry(match, ilo + 1, False, False),),
        'dtype': (Entry(torch.zeros(shape, dtype=torch.float32), ilo, False, False),),
        'hw': (Entry(torch.zeros(shape[0], HW + 1, HW, cs, dtype=TDT), ilo, False, False),),
        'cstride': (Entry(torch.zeros(shape[:3] + (2 * cs,), dtype=TDT), ilo, False, False),),
        'noncontig': (Entry(torch.zeros(shape[:3] + (2 * cs,), dtype=TDT)[..., ::2], ilo, False, False),),
        'roi': (Entry(match, ilo, False, True),),
        'two': (Entry(match, ilo, False, False), Entry(torch.zeros(shape, dtype=TDT), ilo, False, False)),
    }[w]
    # the queue: `queue_len` jobs on tensors of their own; held: one of them reads a view of the waiting tensor's storage
    queued = [(torch.zeros(1, dtype=TDT), torch.zeros(1, dtype=TDT)) for _ in range(c['queue_len'])]
    if c['held']:
        queued = queued[:-1] if queued else queued
        queued.append((torch.zeros(1, dtype=TDT), match.view(-1)[8:]))       # (a second live tensor over the same storage, offset)
    args = {'dim_out': cout, 'relu': c['relu'], 'b': 'b', 'w': 'w', 'residual': {None: None, 'same': 'res', 'upsample': 'res'}[c['residual']],
            'res_mode': 2 if c['residual'] == 'upsample' else 1, 'pads': (pt, k // 2, k // 2), 'strides': (stride, stride)}
    return ConvBwdFacts(
        args=args, train_w=c['train_w'], train_b=c['train_b'], w_in_arena=c['arena'], b_in_arena=c['arena'],
        w_in_gt_arena=c['arena'] and c['gt_arena'], w_sealed=c['sealed'], pw_batch=c['pw_batch'] if (c['arena'] and c['gt_arena']) else 0,
        dy=dy, lo=lo, masked=c['masked'], y_frames=y_frames, y_dt=ops.BF16, y_keyframe=None, src='x', x=x, x_N=c['N'], x_T=T, x_t2c=False,
        x_keyframe=None, waiting=waiting, ncontrib=c['ncontrib'], readers=c['readers'], producer=c['producer'],
        in_no_grad=c['in_no_grad'], fuse_relu=c['fuse_relu'], fuse_relu_sum=c['fuse_relu_sum'], sum_env=c['sum_env'],
        pointwise=(c['groups'] == 1 and kt == 1 and k == 1), groups=c['groups'], cin=cin,
        acc_direct=lambda frames, Tw, H, W, g_frames, ans=c['acc_direct']: ans, queued=queued)


def product(names):
    """Every point of the product of the axes `names`, the others at their first value."""
    base = {k: v[0] for k, v in AXES.items()}
    for vals in itertools.product(*(AXES[k] for k in names)):
        yield dict(base, **dict(zip(names, vals)))


def sample(rng, count):
    """`count` points drawn uniformly from the product of ALL axes."""
    for _ in range(count):
        yield {k: v[rng.randrange(len(v))] for k, v in AXES.items()}
