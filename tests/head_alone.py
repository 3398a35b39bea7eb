"""Test-side helper of tests/test_gpu_batch_invariance.py: run the head of a net on ONE image's RoI features of a B-image forward.

After a forward of B images the workspace holds the `RoIFeatureTransform` outputs of all of them: B equal row segments with one live count
per image.  `run_head_alone` copies image i's segment into a forked workspace (same parameters and packed layers, its own blobs) as a
per-RoI blob with ONE count, and runs the net's remaining ops with `workspace.Executor`'s own `op_*` methods -- the code a forward of that
image alone runs, on bit-identical inputs.  `compare_head` then holds image i's rows of every head blob of the B-image forward to it."""
import torch

from detectandtrack_amd.workspace import Blob, Executor


def _row_axis(b):
    return 2 if b.kind == 'rows' else 0


def head_ops(net):
    """(index of the first RoIFeatureTransform, the ops behind it that are no RoIFeatureTransform)"""
    first = min(i for i, op in enumerate(net.ops) if op.type == 'RoIFeatureTransform')
    return first, [(i, op) for i, op in enumerate(net.ops) if i > first and op.type != 'RoIFeatureTransform']


def run_head_alone(ws, net, image, n_images):
    """The forked workspace after the head of `net` ran on image `image`'s RoI features alone."""
    one = ws.fork()
    first, ops_ = head_ops(net)
    made = set()
    for op in net.ops[first:]:
        if op.type != 'RoIFeatureTransform':
            continue
        b = ws.blobs[op.outputs[0]]
        assert b.kind == 'fmap' and b.roi and isinstance(b.count, torch.Tensor) and b.count.numel() == n_images, (op.outputs[0], b.count)
        assert b.t.shape[0] % n_images == 0 and b.N % n_images == 0
        seg = b.t.shape[0] // n_images
        a = Blob(b.t[image * seg:(image + 1) * seg].clone(), 'fmap', b.N // n_images, b.T, b.C, b.dt, b.five_d)
        a.count, a.roi = b.count.reshape(-1)[image:image + 1].clone(), True
        one.blobs[op.outputs[0]] = a
        made.add(op.outputs[0])
    ex = Executor(one, net)
    ex._plan_rpn_siblings()
    ex._plan_keyframe_dce()
    for i, op in ops_:
        assert i not in ex._skip and i not in ex._fused, 'op %d (%s) of the head is part of a fused RPN launch' % (i, op.type)
        assert all(n in made for n in op.inputs), 'op %d (%s) reads %r, which the head did not make' % (i, op.type, list(op.inputs))
        getattr(ex, 'op_' + op.type)(i, op)
        made.update(op.outputs)
    return one


def compare_head(ws, one, net, image, n_images, skip=()):
    """Names of the head blobs whose rows of image `image` in the B-image forward are NOT bit-equal to the head-alone run; the live rows
    (the image's count) of every blob the head's ops write are compared, up to the blob's real channels.  Returns (differing, compared)."""
    first, ops_ = head_ops(net)
    differing, compared = [], []
    for i, op in ops_:
        for name in op.outputs:
            if name in skip:
                continue
            b, a = ws.blobs[name], one.blobs[name]
            assert b.kind == a.kind and a.t.dtype == b.t.dtype, name
            ax = _row_axis(b)
            n_a = a.t.shape[ax]
            assert b.t.shape[ax] == n_a * n_images, (name, tuple(b.t.shape), tuple(a.t.shape))
            tb = b.t.narrow(ax, image * n_a, n_a)
            ta = a.t
            # live rows: the image's count of RoIs x the rows a RoI has in this blob (a GroupNorm over a per-RoI blob leaves the rows
            # behind the count unwritten)
            feat = one.blobs[net.ops[first].outputs[0]]
            cnt, rois = int(feat.count.reshape(-1)[0].item()), feat.N
            assert cnt > 0 and n_a % rois == 0, (name, cnt, n_a, rois)
            if b.count is not None:
                assert a.count is not None and int(b.count.reshape(-1)[image].item()) == int(a.count.reshape(-1)[0].item()) == cnt, name
            live = cnt * (n_a // rois)
            tb, ta = tb.narrow(ax, 0, live), ta.narrow(ax, 0, live)
            if b.kind in ('fmap', 'rows') and b.C:
                tb, ta = tb[..., :b.C], ta[..., :b.C]
            tb, ta = tb.contiguous(), ta.contiguous()
            it = torch.int16 if tb.element_size() == 2 else torch.int32
            compared.append(name)
            if not torch.equal(tb.view(it), ta.view(it)):
                differing.append(name)
    return differing, compared
