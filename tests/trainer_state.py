"""Helpers of tests/test_gpu_trainer_state.py: the state that lives between the kernels while a model trains.

After every `Trainer.step` the fp32 masters move and everything derived from them has to move too: packed weight images of forward and
data-gradient layers, padded bias copies, layers built from concatenated / permuted / sub-pixel weights.  `resume_report` trains a
shrunk copy of a shipped training configuration for a few steps (trainer A), writes a checkpoint the way tools/train_net.py does, loads
it into a fresh workspace and Trainer (B) and compares, bit for bit, the masters and momentum, every blob of the next forward and every
field of every layer object of the two workspaces.  `update_rule_report` drives `Trainer.step` through a learning-rate schedule and
holds the flat weight / momentum buffers to the reference's update rule in float64, parameter by parameter.

Every helper RETURNS its findings (lists of strings / tuples that name the parameter, blob or layer field); the tests assert on them, so
that the controls of the test module can assert that a planted defect is reported.
"""
import collections
import os
import time

import numpy as np
import torch

from tests import numerics as nm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 128, 160

# case id -> (yaml under configs/, config overrides on top of the common shrink)
CASES = collections.OrderedDict([
    ('train_r18_fpn3d', ('train_r18_fpn3d_synthetic.yaml', {})),
    ('train_r18_fpn3d-fp32', ('train_r18_fpn3d_synthetic.yaml', {'HIP': {'DTYPE': 'fp32'}})),
    ('train_r18_c4_tube', ('train_r18_c4_tube_synthetic.yaml', {})),
    # the reference default keypoint deconv over time moved to channels (group = T), as test_c4_tube_train_step_gradients_match_oracle_autograd
    ('train_r18_c4_tube-deconv_t2c', ('train_r18_c4_tube_synthetic.yaml', {'KRCNN': {'NO_3D_DECONV_TIME_TO_CH': False}})),
    ('train_r18_fpn3d_tube', ('train_r18_fpn3d_tube_synthetic.yaml', {})),
    ('train_r18_2plus1d_fpn3d_bn', ('train_r18_2plus1d_fpn3d_bn_synthetic.yaml', {})),
    ('train_r18_2plus1d_fpn3d_gn', ('train_r18_2plus1d_fpn3d_gn_synthetic.yaml', {})),
    ('train_r18_c4_tube_gn', ('train_r18_c4_tube_gn_synthetic.yaml', {})),
    ('train_r18_fpn3d_gn_kps_head', ('train_r18_fpn3d_gn_kps_head_synthetic.yaml', {})),
    ('train_r18_c5_dilated', ('train_r18_c5_dilated_synthetic.yaml', {})),
    ('train_x50_32x4d_fpn3d', ('train_x50_32x4d_fpn3d_synthetic.yaml', {})),
])
FPN3D, FPN3D_FP32 = 'train_r18_fpn3d', 'train_r18_fpn3d-fp32'
BN, GN = 'train_r18_2plus1d_fpn3d_bn', 'train_r18_2plus1d_fpn3d_gn'

# Forward blobs that are not bit-reproducible between two forwards of ONE workspace, by case id -> {blob name: reason}.  Conv, FC,
# deconv and norm outputs and the losses may never be listed here.
NOT_REPRODUCIBLE = {}

LAYER_FIELDS = ('packed', 'bias', 'scale', 'dgrad_scale', 'w_src')


def configure(case_id):
    """Load the case's yaml into the global cfg and shrink it the way the trainer tests shrink theirs.  Works without a GPU."""
    from detectandtrack_amd.core.config import cfg, cfg_from_file, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    fn, over = CASES[case_id]
    reset_cfg()
    cfg_from_file(os.path.join(REPO, 'configs', fn))
    # the smallest clip length the heads take: the C4 tube heads average / regroup over 3 frames, everything else runs on 2
    T = 3 if 'c4_tube' in fn else 2
    cfg_from_cfg({'TRAIN': {'RPN_PRE_NMS_TOP_N': 400, 'RPN_POST_NMS_TOP_N': 200, 'IMS_PER_BATCH': 1, 'MAX_SIZE': 160,
                            'BATCH_SIZE_PER_IM': 64, 'RPN_STRADDLE_THRESH': -1},
                  'NUM_GPUS': 1, 'VIDEO': {'NUM_FRAMES': T}})
    cfg_from_cfg(over)
    assert_and_infer_cfg()
    return cfg


def create_model(case_id):
    from detectandtrack_amd.modeling import model_builder
    cfg = configure(case_id)
    return model_builder.create(cfg.MODEL.TYPE, train=True)


# ---- which parameters train ------------------------------------------------------------------------------------------------------
def op_params(model, op):
    """Names of the model parameters an op's arguments mention."""
    a = op.args if isinstance(op.args, dict) else {}
    return [v for v in a.values() if isinstance(v, str) and v in model.param_specs]


def params_without_gradient(model):
    """Parameters that only ops at or below the last StopGradient marker use (RESNETS.FREEZE_AT: conv1 / res2 and their affine, BN or GN
    pairs).  The reference builds no gradient for them, so `TrainableParams` (`p in self.param_to_grad`) leaves them out and
    `add_parameter_update_ops` never touches them: no update, no weight decay.  Derived from the op list alone."""
    net = model.net
    stops = [i for i, op in enumerate(net.ops) if op.type == 'StopGradient']
    last = stops[-1] if stops else -1
    below, above = set(), set()
    for i, op in enumerate(net.ops):
        (below if i <= last else above).update(op_params(model, op))
    return below - above


def expected_trainable(model):
    """What the reference updates: the model's trainable list (no AffineChannel pairs, no blacklisted or computed parameters) without
    the parameters that get no gradient."""
    frozen = params_without_gradient(model)
    return [n for n in model.TrainableParams() if n not in frozen]


# ---- one shrunk training case ------------------------------------------------------------------------------------------------------
class Case(object):
    """Model, one synthetic clip, its RPN labels and one fixed RoI sample shared by every workspace of the case."""

    def __init__(self, case_id):
        from detectandtrack_amd.core.config import cfg
        from detectandtrack_amd.utils import net as net_utils
        from detectandtrack_amd.roi_data import rpn as rpn_data, fast_rcnn as frcn_data, synthetic
        from tests.model_util import synthetic_clip
        self.id = case_id
        self.model = create_model(case_id)
        self.cfg = cfg
        T = cfg.VIDEO.NUM_FRAMES
        tube_T = cfg.VIDEO.NUM_FRAMES_MID if cfg.VIDEO.BODY_HEAD_LINK == '' else 1
        self.weights = net_utils.synthetic_params(self.model, 3)
        self.entry = synthetic.synthetic_roidb_entry(H, W, n_persons=3, seed=5, T=tube_T)
        self.data = synthetic_clip(T, H, W)
        rng = np.random.RandomState(0)
        self.labels = rpn_data.add_rpn_blobs({}, 1.0, self.entry, rng)
        fixed = self.fixed = {}
        entry = self.entry

        def sampler(rois, info):     # a fixed sample: successive iterations, and both workspaces, see the same objective
            if not fixed:
                fixed.update(frcn_data.sample_training_blobs(entry, rois, info, rng))
            return fixed
        self.sampler = sampler

    def workspace(self, params=None):
        """A fresh workspace (not the process-wide one: two live side by side), optionally holding `params`."""
        from detectandtrack_amd import workspace
        ws = workspace.Workspace(torch.cuda.current_device())
        for k, v in (params or {}).items():
            ws.set_param(k, v)
        return ws

    def feed(self, ws):
        ws.FeedBlob('data', self.data)
        for k, v in self.labels.items():
            ws.FeedBlob(k, v)
        ws.train_sampler = self.sampler

    def trainer(self, ws):
        from detectandtrack_amd.training import Trainer
        self.feed(ws)
        return Trainer(self.model, ws)

    def fed_names(self):
        return set(['data']) | set(self.labels)


# ---- bit comparison ----------------------------------------------------------------------------------------------------------------
def _bytes(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.uint8) if t.numel() else t


def bit_equal(a, b):
    """Same dtype, shape and bits (NaNs and signed zeros compare as bits)."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and bool(torch.equal(_bytes(a), _bytes(b)))


# ---- forward blobs -----------------------------------------------------------------------------------------------------------------
def forward_blobs(case, ws, ex):
    """name -> a copy of every blob the forward pass wrote (not the fed ones), the loss values and the accuracy counters of `ex` among
    them.  A row-counted blob gives its live rows (what FetchBlob returns): the rows behind the count are never written."""
    out = collections.OrderedDict()
    fed = case.fed_names()
    for name, b in ws.blobs.items():
        if name in fed or not isinstance(b.t, torch.Tensor):
            continue
        if b.count is not None:
            out[name] = np.array(ws.FetchBlob(name), copy=True)
        else:
            out[name] = b.t.detach().clone()
    for name, t in ex.losses.items():
        out['loss:' + name] = t.detach().clone()
    for name, (correct, _rows) in ex.metrics.items():
        out['metric:' + name] = correct.detach().clone()
    return out


def compare_blobs(a, b, skip=()):
    """Names of the blobs that differ between two `forward_blobs` results (a missing blob differs)."""
    bad = []
    for name in sorted(set(a) | set(b)):
        if name in skip:
            continue
        if name not in a or name not in b or not bit_equal(a[name], b[name]):
            bad.append(name)
    return bad


def forward_only(case, ws):
    from detectandtrack_amd.training import TrainExecutor
    ex = TrainExecutor(ws, case.model.net)
    ex.run()
    return ex


# ---- layer tables ------------------------------------------------------------------------------------------------------------------
def layer_objects(ws):
    """key -> layer object of `ws._layers` (the table also caches anchors, folded BN pairs and reader scans)."""
    from detectandtrack_amd.ops import hip_ops as ops
    return collections.OrderedDict((k, l) for k, l in ws._layers.items() if isinstance(l, (ops.ConvLayer, ops.ConvGrad, ops.StemConv)))


def layer_fields(layer):
    """field name -> tensor (or None) of one layer object.  A ConvGrad gives its master view `w`, its `scale` and -- once the data
    gradient ran -- the fields of its data-gradient layer as `data.<field>`."""
    from detectandtrack_amd.ops import hip_ops as ops
    out = collections.OrderedDict()
    if isinstance(layer, ops.ConvGrad):
        out['w'], out['scale'] = layer.w, layer.scale
        if layer._data_layer is not None:
            for f in LAYER_FIELDS:
                out['data.' + f] = getattr(layer._data_layer, f, None)
        return out
    for f in LAYER_FIELDS:
        if hasattr(layer, f):
            out[f] = getattr(layer, f)
    return out


def snapshot_layers(ws):
    """key -> {field: copy} of every layer object."""
    snap = collections.OrderedDict()
    for k, l in layer_objects(ws).items():
        snap[k] = collections.OrderedDict((f, None if t is None else t.detach().clone()) for f, t in layer_fields(l).items())
    return snap


def compare_layers(a, b, keys=None):
    """[(key, field)] of every difference between two layer snapshots: a key only one of them holds is (key, None)."""
    bad = []
    for k in (keys if keys is not None else list(a) + [k for k in b if k not in a]):
        if k not in a or k not in b:
            bad.append((k, None))
            continue
        for f in list(a[k]) + [f for f in b[k] if f not in a[k]]:
            if f not in a[k] or f not in b[k] or not bit_equal(a[k][f], b[k][f]):
                bad.append((k, f))
    return bad


def bias_src_layers(ws):
    """Keys of the layers that keep a padded COPY of their bias (`bias_src`): the ones a refresh has to copy again."""
    from detectandtrack_amd.ops import hip_ops as ops
    keys = []
    for k, l in layer_objects(ws).items():
        lay = l._data_layer if isinstance(l, ops.ConvGrad) else l
        if getattr(lay, 'bias_src', None) is not None:
            keys.append(k)
    return keys


def layer_params(model, key):
    """(weight names, bias names) of the model parameters the layer cached under `key` is built from, read off the op the key names:
    (net, i) and (net, ('grad', i)) are op i; the fused RPN head's key carries its four names.  An AffineChannel shift in the bias slot
    is not a bias parameter of the layer's own."""
    k = key[1]
    if isinstance(k, tuple) and k and k[0] == 'rpnhead':
        return list(k[1:3]), list(k[3:5])
    i = k[1] if (isinstance(k, tuple) and k and k[0] == 'grad') else k
    assert isinstance(i, int), key
    a = model.net.ops[i].args
    return [a['w']], ([a['b']] if (a.get('b') and not a.get('shift')) else [])


# ---- section 1: derived state follows the masters ----------------------------------------------------------------------------------
def device_state(case, ws, trainer):
    """(name -> device master of every model parameter, name -> momentum view)."""
    return ({n: ws.dev_param(n) for n in case.model.params}, dict(trainer.momentum))


def compare_state(a, b):
    bad = []
    for what, da, db in (('master', a[0], b[0]), ('momentum', a[1], b[1])):
        for n in sorted(set(da) | set(db)):
            if n not in da or n not in db or not bit_equal(da[n], db[n]):
                bad.append((what, n))
    return bad


def save_checkpoint(case, ws, trainer, path):
    """What tools/train_net.py does at a snapshot iteration."""
    from detectandtrack_amd.utils import net as net_utils
    ws.params_from_device()
    net_utils.save_model_to_weights_file(path, case.model, ws, trainer.momentum_blobs())


def load_checkpoint(case, path):
    """What tools/train_net.py does on resume: a fresh workspace, the file, a new Trainer, its momentum."""
    from detectandtrack_amd.utils import net as net_utils
    ws = case.workspace(case.weights)        # (initialised first, as train_net.py does: the file is overlaid on it)
    momentum = {}
    net_utils.initialize_from_weights_file(case.model, ws, path, momentum=momentum)
    trainer = case.trainer(ws)
    trainer.load_momentum(momentum)
    return ws, trainer, momentum


class ResumeReport(object):
    """Findings of `resume_report` (every list empty = nothing wrong), and the counts the test prints."""


def resume_report(case, path, lr, k=2):
    skip = set(NOT_REPRODUCIBLE.get(case.id, {}))
    r = ResumeReport()
    r.seconds, t0 = collections.OrderedDict(), [time.perf_counter()]

    def lap(name):       # where the seconds of a case go (printed by the test)
        torch.cuda.synchronize()
        now = time.perf_counter()
        r.seconds[name], t0[0] = round(now - t0[0], 2), now
    trainable = set(expected_trainable(case.model))
    ws_a = case.workspace(case.weights)
    tr_a = case.trainer(ws_a)
    tr_a.step(lr, update=False)                 # builds every layer (forward, gradient): the "before" side of the not-vacuous check
    before = snapshot_layers(ws_a)
    r.losses = []
    for _ in range(k):
        r.losses.append(tr_a.step(lr).loss_values())
    after_steps = snapshot_layers(ws_a)         # (a BN checkpoint clears the table: what the steps left is kept here)
    lap('train')
    save_checkpoint(case, ws_a, tr_a, path)
    lap('save')
    ws_b, tr_b, momentum = load_checkpoint(case, path)
    os.remove(path)                             # (0.5 - 1 GB: not left behind in the test's temporary directory)
    lap('load')
    r.momentum_loaded = len(momentum)
    # masters, momentum, running statistics: before any forward of B (a training-mode SpatialBN moves its running statistics)
    r.state = compare_state(device_state(case, ws_a, tr_a), device_state(case, ws_b, tr_b))
    # B against itself, then A against B
    b1 = forward_blobs(case, ws_b, forward_only(case, ws_b))
    b2 = forward_blobs(case, ws_b, tr_b.step(lr, update=False))
    a2 = forward_blobs(case, ws_a, tr_a.step(lr, update=False))
    r.not_reproducible = compare_blobs(b1, b2)
    r.blobs = compare_blobs(a2, b2, skip)
    r.n_blobs = len([n for n in b2 if n not in skip])
    r.loss_blobs = [n for n in b2 if n.startswith('loss:')]
    lap('forwards')
    # layer tables: what A's steps left AND what A holds after its next pass, against the freshly built B
    tab_a, tab_b = snapshot_layers(ws_a), snapshot_layers(ws_b)
    r.layers = compare_layers(tab_a, tab_b)
    r.layers += [d for d in compare_layers(after_steps, tab_b, keys=list(after_steps)) if d not in r.layers]
    r.n_layers = len(tab_b)
    r.n_refreshed_in_place = len(after_steps)
    r.bias_src = bias_src_layers(ws_a)
    # not vacuous: every layer of a trainable weight changed its packed image, every trainable padded bias its copy
    r.unmoved = []
    r.n_trainable_layers = r.n_trainable_bias_copies = 0
    for key in before:
        wn, bn = layer_params(case.model, key)
        if key not in tab_a:
            r.unmoved.append((key, None))
            continue
        pk = 'data.packed' if 'w' in before[key] else 'packed'
        if any(n in trainable for n in wn) and pk in before[key]:
            r.n_trainable_layers += 1
            if bit_equal(before[key][pk], tab_a[key].get(pk)):
                r.unmoved.append((key, pk))
        if key in r.bias_src and any(n in trainable for n in bn):
            bk = 'data.bias' if 'w' in before[key] else 'bias'
            r.n_trainable_bias_copies += 1
            if bit_equal(before[key][bk], tab_a[key].get(bk)):
                r.unmoved.append((key, bk))
    lap('layers')
    # live reload: the checkpoint into the LIVE workspace of A, parameter by parameter
    # (the values of the file: B's host dict holds them as initialize_from_weights_file read them, `momentum` is what it returned)
    for n in case.model.params:
        ws_a.set_param(n, ws_b.params[n])
    tr_a.load_momentum(momentum)
    r.reload_alias_error = None
    try:
        tr_a._check_aliases()
    except RuntimeError as e:
        r.reload_alias_error = str(e)
    r.reload_state = [d for d in compare_state(device_state(case, ws_a, tr_a), device_state(case, ws_b, tr_b))
                      if not d[1].endswith(('_rm', '_riv'))]       # (B's forwards moved its running statistics meanwhile)
    r.reload_blobs = compare_blobs(forward_blobs(case, ws_a, forward_only(case, ws_a)), b1, skip)
    lap('reload')
    return r


# ---- section 2: the update rule ----------------------------------------------------------------------------------------------------
def torch_bound(ref64, absref64, K):
    """`numerics.bound(..., out_fmt='fp32')` on device tensors (the buffers of an R-18 model hold 70 M elements: the float64 arithmetic
    of the whole check runs on the GPU, numerics.assert_elementwise then words the finding of every parameter this flags)."""
    u = nm.unit_roundoff('fp32')
    return u * ref64.abs() + nm.C * float(np.sqrt(float(K))) * 2.0 ** -24 * absref64 + nm._TINY[torch.float32]


def expected_update(w0, v0, g, is_bias, lr, mu, wd, corr):
    """The reference's rule in float64 (model_builder.add_parameter_update_ops, detector._CorrectMomentum) on flat tensors; `is_bias` a
    bool mask.  -> (v, |v| sum, w, |w| sum): the values and the sums of the magnitudes of their terms."""
    w0, v0, g = w0.double(), v0.double(), g.double()
    gg = torch.where(is_bias, 2.0 * g, g + wd * w0)
    gg_abs = torch.where(is_bias, 2.0 * g.abs(), g.abs() + wd * w0.abs())
    v = mu * (corr * v0) + lr * gg
    v_abs = mu * (abs(corr) * v0.abs()) + lr * gg_abs
    return v, v_abs, w0 - v, w0.abs() + v_abs


def flat_layout(ws, trainer):
    """name -> (offset, size) of every parameter whose device master lies in the Trainer's flat weight buffer."""
    base, n = trainer.flat_w.data_ptr(), trainer.flat_w.numel()
    out = {}
    for name, t in ws._dev_params.items():
        off = (t.data_ptr() - base) // 4
        if 0 <= off < n and t.data_ptr() >= base:
            out[name] = (int(off), int(t.numel()))
    return out


def lr_schedule(lr0):
    return [lr0, lr0, 0.1 * lr0, 0.105 * lr0]


class UpdateReport(object):
    pass


def update_rule_report(case, lr0):
    """Four `Trainer.step`s with lr0, lr0, 0.1 lr0, 0.105 lr0.  -> report: .steps[s] = [(name, 'v' | 'w', message)] of the parameters with an
    element outside the bound at step s; .frozen_changed / .not_moved / .bias_names / .layout."""
    cfg = case.cfg
    model = case.model
    r = UpdateReport()
    ws = case.workspace(case.weights)
    tr = case.trainer(ws)
    initial = {n: ws.dev_param(n).detach().clone() for n in model.params}
    r.layout = flat_layout(ws, tr)
    r.bias_names = sorted(n for n, (off, _) in r.layout.items() if off >= tr.n_weights)
    is_bias = torch.zeros(tr.flat_w.numel(), dtype=torch.bool, device=tr.flat_w.device)
    for n, (off, sz) in r.layout.items():
        if n in model.biases:
            is_bias[off:off + sz] = True
    mu, wd = float(np.float32(cfg.SOLVER.MOMENTUM)), float(np.float32(cfg.SOLVER.WEIGHT_DECAY))
    r.steps, r.corrected, r.losses = [], [], []
    prev = None
    for s, lr in enumerate(lr_schedule(lr0)):
        lr32 = float(np.float32(lr))
        ratio = 1.0 if prev is None else max(lr32 / prev, prev / lr32)
        corrected = ratio > cfg.SOLVER.SCALE_MOMENTUM_THRESHOLD
        corr = lr32 / prev if corrected else 1.0
        r.corrected.append(corrected)
        w0, v0 = tr.flat_w.detach().clone(), tr.flat_v.detach().clone()
        r.losses.append(tr.step(lr).loss_values())
        g = tr.flat_g          # (the SGD kernel takes it const; the next step zeroes it)
        v, v_abs, w, w_abs = expected_update(w0, v0, g, is_bias, lr32, mu, wd, corr)
        K = 4 if corrected else 3
        found = []
        for what, got, ref, absref in (('v', tr.flat_v, v, v_abs), ('w', tr.flat_w, w, w_abs)):
            bad = ~((got.double() - ref).abs() <= torch_bound(ref, absref, K))
            if not bool(bad.any()):
                continue
            for n, (off, sz) in sorted(r.layout.items()):
                if bool(bad[off:off + sz].any()):
                    try:
                        nm.assert_elementwise(got[off:off + sz], ref[off:off + sz], absref[off:off + sz], K, 'fp32',
                                              'step %d %s of %s' % (s + 1, what, n))
                        found.append((n, what, 'flagged on the device, inside the bound on the host'))
                    except AssertionError as e:
                        found.append((n, what, str(e)))
        r.steps.append(found)
        prev = lr32
    trainable = set(expected_trainable(model))
    computed = set(getattr(model, 'computed_params', ()))
    r.n_trainable = len(trainable)
    r.frozen_changed = sorted(n for n in model.params if n not in trainable and n not in computed
                              and not bit_equal(initial[n], ws.dev_param(n)))
    r.n_frozen = len([n for n in model.params if n not in trainable and n not in computed])
    r.not_moved = sorted(n for n in trainable if bit_equal(initial[n], ws.dev_param(n)))
    r.expected_bias_names = sorted(n for n in trainable if n in model.biases)
    r.expected_in_flat = sorted(trainable)
    return r
