"""The state between the kernels of a training run (tests/trainer_state.py), for every shipped training configuration:

1. after `Trainer.step` everything derived from the fp32 masters -- packed forward and data-gradient images, padded bias copies, layers
   built from concatenated / permuted / sub-pixel weights -- is, bit for bit, what a resume from a checkpoint of those masters builds;
2. `Trainer.step` applies the reference's update rule to its flat buffers (float64, every element), corrects the momentum at a
   learning-rate step, leaves what the reference does not update untouched and restores the momentum on resume;
3. controls: the helpers report a skipped refresh, a skipped bias copy and a skipped momentum correction.
"""
import pytest
import torch

from tests import trainer_state as tst

pytestmark = pytest.mark.gpu

# The learning rate of the existing trainer tests.  It is large enough for the not-vacuous check in bf16: two updates move a weight by
# ~lr * |g| per element, and of the >= 10^4 elements of a layer some cross a rounding boundary of the 16-bit packed image.
LR = 0.002


@pytest.fixture(autouse=True)
def _restore_cfg():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    yield
    from detectandtrack_amd.core.config import reset_cfg
    reset_cfg()


_RESUME_FINDINGS = (
    ('not_reproducible', 'two forwards of ONE workspace differ in these blobs'),
    ('state', 'after the resume these differ from the trained workspace'),
    ('blobs', 'forward blobs of the trained workspace differ from the resumed one (stale derived state)'),
    ('layers', 'layer fields of the trained workspace differ from the resumed one'),
    ('unmoved', 'layers of trainable parameters that the steps did not change'),
    ('reload_state', 'set_param / load_momentum into the live workspace left these different'),
    ('reload_blobs', 'the forward after the live reload differs from the resumed workspace in these blobs'),
)


def _assert_resume_clean(r):
    found = ['%s (%d): %r' % (text, len(getattr(r, name)), getattr(r, name)[:6]) for name, text in _RESUME_FINDINGS if getattr(r, name)]
    if r.reload_alias_error is not None:
        found.append(r.reload_alias_error)
    assert not found, '\n'.join(found)


@pytest.mark.parametrize('case_id', list(tst.CASES))
def test_derived_state_follows_the_masters(case_id, tmp_path):
    """Two steps in trainer A, a checkpoint, a resume into a fresh workspace and Trainer B, one forward + backward in each: masters,
    momentum and running statistics, every forward blob (losses among them) and every field of every layer object are bit-equal; the
    steps changed the packed image of every layer of a trainable weight and every padded copy of a trainable bias; the checkpoint set
    into the live workspace of A gives B's forward again."""
    case = tst.Case(case_id)
    r = tst.resume_report(case, str(tmp_path / 'model_iter1.pkl'), LR)
    print('%s: lr %g, %d layer objects compared (%d refreshed in place, %d of trainable weights, %d trainable padded bias copies, %d with a '
          'bias copy), %d forward blobs compared (%d losses), %d momentum blobs restored, not reproducible: %r'
          % (case_id, LR, r.n_layers, r.n_refreshed_in_place, r.n_trainable_layers, r.n_trainable_bias_copies, len(r.bias_src), r.n_blobs,
             len(r.loss_blobs), r.momentum_loaded, r.not_reproducible))
    print('%s: seconds %r' % (case_id, dict(r.seconds)))
    _assert_resume_clean(r)
    assert r.n_layers > 20 and r.n_trainable_layers > 10 and r.n_blobs > 30 and len(r.loss_blobs) >= 4
    assert r.momentum_loaded == len(tst.expected_trainable(case.model))
    if case_id == tst.FPN3D:
        assert r.bias_src, 'cls_score (2 channels) and the fused RPN head keep padded bias copies'
        assert r.n_trainable_bias_copies > 0


@pytest.mark.parametrize('case_id', [tst.FPN3D_FP32, tst.BN, tst.GN])
def test_update_rule_through_trainer_step(case_id):
    """Four steps at lr0, lr0, 0.1 lr0, 0.105 lr0: every element of `flat_v` and `flat_w` within the per-element bound of the float64
    rule (biases: 2 g, no decay; weights: g + decay * w; v = mu (c v) + lr g with c = new / old lr at the third step only); what the
    reference does not update is bit-equal to its initial value, everything it updates moved, the bias half of the flat buffer holds
    exactly the trainable biases."""
    case = tst.Case(case_id)
    r = tst.update_rule_report(case, LR)
    print('%s: %d parameters in the flat buffers, %d treated as biases, %d untouched, corrected steps %r'
          % (case_id, len(r.layout), len(r.bias_names), r.n_frozen, r.corrected))
    assert r.corrected == [False, False, True, False]
    for s, found in enumerate(r.steps):
        assert found == [], 'step %d: %d parameters outside the bound, first: %r' % (s + 1, len(found), found[0])
    assert r.bias_names == r.expected_bias_names
    assert sorted(r.layout) == r.expected_in_flat
    assert r.frozen_changed == [], 'parameters the reference never updates changed: %r' % (r.frozen_changed[:8],)
    assert r.not_moved == [], 'trainable parameters that four steps did not move: %r' % (r.not_moved[:8],)
    assert r.n_frozen > 0 and len(r.bias_names) > 10


# ---- controls: the helpers report a planted defect ---------------------------------------------------------------------------------
def test_control_a_skipped_refresh_is_reported(monkeypatch, tmp_path):
    from detectandtrack_amd.training import Trainer
    monkeypatch.setattr(Trainer, '_refresh_layers', lambda self: None)
    r = tst.resume_report(tst.Case(tst.FPN3D), str(tmp_path / 'm.pkl'), LR)
    assert r.not_reproducible == []
    assert r.blobs, 'layers that still hold the weights of two steps ago went unnoticed by the forward-blob comparison'
    assert any(n.startswith('loss:') for n in r.blobs) and r.layers


def test_control_a_skipped_bias_copy_is_reported(monkeypatch, tmp_path):
    from detectandtrack_amd.ops import hip_ops as ops

    def run_without_bias_loop(self):
        for table, n, total, ntap in self.launches:
            ops.ctx().call('dat_conv3d_pack_weights_batch', ops._stream(), ops._ptr(table), n, total, ntap, self.dtype)
    monkeypatch.setattr(ops.PackBatch, 'run', run_without_bias_loop)
    r = tst.resume_report(tst.Case(tst.FPN3D), str(tmp_path / 'm.pkl'), LR)
    assert r.bias_src
    flagged = [k for k in r.bias_src if (k, 'bias') in r.layers]
    assert flagged, 'stale padded bias copies went unnoticed by the layer-table comparison: %r' % (r.layers[:8],)
    assert all(f == 'bias' for _, f in r.layers), r.layers[:8]


def test_control_a_skipped_momentum_correction_is_reported(monkeypatch):
    from detectandtrack_amd.utils import lr_policy
    monkeypatch.setattr(lr_policy, 'momentum_correction', lambda cur_lr, new_lr: None)
    r = tst.update_rule_report(tst.Case(tst.FPN3D_FP32), LR)
    assert r.steps[0] == [] and r.steps[1] == [], (r.steps[0][:2], r.steps[1][:2])
    assert r.steps[2], 'a learning-rate step without the momentum correction went unnoticed'
    assert all(what in ('v', 'w') for _, what, _ in r.steps[2])
