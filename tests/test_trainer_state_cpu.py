"""The parts of tests/trainer_state.py that need no GPU: the float64 update rule and its bound, the bit comparisons, and -- for every
shipped training configuration -- which parameters the reference updates."""
import numpy as np
import pytest
import torch

from tests import numerics as nm
from tests import trainer_state as tst


@pytest.fixture(autouse=True)
def _restore_cfg():
    yield
    from detectandtrack_amd.core.config import reset_cfg
    reset_cfg()


def test_torch_bound_is_the_bound_of_numerics():
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(1000, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-30, 4, (1000,), generator=g).double()
    absref = ref.abs() * (1.0 + torch.rand(1000, generator=g, dtype=torch.float64))
    for K in (3, 4):
        np.testing.assert_array_equal(tst.torch_bound(ref, absref, K).numpy(), nm.bound(ref, absref, K, 'fp32'))


def test_expected_update_is_the_reference_rule():
    """add_parameter_update_ops: a bias takes 2 g and no decay, a weight g + decay * w; MomentumSGDUpdate v = mu v + lr g, w -= v;
    _CorrectMomentum scales v by new_lr / old_lr first."""
    w0 = torch.tensor([1.0, -2.0, 0.5, 4.0], dtype=torch.float64)
    v0 = torch.tensor([0.1, 0.2, -0.3, 0.0], dtype=torch.float64)
    g = torch.tensor([0.5, -1.0, 2.0, 0.0], dtype=torch.float64)
    is_bias = torch.tensor([False, False, True, True])
    lr, mu, wd = 0.01, 0.9, 1e-4
    v, v_abs, w, w_abs = tst.expected_update(w0, v0, g, is_bias, lr, mu, wd, 1.0)
    want_v = [0.9 * 0.1 + 0.01 * (0.5 + 1e-4 * 1.0), 0.9 * 0.2 + 0.01 * (-1.0 + 1e-4 * -2.0), 0.9 * -0.3 + 0.01 * 4.0, 0.0]
    np.testing.assert_allclose(v.numpy(), want_v, rtol=1e-15)
    np.testing.assert_allclose(w.numpy(), w0.double().numpy() - np.array(want_v), rtol=1e-15)
    assert v.dtype == torch.float64 and bool((v_abs >= v.abs()).all()) and bool((w_abs >= w.abs()).all())
    v_c = tst.expected_update(w0, v0, g, is_bias, lr, mu, wd, 0.1)[0]
    np.testing.assert_allclose(v_c.numpy()[0], 0.9 * 0.01 + 0.01 * (0.5 + 1e-4), rtol=1e-15)
    # a frozen weight with a zero gradient would still decay under this rule: it must not be in the flat buffers at all
    assert float(tst.expected_update(w0, v0 * 0, g * 0, is_bias, lr, mu, wd, 1.0)[2][0]) != 1.0


def test_the_schedule_corrects_the_momentum_at_its_third_step_only():
    from detectandtrack_amd.utils import lr_policy
    tst.configure(tst.FPN3D)
    lrs = [float(np.float32(v)) for v in tst.lr_schedule(0.002)]
    got = [lr_policy.momentum_correction(a, b) for a, b in zip([None] + lrs[:-1], lrs)]
    assert got[0] is None and got[1] is None and got[3] is None
    assert got[2] == lrs[2] / lrs[1] and abs(got[2] - 0.1) < 1e-7


def test_bit_comparisons_name_what_differs():
    a = torch.tensor([0.0, float('nan'), 1.0])
    assert tst.bit_equal(a, a.clone()) and not tst.bit_equal(a, torch.tensor([-0.0, float('nan'), 1.0]))
    assert not tst.bit_equal(a, a.double()) and not tst.bit_equal(a, a.view(1, 3))
    assert tst.bit_equal(torch.zeros(0), torch.zeros(0)) and tst.bit_equal(torch.tensor(2.0), torch.tensor(2.0))
    assert tst.bit_equal(None, None) and not tst.bit_equal(None, a)
    assert tst.bit_equal(np.arange(3), np.arange(3)) and not tst.bit_equal(np.arange(3), np.arange(3.0))
    ta = {'k1': {'packed': a, 'bias': a}, 'k2': {'packed': a}}
    tb = {'k1': {'packed': a.clone(), 'bias': a + 1}, 'k3': {'packed': a}}
    assert tst.compare_layers(ta, tb) == [('k1', 'bias'), ('k2', None), ('k3', None)]
    assert tst.compare_layers(ta, tb, keys=['k1']) == [('k1', 'bias')]
    assert tst.compare_blobs({'x': a, 'y': a, 'z': a}, {'x': a.clone(), 'y': a * 2}, skip=('z',)) == ['y']


@pytest.mark.parametrize('case_id', list(tst.CASES))
def test_which_parameters_the_reference_updates(case_id):
    """The rule of the tests (read off the op list: a parameter only ops at or below the StopGradient marker use gets no gradient)
    against the executor's own (training.param_ready_index: final before the backward pass starts), on every shipped configuration."""
    from detectandtrack_amd.training import param_ready_index
    from detectandtrack_amd.workspace import Executor
    model = tst.create_model(case_id)
    frozen = tst.params_without_gradient(model)
    assert 'conv1_w' in frozen and any(n.startswith('res2_') for n in frozen)
    assert not any(n.startswith(('res3', 'res4', 'res5', 'fc', 'rpn', 'conv_rpn', 'cls_score', 'bbox_pred', 'kps_score', 'conv_fcn', 'fpn'))
                   for n in frozen), sorted(frozen)
    ex = Executor.__new__(Executor)
    ex.net = model.net
    ex._plan_rpn_siblings()
    idx = param_ready_index(model.net, ex._fused)
    listed = model.TrainableParams()
    assert sorted(n for n in listed if idx.get(n, -1) == len(model.net.ops)) == sorted(n for n in listed if n in frozen)
    trainable = tst.expected_trainable(model)
    assert trainable and set(trainable) <= set(listed) and not set(trainable) & frozen
    assert not any(n.endswith(('_rm', '_riv')) for n in trainable)
    biases = [n for n in trainable if n in model.biases]
    assert biases and all(n.endswith('_b') for n in biases)
    if case_id in (tst.BN, tst.GN):     # trainable scale / bias pairs: `_s` is a weight (decayed), `_b` a bias
        norm = [n for n in trainable if model.param_specs[n].get('bn') or model.param_specs[n].get('gn')]
        assert norm and all((n in model.biases) == n.endswith('_b') for n in norm)
        assert any(n.endswith('_s') for n in norm)
