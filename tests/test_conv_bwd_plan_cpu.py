"""The gradient ledger and the plan of the conv backward (detectandtrack_amd/train_plan.py) against the rules they replaced
(tests/conv_bwd_cases.py: `TrainExecutor._take_grad` and the decisions of `TrainExecutor.bwd_Conv` restated from their earlier text).

The product of ALL the axes of conv_bwd_cases.AXES has ~10^10 points, so the plan is held to the parent's rule (a) on the full product of
every group of axes that one decision reads together -- the pre-pass, the frame window, the weight-gradient route, the data-gradient
route with its waiting list, the in-place question -- with the other axes at their first value, and (b) on 20000 points drawn with a
fixed seed from the product of all axes, which is where decisions of different groups meet.
"""
import random

import pytest
import torch

from detectandtrack_amd.ops import hip_ops as ops
from detectandtrack_amd.train_plan import Entry, GradLedger, plan_conv_bwd
from tests import conv_bwd_cases as cases
from tests import conv_bwd_routes as routes


# ---- ledger -----------------------------------------------------------------------------------------------------------------------------
def _random_contributions(rng, gen, tdt):
    """1 to 5 contributions inside a 4-frame blob of [., 2, 3, 8]: mixed target dtype / fp32, RoI accumulators (fp32, all frames),
    non-contiguous slices."""
    lst = []
    for _ in range(rng.choice((1, 1, 2, 2, 3, 4, 5))):
        if rng.random() < 0.15 and not any(getattr(t, '_roi_acc', False) for t, _, _ in lst):      # (a blob has ONE accumulator)
            t = torch.randn(4, 2, 3, 8, generator=gen)
            t._roi_acc = True
            lst.append((t, 0, False))
            continue
        lo = rng.choice((0, 0, 1, 2, 3))
        n = rng.randint(1, 4 - lo) if rng.random() < 0.5 else 4 - lo
        dt = tdt if rng.random() < 0.7 else (torch.float32 if tdt != torch.float32 else torch.bfloat16)   # (the other dtype)
        if rng.random() < 0.25:
            t = torch.randn(n, 2, 3, 16, generator=gen).to(dt)[..., ::2]
        else:
            t = torch.randn(n, 2, 3, 8, generator=gen).to(dt)
        lst.append((t, lo, False))
    if len(lst) == 1 and not getattr(lst[0][0], '_roi_acc', False) and rng.random() < 0.5:
        lst = [(lst[0][0], lst[0][1], True)]
    return lst


@pytest.mark.parametrize('dt', [ops.F32, ops.BF16])
def test_ledger_take_sums_exactly_as_the_rule_it_replaced(dt):
    tdt = ops.tdtype(dt)
    rng, gen = random.Random(7), torch.Generator().manual_seed(7)
    seen = set()
    for _ in range(400):
        lst = _random_contributions(rng, gen, tdt)
        keep = [t.clone() for t, _, _ in lst]
        seen.add(cases.take_branch(lst, dt))
        want, want_lo, want_masked = cases.parent_take_grad(list(lst), dt)
        led = GradLedger()
        for t, lo, masked in lst:
            if getattr(t, '_roi_acc', False):
                led.roi_accumulator('x', t.shape, t.device).copy_(t)
            else:
                led.add('x', t, lo, masked=masked)
        assert led.contributions('x') == len(lst) and len(led.waiting('x')) == len(lst)
        got, got_lo, got_masked = led.take('x', dt)
        assert not led.waiting('x') and led.contributions('x') == 0
        assert got_lo == want_lo and bool(got_masked) == bool(want_masked)
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
        if len(lst) == 1 and lst[0][0].dtype == tdt and not getattr(lst[0][0], '_roi_acc', False):
            assert got is lst[0][0]
        for (t, _, _), k in zip(lst, keep):
            assert torch.equal(t, k)
    assert seen == {'single', 'single cast', 'pair', 'clone start', 'zero start', 'zero start, union'}, seen


def test_ledger_bookkeeping():
    led = GradLedger()
    a, b = torch.zeros(2, 1, 1, 8), torch.ones(2, 1, 1, 8)
    led.add('y', a, 1)
    led.move('y', 'x')
    led.move('nothing', 'x')
    assert led.waiting('y') == () and led.waiting('x') == (Entry(a, 1, False, False),)
    led.summed_into('x', a, False)          # summed in place: the same entry, one more contribution
    assert led.waiting('x') == (Entry(a, 1, False, False),)
    n = led.contributions('x')
    led.summed_into('x', b, True)           # the sum went to a new tensor and carries the mask
    assert led.waiting('x') == (Entry(b, 1, True, False),) and led.contributions('x') == n + 1
    assert led.take('x', ops.F32) == (b, 1, True)
    led.add('z', a)
    led.add('z', b, masked=True)
    with pytest.raises(AssertionError, match='a masked gradient must be the only contribution'):
        led.take('z', ops.F32)
    led.add('w', a)
    led.clear()
    assert led.waiting('w') == () and led.contributions('w') == 0


# ---- plan -------------------------------------------------------------------------------------------------------------------------------
GROUPS = (
    ('relu', 'masked', 'train_b', 'arena', 'cout_is_stride', 'residual'),                                               # the pre-pass
    ('kernel', 'window', 'N'),                                                                                          # the frame window
    ('kernel', 'groups', 'window', 'train_w', 'arena', 'gt_arena', 'pw_batch', 'sealed', 'acc_direct', 'queue_len'),    # weight route
    ('waiting', 'producer', 'readers', 'ncontrib', 'fuse_relu', 'fuse_relu_sum', 'sum_env', 'groups', 'in_no_grad', 'cin_is_stride',
     'window'),                                                                                                         # data route
    ('waiting', 'held', 'queue_len', 'kernel', 'pw_batch', 'relu', 'train_w', 'acc_direct', 'gt_arena'),                 # in place?
)


def _outcome(fn, f):
    try:
        return tuple(fn(f))
    except (AssertionError, RuntimeError) as e:
        return (type(e).__name__, str(e))


def _points():
    for g in GROUPS:
        for c in cases.product(g):
            yield c
    for c in cases.sample(random.Random(11), 20000):
        yield c


def test_plan_decides_what_bwd_conv_decided():
    wroutes, droutes, inplace, errors, n = set(), set(), set(), set(), 0
    for c in _points():
        f = cases.facts(c)
        want, got = _outcome(cases.parent_conv_bwd, f), _outcome(plan_conv_bwd, f)
        assert got == want, (c, got, want)
        n += 1
        if len(got) == 2:
            errors.add(got[1][:40])
            continue
        wroutes.add(got[9])
        droutes.add(got[10])
        inplace.add(got[11])
    print('%d points, errors %r' % (n, sorted(errors)))
    assert wroutes == {'none', 'queue', 'acc', 'immediate'} and droutes == {'none', 'plain', 'sum', 'mask', 'sum_mask'}
    assert inplace == {True, False}
    assert any(e.startswith('frame-window gradients assume one clip') for e in errors)


def test_plan_refuses_what_bwd_conv_refused():
    base = next(cases.product(()))
    f = cases.facts(dict(base, waiting='match'))
    f = f._replace(waiting=(f.waiting[0]._replace(masked=True),))
    with pytest.raises(AssertionError, match='a ReLU-masked gradient is the ONLY contribution of its blob'):
        plan_conv_bwd(f)
    with pytest.raises(AssertionError, match='a ReLU-masked gradient is the ONLY contribution of its blob'):
        cases.parent_conv_bwd(f)
    f = cases.facts(dict(base, sealed=True))
    for fn in (plan_conv_bwd, cases.parent_conv_bwd):
        with pytest.raises(RuntimeError, match="gradient contribution to 'w' after its bucket was handed to the all-reduce"):
            fn(f)
    f = cases.facts(base)._replace(x_t2c=True)
    with pytest.raises(AssertionError, match='time->channel heads'):
        plan_conv_bwd(f)


def test_plan_is_pure():
    """No mutation of the facts: the same facts give the same plan twice, and the waiting list and the queue are as they were."""
    f = cases.facts(dict(next(cases.product(())), waiting='match', held=True, readers=2, ncontrib=1))
    waiting, queued = tuple(f.waiting), list(f.queued)
    p = plan_conv_bwd(f)
    assert plan_conv_bwd(f) == p and tuple(f.waiting) == waiting and list(f.queued) == queued
    assert p.dgrad == 'sum_mask' and not p.inplace
    with pytest.raises(AttributeError):
        p.dgrad = 'plain'


def test_the_recorded_fpn3d_step_reaches_every_route():
    """Not vacuous: the recorded R-18 FPN3D step (tests/conv_bwd_routes.json, compared on the GPU by test_gpu_conv_bwd_routes.py) has a plain,
    a summing, a masking and a sum + mask data gradient and a queued batch."""
    d = routes.load_recorded()['train_r18_fpn3d']
    modes = {int(k.split(',')[0].split()[1]) for k in d['dgrad']}
    assert {0, 1, 3, 4} <= modes, d['dgrad']
    assert d['sum_mask'] > 0 and d['acc_batch_jobs'] and max(d['acc_batch_jobs']) > 1
    assert d['wgrad_finish_batch'] > 0 and d['relu_bias_bwd']
