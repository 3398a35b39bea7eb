"""Which routes the conv backward takes on the shipped training graphs (tests/conv_bwd_routes.py).

Every case of tests/trainer_state.CASES, shrunk as the trainer-state tests shrink it, runs one `Trainer.step(0.0)` under a trace of the
library calls; the histogram of its data-gradient epilogues, ReLU / bias pre-passes, weight-gradient routes and queued batches must be
the one recorded in tests/conv_bwd_routes.json at the commit before `bwd_Conv` was split into plan and launch.  The whole-model parity
tests pass just as well when a fusion stops firing; this one does not.

CONV_BWD_ROUTES_RECORD=<file>: record mode -- the histograms are written into that file instead of being compared (how the committed
file was made, at that earlier commit).
"""
import json
import os

import pytest
import torch

from tests import conv_bwd_routes as routes
from tests import trainer_state as tst

pytestmark = pytest.mark.gpu

RECORD = os.environ.get('CONV_BWD_ROUTES_RECORD')


@pytest.fixture(autouse=True)
def _restore_cfg():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    yield
    from detectandtrack_amd.core.config import reset_cfg
    reset_cfg()


def _as_json(h):
    return json.loads(json.dumps(h))


@pytest.mark.parametrize('case_id', list(tst.CASES))
def test_conv_backward_routes_are_the_recorded_ones(case_id, monkeypatch):
    case = tst.Case(case_id)
    tr = case.trainer(case.workspace(case.weights))
    _, calls = routes.trace_step(monkeypatch, tr)
    got = _as_json(routes.histogram(calls))
    print('%s: %d library calls, %s' % (case_id, len(calls), json.dumps(got)))
    if RECORD:
        rec = {}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                rec = json.load(f)
        rec[case_id] = got
        with open(RECORD, 'w') as f:
            json.dump(rec, f, indent=1, sort_keys=True)
        return
    assert got == routes.load_recorded()[case_id]

