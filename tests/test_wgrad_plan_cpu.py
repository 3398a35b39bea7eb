"""The launch plan of the dense weight gradient (dat_conv3d_wgrad_plan; csrc/train_ops.hip wgrad_plan), held to the independent statement
of tests/wgrad_plan_cases.py -- on a machine without a GPU: the plan is a pure function of the knobs, the CU count and the layer.  Every
case asks with a NULL context and 256 compute units; a case that needs a knob asks a child process that has it in its environment."""
import ctypes as C

from tests import test_gpu_wgrad as g
from tests import wgrad_plan_cases as c
from tests.wgrad_plan_cases import BF16, DIRECT, F32, NINE_TAP, POINTWISE, REPACK

SWEEP = c.sweep()
FIELDS = ('family', 'variant', 'ncopies', 'npack', 'strip', 'tile_co', 'tile_ci', 'n_co_tiles', 'n_ci_tiles', 'taps', 'ksplit', 'atomic',
          'memset_first', 'finish', 'blocks', 'threads', 'lds_bytes', 'tiles', 'r_begin', 'r_end', 'nchunks')
KNOB_VARIANTS = [{'DAT_WGRAD_SUB': 1}, {'DAT_WGRAD_KS': 1}, {'DAT_WGRAD_KS': 3}, {'DAT_WGRAD_KS': 1000}, {'DAT_WGRAD_SUB': 1, 'DAT_WGRAD_KS': 5},
                 {'DAT_WGRAD_PW': 0}, {'DAT_WGRAD_PW': 10}, {'DAT_WGRAD_PW': 20}, {'DAT_WGRAD_PW': 40}, {'DAT_WGRAD_DIRECT': 0},
                 {'DAT_WGRAD_DIRECT': 2}]


def library_plans(layers, env, acc=False, num_cu=256):
    """[plan dict] of layers the library must accept."""
    got = c.plans_in_child(layers, env, num_cu, acc) if env else [c.plan(L, acc, num_cu) for L in layers]
    for L, (rc, _) in zip(layers, got):
        assert rc == 0, (rc, env, acc, L)
    return [p for _, p in got]


def assert_restated(layers, env, acc=False, num_cu=256):
    for L, p in zip(layers, library_plans(layers, env, acc, num_cu)):
        want = c.expect(L, env, num_cu, acc)
        assert set(want) == set(FIELDS) == set(p)
        assert p == want, (env, acc, L, {k: (p[k], want[k]) for k in FIELDS if p[k] != want[k]})


def gpu_test_variants():
    """Every (layers, env, acc) tests/test_gpu_wgrad.py launches."""
    nine = [c.from_case(k) for k in g.NINE_TAP_CASES]
    pw = [c.from_case(k) for k in g.POINTWISE_CASES]
    direct = [c.from_case(k) for k in g.DIRECT_CASES]
    out = []
    for sub, forced in g.NINE_TAP_VARIANTS:
        out.append((nine, dict(({'DAT_WGRAD_SUB': 1} if sub == 1 else {}), **({'DAT_WGRAD_KS': forced} if forced else {})), False))
    out += [(nine, {}, True), (nine, {'DAT_WGRAD_SUB': 1}, True)]
    for _, env in g.POINTWISE_VARIANTS:
        out.append((pw, {k: int(v) for k, v in env.items()}, False))
    out += [(pw, {}, True), (direct, {}, False), (direct, {}, True), (pw, {'DAT_WGRAD_PW': 0}, False), (pw, {'DAT_WGRAD_PW': 0}, True)]
    one_column = [L for L in nine if c.one_column_refusal(L['d'], dict(c.KNOBS, DAT_WGRAD_DIRECT=2))]
    assert len(one_column) == 1
    out += [(nine, {'DAT_WGRAD_DIRECT': 2}, False), ([L for L in nine if L not in one_column], {'DAT_WGRAD_DIRECT': 2}, True)]
    out.append(([c.from_case(k, F32) for k in g.NINE_TAP_CASES + g.POINTWISE_CASES + g.DIRECT_CASES], {}, False))
    out.append(([c.from_case(k) for k in g.REPACK_16BIT_CASES], {'DAT_WGRAD_DIRECT': 0}, False))
    return out


def test_the_plan_of_every_gpu_test_case_and_variant_equals_the_restatement():
    for layers, env, acc in gpu_test_variants():
        assert_restated(layers, env, acc)


def test_the_plan_of_every_swept_layer_equals_the_restatement_under_every_knob():
    assert_restated(SWEEP, {})
    assert_restated(SWEEP, {}, num_cu=304)
    direct_ok = [L for L in SWEEP if c.direct_eligible(L, c.KNOBS)]
    assert len(SWEEP) // 3 < len(direct_ok) < len(SWEEP)
    assert_restated(direct_ok, {}, acc=True)
    for env in KNOB_VARIANTS:
        assert_restated(SWEEP, env)


def test_acc_mode_is_refused_exactly_where_the_layer_re_packs():
    """dat_conv3d_wgrad_acc_supported == (family is not REPACK) == (the acc-mode plan is not refused), for the default knobs."""
    n = 0
    for L, p in zip(SWEEP, library_plans(SWEEP, {})):
        rc, _ = c.plan(L, acc=True)
        assert c.acc_supported(L) == (p['family'] != REPACK) == (rc == 0), (L, p, rc)
        n += p['family'] == REPACK
    assert 0 < n < len(SWEEP)


def test_every_plan_of_the_sweep_is_well_formed():
    for env, acc in [({}, False), ({}, True), ({'DAT_WGRAD_SUB': 1}, False), ({'DAT_WGRAD_KS': 1000}, False), ({'DAT_WGRAD_KS': 5}, True)]:
        layers = [L for L in SWEEP if not acc or c.direct_eligible(L, c.KNOBS)]
        for L, p in zip(layers, library_plans(layers, env, acc)):
            what = (env, acc, L, p)
            assert 1 <= p['ksplit'] <= max(p['nchunks'], 1), what
            per_block = 2 if (p['family'], p['variant']) == (NINE_TAP, 2) else 1
            assert p['ksplit'] % per_block == 0, what
            assert p['atomic'] in (0, 1) and (p['atomic'] or not acc), what
            assert p['memset_first'] == int(p['atomic'] and not acc) and p['finish'] == int(not acc), what
            assert p['tiles'] == p['n_co_tiles'] * p['n_ci_tiles'] * (L['d']['KT'] if p['family'] == NINE_TAP else p['taps']), what
            assert p['blocks'] == p['tiles'] * p['ksplit'] // per_block and 0 < p['blocks'] < 2 ** 31, what
            assert p['n_co_tiles'] == c.cdiv(L['cout'], p['tile_co']) and p['n_ci_tiles'] == c.cdiv(L['cin'], p['tile_ci']), what
            assert 0 <= p['lds_bytes'] <= 160 * 1024 and p['threads'] in (256, 512), what
            assert 0 <= p['r_begin'] < p['r_end'], what


def test_the_sweep_reaches_every_family_variant_and_edge():
    """A sweep that stops reaching one of these would let the agreement tests pass vacuously for it."""
    plans = library_plans(SWEEP, {})
    sub1 = library_plans(SWEEP, {'DAT_WGRAD_SUB': 1})
    assert {p['family'] for p in plans} == {REPACK, NINE_TAP, POINTWISE, DIRECT}
    nine = {(p['variant'], bool(p['atomic'])) for p in plans + sub1 if p['family'] == NINE_TAP}
    assert nine == {(2, False), (2, True), (1, False), (1, True)}, nine
    assert {(2, False), (2, True), (1, False)} <= {(p['variant'], bool(p['atomic'])) for p in plans if p['family'] == NINE_TAP}
    assert {p['variant'] for p in plans if p['family'] == POINTWISE} == {1, 2, 4}
    assert {p['family'] for p in plans if p['strip']} == {POINTWISE, DIRECT}
    refused = [L for L, p in zip(SWEEP, plans) if p['family'] == REPACK and c.one_column_refusal(L['d'], c.KNOBS) and
               L['d']['dtype'] == BF16 and L['d']['Cin'] % 64 == 0 and L['g_cstride'] % 64 == 0]
    assert refused, 'no 16-bit layer with spatial taps on a one-column map that only that rule keeps off the direct kernels'
    off = [p for L, p in zip(SWEEP, plans) if p['family'] == REPACK and p['r_begin'] > 0 and
           L['d']['out_t0'] * c.repack_geometry(L['d'])[0] * c.repack_geometry(L['d'])[1] != p['r_begin']]
    assert off, 'no window whose first padded position lies off a K-step boundary behind a non-zero k_begin'
    assert any(p['ksplit'] > 1 for p in plans if p['family'] == REPACK) and any(p['ksplit'] > 1 for p in plans if p['family'] == DIRECT)
    assert any(p['ksplit'] > 1 for p in plans if p['family'] == POINTWISE)


def test_the_batched_pointwise_rule_of_a_gradient_bucket():
    """wgrad_plan_cases.batched_ksplits on hand-worked buckets (dat_conv3d_wgrad_acc_batch re-splits the pointwise plans by it; the GPU
    tests hold its results): 2 blocks per CU over all layers, one per CU for a single layer, at least 4 chunks per block."""
    assert c.batched_ksplits([(1, 4096)], 256) == [256]                       # one layer: 16 chunks per block
    assert c.batched_ksplits([(1, 4096), (1, 4096)], 256) == [256, 256]       # two: 512 blocks
    assert c.batched_ksplits([(4, 1024), (1, 10)], 256) == [114, 2]           # cpb = ceil(4106 / 512) = 9
    assert c.batched_ksplits([(1, 7), (2, 3)], 256) == [2, 1]                 # cpb floors at 4
    assert c.batched_ksplits([(1, 7), (2, 3)], 256, forced_ks=5) == [5, 3]    # a forced value is clamped to the chunks


def test_the_literal_expectations_of_the_gpu_coverage_tests_without_a_gpu():
    """What tests/test_gpu_wgrad.py asserts of the live context, asked here of a NULL context (none of it depends on the CU count)."""
    nine = [c.from_case(k) for k in g.NINE_TAP_CASES]
    forced5 = library_plans(nine[:2], {'DAT_WGRAD_KS': 5})
    assert [(p['variant'], p['ksplit'], bool(p['atomic'])) for p in forced5] == [(2, 2, False), (2, 4, True)]
    split = library_plans([c.from_case(k) for k in g.DIRECT_SPLIT_CASES], {})
    assert [(p['family'], p['ksplit']) for p in split] == [(DIRECT, k) for k in (2, 4, 2, 2, 2)]
    rest = library_plans([c.from_case(k) for k in g.DIRECT_CASES if k not in g.DIRECT_SPLIT_CASES], {})
    assert all((p['family'], p['ksplit']) == (DIRECT, 1) for p in rest)
    layers = [c.from_case(k) for k in g.REPACK_16BIT_CASES]
    repack = library_plans(layers, {'DAT_WGRAD_DIRECT': 0})
    first = [L['d']['out_t0'] * c.repack_geometry(L['d'])[0] * c.repack_geometry(L['d'])[1] for L in layers]
    assert [(p['r_begin'], f, p['ksplit']) for p, f in zip(repack, first)] == [(64, 96, 1), (384, 440, 1), (0, 0, 1), (0, 0, 2)]
    assert all((p['family'], p['variant']) == (REPACK, BF16) for p in repack)


def test_the_plan_does_not_depend_on_earlier_calls_and_refuses_bad_arguments():
    first = [c.plan(L) for L in SWEEP[:400]]
    assert [c.plan(L) for L in reversed(SWEEP[:400])] == first[::-1]
    assert c.plan(SWEEP[0], num_cu=304) == c.plan(SWEEP[0], num_cu=304)
    from detectandtrack_amd import libdat
    out, cd = libdat.WgradPlan(), libdat.ConvDesc()
    for name, v in SWEEP[0]['d'].items():
        setattr(cd, name, int(v))
    query = libdat.lib().dat_conv3d_wgrad_plan
    assert query(None, C.byref(cd), SWEEP[0]['g_cstride'], SWEEP[0]['cin'], SWEEP[0]['cout'], 0, 256, C.byref(out)) == 0
    assert query(None, None, 64, 64, 64, 0, 256, C.byref(out)) != 0
    assert query(None, C.byref(cd), SWEEP[0]['g_cstride'], SWEEP[0]['cin'], SWEEP[0]['cout'], 0, 0, C.byref(out)) != 0      # no context: the CU count must be given
    # what the launch refuses, with the launch's codes (DAT_ERR_ARG = 1 for a window outside the clip, DAT_ERR_UNSUPPORTED for dilation at stride 2)
    bad_window = c.layer(64, 64, (3, 3, 3), 1, 1, 4, 9, 17, (3, 2))
    rc_arg, _ = c.plan(bad_window)
    dilated_s2 = c.layer(64, 64, (1, 3, 3), 2, 1, 2, 9, 17, dil=2)
    rc_unsupported, _ = c.plan(dilated_s2)
    assert rc_arg != 0 and rc_unsupported != 0 and rc_arg != rc_unsupported
    two_clips = c.layer(64, 64, (3, 3, 3), 1, 2, 4, 9, 17)
    two_clips['d'].update(out_t0=3, out_tn=2)
    assert c.plan(two_clips)[0] == 0                        # (the window is that of ONE clip: with two it does not apply)
