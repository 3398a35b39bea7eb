"""tests/dgrad_refs.py against itself and against autograd, on the CPU: the packed-layout restatement is a bijection and round-trips,
the float64 data gradient equals autograd's x.grad (full and sampled form), and every seeded defect of the device pipeline leaves
the per-element bound that tests/test_gpu_dgrad.py uses -- at every small case of its table, in fp32, bf16 and fp16 -- so that bound
can tell a wrong kernel from a right one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dgrad_refs as dr
from tests import numerics as nm

FMTS = ('fp32', 'bf16', 'fp16')
_ids = lambda cs: [c['name'] for c in cs]


# ---- the packed layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('pc', dr.PACK_CASES, ids=dr.pack_case_id)
def test_pack_index_is_a_bijection(pc, dtype):
    shape, dgrad = pc
    rows, cols = (shape[1], shape[0]) if dgrad else (shape[0], shape[1])
    d = dr.pack_desc(rows, cols, int(np.prod(shape[2:])))
    tap, co, ci = np.meshgrid(np.arange(d['ntap']), np.arange(d['cout_pad']), np.arange(d['cin']), indexing='ij')
    idx = dr.pack_index(tap, co, ci, d, dtype).reshape(-1)
    n = d['ntap'] * d['cout_pad'] * d['cin']
    assert idx.min() == 0 and idx.max() == n - 1 and np.unique(idx).size == n
    # the lane and slot rule of the layout comment, on one element: row 37, channel 85 of tap 1 (where the case has them)
    if d['ntap'] > 1 and d['cout_pad'] > 37 and d['cin'] > 85:
        es = 4 if dtype == 'fp32' else 2
        ck, eps = 128 // es, 16 // es
        chunk, within = 85 // ck, 85 % ck
        slot = within // eps
        lane = (slot % 2) * 32 + 37 % 32
        want = ((((1 * (d['cin'] // ck) + chunk) * (d['cout_pad'] // 32) + 37 // 32) * 4 + slot // 2) * 64 + lane) * eps + within % eps
        assert int(dr.pack_index(1, 37, 85, d, dtype)) == want


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
def test_unpack_of_pack_round_trips(dtype):
    for shape, dgrad in dr.PACK_CASES[:8]:
        w, scale = dr.pack_master(shape)
        logical, d = dr.packed_expected(w, scale, dgrad, dtype)
        img = dr.pack(logical, dtype)
        back = dr.unpack(img.view(torch.uint8), d, dtype)
        assert torch.equal(dr.bits(back), dr.bits(logical))
        # every element sits where pack_index says
        rs = np.random.RandomState(1)
        for _ in range(20):
            t, co, ci = rs.randint(d['ntap']), rs.randint(d['cout_pad']), rs.randint(d['cin'])
            assert dr.bits(img)[int(dr.pack_index(t, co, ci, d, dtype))] == dr.bits(logical)[t, co, ci]


def test_packed_expected_values_and_padding():
    w, scale = dr.pack_master((10, 7, 1, 3, 3))
    fwd, d = dr.packed_expected(w, None, False, 'fp32')
    assert (d['ntap'], d['cout_pad'], d['cin']) == (9, 64, 64)
    assert float(fwd[4, 3, 5]) == float(w.reshape(10, 7, 9)[3, 5, 4])
    assert torch.equal(dr.bits(fwd[:, 10:]), torch.zeros_like(dr.bits(fwd[:, 10:]))) and not fwd[:, :, 7:].any()
    dg, d = dr.packed_expected(w, scale, True, 'bf16')
    assert (d['cout_pad'], d['cin']) == (64, 64) and dg.dtype == torch.bfloat16
    want = torch.tensor(np.float32(w.reshape(10, 7, 9)[6, 2, 9 - 1 - 3]) * np.float32(scale[6])).to(torch.bfloat16)
    assert dr.bits(dg[3, 2, 6]) == dr.bits(want)
    assert torch.equal(dr.bits(dg[:, 7:]), torch.zeros_like(dr.bits(dg[:, 7:]))) and not dg[:, :, 10:].float().any()


@pytest.mark.parametrize('defect', dr.PACK_DEFECTS)
def test_every_packer_defect_changes_the_packed_bits(defect):
    """Bit equality with packed_expected is the whole criterion of tests/test_gpu_weight_pack.py: each defect must break it."""
    for shape in ((40, 24, 3, 3, 3), (24, 40, 3, 1, 1), (32, 32, 1, 3, 3)):
        k = shape[2:]
        case = dict(k=k, pads=(0, 0, 0), stride=(1, 1), H=8, W=8)
        w, scale = dr.pack_master(shape)
        for fmt in FMTS:
            if not dr.defect_applicable(defect, case, fmt):
                continue
            good, _ = dr.packed_expected(w, scale, True, fmt)
            bad, _ = dr.packed_expected(w, scale, True, fmt, defect=defect)
            assert not torch.equal(dr.bits(good), dr.bits(bad)), (defect, shape, fmt)


# ---- the float64 data gradient ---------------------------------------------------------------------------------------------------------
def _autograd_dx(case, o, base, mask):
    """x.grad of sum(y * g) through the forward conv in float64, + base, masked"""
    kt, pt = case['k'][0], case['pads'][0]
    x = torch.zeros(dr.x_shape(case), dtype=torch.float64, requires_grad=True)
    xp = F.pad(x, (0, 0, 0, 0, pt, kt - 1 - pt))
    y = F.conv3d(xp, torch.from_numpy(o['w']).double(), None, stride=(1,) + case['stride'], padding=(0,) + case['pads'][1:])
    y = y * torch.from_numpy(o['scale']).double().view(1, -1, 1, 1, 1)
    y.backward(torch.from_numpy(o['g']).double())
    dx = x.grad
    if base is not None:
        dx = dx + torch.from_numpy(base).double()
    if mask is not None:
        dx = torch.where(torch.from_numpy(mask).double() > 0, dx, torch.zeros_like(dx))
    return dx.numpy()


_REF = {}


def _ref(case, fmt, mode):
    key = (case['name'], fmt, mode)
    if key not in _REF:
        o = dr.case_operands(case, fmt)
        base, mask = dr.mode_operands(o, mode)
        _REF[key] = dr.dgrad_ref64(o['g'], o['w'], o['scale'], case['stride'], case['pads'], dr.x_shape(case), base, mask)
    return _REF[key]


@pytest.mark.parametrize('case', dr.SMALL_CASES, ids=_ids(dr.SMALL_CASES))
def test_dgrad_ref64_equals_autograd(case):
    o = dr.case_operands(case, 'fp32')
    for mode in ('plain', 'mask_accumulate'):
        base, mask = dr.mode_operands(o, mode)
        ref, absref = _ref(case, 'fp32', mode)
        want = _autograd_dx(case, o, base, mask)
        assert ref.shape == want.shape == dr.x_shape(case)
        scale_ = max(1.0, float(np.abs(want).max()))
        assert np.abs(ref - want).max() <= 1e-12 * scale_
        assert (absref + 1e-300 >= np.abs(ref)).all()


@pytest.mark.parametrize('case', dr.SMALL_CASES, ids=_ids(dr.SMALL_CASES))
def test_sampled_reference_equals_the_full_one(case):
    o = dr.case_operands(case, 'bf16')
    pos = dr.sample_positions(case['N'], case['T'], case['H'], case['W'], n_min=300, seed=3)
    for mode in ('plain', 'mask_accumulate'):
        base, mask = dr.mode_operands(o, mode)
        ref, absref = _ref(case, 'bf16', mode)
        sref, sabs = dr.dgrad_ref64(o['g'], o['w'], o['scale'], case['stride'], case['pads'], dr.x_shape(case), base, mask, positions=pos)
        assert sref.shape == (len(pos), case['cin'])
        assert np.abs(sref - dr.gather(ref, pos)).max() <= 1e-12 * max(1.0, float(np.abs(ref).max()))
        assert np.abs(sabs - dr.gather(absref, pos)).max() <= 1e-12 * max(1.0, float(absref.max()))


def test_g_frames_window_zeroes_the_other_frames():
    case = dr.SMALL_BY_NAME['k333_same']
    o = dr.case_operands(case, 'fp32')
    gw = o['g'].copy()
    gw[:, :, :1] = 0
    gw[:, :, 3:] = 0
    a = dr.dgrad_ref64(o['g'], o['w'], o['scale'], case['stride'], case['pads'], dr.x_shape(case), g_frames=(1, 2))
    b = dr.dgrad_ref64(gw, o['w'], o['scale'], case['stride'], case['pads'], dr.x_shape(case))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.abs(a[0]).max() > 0


def test_sample_positions_hold_what_every_sample_must():
    for case in dr.LARGE_CASES + dr.SMALL_CASES[:3]:
        pos = dr.sample_positions(case['N'], case['T'], case['H'], case['W'], seed=7)
        held = dr.sample_holds_the_required(pos, case['N'], case['T'], case['H'], case['W'])
        assert all(held.values()), (case['name'], held)
        assert len({tuple(p) for p in pos}) == len(pos)
    # ... and the check itself notices a sample without them
    case = dr.LARGE_CASES[2]
    pos = dr.sample_positions(case['N'], case['T'], case['H'], case['W'], seed=7)
    held = dr.sample_holds_the_required(pos[1:], case['N'], case['T'], case['H'], case['W'])
    assert not held['corners']


# ---- the bound separates right from wrong ------------------------------------------------------------------------------------------------
def test_the_case_table_has_the_shapes_a_flip_or_padding_mix_up_needs():
    ks = {c['k'] for c in dr.SMALL_CASES}
    assert (3, 1, 1) in ks and (1, 3, 3) in ks and any(c['k'] == (3, 3, 3) and c['pads'] == (1, 1, 1) for c in dr.SMALL_CASES)
    assert any(c['k'][0] == 3 and c['pads'][0] == 0 for c in dr.SMALL_CASES)          # k - 1 - p = 2 on the T axis
    assert any(c['cin'] != c['cout'] for c in dr.SMALL_CASES)
    # every defect is applicable somewhere, and no case hides more than one class of them behind a listed exclusion
    for d in dr.DX_DEFECTS:
        assert any(dr.defect_applicable(d, c) for c in dr.SMALL_CASES), d
    for c in dr.SMALL_CASES:
        assert len({dr.DEFECT_CLASS[d] for (n, d) in dr.INVISIBLE if n == c['name']}) <= 1


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('case', dr.SMALL_CASES, ids=_ids(dr.SMALL_CASES))
def test_the_correct_pipeline_is_inside_the_bound_and_every_seeded_defect_outside(case, fmt):
    """The device pipeline restated in float64 (packed weights rounded to the format, zero insertion, stride-1 conv with padding
    k - 1 - p, epilogue): without a defect inside the GPU test's bound at every element and in every mode -- the bound grants the
    packer's rounding -- and with each applicable defect outside it at some element."""
    o = dr.case_operands(case, fmt)
    xs = dr.x_shape(case)
    for mode in dr.MODES:
        base, mask = dr.mode_operands(o, mode)
        ref, absref = _ref(case, fmt, mode)
        got = dr.pipeline_dx64(o['g'], o['w'], o['scale'], case['stride'], case['pads'], xs, fmt, base, mask)
        b = dr.dx_bound(ref, absref, case, fmt)
        assert (np.abs(got - ref) <= b).all(), (mode, float((np.abs(got - ref) / b).max()))
    for defect in dr.DX_DEFECTS:
        if not dr.defect_applicable(defect, case, fmt) or (case['name'], defect) in dr.INVISIBLE:
            continue
        mode = 'mask_accumulate' if defect == 'mask_before_sum' else 'plain'
        base, mask = dr.mode_operands(o, mode)
        ref, absref = _ref(case, fmt, mode)
        bad = dr.pipeline_dx64(o['g'], o['w'], o['scale'], case['stride'], case['pads'], xs, fmt, base, mask, defect=defect)
        ratio = np.abs(bad - ref) / dr.dx_bound(ref, absref, case, fmt)
        assert ratio.max() > 1.0, 'defect %s stays inside the bound at %s in %s (worst err / bound %.3f)' % (defect, case['name'], fmt, ratio.max())
