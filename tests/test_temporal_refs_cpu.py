"""tests/temporal_refs.py on the CPU: the windowed float64 reference against an explicit per-frame, per-tap loop; every seeded frame-
indexing defect outside the per-element bound at every case of the GPU table (and the rounded reference inside it) in bf16, fp16 and
fp32; and what the table reaches of the kernels' frame bookkeeping."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import numerics as nm
from tests import temporal_refs as tr

FORMATS = ['bf16', 'fp16', 'fp32']


def _loop_ref(x, w, stride, pads, out_t, in_t):
    """out[n, :, fc] = sum over kt of conv2d(x[n, :, t + kt - pad_t], w[:, :, kt]), t = ot0 + fc, frames outside [0, T) and in_t skipped"""
    x, w = torch.from_numpy(x).double(), torch.from_numpy(w).double()
    N, _, T = x.shape[:3]
    KT = w.shape[2]
    ot0, otn = out_t if out_t is not None else (0, T)
    lo, hi = (in_t[0], in_t[0] + in_t[1]) if in_t is not None else (0, T)
    frames = []
    for n in range(N):
        for fc in range(otn):
            acc = None
            for kt in range(KT):
                tf = ot0 + fc + kt - pads[0]
                if tf < 0 or tf >= T or tf < lo or tf >= hi:
                    continue
                v = F.conv2d(x[n:n + 1, :, tf], w[:, :, kt], None, stride=stride, padding=(pads[1], pads[2]))[0]
                acc = v if acc is None else acc + v
            if acc is None:
                ho = (x.shape[3] + 2 * pads[1] - w.shape[3]) // stride[0] + 1
                wo = (x.shape[4] + 2 * pads[2] - w.shape[4]) // stride[1] + 1
                acc = torch.zeros((w.shape[0], ho, wo), dtype=torch.float64)
            frames.append(acc)
    return torch.stack(frames).view(N, otn, *frames[0].shape).permute(0, 2, 1, 3, 4).numpy()


LOOP_CASES = [
    # N, Cin, Cout, T, H, W, k, stride, pads, out_t, in_t
    (2, 3, 4, 4, 5, 6, (3, 3, 3), (1, 1), (1, 1, 1), None, None),
    (2, 3, 4, 4, 5, 6, (3, 3, 3), (1, 1), (1, 1, 1), (1, 2), None),
    (2, 3, 4, 4, 5, 6, (3, 3, 3), (2, 2), (1, 1, 1), None, (3, 1)),
    (2, 3, 4, 4, 5, 6, (3, 3, 3), (1, 1), (1, 1, 1), (2, 2), (1, 1)),      # both windows; frame 3 has no valid tap
    (3, 2, 5, 3, 4, 3, (3, 1, 1), (1, 1), (0, 0, 0), (0, 1), None),        # KT == T, pad_t 0: time moved to channels
    (3, 2, 5, 2, 4, 3, (2, 1, 1), (1, 1), (0, 0, 0), (0, 1), None),
    (2, 2, 3, 5, 4, 5, (3, 3, 3), (1, 1), (2, 1, 1), (2, 3), (1, 3)),      # pad_t == KT - 1
    (2, 2, 3, 5, 4, 5, (3, 1, 1), (1, 1), (0, 0, 0), (0, 5), (2, 2)),
    (1, 2, 3, 1, 4, 5, (3, 3, 3), (1, 1), (1, 1, 1), None, None),          # T = 1
]


@pytest.mark.parametrize('case', LOOP_CASES, ids=lambda c: 'T%d_k%d_pt%d_out%s_in%s' % (c[3], c[6][0], c[8][0], c[9], c[10]))
def test_reference_equals_the_per_frame_per_tap_loop(case):
    N, Cin, Cout, T, H, W, k, stride, pads, out_t, in_t = case
    rs = np.random.RandomState(T * 7 + k[0])
    x = rs.randn(N, Cin, T, H, W).astype(np.float32)
    w = rs.randn(Cout, Cin, *k).astype(np.float32)
    want = _loop_ref(x, w, stride, pads, out_t, in_t)
    ref, absref = tr.windowed_conv_ref64(x, w, None, None, None, stride, pads, False, out_t, in_t)
    assert ref.shape == want.shape
    np.testing.assert_allclose(ref, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(absref, _loop_ref(np.abs(x), np.abs(w), stride, pads, out_t, in_t), rtol=0, atol=1e-12)
    # the tap products every seeded defect is built from restate the same sum
    tp = tr.TapProducts(x, w, stride, pads)
    np.testing.assert_allclose(tp.sums(out_t, in_t).numpy(), want, rtol=0, atol=1e-12)
    # the epilogue chain: affine, + residual, ReLU, mask; mode 4 adds the addend under the mask
    otn = want.shape[2]
    scale, bias = rs.uniform(0.5, 1.5, Cout), rs.randn(Cout)
    res, mask, addend = (rs.randn(*want.shape) for _ in range(3))
    v = want * scale[None, :, None, None, None] + bias[None, :, None, None, None]
    got = tr.windowed_conv_ref64(x, w, scale, bias, res, stride, pads, True, out_t, in_t)[0]
    np.testing.assert_allclose(got, np.maximum(v + res, 0), rtol=0, atol=1e-12)
    got = tr.windowed_conv_ref64(x, w, scale, bias, None, stride, pads, False, out_t, in_t, mask=mask)[0]
    np.testing.assert_allclose(got, np.where(mask > 0, v, 0), rtol=0, atol=1e-12)
    got, a4 = tr.windowed_conv_ref64(x, w, scale, bias, None, stride, pads, False, out_t, in_t, mask=mask, addend=addend)
    np.testing.assert_allclose(got, np.where(mask > 0, v + addend, 0), rtol=0, atol=1e-12)
    assert (a4 >= np.abs(got) - 1e-12).all() and otn == (out_t[1] if out_t else T)


def test_bookkeeping_helper_on_known_frames():
    bk = tr.frame_bookkeeping(4, 3, 1)
    assert [f['n_kt'] for f in bk] == [2, 3, 3, 2] and [f['kshift'] for f in bk] == [False, False, True, False]
    bk = tr.frame_bookkeeping(4, 3, 1, in_t=(1, 1))
    assert [f['n_kt'] for f in bk] == [1, 1, 1, 0]
    bk = tr.frame_bookkeeping(4, 3, 1, out_t=(2, 2), in_t=(1, 1))
    assert [(f['t'], f['n_kt']) for f in bk] == [(2, 1), (3, 0)]
    # T = 1: one valid tap, the launcher allows (KT - 1) * n_cchunks = 2 splits (a forced 3 is capped to 2): split 0 gets [0, 0)
    assert tr.frame_bookkeeping(1, 3, 1, n_cchunks=1, ksplit=1)[0]['empty_split'] is False
    assert tr.frame_bookkeeping(1, 3, 1, n_cchunks=1, ksplit=2)[0]['empty_split'] is True
    assert tr.frame_bookkeeping(1, 3, 1, n_cchunks=1, ksplit=3)[0]['empty_split'] is True
    assert tr.frame_bookkeeping(1, 3, 1, n_cchunks=2, ksplit=2)[0]['empty_split'] is False
    assert tr.frame_bookkeeping(3, 3, 0, out_t=(0, 1))[0] == dict(t=0, n_kt=3, kshift=False, empty_split=False)


_TP = {}


COUT_KEPT = 32      # of a dense row's filters: which frames a result reads does not depend on the filter, the cost of this file does


def _kept(row):
    r = tr.ROWS[row]
    return slice(0, COUT_KEPT if r.get('groups', 1) == 1 else r['Cout'])


def _tap_products(row, fmt):
    if (row, fmt) not in _TP:
        r = tr.ROWS[row]
        x, w = tr.row_operands(row, fmt)[:2]
        _TP[(row, fmt)] = tr.TapProducts(x, w[_kept(row)], r['stride'], r['pads'], r.get('groups', 1))
    return _TP[(row, fmt)]


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('case', tr.CASES, ids=[c['id'] for c in tr.CASES])
def test_every_applicable_defect_is_outside_the_bound_and_the_reference_inside(case, fmt):
    r = tr.ROWS[case['row']]
    o, keep = tr.case_operands(case, fmt), _kept(case['row'])
    o.update({k: o[k][keep] for k in ('w', 'scale', 'bias') if o[k] is not None})
    o.update({k: o[k][:, keep] for k in ('res', 'mask', 'addend') if o[k] is not None})
    ref, absref = tr.case_ref64(case, fmt, o)
    K = nm.conv_k(r['Cin'] // r.get('groups', 1), r['k'])
    once = torch.from_numpy(ref).to(nm._fmt(fmt)).double().numpy()            # one correct rounding to the output format
    nm.assert_elementwise(once, ref, absref, K, fmt, case['id'])
    # discriminating inputs: x non-zero on the edge frames of the input window, clips and frames all different
    ot0, otn, in_lo, in_hi = tr._windows(r['T'], case['out_t'], case['in_t'])
    x = o['x']
    assert all(np.abs(x[n, :, t]).max() > 0.5 for n in range(r['N']) for t in (in_lo, in_hi - 1))
    assert not np.abs(x[:, :, :in_lo]).any() and not np.abs(x[:, :, in_hi:]).any()
    if r['N'] > 1:
        assert np.abs(x[0, :, in_lo] - x[1, :, in_lo]).max() > 0.5
    for a in (o['res'], o['mask'], o['addend']):
        if a is not None and a.shape[0] * a.shape[2] > 1:
            flat = a.transpose(0, 2, 1, 3, 4).reshape(a.shape[0] * a.shape[2], -1)
            assert all(np.abs(flat[i] - flat[j]).max() > 0.5 for i in range(len(flat)) for j in range(i))
    tp = _tap_products(case['row'], fmt)
    frame_operand = any(o[k] is not None for k in ('res', 'mask', 'addend'))
    np.testing.assert_allclose(tr.defective_ref64(tp, None, o['scale'], o['bias'], o['res'], o['relu'], case['out_t'], case['in_t'], o['mask'],
                                                  o['addend']), ref, rtol=0, atol=1e-9)
    applied = []
    for defect in tr.DEFECTS:
        if not tp.applicable(defect, case['out_t'], case['in_t'], frame_operand):
            continue
        bad = tr.defective_ref64(tp, defect, o['scale'], o['bias'], o['res'], o['relu'], case['out_t'], case['in_t'], o['mask'], o['addend'])
        try:
            nm.assert_elementwise(torch.from_numpy(bad).to(nm._fmt(fmt)).double().numpy(), ref, absref, K, fmt, defect)
        except AssertionError as e:
            assert 'outside the per-element bound' in str(e)
        else:
            pytest.fail('%s: the seeded defect %r stays inside the bound: the inputs do not discriminate' % (case['id'], defect))
        applied.append(defect)
    assert applied, 'no seeded defect applies to %s: the case checks no frame index' % case['id']


def test_the_case_table_reaches_every_bookkeeping_path():
    n_kts, kshift, empty, inner_window, first, last = set(), False, False, False, False, False
    defects = set()
    for case in tr.CASES:
        r = tr.ROWS[case['row']]
        T = r['T']
        for fmt in FORMATS:
            for ks in case['ksplits']:
                for f in tr.frame_bookkeeping(T, r['k'][0], r['pads'][0], case['out_t'], case['in_t'], tr.n_cchunks(case['row'], fmt), ks):
                    n_kts.add(f['n_kt'])
                    kshift |= f['kshift']
                    empty |= f['empty_split'] and ks > 1
        ot0, otn, in_lo, in_hi = tr._windows(T, case['out_t'], case['in_t'])
        inner_window |= otn > 1 and ot0 > 0
        for lo, hi in ([(ot0, ot0 + otn)] if case['out_t'] else []) + ([(in_lo, in_hi)] if case['in_t'] else []):
            first |= lo == 0 and hi < T
            last |= hi == T and lo > 0
        tp_like = tr.TapProducts.__new__(tr.TapProducts)
        tp_like.N, tp_like.T, tp_like.KT, tp_like.pads = r['N'], T, r['k'][0], r['pads']
        defects |= {d for d in tr.DEFECTS if tp_like.applicable(d, case['out_t'], case['in_t'], case['epi'] != 'none')}
    assert {0, 1, 2, 3} <= n_kts, n_kts
    assert kshift and empty and inner_window and first and last, (kshift, empty, inner_window, first, last)
    assert defects == set(tr.DEFECTS), set(tr.DEFECTS) - defects
    # every kernel family meets a frame without a valid tap and an output window that does not start at frame 0
    for rows in (('dense',), ('k311',), ('big_tile',), ('grouped', 'grouped_s2')):
        cs = [c for c in tr.CASES if c['row'] in rows]
        assert any(c['out_t'] and c['out_t'][0] > 0 for c in cs), rows
        assert any(f['n_kt'] == 0 for c in cs for f in tr.frame_bookkeeping(tr.ROWS[c['row']]['T'], 3, 1, c['out_t'], c['in_t'])), rows
