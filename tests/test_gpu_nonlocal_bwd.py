"""dat_nonlocal_attention_lse / dat_nonlocal_attention_bwd / dat_maxpool_hw_bwd (the training kernels of the spacetime non-local block,
DESIGN.md section 3.17) on the MI355X, in fp32 and in the loaded build's 16-bit format: dq, dk, dv of every case against float64 within
the propagated bound of tests/nonlocal_grad_ref.py, the stored lse within its fp32 bound, y of the lse form bit-equal to the plain
forward; a frame window of the queries, strided operands with sentinel neighbours, reproducibility, clip independence, the refusals; and
the pool backward bit-equal to the float64 routing on odd maps with planted ties."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import nonlocal_grad_ref as G
from tests import numerics as nm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _modes(ops):
    return {'fp32': ('fp32', ops.F32, torch.float32), 'h16': ('fp16' if ops.H16_DTYPE == torch.float16 else 'bf16', ops.BF16, ops.H16_DTYPE)}


def _dev(a, td):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(td)


def _host(t):
    return t.float().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


_REF = {}


def _case(name, fmt):
    """Operands, float64 reference and bounds of a case, computed once per format and left unchanged."""
    if (name, fmt) not in _REF:
        q, k, v, dy, scale, clips = G.make_grad_case(name, fmt)
        ref = G.reference(q, k, v, dy, scale, clips)
        _REF[(name, fmt)] = (q, k, v, dy, scale, clips, ref, G.bounds(ref, fmt))
    return _REF[(name, fmt)]


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
@pytest.mark.parametrize('name', G.GRAD_CASES)
def test_gradients_lse_and_y(ops, name, mode):
    fmt, dt, td = _modes(ops)[mode]
    q, k, v, dy, scale, clips, ref, bnd = _case(name, fmt)
    D = q.shape[1]
    qd, kd, vd, dyd = (_dev(a, td) for a in (q, k, v, dy))
    y, lse = ops.nonlocal_attention_lse(qd, kd, vd, dt, clips, D, scale)
    plain = ops.nonlocal_attention(qd, kd, vd, dt, clips, D, scale)
    assert torch.equal(_bits(y), _bits(plain)), 'y of the lse form differs from the plain forward'
    lse_err = np.abs(lse.double().cpu().numpy() - ref['lse'])
    lse_ratio = float((lse_err / G.lse_bound(ref)).max())
    print('%s %s: lse worst err / bound %.3f' % (name, fmt, lse_ratio))
    assert np.isfinite(lse_err).all() and lse_ratio <= 1.0, 'lse: worst err / bound %.3g' % lse_ratio
    dq, dk, dv = ops.nonlocal_attention_bwd(qd, kd, vd, y, dyd, lse, dt, clips, D, scale)
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape and dq.dtype == td
    for n, t in (('dq', dq), ('dk', dk), ('dv', dv)):
        worst = G.check(_host(t), ref, bnd, n, name, fmt)
        print('%s %s: %s worst err / bound %.3f' % (name, fmt, n, worst))


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
def test_a_window_of_query_rows(ops, mode):
    """One clip: the backward over query rows [lo, lo + n) (contiguous row ranges of q, y, lse and dy) gives dq of that window and dk / dv
    over ALL keys -- the gradient of a dy that is zero outside the window."""
    fmt, dt, td = _modes(ops)[mode]
    q, k, v, dy, scale, clips, _, _ = _case('blocks', fmt)
    D, lo, n = q.shape[1], 150, 211
    dyw = np.zeros_like(dy)
    dyw[lo:lo + n] = dy[lo:lo + n]
    ref = G.reference(q, k, v, dyw, scale, 1)
    bnd = G.bounds(ref, fmt)
    qd, kd, vd, dyd = (_dev(a, td) for a in (q, k, v, dy))
    y, lse = ops.nonlocal_attention_lse(qd, kd, vd, dt, 1, D, scale)
    dq, dk, dv = ops.nonlocal_attention_bwd(qd[lo:lo + n], kd, vd, y[lo:lo + n], dyd[lo:lo + n], lse[lo:lo + n], dt, 1, D, scale)
    assert dq.shape == (n, D) and dk.shape == k.shape
    full = np.zeros_like(ref['dq'])
    full[lo:lo + n] = _host(dq)
    for nme, got in (('dq', full), ('dk', _host(dk)), ('dv', _host(dv))):
        print('window %s: %s worst err / bound %.3f' % (fmt, nme, G.check(got, ref, bnd, nme, 'window', fmt)))


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
def test_strided_operands_and_untouched_neighbours(ops, mode):
    """Every operand and output is a channel range and a row range of a wider, longer blob filled with a sentinel: the padding channels and
    the rows before and after keep it."""
    fmt, dt, td = _modes(ops)[mode]
    q, k, v, dy, scale, clips, ref, bnd = _case('ragged', fmt)
    L, D = q.shape
    Lk = k.shape[0]
    S = 500.0

    def wide(a, rows, width, c0, r0):
        t = torch.full((rows, width), S, dtype=td, device='cuda')
        if a is not None:
            t[r0:r0 + a.shape[0], c0:c0 + D] = _dev(a, td)
        return t

    qw, dyw = wide(q, L + 5, 192, 64, 2), wide(dy, L + 3, 72, 8, 1)
    kv = torch.full((Lk + 4, 200), S, dtype=td, device='cuda')
    kv[3:3 + Lk, :64], kv[3:3 + Lk, 128:192] = _dev(k, td), _dev(v, td)
    qv, kview, vview, dyv = qw[2:2 + L, 64:128], kv[3:3 + Lk, :64], kv[3:3 + Lk, 128:192], dyw[1:1 + L, 8:72]
    y, lse = ops.nonlocal_attention_lse(qv, kview, vview, dt, 1, D, scale)
    dqw, dkw, dvw = wide(None, L + 4, 136, 0, 0), wide(None, Lk + 6, 72, 0, 0), wide(None, Lk + 2, 128, 0, 0)
    dq, dk, dv = dqw[3:3 + L, 64:128], dkw[5:5 + Lk, 8:72], dvw[1:1 + Lk, :64]
    ops.nonlocal_attention_bwd(qv, kview, vview, y, dyv, lse, dt, 1, D, scale, dq=dq, dk=dk, dv=dv)
    for n, t in (('dq', dq), ('dk', dk), ('dv', dv)):
        print('strided %s: %s worst err / bound %.3f' % (fmt, n, G.check(_host(t), ref, bnd, n, 'strided', fmt)))
    for name, t, r0, rows, c0 in (('dq', dqw, 3, L, 64), ('dk', dkw, 5, Lk, 8), ('dv', dvw, 1, Lk, 0)):
        h = _host(t)
        h[r0:r0 + rows, c0:c0 + D] = S
        assert (h == S).all(), 'the backward wrote outside the %s view' % name
    for name, t, r0, rows, cols in (('q', qw, 2, L, (64, 128)), ('dy', dyw, 1, L, (8, 72))):
        h = _host(t)
        h[r0:r0 + rows, cols[0]:cols[1]] = S
        assert (h == S).all(), 'the neighbours of %s changed' % name
    h = _host(kv)
    h[3:3 + Lk, :64] = S
    h[3:3 + Lk, 128:192] = S
    assert (h == S).all(), 'the neighbours of k / v changed'


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
def test_two_calls_and_a_clip_alone_are_bit_identical(ops, mode):
    fmt, dt, td = _modes(ops)[mode]
    q, k, v, dy, scale, clips, _, _ = _case('clips', fmt)
    L, Lk, D = q.shape[0] // clips, k.shape[0] // clips, q.shape[1]
    qd, kd, vd, dyd = (_dev(a, td) for a in (q, k, v, dy))
    y, lse = ops.nonlocal_attention_lse(qd, kd, vd, dt, clips, D, scale)
    a = ops.nonlocal_attention_bwd(qd, kd, vd, y, dyd, lse, dt, clips, D, scale)
    b = ops.nonlocal_attention_bwd(qd, kd, vd, y, dyd, lse, dt, clips, D, scale)
    for x, z in zip(a, b):
        assert torch.equal(_bits(x), _bits(z))
    qs, ks = slice(L, 2 * L), slice(Lk, 2 * Lk)
    y1, lse1 = ops.nonlocal_attention_lse(qd[qs].clone(), kd[ks].clone(), vd[ks].clone(), dt, 1, D, scale)
    assert torch.equal(_bits(y1), _bits(y[qs])) and torch.equal(_bits(lse1), _bits(lse[qs]))
    alone = ops.nonlocal_attention_bwd(qd[qs].clone(), kd[ks].clone(), vd[ks].clone(), y1, dyd[qs].clone(), lse1, dt, 1, D, scale)
    for n, x, z in zip(('dq', 'dk', 'dv'), a, alone):
        assert torch.equal(_bits(x[qs] if n == 'dq' else x[ks]), _bits(z)), '%s of clip 1 of 3 differs from the same clip run alone' % n


def test_argument_errors_carry_their_text(ops):
    from detectandtrack_amd import libdat as L
    x = torch.zeros((64, 128), dtype=torch.float32, device='cuda')
    f = torch.zeros(64, dtype=torch.float32, device='cuda')

    def call(D=64, lddk=128, Lq=64, dq=x, dtype=ops.F32, lse=f):
        d = L.NonLocalBwdDesc()
        d.dtype, d.clips, d.Lq, d.Lk, d.D = dtype, 1, Lq, 64, D
        d.ldq, d.ldk, d.ldv, d.ldy, d.lddy, d.lddq, d.lddk, d.lddv, d.scale = 128, 128, 128, 128, 128, 128, lddk, 128, 1.0
        ops.ctx().call('dat_nonlocal_attention_bwd', ops._stream(), C.byref(d), ops._ptr(x), ops._ptr(x), ops._ptr(x), ops._ptr(x), ops._ptr(x),
                       ops._ptr(lse), ops._ptr(f), ops._ptr(dq), ops._ptr(x), ops._ptr(x))

    for kw, match, code in (({'D': 96}, r'D = 96 channels', -4), ({'lddk': 68}, r'lddk = 68', -1), ({'dq': None}, r'null pointer', -1),
                            ({'Lq': 0}, r'Lq = 0', -1), ({'dtype': 2}, r'dtype 2', -4), ({'lse': None}, r'null pointer', -1)):
        with pytest.raises(L.DatError, match=match) as e:
            call(**kw)
        assert '(code %d)' % code in str(e.value), str(e.value)
    with pytest.raises(L.DatError, match=r'windows must not overlap') as e:
        ops.ctx().call('dat_maxpool_hw_bwd', ops._stream(), ops.F32, ops._ptr(x), ops._ptr(x), ops._ptr(x), 1, 8, 8, 128, 3, 2, 0)
    assert '(code -1)' in str(e.value)
    d = L.NonLocalDesc()
    d.dtype, d.clips, d.Lq, d.Lk, d.D = ops.F32, 1, 64, 64, 64
    d.ldq, d.ldk, d.ldv, d.ldy, d.scale = 128, 128, 128, 128, 1.0
    with pytest.raises(L.DatError, match=r'lse is null'):
        ops.ctx().call('dat_nonlocal_attention_lse', ops._stream(), C.byref(d), ops._ptr(x), ops._ptr(x), ops._ptr(x), ops._ptr(x), None)
    torch.cuda.synchronize()
    assert bool((x == 0).all())


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
@pytest.mark.parametrize('c', [64, 128])
def test_maxpool_backward_routes_to_the_first_maximum(ops, c, mode):
    """The block's pool (k 2, stride 2, pad 0) on an odd map with planted ties (whole windows of equal values, pairs of equal maxima): dx
    is bit-equal to the float64 routing -- the gradient is copied, nothing is rounded -- and the last row and column get zero."""
    fmt, dt, td = _modes(ops)[mode]
    g = torch.Generator().manual_seed(c)
    x = torch.randn((3, 9, 11, c), generator=g).to(td).float()
    x[:, 2:4, 4:6, :] = 0.25                        # a window of four equal values
    x[:, 0, 1, ::2] = x[:, 0, 0, ::2] = 7.0         # two equal maxima side by side in every second channel
    x[:, 5, 6, 1::3] = x[:, 4, 7, 1::3] = 9.0       # ... and on the diagonal
    dy = torch.randn((3, 4, 5, c), generator=g).to(td).float()
    ref = G.maxpool_bwd(x.numpy(), dy.numpy(), 2, 2, 0)
    dx = ops.maxpool_hw_bwd(x.cuda().to(td), dy.cuda().to(td), dt, 2, 2, 0)
    assert dx.shape == x.shape and dx.dtype == td
    got = dx.float().cpu().numpy().astype(np.float64)
    assert np.array_equal(got, ref), '%d elements differ' % int((got != ref).sum())
    assert (got[:, 8] == 0).all() and (got[:, :, 10] == 0).all()
    # the P6 form (k 1, stride 2) is the same kernel's other non-overlapping case
    dy1 = torch.randn((3, 5, 6, c), generator=g).to(td).float()
    dx1 = ops.maxpool_hw_bwd(x.cuda().to(td), dy1.cuda().to(td), dt, 1, 2, 0)
    assert np.array_equal(dx1.float().cpu().numpy().astype(np.float64), G.maxpool_bwd(x.numpy(), dy1.numpy(), 1, 2, 0))
