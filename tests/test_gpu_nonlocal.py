"""dat_nonlocal_attention (the fused attention of the spacetime non-local block) on the MI355X, through the C ABI,
in fp32 and in the loaded build's 16-bit format: every output element against float64 within the propagated bound of
tests/nonlocal_ref.py, plus the mean signed error that separates a P rounded to nearest from a truncated one; reproducibility, clip
independence, graph capture, the refusals; and dat_maxpool_hw with the block's pool parameters (k 2, stride 2, pad 0) on odd maps."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import nonlocal_ref as R
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


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


_REF = {}


def _case(name, fmt):
    """Operands and float64 reference of a case, computed once per format."""
    if (name, fmt) not in _REF:
        q, k, v, scale, clips = R.make_case(name, fmt)
        rows = R.bench_rows(q.shape[0]) if name == 'res4_bench' else None
        ref = R.reference(q if rows is None else q[rows], k, v, scale, clips)
        _REF[(name, fmt)] = (q, k, v, scale, clips, rows, ref)
    return _REF[(name, fmt)]


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
@pytest.mark.parametrize('name', [n for n in R.CASES if n not in ('strided', 'res4_bench')])
def test_attention_within_the_propagated_bound(ops, name, mode):
    fmt, dt, td = _modes(ops)[mode]
    q, k, v, scale, clips, _, ref = _case(name, fmt)
    D = q.shape[1]
    y = ops.nonlocal_attention(_dev(q, td), _dev(k, td), _dev(v, td), dt, clips, D, scale)
    assert y.shape == (q.shape[0], D) and y.dtype == td
    got = y.float().cpu().numpy()
    worst = R.check(got, ref, D, fmt, name)
    print('%s %s: worst err / bound %.3f' % (name, fmt, worst))
    if name == 'posv' and mode == 'h16':
        stat = R.truncation_statistic(got, ref) / nm.unit_roundoff(fmt)
        print('posv %s: mean signed error / A = %.4f u16' % (fmt, stat))
        assert abs(stat) <= 0.1, 'mean of (got - ref) / A is %.3f u16: P is not rounded to nearest before the PV product' % stat


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
def test_strided_operands_and_untouched_neighbours(ops, mode):
    """k and v are channels [0, 128) and [128, 256) of one [L', 320] blob, q sits at channel offset 64 of a wider blob full of junk, and
    y's rows are 192 wide: the other 64 channels keep their sentinel."""
    fmt, dt, td = _modes(ops)[mode]
    q, k, v, scale, clips, _, ref = _case('strided', fmt)
    L, D = q.shape
    Lk = k.shape[0]
    kv = torch.full((Lk, 320), 1000.0, dtype=td, device='cuda')
    kv[:, :128], kv[:, 128:256] = _dev(k, td), _dev(v, td)
    qw = torch.full((L, 256), 1000.0, dtype=td, device='cuda')
    qw[:, 64:192] = _dev(q, td)
    out = torch.full((L, 192), -7.0, dtype=td, device='cuda')
    ops.nonlocal_attention(qw[:, 64:192], kv[:, :128], kv[:, 128:256], dt, clips, D, scale, out=out)
    worst = R.check(out[:, :D].float().cpu().numpy(), ref, D, fmt, 'strided')
    print('strided %s: worst err / bound %.3f' % (fmt, worst))
    assert bool((out[:, D:] == -7.0).all()), 'channels behind D of the y rows were written'
    assert bool((kv[:, 256:] == 1000.0).all()) and bool((qw[:, :64] == 1000.0).all())


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
def test_res4_bench_shape_index_arithmetic_and_memory(ops, mode):
    """One res4 block of the benched clip (8 x 48 x 84 queries, 8 x 24 x 42 pooled keys, D 128): every 97th row and the last 64 against
    float64, and the call allocates y and nothing of the size of the scores (1 GB)."""
    fmt, dt, td = _modes(ops)[mode]
    q, k, v, scale, clips, rows, ref = _case('res4_bench', fmt)
    D = q.shape[1]
    qd, kd, vd = _dev(q, td), _dev(k, td), _dev(v, td)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    y = ops.nonlocal_attention(qd, kd, vd, dt, clips, D, scale)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert grown <= y.numel() * y.element_size() + (1 << 20), 'the call allocated %d bytes beyond y' % (grown - y.numel() * y.element_size())
    worst = R.check(y[torch.from_numpy(rows).cuda()].float().cpu().numpy(), ref, D, fmt, 'res4_bench')
    print('res4_bench %s: worst err / bound %.3f over %d rows' % (fmt, worst, len(rows)))


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
def test_two_calls_and_a_clip_alone_are_bit_identical(ops, mode):
    fmt, dt, td = _modes(ops)[mode]
    q, k, v, scale, clips, _, _ = _case('clips', fmt)
    L, Lk, D = q.shape[0] // clips, k.shape[0] // clips, q.shape[1]
    qd, kd, vd = _dev(q, td), _dev(k, td), _dev(v, td)
    a = ops.nonlocal_attention(qd, kd, vd, dt, clips, D, scale)
    b = ops.nonlocal_attention(qd, kd, vd, dt, clips, D, scale)
    assert torch.equal(_bits(a), _bits(b))
    alone = ops.nonlocal_attention(qd[L:2 * L].clone(), kd[Lk:2 * Lk].clone(), vd[Lk:2 * Lk].clone(), dt, 1, D, scale)
    assert torch.equal(_bits(a[L:2 * L]), _bits(alone)), 'clip 1 of 3 differs from the same clip run alone'


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
def test_captured_call_replayed_on_new_inputs_equals_eager(ops, mode):
    fmt, dt, td = _modes(ops)[mode]
    q, k, v, scale, clips, _, _ = _case('ragged', fmt)
    D = q.shape[1]
    qd, kd, vd = _dev(q, td), _dev(k, td), _dev(v, td)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = torch.empty((q.shape[0], D), dtype=td, device='cuda')
        ops.nonlocal_attention(qd, kd, vd, dt, clips, D, scale, out=out)        # warm-up on the capture stream (its context, the LDS limit)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ops.nonlocal_attention(qd, kd, vd, dt, clips, D, scale, out=out)
        q2, k2, v2 = R.make_case('ragged', fmt)[:3]
        qd.copy_(_dev(q2[::-1].copy(), td)); kd.copy_(_dev(0.5 * k2[::-1], td)); vd.copy_(_dev(v2[::-1].copy() + 1.0, td))
        g.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        eager = ops.nonlocal_attention(qd, kd, vd, dt, clips, D, scale)
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(_bits(replayed), _bits(eager))


def test_argument_errors_carry_their_text(ops):
    from detectandtrack_amd import libdat as L
    x = torch.zeros((64, 128), dtype=torch.float32, device='cuda')

    def call(D=64, ldq=128, Lk=64, q=x, dtype=ops.F32):
        d = L.NonLocalDesc()
        d.dtype, d.clips, d.Lq, d.Lk, d.D = dtype, 1, 64, Lk, D
        d.ldq, d.ldk, d.ldv, d.ldy, d.scale = ldq, 128, 128, 128, 1.0
        ops.ctx().call('dat_nonlocal_attention', ops._stream(), C.byref(d), ops._ptr(q), ops._ptr(x), ops._ptr(x), ops._ptr(x))

    call()
    for kw, match, code in (({'D': 96}, r'D = 96 channels', -4), ({'ldq': 68}, r'ldq = 68', -1), ({'q': None}, r'null pointer', -1),
                            ({'Lk': 0}, r'Lk = 0', -1), ({'dtype': 2}, r'dtype 2', -4)):
        with pytest.raises(L.DatError, match=match) as e:
            call(**kw)
        assert '(code %d)' % code in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((x == 0).all())


@pytest.mark.parametrize('mode', ['fp32', 'h16'])
@pytest.mark.parametrize('c', [64, 128])
def test_maxpool_k2_s2_p0_on_odd_maps(ops, c, mode):
    """The pool of the phi / g branches: MaxPool [1, 2, 2], stride [1, 2, 2], pad 0 (floor) -- the last row and column of an odd map are
    dropped.  Exact: a maximum rounds nothing."""
    _, dt, td = _modes(ops)[mode]
    x = torch.randn((3, 9, 11, c), generator=torch.Generator().manual_seed(c)).cuda().to(td)
    y = ops.maxpool_hw(x, dt, 2, 2, 0)
    ref = torch.nn.functional.max_pool2d(x.float().permute(0, 3, 1, 2), kernel_size=2, stride=2, padding=0).permute(0, 2, 3, 1)
    assert y.shape == (3, 4, 5, c)
    assert torch.equal(y.float(), ref)
