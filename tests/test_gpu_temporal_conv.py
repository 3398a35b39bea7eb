"""The temporal-tap K-streaming kernel (conv_kt1x1_ks_kernel): the kT x 1 x 1 convs of ResNet-(2+1)D blocks through
hip_ops.ConvLayer, every output element against a float64 reference under the per-element bound of tests/numerics.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import numerics as nm

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = 2560351                           # dispatcher tag of the kernel (256 channels x 256 positions per block, bf16)
GENERIC = 1281281                       # the generic kernel's plan for these layers (128 x 128, no split-K)

# name, clips N, T, H, W, Cin_real, Cout, kT, res_mode, relu.  H * W is never a multiple of 256 (tiles straddle frames and clips);
# every grid fills at least 3/4 of a round of the CUs, so the DEFAULT dispatch takes the kernel.
CASES = [
    ('m230_c256', 3, 8, 45, 47, 230, 256, 3, 0, True),                 # Cin 230 in a 256 stride (res3_0's mid planes)
    ('m288_c256_sum', 2, 5, 71, 73, 288, 256, 3, 1, True),             # Cin 288 in a 320 stride: Sum + ReLU
    ('res4_2a_m460_c256', 3, 3, 63, 95, 460, 256, 3, 0, False),        # R-18 res4_0_branch2a_temporal, no ReLU
    ('res4_2b_m576_c256_t1', 3, 1, 150, 115, 576, 256, 3, 1, True),    # T = 1: both side taps read zeros only
    ('res5_2a_m921_c512_t8', 2, 8, 39, 41, 921, 512, 3, 1, True),      # R-18 res5_0_branch2a_temporal: two cout blocks
    ('res5_2b_m1152_c512', 3, 5, 29, 59, 1152, 512, 3, 0, True),       # R-18 res5_x / R-50 res5 branch2b_temporal
    ('m256_c200_pad_t2', 2, 2, 99, 131, 256, 200, 3, 1, False),        # Cout padded to 256 in the blob: padding stays zero
    ('m256_c256_kt5_t8', 1, 8, 81, 79, 256, 256, 5, 1, True),          # TIME_KERNEL_DIM 5
]


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    if hip_ops.L.H16 == 'fp16':
        pytest.skip('the temporal kernel serves the bf16 build; the fp16 build keeps the generic kernel')
    return hip_ops


def _operands(case, seed=None):
    """bf16 NDHWC input (zero padding channels), fp32 weights / affine / residual with bf16 values, on the GPU."""
    name, N, T, H, W, cin, cout, kt, res_mode, relu = case
    g = torch.Generator(device='cuda')
    g.manual_seed(seed if seed is not None else sum(map(ord, name)))
    cs = (cin + 63) // 64 * 64
    x = torch.zeros((N * T, H, W, cs), dtype=torch.bfloat16, device='cuda')
    x[..., :cin] = torch.randn((N * T, H, W, cin), generator=g, device='cuda').to(torch.bfloat16)
    w = (torch.randn((cout, cin, kt, 1, 1), generator=g, device='cuda') * (2.0 / (cin * kt)) ** 0.5).to(torch.bfloat16).float()
    scale = torch.rand(cout, generator=g, device='cuda') + 0.5
    bias = torch.randn(cout, generator=g, device='cuda') * 0.1
    cstride = (cout + 63) // 64 * 64
    res = None
    if res_mode == 1:
        res = torch.zeros((N * T, H, W, cstride), dtype=torch.bfloat16, device='cuda')
        res[..., :cout] = torch.randn((N * T, H, W, cout), generator=g, device='cuda').to(torch.bfloat16)
    return x, w, scale, bias, res


def _ref64(case, x, w, scale, bias, res):
    """(ref, absref) float64, [N * T, H, W, Cout]: y[n, t] = sum_kt x[n, t + kt - kt // 2] W[:, :, kt]^T (zero frames outside the
    clip) * scale + bias (+ res), ReLU -- and the same chain on absolute values."""
    name, N, T, H, W, cin, cout, kt, res_mode, relu = case
    pt = kt // 2
    xd = x[..., :cin].double().reshape(N, T, H * W, cin)
    wd = w.double()[:, :, :, 0, 0]
    outs = []
    for absolute in (False, True):
        f = (lambda v: v.abs()) if absolute else (lambda v: v)
        xa, wa = f(xd), f(wd)
        y = torch.zeros((N, T, H * W, cout), dtype=torch.float64, device=x.device)
        for k in range(kt):
            lo, hi = max(0, pt - k), min(T, T + pt - k)          # output frames whose source frame t + k - pt lies in the clip
            if lo < hi:
                y[:, lo:hi] += torch.matmul(xa[:, lo + k - pt:hi + k - pt], wa[:, :, k].t())
        y = y * f(scale.double()) + f(bias.double())
        if res is not None:
            y = y + f(res[..., :cout].double().reshape(N, T, H * W, cout))
        if relu and not absolute:
            y = torch.relu(y)
        outs.append(y.reshape(N * T, H, W, cout).cpu().numpy())
    return outs


def _layer(ops, case, w, scale, bias):
    name, N, T, H, W, cin, cout, kt, res_mode, relu = case
    return ops.ConvLayer(w, scale, bias, stride=(1, 1), pads=(kt // 2, 0, 0), relu=relu, dtype=ops.BF16)


def _run(ops, layer, x, T, res, res_mode):
    prof = ops.ConvProfiler(capacity=8)
    prof.start()
    y = layer(x, T=T, residual=res, res_mode=res_mode)
    rec = prof.stop()
    return y, [t for t, _, _ in rec], rec


def _check(case, y, ref, what):
    name, N, T, H, W, cin, cout, kt, res_mode, relu = case
    nm.assert_elementwise(y[..., :cout].float(), ref[0], ref[1], nm.conv_k(cin, (kt, 1, 1)), 'bf16', what)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_temporal_conv_against_float64(ops, case):
    name, N, T, H, W, cin, cout, kt, res_mode, relu = case
    x, w, scale, bias, res = _operands(case)
    layer = _layer(ops, case, w, scale, bias)
    y, tags, rec = _run(ops, layer, x, T, res, res_mode)
    assert tags == [TAG], 'the default dispatch did not take the temporal kernel: tags %r' % (tags,)
    ref = _ref64(case, x, w, scale, bias, res)
    _check(case, y, ref, 'temporal ' + name)
    if layer.cstride > cout:       # (the allocation contract of ConvLayer: the kernel, like conv1x1_ks_kernel, stores no channel >= Cout)
        assert not y[..., cout:].any(), 'padding channels of the output are not zero'
    # the generic kernel (a forced plan keeps it) on the same operands: within the same bound
    try:
        assert ops.tune_plan(128, 1) == 0
        y_gen, tags_gen, _ = _run(ops, layer, x, T, res, res_mode)
    finally:
        ops.tune_plan(0, 0)
    assert tags_gen == [GENERIC], tags_gen
    _check(case, y_gen, ref, 'generic ' + name)
    print('temporal %s: %.1f us' % (name, 1e3 * rec[0][2]))


def test_a_clip_alone_equals_the_same_clip_in_a_batch_of_three(ops):
    """Tiles of the batch straddle clip boundaries; no row may read another clip's frames: clip 1 of a batch of three is bit for bit
    clip 1 computed alone (both grids are large enough for the kernel)."""
    case = ('clip_vs_batch', 3, 8, 49, 63, 921, 512, 3, 1, True)
    name, N, T, H, W, cin, cout, kt, res_mode, relu = case
    x, w, scale, bias, res = _operands(case)
    layer = _layer(ops, case, w, scale, bias)
    y3, tags3, _ = _run(ops, layer, x, T, res, res_mode)
    y1, tags1, _ = _run(ops, layer, x[T:2 * T].contiguous(), T, res[T:2 * T].contiguous(), res_mode)
    assert tags3 == tags1 == [TAG], (tags3, tags1)
    assert torch.equal(y1, y3[T:2 * T]), 'clip 1 differs alone and in the batch in %d elements' % int((y1 != y3[T:2 * T]).sum())
    _check(case, y3, _ref64(case, x, w, scale, bias, res), 'batch of three')


@pytest.mark.parametrize('shape', [(2, 8, 96, 168, 288, 128), (1, 8, 24, 42, 1152, 512), (1, 8, 48, 84, 576, 256)],
                         ids=['res3_c128_2clips', 'res5_1clip', 'res4_1clip'])
def test_layers_the_kernel_loses_stay_on_the_generic_kernel(ops, shape):
    """The dispatch rule follows the measured A/B: Cout-128 layers (res3) and grids under 3/4 block per CU (res4 /
    res5 of one 768 x 1344 clip) keep the generic kernel."""
    N, T, H, W, cin, cout = shape
    case = ('generic', N, T, H, W, cin, cout, 3, 1, True)
    x, w, scale, bias, res = _operands(case)
    y, tags, _ = _run(ops, _layer(ops, case, w, scale, bias), x, T, res, 1)
    assert tags == [GENERIC], tags


def _child(path):
    """DAT_CONV_TEMPORAL=0 child: the layer of `path` (.pt of operands) on the old dispatch; writes its output and tags."""
    from detectandtrack_amd.ops import hip_ops as ops
    d = torch.load(path)
    case = tuple(d['case'])
    x, w, scale, bias, res = [None if d[k] is None else d[k].cuda() for k in ('x', 'w', 'scale', 'bias', 'res')]
    y, tags, _ = _run(ops, _layer(ops, case, w, scale, bias), x, case[2], res, case[8])
    torch.cuda.synchronize()
    torch.save({'y': y.cpu(), 'tags': tags}, path + '.out')


@pytest.mark.parametrize('idx', [1, 4])
def test_old_dispatch_child_agrees_within_the_bound(ops, tmp_path, idx):
    case = CASES[idx]
    name = case[0]
    x, w, scale, bias, res = _operands(case)
    path = str(tmp_path / 'operands.pt')
    torch.save({'case': list(case), 'x': x.cpu(), 'w': w.cpu(), 'scale': scale.cpu(), 'bias': bias.cpu(),
                'res': None if res is None else res.cpu()}, path)
    env = dict(os.environ, DAT_CONV_TEMPORAL='0')
    code = 'import sys; sys.path.insert(0, %r); from tests.test_gpu_temporal_conv import _child; _child(%r)' % (REPO, path)
    p = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors='replace')[-4000:]
    out = torch.load(path + '.out')
    assert out['tags'] == [GENERIC], out['tags']
    layer = _layer(ops, case, w, scale, bias)
    y, tags, _ = _run(ops, layer, x, case[2], res, case[8])
    assert tags == [TAG], tags
    ref = _ref64(case, x, w, scale, bias, res)
    _check(case, out['y'], ref, 'DAT_CONV_TEMPORAL=0 ' + name)
    _check(case, y, ref, 'temporal ' + name)


@pytest.mark.parametrize('accumulate', [False, True])
def test_bf16_data_gradient_of_a_temporal_layer(ops, accumulate):
    """The data gradient of a kT x 1 x 1 layer in a bf16 training step (hip_ops.ConvGrad.data: flipped, transposed, scale-folded
    weights) takes the kernel too -- plain, and summed in place into the other contribution (res_mode 1, residual == output).
    Against float64: dx[t] = sum_k g[t + pt - k] (w[:, :, k] * scale)."""
    N, T, H, W, cin, cout, kt = 2, 8, 45, 71, 460, 256, 3           # R-18 res4_0_branch2a_temporal (M = 460 -> 256)
    pt = kt // 2
    gen = torch.Generator(device='cuda')
    gen.manual_seed(11 + accumulate)
    w = (torch.randn((cout, cin, kt, 1, 1), generator=gen, device='cuda') * (2.0 / (cin * kt)) ** 0.5).to(torch.bfloat16).float()
    scale = 2.0 ** torch.randint(-1, 2, (cout,), generator=gen, device='cuda').float()    # powers of two: w * scale stays a bf16 value
    g = torch.randn((N * T, H, W, cout), generator=gen, device='cuda').to(torch.bfloat16)
    cs = (cin + 63) // 64 * 64                                         # dL/dx's channel stride (512)
    acc = None
    if accumulate:
        acc = torch.zeros((N * T, H, W, cs), dtype=torch.bfloat16, device='cuda')
        acc[..., :cin] = torch.randn((N * T, H, W, cin), generator=gen, device='cuda').to(torch.bfloat16)
    acc0 = None if acc is None else acc.clone()
    cg = ops.ConvGrad(w, scale, (1, 1), (pt, 0, 0), ops.BF16, cs, cout)
    prof = ops.ConvProfiler(capacity=8)
    prof.start()
    dx = cg.data(g, T, H, W, accumulate_into=acc)
    tags = [t for t, _, _ in prof.stop()]
    assert tags == [TAG], 'the data gradient did not take the temporal kernel: tags %r' % (tags,)   # (its Cout 460 pads to 512)
    if accumulate:
        assert dx.data_ptr() == acc.data_ptr()
    ws = (w * scale.view(-1, 1, 1, 1, 1)).double()[:, :, :, 0, 0]             # [cout, cin, kt]
    gd = g.double().reshape(N, T, H * W, cout)
    outs = []
    for absolute in (False, True):
        f = (lambda v: v.abs()) if absolute else (lambda v: v)
        ref = torch.zeros((N, T, H * W, cin), dtype=torch.float64, device='cuda')
        for k in range(kt):
            lo, hi = max(0, k - pt), min(T, T + k - pt)           # input frames t whose output frame t + pt - k lies in the clip
            if lo < hi:
                ref[:, lo:hi] += torch.matmul(f(gd[:, lo + pt - k:hi + pt - k]), f(ws[:, :, k]))
        if acc0 is not None:
            ref = ref + f(acc0[..., :cin].double().reshape(N, T, H * W, cin))
        outs.append(ref.reshape(N * T, H, W, cin).cpu().numpy())
    assert dx.shape == (N * T, H, W, cs) and not dx[..., cin:].any()
    nm.assert_elementwise(dx[..., :cin].float(), outs[0], outs[1], nm.conv_k(cout, (kt, 1, 1)), 'bf16', 'data gradient, accumulate=%s' % accumulate)
