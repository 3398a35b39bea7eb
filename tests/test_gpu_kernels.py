"""GPU parity tests: every HIP kernel, called through the C ABI, against the CPU oracle."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import numerics as nm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bf16_only(ops):
    """Tests of the bf16-only modes (bf16x3, split_bf16x2): the fp16 build refuses them."""
    if ops.L.H16 == 'fp16':
        pytest.skip('bf16 build only')


def _bound(got, ref_args, cin, k, what, extra=0.0):
    """The per-element bound (tests/numerics.py) of a conv output in the build's 16-bit format: ref_args = the conv_ref64 arguments."""
    ref64, abs64 = nm.conv_ref64(*ref_args)
    nm.assert_elementwise(got, ref64, abs64, nm.conv_k(cin, k), nm.h16(), what, extra)


# ------------------------------------------------------------------------------------------------------
def test_zero_even(ops):
    # reference tests/test_zero_even_op.py:24-113: empty, odd/even lengths, shape error text
    for n in (0, 1, 2, 5, 6, 1001):
        x = torch.arange(1, n + 1, dtype=torch.float32).cuda()
        y = ops.zero_even(x.clone()).cpu().numpy()
        exp = np.arange(1, n + 1, dtype=np.float32)
        exp[0::2] = 0
        np.testing.assert_array_equal(y, exp)
    from detectandtrack_amd.libdat import DatError
    with pytest.raises(DatError, match=r'X\.ndim\(\) == 1'):
        ops.zero_even(torch.zeros(2, 2).cuda())


@pytest.mark.parametrize('shape', [(2, 5, 7), (1, 64, 3, 8, 12), (3, 16, 4, 4), (1, 3, 2, 5, 5)])
def test_affine_channel_nd(ops, shape):
    rs = np.random.RandomState(0)
    x = rs.randn(*shape).astype(np.float32)
    s = rs.uniform(0.5, 1.5, shape[1]).astype(np.float32)
    b = rs.randn(shape[1]).astype(np.float32)
    bs = [1, -1] + [1] * (len(shape) - 2)
    exp = x * s.reshape(bs) + b.reshape(bs)
    xd = _dev(x)
    y = ops.affine_channel_nd(xd, _dev(s), _dev(b))
    np.testing.assert_allclose(y.cpu().numpy(), exp, rtol=0, atol=1e-6)
    ops.affine_channel_nd(xd, _dev(s), _dev(b), out=xd)  # in-place (affine_channel_nd_op.cc:23-24)
    np.testing.assert_allclose(xd.cpu().numpy(), exp, rtol=0, atol=1e-6)
    g = ops.affine_channel_nd_grad(_dev(x), _dev(s))
    np.testing.assert_allclose(g.cpu().numpy(), x * s.reshape(bs), rtol=0, atol=1e-6)


def _digest(t):
    import hashlib
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def _affine_digests():
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_affine_gpu.json')) as f:
        return json.load(f)


def _ref_affine():
    from oracle import build_ref
    lib = build_ref.load_affine()
    if lib is None:
        pytest.skip('oracle/_ref/libref_affine.so was never built (oracle/build_ref.py needs /root/reference once)')
    return lib


@pytest.mark.parametrize('shape', [(2, 5, 7), (1, 64, 8, 48, 84), (3, 16, 4, 4), (1, 3, 2, 5, 5), (4, 256, 1), (1, 64, 3, 191, 333),
                                   (8, 2048, 1, 24, 42)])
def test_affine_channel_nd_matches_the_reference_cuda_op_compiled_for_gfx950(ops, shape):
    """VERDICT r4 item 3b -- the ONE floating-point operator whose source is in the reference tree, pinned: the reference's own
    `AffineChannelNdOp<float, CUDAContext>::RunOnDevice` / `AffineChannelNdGradientOp` (lib/ops/affine_channel_nd_op.cu:50-92, its kernels
    :20-46, its grid computation) compiled by hipcc from where the file lies (oracle/build_ref.py -> oracle/_ref/libref_affine.so) and run
    on this GPU.  dat_affine_channel_nd_fwd / _bwd are BIT-IDENTICAL to it (same x*s + b per element, both contracted to one fma by
    hipcc), out of place and in place; the NumPy / torch oracle expression (separate multiply and add) is within one rounding of it.
    Where oracle/_ref was never built, the reference op's outputs on these inputs are the SHA-256 digests stored in
    tests/golden/reference_affine_gpu.json (make_golden.py golden_affine_gpu): a result that hashes to one IS bit-identical to it."""
    import ctypes as C
    from oracle import build_ref
    lib = build_ref.load_affine()
    want = None if lib is not None else _affine_digests()['x'.join(str(v) for v in shape)]
    rs = np.random.RandomState(5)
    n, c = shape[0], shape[1]
    inner = int(np.prod(shape[2:]))
    x = (rs.randn(*shape) * 3).astype(np.float32)
    s = rs.uniform(0.5, 1.5, c).astype(np.float32)
    b = rs.randn(c).astype(np.float32)
    xd, sd, bd = _dev(x), _dev(s), _dev(b)
    err = C.create_string_buffer(256)
    y = ops.affine_channel_nd(xd, sd, bd)
    torch.cuda.synchronize()
    if lib is not None:
        y_ref = torch.empty_like(xd)
        assert lib.ref_affine_channel_nd_fwd(xd.data_ptr(), sd.data_ptr(), bd.data_ptr(), y_ref.data_ptr(), n, c, inner, c, err, 256) == 0, err.value
        torch.cuda.synchronize()
        np.testing.assert_array_equal(y.cpu().numpy(), y_ref.cpu().numpy())
    else:
        assert _digest(y) == want['fwd']
        y_ref = y.clone()
    # the oracle's expression (oracle/net3d.py Net.affine: x * s + b, two roundings) against the reference's fused one
    bs = [1, -1] + [1] * (len(shape) - 2)
    exp = x * s.reshape(bs) + b.reshape(bs)
    ulp = np.spacing(np.maximum(np.abs(exp), np.abs(x * s.reshape(bs))).astype(np.float32))
    assert np.all(np.abs(exp - y_ref.cpu().numpy()) <= ulp)
    # in place: the op's schema allows Y == X (affine_channel_nd_op.cc:23-24)
    x2, x3 = xd.clone(), xd.clone()
    ops.affine_channel_nd(x3, sd, bd, out=x3)
    if lib is not None:
        assert lib.ref_affine_channel_nd_fwd(x2.data_ptr(), sd.data_ptr(), bd.data_ptr(), x2.data_ptr(), n, c, inner, c, err, 256) == 0
        np.testing.assert_array_equal(x3.cpu().numpy(), x2.cpu().numpy())
    else:
        assert _digest(x3) == want['fwd_in_place']
        x2 = x3
    np.testing.assert_array_equal(x2.cpu().numpy(), y_ref.cpu().numpy())
    # gradient: dX = dY * scale (no scale / bias gradients, affine_channel_nd_op.cu:74-92) -- exact in any evaluation order
    g = ops.affine_channel_nd_grad(xd, sd)
    if lib is not None:
        g_ref = torch.empty_like(xd)
        assert lib.ref_affine_channel_nd_bwd(sd.data_ptr(), xd.data_ptr(), g_ref.data_ptr(), n, c, inner, c, err, 256) == 0
        np.testing.assert_array_equal(g.cpu().numpy(), g_ref.cpu().numpy())
    else:
        assert _digest(g) == want['bwd']
        g_ref = g
    np.testing.assert_array_equal(g_ref.cpu().numpy(), x * s.reshape(bs))


def test_reference_affine_op_enforces_the_channel_count():
    """The reference op CAFFE_ENFORCEs X.dim32(1) == scale.size() (affine_channel_nd_op.cu:64-65); the compiled reference reports it."""
    import ctypes as C
    lib = _ref_affine()
    x = torch.zeros(1, 4, 6, device='cuda')
    s = torch.ones(3, device='cuda')
    err = C.create_string_buffer(256)
    assert lib.ref_affine_channel_nd_fwd(x.data_ptr(), s.data_ptr(), s.data_ptr(), x.data_ptr(), 1, 4, 6, 3, err, 256) == -1
    assert b'X.dim32(1)' in err.value and b'scale.size()' in err.value


@pytest.mark.parametrize('dtype', [0, 1])
def test_layout_roundtrip(ops, dtype):
    rs = np.random.RandomState(1)
    x = rs.randn(2, 5, 3, 9, 11).astype(np.float32)
    nd = ops.to_ndhwc(_dev(x), dtype, 64)
    assert nd.shape == (6, 9, 11, 64)
    ref = np.transpose(x, (0, 2, 3, 4, 1)).reshape(6, 9, 11, 5)
    got = nd.float().cpu().numpy()
    tol = 0 if dtype == 0 else 2e-2
    np.testing.assert_allclose(got[..., :5], ref, rtol=tol, atol=tol)
    assert np.all(got[..., 5:] == 0)
    back = ops.to_ncdhw(nd, dtype, 2, 5, 3).cpu().numpy()
    np.testing.assert_allclose(back, x, rtol=tol, atol=tol)
    if dtype == 1:      # the conversion is torch's round to nearest even, bit for bit, and the way back is exact
        assert nd.dtype == nm.h16()
        np.testing.assert_array_equal(got[..., :5], nm.q16(ref))
        np.testing.assert_array_equal(back, nm.q16(x))


# ------------------------------------------------------------------------------------------------------
CONV_CASES = [
    # name, N, T, H, W, Cin, Cout, (kt,kh,kw), (sh,sw), relu, res_mode, affine
    ('1x1', 1, 2, 12, 20, 64, 128, (1, 1, 1), (1, 1), False, 0, True),
    ('3x3_2d', 1, 1, 17, 23, 64, 64, (1, 3, 3), (1, 1), True, 0, True),
    ('3x3x3', 1, 4, 14, 18, 64, 128, (3, 3, 3), (1, 1), True, 1, True),
    ('3x3x3_thin', 1, 4, 14, 18, 128, 64, (3, 3, 3), (1, 1), True, 1, True),    # 3 taps per step, 6 patches
    ('3x3x3_c256', 1, 3, 9, 21, 128, 256, (3, 3, 3), (1, 1), False, 0, False),
    ('3x3_s2', 1, 2, 20, 28, 64, 128, (3, 3, 3), (2, 2), True, 0, True),
    ('1x1_s2', 1, 2, 20, 28, 128, 256, (1, 1, 1), (2, 2), False, 0, True),
    ('1x1_up2', 1, 2, 8, 12, 128, 256, (1, 1, 1), (1, 1), False, 2, False),
    ('3x3_batch', 3, 1, 14, 14, 64, 64, (1, 3, 3), (1, 1), True, 0, False),
    ('cout12', 1, 1, 10, 14, 64, 12, (1, 1, 1), (1, 1), False, 0, False),
    ('fc_like', 1, 1, 1, 37, 448, 96, (1, 1, 1), (1, 1), True, 0, False),
    ('wide', 1, 1, 6, 150, 64, 64, (1, 3, 3), (1, 1), False, 0, True),
    ('1x1_s2_big', 1, 2, 400, 384, 128, 256, (1, 1, 1), (2, 2), False, 0, True),       # 76800 outputs: strided 1x1 on a large grid
    # RoI-head maps: linear position tiling (tiles of consecutive positions across rows and maps, border taps read a zero row)
    ('heads_14x14', 7, 1, 14, 14, 128, 256, (1, 3, 3), (1, 1), True, 1, True),
    ('heads_7x7', 9, 1, 7, 7, 64, 128, (1, 3, 3), (1, 1), True, 0, False),
    ('heads_14x14_many', 40, 1, 14, 14, 64, 128, (1, 3, 3), (1, 1), False, 0, True),
    ('heads_5x9_odd', 11, 1, 5, 9, 64, 192, (1, 3, 3), (1, 1), True, 1, False),
    # a grid just above one block per CU: 308 linear tiles of 256 positions
    ('heads_100x14x14_c512', 100, 1, 14, 14, 64, 512, (1, 3, 3), (1, 1), True, 1, True),
    # temporal taps on maps that 2-D tiles cover badly (res5 / res4 of the 3-D bodies): one linear strip per frame, two clips
    ('res5_like_24x42', 2, 4, 24, 42, 128, 256, (3, 3, 3), (1, 1), True, 1, True),
    ('res4_like_48x84', 1, 3, 48, 84, 64, 128, (3, 3, 3), (1, 1), True, 0, True),
]


def _conv_ref(x, w, scale, bias, res, stride, pads, relu):
    y = F.conv3d(torch.from_numpy(x), torch.from_numpy(w), None, stride=(1,) + stride, padding=pads)
    if scale is not None:
        y = y * torch.from_numpy(scale).view(1, -1, 1, 1, 1)
    if bias is not None:
        y = y + torch.from_numpy(bias).view(1, -1, 1, 1, 1)
    if res is not None:
        y = y + torch.from_numpy(res)
    return (F.relu(y) if relu else y).numpy()


@pytest.mark.parametrize('dtype', [0, 1, 2], ids=['fp32', 'bf16', 'bf16x3'])
@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv3d(ops, case, dtype):
    """dtype 2 = the bf16x3 mode (round 4): fp32 tensors, the conv on hi / lo bf16 splits of both operands (three bf16 MFMAs per
    k-slice, fp32 accumulate) -- held to 5e-4 against the fp32 reference (fp32 MFMA mode: 2e-4; plain bf16: 3e-2)."""
    name, N, T, H, W, Cin, Cout, k, s, relu, res_mode, affine = case
    x3, dtype = dtype == 2, (0 if dtype == 2 else dtype)
    if x3:
        _bf16_only(ops)
    rs = np.random.RandomState(abs(hash(name)) % 1000)
    x = rs.randn(N, Cin, T, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, *k) * np.sqrt(2.0 / (Cin * k[0] * k[1] * k[2]))).astype(np.float32)
    scale = rs.uniform(0.5, 1.5, Cout).astype(np.float32) if affine else None
    bias = (rs.randn(Cout) * 0.1).astype(np.float32)
    pads = (k[0] // 2, k[1] // 2, k[2] // 2)
    Ho = (H + 2 * pads[1] - k[1]) // s[0] + 1
    Wo = (W + 2 * pads[2] - k[2]) // s[1] + 1
    res = None
    res_small = None
    if res_mode == 1:
        res = rs.randn(N, Cout, T, Ho, Wo).astype(np.float32)
    elif res_mode == 2:
        res_small = rs.randn(N, Cout, T, Ho // 2, Wo // 2).astype(np.float32)
        res = np.repeat(np.repeat(res_small, 2, axis=3), 2, axis=4)
    if dtype == 1:  # 16-bit: quantise the operands the kernel will see, so only accumulation order differs
        q = nm.q16
        x, w = q(x), q(w)
        if res is not None:
            res = q(res)
            res_small = q(res_small) if res_small is not None else None
    ref = _conv_ref(x, w, scale, bias, res, s, pads, relu)
    layer = ops.ConvLayer(_dev(w), None if scale is None else _dev(scale), _dev(bias), stride=s, pads=pads,
                          relu=relu, dtype=dtype, x3=x3)
    xd = ops.to_ndhwc(_dev(x), dtype)
    rd = None
    if res_mode == 1:
        rd = ops.to_ndhwc(_dev(res), dtype, layer.cstride)
    elif res_mode == 2:
        rd = ops.to_ndhwc(_dev(res_small), dtype, layer.cstride)
    y = layer(xd, T=T, residual=rd, res_mode=res_mode)
    if x3 and layer.cstride == layer.cout:
        # the split of the OUTPUT written by the same launch (dat_conv3d_fwd_x3) is bit for bit dat_split_bf16x2 of the stored output --
        # under the planner's plan and under a forced split-K plan (the finish kernel writes it then)
        for plan in ((0, 0), (128, 2)):
            try:
                assert ops.tune_plan(*plan) == 0
                y2 = layer(xd, T=T, residual=rd, res_mode=res_mode, want_split=True)
            finally:
                ops.tune_plan(0, 0)
            assert y2._split is not None and y2._split.shape[-1] == 2 * layer.cstride
            assert torch.equal(y2._split, ops.split_bf16x2(y2)), (name, plan)
            if plan == (0, 0):
                assert torch.equal(y2, y)
    got = ops.to_ncdhw(y, dtype, N, Cout, T).cpu().numpy()
    err = np.abs(got - ref).max()
    tol = (5e-4 if x3 else 2e-4) if dtype == 0 else 3e-2 * max(1.0, np.abs(ref).max() / 4)
    print('conv %s dtype=%s max-abs err %.3e (ref max %.2f)' % (name, 'bf16x3' if x3 else dtype, err, np.abs(ref).max()))
    assert err < tol
    if dtype == 1:
        _bound(got, (x, w, scale, bias, res, s, pads, relu), Cin, k, 'conv ' + name)
        try:                    # the same layer under a forced split-K plan (the split-K finish kernel writes the output)
            assert ops.tune_plan(128, 2) == 0
            y_sk = layer(xd, T=T, residual=rd, res_mode=res_mode)
        finally:
            ops.tune_plan(0, 0)
        _bound(ops.to_ncdhw(y_sk, dtype, N, Cout, T).cpu().numpy(), (x, w, scale, bias, res, s, pads, relu), Cin, k,
               'conv split-K ' + name)


WS64_CASES = [
    # name, frames, H, W, relu, residual, affine   (3x3, 64 -> 64, bf16: the persistent weights-stationary kernel)
    ('ragged_16x16', 2, 37, 53, True, True, True),          # 16 x 16 tiles, ragged in both directions
    ('tiny', 1, 3, 5, False, False, False),                 # smaller than one tile
    ('long_rows_8x32', 1, 8, 9600, True, False, True),      # 8 x 32 tiles (fewer rounds of the persistent grid), > 256 tiles
    ('res2_like', 8, 96, 168, True, True, True),            # many tiles per block: the double-buffered patch pipeline
]


@pytest.mark.parametrize('case', WS64_CASES, ids=[c[0] for c in WS64_CASES])
def test_conv3x3_c64_weights_stationary(ops, case):
    """conv3x3_c64_ws_kernel (3x3, 64 -> 64 channels, bf16; weights resident in registers, persistent blocks) against torch on the
    same bf16 operands, and bit for bit against the generic kernel (forced plan: same tap / k-slice accumulation order)."""
    name, frames, H, W, relu, with_res, affine = case
    rs = np.random.RandomState(len(name) * 7 + H)
    q = nm.q16
    x = q(rs.randn(1, 64, frames, H, W).astype(np.float32))
    w = q((rs.randn(64, 64, 1, 3, 3) * np.sqrt(2.0 / (64 * 9))).astype(np.float32))
    scale = rs.uniform(0.5, 1.5, 64).astype(np.float32) if affine else None
    bias = (rs.randn(64) * 0.1).astype(np.float32)
    res = q(rs.randn(1, 64, frames, H, W).astype(np.float32)) if with_res else None
    ref = _conv_ref(x, w, scale, bias, res, (1, 1), (0, 1, 1), relu)
    layer = ops.ConvLayer(_dev(w), None if scale is None else _dev(scale), _dev(bias), stride=(1, 1), pads=(0, 1, 1), relu=relu, dtype=1)
    xd = ops.to_ndhwc(_dev(x), 1)
    rd = ops.to_ndhwc(_dev(res), 1, layer.cstride) if with_res else None
    y = layer(xd, T=frames, residual=rd, res_mode=1 if with_res else 0)
    try:
        assert ops.tune_plan(128, 1) == 0          # a forced plan selects the generic kernel
        y_gen = layer(xd, T=frames, residual=rd, res_mode=1 if with_res else 0)
    finally:
        ops.tune_plan(0, 0)
    assert torch.equal(y, y_gen)
    got = ops.to_ncdhw(y, 1, 1, 64, frames).cpu().numpy()
    err = np.abs(got - ref).max()
    assert err < 3e-2 * max(1.0, np.abs(ref).max() / 4), err
    _bound(got, (x, w, scale, bias, res, (1, 1), (0, 1, 1), relu), 64, (1, 3, 3), 'ws64 ' + name)


@pytest.mark.parametrize('dtype', [0, 1])
def test_batched_weight_repack_equals_per_layer_packing(ops, dtype):
    """dat_conv3d_pack_weights_batch (one launch over a device table of layers: forward and data-gradient packings, different tap
    counts and channel paddings) leaves every packed buffer bit-identical to the per-layer dat_conv3d_pack_weights[_dgrad]."""
    g = torch.Generator().manual_seed(7)
    specs = [((128, 64, 3, 3, 3), False), ((256, 128, 1, 1, 1), False), ((64, 64, 1, 3, 3), False), ((12, 200, 1, 1, 1), False),
             ((128, 64, 3, 3, 3), True), ((96, 256, 1, 3, 3), True), ((512, 256, 1, 1, 1), True), ((1024, 256, 1, 1, 1), False),
             ((64, 256, 3, 1, 1), False), ((40, 72, 1, 1, 1), True)]
    layers, masters = [], []
    for shape, dgrad in specs:
        w = (torch.randn(shape, generator=g) * 0.1).cuda()
        masters.append(w)
        if dgrad:
            scale = (torch.rand(shape[0], generator=g) + 0.5).cuda()
            pads = tuple(k - 1 - k // 2 for k in shape[2:])
            layers.append(ops.ConvLayer(None, None, None, stride=(1, 1), pads=pads, relu=False, dtype=dtype, dgrad_of=(w, scale)))
        else:
            layers.append(ops.ConvLayer(w, None, None, stride=(1, 1), pads=tuple(k // 2 for k in shape[2:]), relu=False, dtype=dtype))
    batch = ops.PackBatch(layers)
    for w in masters:                       # an "SGD step" in place
        w.mul_(0.9).add_(0.01)
    for l in layers:
        l.packed.zero_()
    batch.run()
    got = [l.packed.clone() for l in layers]
    for l in layers:
        l.packed.zero_()
        l.repack(weights_only=True)
    for l, gpk in zip(layers, got):
        assert torch.equal(l.packed, gpk)


PW256_CASES = [
    # name, T, H, W, relu, res_mode, affine   (1x1, 64 -> 256, bf16: the weights-stationary lateral kernel)
    ('up2_ragged', 2, 26, 38, False, 2, False),       # 1976 positions: the last wave tile is partial
    ('sum_relu', 3, 17, 19, True, 1, True),
    ('plain_tiny', 1, 3, 5, False, 0, True),           # fewer positions than one wave tile
    ('many_tiles', 4, 96, 168, False, 2, False),       # > 1 tile per wave of the persistent grid
]


@pytest.mark.parametrize('case', PW256_CASES, ids=[c[0] for c in PW256_CASES])
def test_conv1x1_k64_c256_weights_stationary(ops, case):
    """conv1x1_k64_c256_ws_kernel against torch on the same bf16 operands and bit for bit against the generic kernel (forced plan)."""
    name, T, H, W, relu, res_mode, affine = case
    rs = np.random.RandomState(len(name) * 5 + W)
    q = nm.q16
    x = q(rs.randn(1, 64, T, H, W).astype(np.float32))
    w = q((rs.randn(256, 64, 1, 1, 1) * np.sqrt(2.0 / 64)).astype(np.float32))
    scale = rs.uniform(0.5, 1.5, 256).astype(np.float32) if affine else None
    bias = (rs.randn(256) * 0.1).astype(np.float32)
    res = res_small = None
    if res_mode == 1:
        res = q(rs.randn(1, 256, T, H, W).astype(np.float32))
    elif res_mode == 2:
        res_small = q(rs.randn(1, 256, T, H // 2, W // 2).astype(np.float32))
        res = np.repeat(np.repeat(res_small, 2, axis=3), 2, axis=4)
    ref = _conv_ref(x, w, scale, bias, res, (1, 1), (0, 0, 0), relu)
    layer = ops.ConvLayer(_dev(w), None if scale is None else _dev(scale), _dev(bias), stride=(1, 1), pads=(0, 0, 0), relu=relu, dtype=1)
    xd = ops.to_ndhwc(_dev(x), 1)
    rd = ops.to_ndhwc(_dev(res if res_mode == 1 else res_small), 1, layer.cstride) if res_mode else None
    y = layer(xd, T=T, residual=rd, res_mode=res_mode)
    try:
        assert ops.tune_plan(128, 1) == 0          # a forced plan selects the generic kernel
        y_gen = layer(xd, T=T, residual=rd, res_mode=res_mode)
    finally:
        ops.tune_plan(0, 0)
    assert torch.equal(y, y_gen)
    got = ops.to_ncdhw(y, 1, 1, 256, T).cpu().numpy()
    assert np.abs(got - ref).max() < 3e-2 * max(1.0, np.abs(ref).max() / 4)
    _bound(got, (x, w, scale, bias, res, (1, 1), (0, 0, 0), relu), 64, (1, 1, 1), 'pw256 ' + name)


def _in_fresh_context(env, fn):
    """Runs fn() on a new HIP stream -- i.e. on a NEW C-ABI context, which reads the library's environment switches when it is
    created -- with `env` set; restores the environment."""
    torch.cuda.synchronize()
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        from detectandtrack_amd.ops import hip_ops
        with torch.cuda.stream(torch.cuda.Stream()):
            # torch's stream handles come from a pool and recur: drop whatever context is cached for this handle, and drop ours
            # afterwards so that a later user of the handle does not inherit a context made under THIS environment
            hip_ops.drop_ctx()
            try:
                out = fn()
                torch.cuda.synchronize()
            finally:
                torch.cuda.synchronize()
                hip_ops.drop_ctx()
        return out
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def test_conv3x3_linear_tiles_100_maps_512_channels(ops):
    """The linear tiles of the default dispatch on a grid just above one block per CU (100 maps of 14 x 14, 512 output channels = 308
    blocks of 256 positions) against torch and bit for bit against the 2-D tiling (DAT_CONV_LINEAR=0)."""
    rs = np.random.RandomState(5)
    q = nm.q16
    N, H, W, Cin, Cout = 100, 14, 14, 64, 512
    x = q(rs.randn(N, Cin, 1, H, W).astype(np.float32))
    w = q((rs.randn(Cout, Cin, 1, 3, 3) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32))
    bias = (rs.randn(Cout) * 0.1).astype(np.float32)
    res = q(rs.randn(N, Cout, 1, H, W).astype(np.float32))
    ref = _conv_ref(x, w, None, bias, res, (1, 1), (0, 1, 1), True)
    layer = ops.ConvLayer(_dev(w), None, _dev(bias), stride=(1, 1), pads=(0, 1, 1), relu=True, dtype=1)
    xd, rd = ops.to_ndhwc(_dev(x), 1), ops.to_ndhwc(_dev(res), 1, layer.cstride)
    run = lambda: layer(xd, T=1, residual=rd, res_mode=1)
    y_lin = _in_fresh_context({}, run)
    y2d = _in_fresh_context({'DAT_CONV_LINEAR': '0'}, run)
    assert torch.equal(y_lin, y2d)
    got = ops.to_ncdhw(y_lin, 1, N, Cout, 1).cpu().numpy()
    assert np.abs(got - ref).max() < 3e-2 * max(1.0, np.abs(ref).max() / 4)
    _bound(got, (x, w, None, bias, res, (1, 1), (0, 1, 1), True), Cin, (1, 3, 3), 'linear 100 maps')


@pytest.mark.parametrize('plan', [(256, 1), (256, 2), (128, 1), (128, 3)], ids=lambda p: 'bp%d_ks%d' % p)
@pytest.mark.parametrize('shape', [(2, 4, 24, 42, 128, 256), (1, 3, 48, 84, 64, 128), (2, 2, 12, 21, 64, 64)], ids=lambda s: '%dx%dx%dx%d_%d_%d' % s)
def test_conv3x3x3_linear_strips_per_frame(ops, shape, plan):
    """3x3x3 layers on maps that power-of-two tiles cover badly run one LINEAR strip of positions per frame (round 3: res4 / res5 / P4 /
    P5 of the 3-D bodies; a tile must not span frames because the valid temporal taps differ): against torch and bit for bit against the
    2-D tiling (DAT_CONV_LINEAR=0; same patch / tap / k-slice accumulation order), at both tile sizes and with split-K, residual + ReLU,
    two clips (the clip / frame decode and the temporal zero padding at clip borders)."""
    N, T, H, W, Cin, Cout = shape
    rs = np.random.RandomState(H * W + Cin)
    q = nm.q16
    x = q(rs.randn(N, Cin, T, H, W).astype(np.float32))
    w = q((rs.randn(Cout, Cin, 3, 3, 3) * np.sqrt(2.0 / (Cin * 27))).astype(np.float32))
    scale = rs.uniform(0.5, 1.5, Cout).astype(np.float32)
    bias = (rs.randn(Cout) * 0.1).astype(np.float32)
    res = q(rs.randn(N, Cout, T, H, W).astype(np.float32))
    ref = _conv_ref(x, w, scale, bias, res, (1, 1), (1, 1, 1), True)
    layer = ops.ConvLayer(_dev(w), _dev(scale), _dev(bias), stride=(1, 1), pads=(1, 1, 1), relu=True, dtype=1)
    xd, rd = ops.to_ndhwc(_dev(x), 1), ops.to_ndhwc(_dev(res), 1, layer.cstride)

    def run():
        try:
            assert ops.tune_plan(*plan) == 0
            return layer(xd, T=T, residual=rd, res_mode=1)
        finally:
            ops.tune_plan(0, 0)
    y_lin = _in_fresh_context({'DAT_CONV_LINEAR': '1'}, run)
    y_2d = _in_fresh_context({'DAT_CONV_LINEAR': '0'}, run)
    assert torch.equal(y_lin, y_2d)
    got = ops.to_ncdhw(y_lin, 1, N, Cout, T).cpu().numpy()
    assert np.abs(got - ref).max() < 3e-2 * max(1.0, np.abs(ref).max() / 4)
    _bound(got, (x, w, scale, bias, res, (1, 1), (1, 1, 1), True), Cin, (3, 3, 3), 'strips %r %r' % (shape, plan))


def test_conv3x3x3_linear_strips_with_key_frame_outputs(ops):
    """out_t (only the centre frame of every clip is computed: cfg.HIP.KEYFRAME_DCE) on a map that takes the per-frame linear strips:
    the selected frames equal those of the full conv bit for bit, with the 2-D tiling as well."""
    N, T, H, W, Cin, Cout = 2, 4, 24, 42, 128, 256
    rs = np.random.RandomState(11)
    x = torch.from_numpy(nm.q16(rs.randn(N, Cin, T, H, W).astype(np.float32)))
    w = torch.from_numpy(nm.q16((rs.randn(Cout, Cin, 3, 3, 3) * np.sqrt(2.0 / (Cin * 27))).astype(np.float32)))
    layer = ops.ConvLayer(_dev(w.numpy()), None, _dev(np.zeros(Cout, np.float32)), stride=(1, 1), pads=(1, 1, 1), relu=True, dtype=1)
    xd = ops.to_ndhwc(_dev(x.numpy()), 1)
    full = layer(xd, T=T)                                     # [N*T, H, W, C]
    t0 = T // 2
    key = layer(xd, T=T, out_t=(t0, 1))                       # [N, H, W, C]
    assert key.shape[0] == N
    assert torch.equal(key, full.view(N, T, H, W, -1)[:, t0])
    key2d = _in_fresh_context({'DAT_CONV_LINEAR': '0'}, lambda: layer(xd, T=T, out_t=(t0, 1)))
    assert torch.equal(key, key2d)
    got = key.float().cpu()[..., :Cout].permute(0, 3, 1, 2).numpy()           # [N, Cout, H, W] of frame t0
    ref64, abs64 = nm.conv_ref64(x, w, None, None, None, (1, 1), (1, 1, 1), True)
    nm.assert_elementwise(got, ref64[:, :, t0], abs64[:, :, t0], nm.conv_k(Cin, (3, 3, 3)), nm.h16(), 'key-frame strips')


BT_CASES = [
    # name, T, H, W, Cin, Cout, kt, relu, res_mode, affine   (3x3 bf16 layers with >= 384 tiles of 256 x 256: the big-tile kernel)
    ('3x3x3_ragged_16x16', 3, 120, 250, 128, 256, 3, True, 1, True),
    ('2d_cout512_up2', 3, 100, 180, 64, 512, 1, False, 2, False),
    ('2d_8x32_tiles', 4, 120, 256, 64, 256, 1, True, 0, True),
]


@pytest.mark.parametrize('case', BT_CASES, ids=[c[0] for c in BT_CASES])
def test_conv3x3_big_tile(ops, case):
    """conv3x3_bt_kernel (256 channels x 256 positions per block, hand-scheduled main loop) against torch on the same bf16 operands
    and bit for bit against the generic kernel (forced plan; same patch / tap / k-slice accumulation order)."""
    name, T, H, W, Cin, Cout, kt, relu, res_mode, affine = case
    rs = np.random.RandomState(len(name) * 3 + W)
    q = nm.q16
    x = q(rs.randn(1, Cin, T, H, W).astype(np.float32))
    w = q((rs.randn(Cout, Cin, kt, 3, 3) * np.sqrt(2.0 / (Cin * 9 * kt))).astype(np.float32))
    scale = rs.uniform(0.5, 1.5, Cout).astype(np.float32) if affine else None
    bias = (rs.randn(Cout) * 0.1).astype(np.float32)
    res = res_small = None
    if res_mode == 1:
        res = q(rs.randn(1, Cout, T, H, W).astype(np.float32))
    elif res_mode == 2:
        res_small = q(rs.randn(1, Cout, T, H // 2, W // 2).astype(np.float32))
        res = np.repeat(np.repeat(res_small, 2, axis=3), 2, axis=4)
    ref = _conv_ref(x, w, scale, bias, res, (1, 1), (kt // 2, 1, 1), relu)
    layer = ops.ConvLayer(_dev(w), None if scale is None else _dev(scale), _dev(bias), stride=(1, 1), pads=(kt // 2, 1, 1), relu=relu, dtype=1)
    xd = ops.to_ndhwc(_dev(x), 1)
    rd = None
    if res_mode:
        rd = ops.to_ndhwc(_dev(res if res_mode == 1 else res_small), 1, layer.cstride)
    # The dispatcher keeps this kernel for grids that fill the chip >= 4 times; DAT_CONV_BT=2 selects it for these test-sized grids too.
    def both():
        y_ = layer(xd, T=T, residual=rd, res_mode=res_mode)
        try:
            assert ops.tune_plan(256, 1) == 0          # a forced plan selects the generic kernel
            g_ = layer(xd, T=T, residual=rd, res_mode=res_mode)
        finally:
            ops.tune_plan(0, 0)
        return y_, g_
    y, y_gen = _in_fresh_context({'DAT_CONV_BT': '2'}, both)
    assert torch.equal(y, y_gen)
    got = ops.to_ncdhw(y, 1, 1, Cout, T).cpu().numpy()
    err = np.abs(got - ref).max()
    assert err < 3e-2 * max(1.0, np.abs(ref).max() / 4), err
    # (the generic kernel and torch agree as well: the comparison above is not vacuous)
    assert np.abs(ops.to_ncdhw(y_gen, 1, 1, Cout, T).cpu().numpy() - ref).max() < 3e-2 * max(1.0, np.abs(ref).max() / 4)
    _bound(got, (x, w, scale, bias, res, (1, 1), (kt // 2, 1, 1), relu), Cin, (kt, 3, 3), 'big-tile ' + name)


@pytest.mark.parametrize('case', [('split_k_4_cout_blocks', 4, 24, 42, 512, 512, 3), ('two_cout_blocks', 3, 60, 84, 128, 256, 3), ('2d', 2, 48, 84, 256, 384, 1)],
                         ids=lambda c: c[0])
def test_conv_block_order_switch_is_bit_identical(ops, case):
    """DAT_CONV_ORDER=1 (tile-fastest / weight-stationary block order inside an XCD's queue, an experiment switch: DESIGN.md section 3)
    only permutes which block computes which (tile, cout block, split): same bits as the default order, split-K included."""
    name, T, H, W, Cin, Cout, kt = case
    rs = np.random.RandomState(len(name) + W)
    q = nm.q16
    x = q(rs.randn(1, Cin, T, H, W).astype(np.float32))
    w = q((rs.randn(Cout, Cin, kt, 3, 3) * np.sqrt(2.0 / (Cin * 9 * kt))).astype(np.float32))
    bias = (rs.randn(Cout) * 0.1).astype(np.float32)
    layer = ops.ConvLayer(_dev(w), None, _dev(bias), stride=(1, 1), pads=(kt // 2, 1, 1), relu=True, dtype=1)
    xd = ops.to_ndhwc(_dev(x), 1)
    run = lambda: layer(xd, T=T)
    y1 = _in_fresh_context({'DAT_CONV_ORDER': '1'}, run)
    y0 = _in_fresh_context({'DAT_CONV_ORDER': '0'}, run)
    assert torch.equal(y0, y1)
    ref = _conv_ref(x, w, None, bias, None, (1, 1), (kt // 2, 1, 1), True)
    assert np.abs(ops.to_ncdhw(y1, 1, 1, Cout, T).cpu().numpy() - ref).max() < 3e-2 * max(1.0, np.abs(ref).max() / 4)
    _bound(ops.to_ncdhw(y1, 1, 1, Cout, T).cpu().numpy(), (x, w, None, bias, None, (1, 1), (kt // 2, 1, 1), True), Cin, (kt, 3, 3),
           'block order ' + name)


PW_CASES = [
    # name, T, H, W, Cin, Cout, relu, res_mode, affine   (HBM-bound pointwise layers at a realistic number of positions)
    ('lateral_up2', 2, 126, 162, 64, 256, False, 2, False),
    ('expander_sum', 3, 100, 140, 128, 512, True, 1, True),
    ('cout_200', 2, 128, 160, 256, 200, True, 0, True),
    ('cin_192', 2, 130, 160, 192, 256, False, 0, False),
    # > 65536 positions and several channel chunks (the table-driven loop of the bandwidth-bound 1x1 layers; 5 chunks)
    ('group4_k256_sum', 2, 192, 200, 256, 128, True, 1, True),
    ('group4_k320', 2, 192, 200, 320, 64, False, 0, False),
]


@pytest.mark.parametrize('dtype', [0, 1, 2], ids=['fp32', 'bf16', 'bf16x3'])
@pytest.mark.parametrize('case', PW_CASES, ids=[c[0] for c in PW_CASES])
def test_conv3d_large_pointwise_layers(ops, case, dtype):
    """1x1x1 stride-1 convs with tens of thousands of positions (FPN laterals, bottleneck expanders): ragged last tile, Cout not
    a multiple of 128, 1-4 channel chunks, both residual modes, the hardware bf16 rounding of the epilogue; a forced launch plan
    must give the identical result (same K order)."""
    from detectandtrack_amd import libdat as L
    name, T, H, W, Cin, Cout, relu, res_mode, affine = case
    x3, dtype = dtype == 2, (0 if dtype == 2 else dtype)       # (bf16x3: fp32 tensors, split-operand conv)
    if x3:
        _bf16_only(ops)
    rs = np.random.RandomState(abs(hash(name)) % 1000)
    x = rs.randn(1, Cin, T, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, 1, 1, 1) * np.sqrt(2.0 / Cin)).astype(np.float32)
    scale = rs.uniform(0.5, 1.5, Cout).astype(np.float32) if affine else None
    bias = (rs.randn(Cout) * 0.1).astype(np.float32)
    res = res_small = None
    if res_mode == 1:
        res = rs.randn(1, Cout, T, H, W).astype(np.float32)
    elif res_mode == 2:
        res_small = rs.randn(1, Cout, T, H // 2, W // 2).astype(np.float32)
        res = np.repeat(np.repeat(res_small, 2, axis=3), 2, axis=4)
    if dtype == 1:
        q = nm.q16
        x, w = q(x), q(w)
        if res is not None:
            res = q(res)
            res_small = q(res_small) if res_small is not None else None
    ref = _conv_ref(x, w, scale, bias, res, (1, 1), (0, 0, 0), relu)
    layer = ops.ConvLayer(_dev(w), None if scale is None else _dev(scale), _dev(bias), stride=(1, 1), pads=(0, 0, 0),
                          relu=relu, dtype=dtype, x3=x3)
    xd = ops.to_ndhwc(_dev(x), dtype)
    rd = None
    if res_mode == 1:
        rd = ops.to_ndhwc(_dev(res), dtype, layer.cstride)
    elif res_mode == 2:
        rd = ops.to_ndhwc(_dev(res_small), dtype, layer.cstride)
    got = ops.to_ncdhw(layer(xd, T=T, residual=rd, res_mode=res_mode), dtype, 1, Cout, T).cpu().numpy()
    try:
        assert ops.tune_plan(128, 1) == 0
        gen = ops.to_ncdhw(layer(xd, T=T, residual=rd, res_mode=res_mode), dtype, 1, Cout, T).cpu().numpy()
    finally:
        ops.tune_plan(0, 0)
    err = np.abs(got - ref).max()
    tol = (5e-4 if x3 else 2e-4) if dtype == 0 else 3e-2 * max(1.0, np.abs(ref).max() / 4)
    print('pointwise %s dtype=%d max-abs err %.3e (ref max %.2f), vs forced plan %.3e' % (name, dtype, err, np.abs(ref).max(),
                                                                                            np.abs(got - gen).max()))
    assert err < tol
    np.testing.assert_array_equal(got, gen)
    if dtype == 1:
        _bound(got, (x, w, scale, bias, res, (1, 1), (0, 0, 0), relu), Cin, (1, 1, 1), 'pointwise ' + name)


def test_conv3d_forced_plans_agree(ops):
    """dat_conv3d_tune_plan: every launch plan (128 / 256 positions per block, split-K 1..4) of a res4-like layer computes the same
    convolution — fp32 mode vs torch within 2e-4, and the plans among themselves (only the split-K summation order differs)."""
    from detectandtrack_amd import libdat as L
    rs = np.random.RandomState(11)
    N, T, H, W, Cin, Cout, k = 1, 4, 24, 40, 256, 256, (3, 3, 3)
    x = rs.randn(N, Cin, T, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, *k) * np.sqrt(2.0 / (Cin * 27))).astype(np.float32)
    bias = (rs.randn(Cout) * 0.1).astype(np.float32)
    ref = _conv_ref(x, w, None, bias, None, (1, 1), (1, 1, 1), True)
    layer = ops.ConvLayer(_dev(w), None, _dev(bias), stride=(1, 1), pads=(1, 1, 1), relu=True, dtype=0)
    xd = ops.to_ndhwc(_dev(x), 0)
    outs = {}
    try:
        for bp, ks in ((0, 0), (128, 1), (256, 1), (128, 2), (256, 3), (128, 4)):
            assert ops.tune_plan(bp, ks) == 0
            outs[(bp, ks)] = ops.to_ncdhw(layer(xd, T=T), 0, N, Cout, T).cpu().numpy()
        assert ops.tune_plan(64, 1) != 0          # rejected: not a tile size
    finally:
        ops.tune_plan(0, 0)
    for key, got in outs.items():
        err = np.abs(got - ref).max()
        assert err < 2e-4, (key, err)
    np.testing.assert_array_equal(outs[(128, 1)], outs[(256, 1)])   # same K order, different tiling: bit-identical


@pytest.mark.parametrize('dtype', [0, 1])
def test_stem_conv1(ops, dtype):
    rs = np.random.RandomState(5)
    N, T, H, W = 1, 2, 38, 50
    x = (rs.uniform(0, 255, (N, 3, T, H, W)) - 110).astype(np.float32)
    w = (rs.randn(64, 3, 1, 7, 7) * 0.05).astype(np.float32)
    s = rs.uniform(0.5, 1.5, 64).astype(np.float32)
    b = (rs.randn(64) * 0.1).astype(np.float32)
    if dtype == 1:
        q = nm.q16
        x, w = q(x), q(w)
    ref = _conv_ref(x, w, s, b, None, (2, 2), (0, 3, 3), True)
    layer = ops.stem_layer(_dev(w), _dev(s), _dev(b), dtype)
    packed = ops.stem_pack(_dev(x), dtype)
    y = layer(packed, T=T)
    got = ops.to_ncdhw(y, dtype, N, 64, T).cpu().numpy()
    err = np.abs(got - ref).max()
    print('stem dtype=%d err %.3e ref max %.1f' % (dtype, err, np.abs(ref).max()))
    assert got.shape == ref.shape
    assert err < (2e-3 if dtype == 0 else 0.02 * np.abs(ref).max())
    if dtype == 1:
        _bound(got, (x, w, s, b, None, (2, 2), (0, 3, 3), True), 3, (1, 7, 7), 'stem')


@pytest.mark.parametrize('dtype', [0, 1])
def test_maxpool(ops, dtype):
    rs = np.random.RandomState(6)
    x = rs.randn(1, 64, 2, 13, 18).astype(np.float32)
    if dtype == 1:
        x = nm.q16(x)
    ref = F.max_pool3d(torch.from_numpy(x), (1, 3, 3), (1, 2, 2), (0, 1, 1)).numpy()
    y = ops.maxpool_hw(ops.to_ndhwc(_dev(x), dtype), dtype, 3, 2, 1)
    np.testing.assert_array_equal(ops.to_ncdhw(y, dtype, 1, 64, 2).cpu().numpy(), ref)
    # P6 = MaxPool k1 s2 (FPN3D.py:158-163)
    ref6 = x[:, :, :, ::2, ::2]
    y6 = ops.maxpool_hw(ops.to_ndhwc(_dev(x), dtype), dtype, 1, 2, 0)
    np.testing.assert_array_equal(ops.to_ncdhw(y6, dtype, 1, 64, 2).cpu().numpy(), ref6)


def test_time_avg(ops):
    rs = np.random.RandomState(7)
    x = rs.randn(2, 64, 3, 5, 6).astype(np.float32)
    y = ops.time_avg(ops.to_ndhwc(_dev(x), 0), 0, 2, 3)
    got = ops.to_ncdhw(y, 0, 2, 64, 1).cpu().numpy()[:, :, 0]
    np.testing.assert_allclose(got, x.mean(axis=2), atol=1e-6)


# ------------------------------------------------------------------------------------------------------
def _rand_rois(rs, n, W, H, T=1, batch=1):
    r = np.zeros((n, 4 * T + 1), dtype=np.float32)
    r[:, 0] = rs.randint(0, batch, n)
    x1 = rs.uniform(-10, W - 20, n)
    y1 = rs.uniform(-10, H - 20, n)
    w = rs.uniform(2, W * 0.8, n)
    h = rs.uniform(2, H * 0.8, n)
    for t in range(T):
        j = rs.uniform(-4, 4, (4, n))
        r[:, 1 + 4 * t] = x1 + j[0]
        r[:, 2 + 4 * t] = y1 + j[1]
        r[:, 3 + 4 * t] = x1 + w + j[2]
        r[:, 4 + 4 * t] = y1 + h + j[3]
    return r


@pytest.mark.parametrize('dtype', [0, 1])
def test_roi_align_single_level(ops, dtype):
    from oracle.roi_align import roi_align_2d
    rs = np.random.RandomState(8)
    feat = rs.randn(2, 64, 1, 20, 30).astype(np.float32)
    if dtype == 1:
        feat = nm.q16(feat)
    rois = _rand_rois(rs, 23, 30 * 16, 20 * 16, batch=2)
    ref = roi_align_2d(feat[:, :, 0], rois, 7, 1. / 16., 2)
    fd = ops.to_ndhwc(_dev(feat), dtype)
    out = ops.roi_align([fd], [1. / 16.], dtype, _dev(rois), T=1, Tr=1, t0=0, pooled=7, sampling=2)
    got = out.float().cpu().numpy().transpose(0, 3, 1, 2)
    err = np.abs(got - ref).max()
    print('roi_align dtype=%d err %.3e' % (dtype, err))
    assert err < (1e-4 if dtype == 0 else 3e-2)
    if dtype == 1:
        # K = 2 x 2 samples of 4 bilinear taps; the output is stored in the feature's format
        absref = roi_align_2d(np.abs(feat[:, :, 0]), rois, 7, 1. / 16., 2)
        nm.assert_elementwise(got, ref, absref, 16, out.dtype, 'roi_align single level')


def test_roi_align_tube_and_keyframe(ops):
    from oracle.roi_align import roi_align_tube, roi_align_2d
    rs = np.random.RandomState(9)
    T = 3
    feat = rs.randn(1, 64, T, 16, 20).astype(np.float32)
    rois = _rand_rois(rs, 9, 20 * 16, 16 * 16, T=T)
    ref = roi_align_tube(feat, rois, 14, 1. / 16., 2)  # (R, C, T, P, P)
    fd = ops.to_ndhwc(_dev(feat), 0)
    out = ops.roi_align([fd], [1. / 16.], 0, _dev(rois), T=T, Tr=T, t0=0, pooled=14, sampling=2)
    got = out.cpu().numpy().reshape(9, T, 14, 14, 64).transpose(0, 4, 1, 2, 3)
    assert np.abs(got - ref).max() < 1e-4
    # 2D rois on the key frame of a T-frame feature (slice-center link)
    rois2 = _rand_rois(rs, 7, 20 * 16, 16 * 16)
    ref2 = roi_align_2d(feat[:, :, 1], rois2, 7, 1. / 16., 2)
    out2 = ops.roi_align([fd], [1. / 16.], 0, _dev(rois2), T=T, Tr=1, t0=1, pooled=7, sampling=2)
    assert np.abs(out2.cpu().numpy().transpose(0, 3, 1, 2) - ref2).max() < 1e-4


def test_roi_align_fpn_levels(ops):
    from oracle import proposals as op
    from oracle.roi_align import roi_align_2d
    rs = np.random.RandomState(10)
    feats = [rs.randn(1, 64, 1, 64 // 2 ** i, 96 // 2 ** i).astype(np.float32) for i in range(4)]  # P2..P5
    rois = _rand_rois(rs, 60, 96 * 4, 64 * 4)
    rois[:10, 3] = rois[:10, 1] + rs.uniform(200, 380, 10)
    rois[:10, 4] = rois[:10, 2] + rs.uniform(150, 250, 10)
    lvls = op.map_rois_to_fpn_levels(rois[:, 1:], 2, 5)
    assert len(np.unique(lvls)) >= 3
    ref = np.zeros((60, 64, 7, 7), np.float32)
    for i in range(60):
        l = int(lvls[i])
        ref[i] = roi_align_2d(feats[l - 2][:, :, 0], rois[i:i + 1], 7, 1. / 2 ** l, 2)[0]
    fds = [ops.to_ndhwc(_dev(f), 0) for f in feats]
    out = ops.roi_align(fds, [1. / 2 ** l for l in range(2, 6)], 0, _dev(rois), T=1, Tr=1, t0=0, pooled=7, sampling=2)
    assert np.abs(out.cpu().numpy().transpose(0, 3, 1, 2) - ref).max() < 1e-4


# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ['nms_n300_t3', 'nms_n300_t5', 'nms_n1000_t7', 'nms_n1_t5', 'nms_n2_t5'])
def test_nms_boxes_bit_exact_vs_reference(ops, golden, key):
    dets = golden[key + '_dets']
    keep = ops.nms(_dev(dets), float(key.split('_t')[1]) / 10.).cpu().numpy()
    np.testing.assert_array_equal(keep, golden[key + '_keep'])


@pytest.mark.parametrize('key,thr', [('tnms_n200_T3_t5', 0.5), ('tnms_n120_T8_t7', 0.7), ('tnms_n1_T3_t5', 0.5)])
def test_nms_tubes_bit_exact_vs_reference(ops, golden, key, thr):
    keep = ops.nms(_dev(golden[key + '_dets']), thr).cpu().numpy()
    np.testing.assert_array_equal(keep, golden[key + '_keep'])


def test_nms_fuzz_and_host_wrapper(ops):
    from oracle import nms as onms
    rs = np.random.RandomState(12)
    for n in (3, 64, 65, 129, 777, 2500, 4096):
        d = _random_dets(rs, n)
        for thr in (0.3, 0.7):
            np.testing.assert_array_equal(ops.nms(_dev(d), thr).cpu().numpy(), onms.nms_boxes(d, thr))
    # empty
    assert ops.nms(torch.zeros((0, 5)).cuda(), 0.5).numel() == 0
    # `_nms` convention (lib/nms/gpu_nms.hpp:3-9): pre-sorted host boxes, keep = positions
    d = d[np.argsort(-d[:, 4], kind='stable')]
    keep = ops.nms_host(d, 0.5)
    np.testing.assert_array_equal(keep, onms.nms_boxes(d, 0.5))
    # heavy-overlap adversarial: identical boxes, only the best survives
    same = np.tile(np.array([[10, 10, 50, 50]], np.float32), (500, 1))
    dd = np.hstack((same, rs.uniform(0, 1, (500, 1)).astype(np.float32)))
    k = ops.nms(_dev(dd), 0.5).cpu().numpy()
    assert k.tolist() == [int(np.argmax(dd[:, 4]))]


def _random_dets(rs, n, span=300.0):
    b = rs.uniform(0, span, (n, 4)).astype(np.float32)
    b[:, 2:] = b[:, :2] + rs.uniform(1, 80, (n, 2)).astype(np.float32)
    return np.hstack((b, rs.uniform(0, 1, (n, 1)).astype(np.float32)))


@pytest.mark.parametrize('n', [4097, 8191, 12000, 16384])
def test_nms_beyond_4096_boxes_bit_exact_vs_reference_cython(ops, n):
    """The reference's default RPN_PRE_NMS_TOP_N is 12000 (lib/core/config.py:110,183): keep indices of the device NMS are
    identical to the reference's own Cython (compiled from lib/utils/cython_nms.pyx) up to 16384 boxes: its answers stored in
    tests/golden/reference_cython.npz (make_golden.py golden_cython), and live as well when oracle/_ref holds the compiled module."""
    from oracle import build_ref
    ref = build_ref.load()
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_cython.npz'))
    rs = np.random.RandomState(n)
    d = _random_dets(rs, n, span=2000.0)
    np.testing.assert_allclose(d.astype(np.float64).sum(), g['large_%d_dets_sum' % n], rtol=1e-12)     # (the stored answers' input)
    for thr in (0.5, 0.7):
        keep = ops.nms(_dev(d), thr).cpu().numpy()
        np.testing.assert_array_equal(keep, g['large_%d_keep_%g' % (n, thr)])
        if ref is not None:
            np.testing.assert_array_equal(keep, np.asarray(ref[0].nms(d, np.float32(thr))))
    with pytest.raises(Exception):
        ops.nms(_dev(_random_dets(rs, 16385)), 0.5)


def test_reference_nms_symbol_exact_prototype(ops):
    """`void _nms(int*, int*, const float*, int, int, float, int)` (lib/nms/gpu_nms.hpp:3-9) called through ctypes with exactly that
    prototype, the way lib/nms/gpu_nms.pyx:14-34 binds it: pre-sorted host boxes, strict > threshold, positions out."""
    import ctypes as C
    from detectandtrack_amd import libdat as L
    from oracle import nms as onms
    fn = C.CDLL(L.LIB_PATH)._nms
    fn.restype = None
    fn.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_float, C.c_int]
    rs = np.random.RandomState(5)
    for n in (1, 2, 63, 64, 65, 1000, 6000, 12000):
        d = _random_dets(rs, n, span=300.0 if n <= 1000 else 1500.0)
        d = np.ascontiguousarray(d[np.argsort(-d[:, 4], kind='stable')])
        for thr in (0.3, 0.7):
            keep = np.zeros(n, np.int32)
            num = C.c_int(-1)
            fn(keep.ctypes.data_as(C.POINTER(C.c_int)), C.byref(num), d.ctypes.data_as(C.POINTER(C.c_float)), n, 5, thr, 0)
            np.testing.assert_array_equal(keep[:num.value], onms.gpu_nms_presorted(d, thr))
    # the strict threshold: IoU exactly 1/3 is kept by `_nms` and removed by the >= convention of dat_nms_host
    b = np.array([[0, 0, 9, 9, 0.9], [5, 0, 14, 9, 0.8]], np.float32)
    third = float(np.float32(50.0) / np.float32(150.0))
    keep, num = np.zeros(2, np.int32), C.c_int(-1)
    fn(keep.ctypes.data_as(C.POINTER(C.c_int)), C.byref(num), b.ctypes.data_as(C.POINTER(C.c_float)), 2, 5, third, 0)
    assert num.value == 2
    assert ops.nms_host(b, third).tolist() == [0]
    # empty input / bad device id: num_out = 0, no crash (the reference only prints)
    num = C.c_int(-1)
    fn(keep.ctypes.data_as(C.POINTER(C.c_int)), C.byref(num), b.ctypes.data_as(C.POINTER(C.c_float)), 0, 5, 0.5, 0)
    assert num.value == 0
    fn(keep.ctypes.data_as(C.POINTER(C.c_int)), C.byref(num), b.ctypes.data_as(C.POINTER(C.c_float)), 2, 5, 0.5, 63)
    assert num.value == 0


def test_two_contexts_two_threads_are_independent(ops):
    """thread-safe per dat_ctx, N contexts per process.  Two host threads, each with its own context and HIP stream,
    run convs (one under a forced launch plan -- plan overrides are per-context state), NMS and `_nms` concurrently; every result
    equals the single-threaded one."""
    import ctypes as C
    import threading
    from detectandtrack_amd import libdat as L
    from oracle import nms as onms
    rs = np.random.RandomState(21)
    T, H, W, Cin, Cout = 2, 40, 56, 128, 128
    x = rs.randn(1, Cin, T, H, W).astype(np.float32)
    w = (rs.randn(Cout, Cin, 3, 3, 3) * np.sqrt(2.0 / (Cin * 27))).astype(np.float32)
    layer = ops.ConvLayer(_dev(w), None, None, stride=(1, 1), pads=(1, 1, 1), relu=True, dtype=1)
    xd = ops.to_ndhwc(_dev(x), 1)
    base = layer(xd, T=T).float().cpu().numpy()
    dets = _random_dets(rs, 3000)
    dsorted = np.ascontiguousarray(dets[np.argsort(-dets[:, 4], kind='stable')])
    keep_ref = onms.nms_boxes(dets, 0.5)
    gpu_ref = onms.gpu_nms_presorted(dsorted, 0.5)
    torch.cuda.synchronize()
    fn = C.CDLL(L.LIB_PATH)._nms
    fn.restype = None
    fn.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_float, C.c_int]
    errors, ctx_handles = [], []

    def worker(k):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                ctx_handles.append(ops.ctx().h.value)
                if k == 1:
                    assert ops.tune_plan(128, 2) == 0        # this context only
                dd = _dev(dets)
                for _ in range(15):
                    y = layer(xd, T=T).float().cpu().numpy()
                    if k == 0:
                        np.testing.assert_array_equal(y, base)           # unaffected by the other context's plan
                    else:
                        np.testing.assert_allclose(y, base, atol=0.05)   # split-K: different summation order
                    np.testing.assert_array_equal(ops.nms(dd, 0.5).cpu().numpy(), keep_ref)
                    keep, num = np.zeros(len(dsorted), np.int32), C.c_int(-1)
                    fn(keep.ctypes.data_as(C.POINTER(C.c_int)), C.byref(num), dsorted.ctypes.data_as(C.POINTER(C.c_float)),
                       len(dsorted), 5, 0.5, 0)
                    np.testing.assert_array_equal(keep[:num.value], gpu_ref)
                if k == 1:
                    ops.tune_plan(0, 0)
        except Exception as e:   # noqa
            import traceback
            errors.append(traceback.format_exc())
    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]
    assert len(set(ctx_handles)) == 2, 'each (device, stream) must get its own dat_ctx'


def test_rpn_proposals_with_the_reference_default_pre_nms_12000(ops):
    """RPN_PRE_NMS_TOP_N 12000 / POST 2000 (the reference's defaults, lib/core/config.py:110-112,183-185) on a P2-sized level."""
    from oracle import proposals as op
    from oracle.anchors import generate_anchors
    rs = np.random.RandomState(77)
    H0, W0 = 384, 640
    im_info = np.array([[H0, W0, 1.0]], np.float32)
    specs, ref_r, ref_p = [], [], []
    for lvl in (2, 3):
        H, W = H0 >> lvl, W0 >> lvl
        anchors = generate_anchors(2. ** lvl, (32 * 2. ** (lvl - 2),), (0.5, 1, 2))
        scores = rs.uniform(0.001, 0.999, (1, 3, H, W)).astype(np.float32)
        deltas = (rs.randn(1, 12, H, W) * 0.3).astype(np.float32)
        head, _ = _head_tensor(ops, scores, deltas, 0)
        lg = ops.to_ncdhw(head, 0, 1, 3, 1).cpu().numpy()[:, :, 0]
        probs_dev = (1.0 / (1.0 + np.exp(-lg.astype(np.float32)))).astype(np.float32)
        r, p = op.generate_proposals(probs_dev, deltas, im_info, anchors, 1. / 2 ** lvl, 12000, 2000, 0.7, 0)
        ref_r.append(r)
        ref_p.append(p)
        specs.append(ops.RpnLevelSpec(head, H, W, 3, 1, float(2 ** lvl), 64, 0, 3, 0, _dev(anchors.astype(np.float32))))
    rois, probs, counts = ops.rpn_proposals(specs, 0, im_info[0], 12000, 2000, 0.7, 0.)
    cnt = counts.cpu().numpy()
    for i in range(2):
        assert cnt[i] == ref_r[i].shape[0], (i, cnt[i], ref_r[i].shape)
        np.testing.assert_allclose(rois[i, :cnt[i]].cpu().numpy(), ref_r[i], atol=3e-3)
    out, n_out = ops.collect_rois(rois, probs, counts, 2000)
    exp = op.collect(ref_r, ref_p, 2000)
    assert int(n_out.item()) == exp.shape[0]
    np.testing.assert_allclose(out[:exp.shape[0]].cpu().numpy(), exp, atol=3e-3)


@pytest.mark.parametrize('T,K,R,D', [(1, 2, 1000, 100), (1, 5, 700, 100), (3, 2, 300, 40), (1, 2, 50, 100), (1, 3, 400, 0)])
def test_box_results_on_device_match_the_oracle(ops, T, K, R, D):
    """dat_box_results vs oracle/box_results.py (lib/core/test.py:211-244 decode + clip, :750-806 threshold / per-class NMS /
    DETECTIONS_PER_IM, :78-123 keypoint rois): same detections in the same order, scores bit-equal, boxes to exp rounding
    (NumPy's float32 exp is within 1 ulp of the correctly rounded one used on the device), keypoint rois to the same tolerance."""
    from oracle import box_results as obr
    rs = np.random.RandomState(100 * T + K)
    H, W, scale = 720, 1280, 800.0 / 720.0
    cap = R + 24                                             # the proposal blob has spare capacity rows past its count
    xy = np.stack([rs.uniform(0, W * scale - 60, cap), rs.uniform(0, H * scale - 60, cap)], axis=1)
    wh = rs.uniform(8, 300, (cap, 2))
    rois = np.zeros((cap, 4 * T + 1), np.float32)
    for t in range(T):
        jit = rs.uniform(-4, 4, (cap, 2))
        rois[:, 1 + 4 * t:3 + 4 * t] = xy + jit
        rois[:, 3 + 4 * t:5 + 4 * t] = xy + jit + wh
    logits = rs.randn(cap, K).astype(np.float32) * 2
    prob = (np.exp(logits) / np.exp(logits).sum(axis=1, keepdims=True)).astype(np.float32)
    pred = (rs.randn(cap, K * 4 * T) * np.tile([1.0, 1.0, 2.0, 2.0], K * T)).astype(np.float32)
    dets, kp, n_out = ops.box_results(_dev(rois), torch.tensor([R], dtype=torch.int32).cuda(), _dev(prob), _dev(pred), K, T, scale,
                                      (H, W, 3), (10., 10., 5., 5.), float(np.float32(np.log(1000. / 16.))), 0.05, 0.5, D,
                                      D if D > 0 else cap * (K - 1))
    n = n_out.cpu().numpy()
    scores, boxes = obr.read_bbox_outputs(rois[:R], prob[:R], pred[:R], scale, (H, W, 3))
    ref_scores, ref_boxes, ref_cls = obr.box_results_with_nms_and_limit(scores, boxes, K, 0.05, 0.5, D)
    assert n[1] == ref_boxes.shape[0], (n, ref_boxes.shape)
    assert n[0] == min(n[1], D if D > 0 else cap * (K - 1))
    k = int(n[0])
    d = dets.cpu().numpy()
    ref_cls_col = np.concatenate([np.full((len(ref_cls[j]),), j, np.float32) for j in range(1, K)])
    np.testing.assert_array_equal(d[:k, 4 * T], ref_scores[:k])
    np.testing.assert_array_equal(d[:k, 4 * T + 1], ref_cls_col[:k])
    np.testing.assert_allclose(d[:k, :4 * T], ref_boxes[:k], rtol=0, atol=2e-3)
    np.testing.assert_allclose(kp.cpu().numpy()[:k], obr.get_rois_blob(ref_boxes[:k], scale), rtol=0, atol=3e-3)
    assert not kp.cpu().numpy()[k:].any() and not d[k:].any()


@pytest.mark.parametrize('name', ['pp_boxes_k2', 'pp_boxes_k5', 'pp_tubes_k2', 'pp_nolimit'])
def test_box_results_on_device_match_the_real_reference(ops, name):
    """dat_box_results against outputs of the reference's own box_results_with_nms_and_limit (core/test.py:750-806 run under py3
    shims with its compiled Cython NMS; tests/golden/reference_postproc.npz): same detections, same order, scores bit-equal, boxes
    to the 1-ulp exp difference."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_postproc.npz'))
    T, K, R, D, thr, nms_thr = g[name + '_cfg']
    T, K, R, D = int(T), int(K), int(R), int(D)
    rois = np.hstack((np.zeros((R, 1), np.float32), g[name + '_boxes']))
    out_cap = D if D > 0 else R * (K - 1)
    dets, kp, n_out = ops.box_results(_dev(rois), torch.tensor([R], dtype=torch.int32).cuda(), _dev(g[name + '_scores']),
                                      _dev(g[name + '_deltas']), K, T, 1.0, (720, 1280, 3), (10., 10., 5., 5.),
                                      float(np.float32(np.log(1000. / 16.))), float(thr), float(nms_thr), D, out_cap)
    n = n_out.cpu().numpy()
    ref_s, ref_b = g[name + '_out_scores'], g[name + '_out_boxes']
    assert n[0] == n[1] == ref_s.shape[0], (n, ref_s.shape)
    d = dets.cpu().numpy()[:n[0]]
    np.testing.assert_array_equal(d[:, 4 * T], ref_s)
    np.testing.assert_allclose(d[:, :4 * T], ref_b, rtol=0, atol=2e-3)
    counts = [int((d[:, 4 * T + 1] == j).sum()) for j in range(1, K)]
    assert counts == g[name + '_out_counts'].tolist()


def _head_tensor(ops, scores, deltas, dtype, logits=True):
    """scores (1,A,H,W) probabilities, deltas (1,4AT,H,W) -> head [1,H,W,cs] holding LOGITS (or probs) + deltas."""
    A = scores.shape[1]
    first = scores
    if logits:
        p = np.clip(scores.astype(np.float64), 1e-7, 1 - 1e-7)
        first = np.log(p / (1 - p)).astype(np.float32)
    cat = np.concatenate([first, deltas], axis=1)
    cs = (cat.shape[1] + 63) // 64 * 64
    return ops.to_ndhwc(_dev(cat), dtype, cs), cs


@pytest.mark.parametrize('name', ['gp_fpn3', 'gp_fpn2_min', 'gp_c4_T3'])
def test_rpn_proposals_vs_reference_golden(ops, golden, name):
    """Device GenerateProposals vs the REAL reference op's output (tests/golden/make_golden.py).

    Probabilities are fed as-is (apply_sigmoid=0 == the reference op boundary, which takes rpn_cls_probs), so
    the sort order is identical; boxes agree to 2e-3 px (device exp is correctly rounded, numpy's is ~1 ulp)."""
    stride, pre, post, thr, min_size = golden[name + '_cfg']
    scores, deltas = golden[name + '_scores'], golden[name + '_deltas']
    anchors = golden[name + '_anchors']
    A, T = anchors.shape[0], anchors.shape[1] // 4
    head, cs = _head_tensor(ops, scores, deltas, 0, logits=False)
    H, W = scores.shape[2:]
    lvl = ops.RpnLevelSpec(head, H, W, A, T, float(stride), cs, 0, A, 0, _dev(anchors.astype(np.float32)),
                           apply_sigmoid=False)
    rois, probs, counts = ops.rpn_proposals([lvl], 0, golden[name + '_im_info'][0], int(pre), int(post), float(thr),
                                            float(min_size))
    n = int(counts[0].item())
    ref_rois, ref_probs = golden[name + '_rois'], golden[name + '_probs']
    assert n == ref_rois.shape[0]
    np.testing.assert_allclose(rois[0, :n].cpu().numpy(), ref_rois, rtol=0, atol=2e-3)
    np.testing.assert_allclose(probs[0, :n].cpu().numpy(), ref_probs[:, 0], rtol=0, atol=1e-6)


def test_rpn_proposals_multilevel_and_collect(ops):
    from oracle import proposals as op
    from oracle.anchors import generate_anchors
    rs = np.random.RandomState(13)
    shapes = {2: (48, 64), 3: (24, 32), 4: (12, 16), 5: (6, 8), 6: (3, 4)}
    im_info = np.array([[192., 256., 1.0]], np.float32)
    specs, ref_r, ref_p = [], [], []
    for lvl in range(2, 7):
        H, W = shapes[lvl]
        anchors = generate_anchors(2. ** lvl, (32 * 2. ** (lvl - 2),), (0.5, 1, 2))
        scores = rs.uniform(0.01, 0.99, (1, 3, H, W)).astype(np.float32)
        deltas = (rs.randn(1, 12, H, W) * 0.3).astype(np.float32)
        head, _ = _head_tensor(ops, scores, deltas, 0)
        # the oracle must see exactly the probabilities the device will compute from the logits
        lg = ops.to_ncdhw(head, 0, 1, 3, 1).cpu().numpy()[:, :, 0]
        probs_dev = (1.0 / (1.0 + np.exp(-lg.astype(np.float32)))).astype(np.float32)
        r, p = op.generate_proposals(probs_dev, deltas, im_info, anchors, 1. / 2 ** lvl, 1000, 300, 0.7, 0)
        ref_r.append(r)
        ref_p.append(p)
        specs.append(ops.RpnLevelSpec(head, H, W, 3, 1, float(2 ** lvl), 64, 0, 3, 0, _dev(anchors.astype(np.float32))))
    rois, probs, counts = ops.rpn_proposals(specs, 0, im_info[0], 1000, 300, 0.7, 0.)
    cnt = counts.cpu().numpy()
    for i in range(5):
        assert cnt[i] == ref_r[i].shape[0], (i, cnt[i], ref_r[i].shape)
        np.testing.assert_allclose(rois[i, :cnt[i]].cpu().numpy(), ref_r[i], atol=2e-3)
    out, n_out = ops.collect_rois(rois, probs, counts, 300)
    exp = op.collect([r for r in ref_r], [p for p in ref_p], 300)
    assert int(n_out.item()) == exp.shape[0]
    np.testing.assert_allclose(out[:exp.shape[0]].cpu().numpy(), exp, atol=2e-3)


def test_rpn_proposals_ties_and_small_levels(ops):
    """All-equal scores (zero-initialised RPN): ties resolve to the lowest (h, w, a) index; N < pre_nms."""
    from oracle import proposals as op
    from oracle.anchors import generate_anchors
    anchors = generate_anchors(16., (64,), (0.5, 1, 2))
    H, W = 40, 50   # N = 6000 > pre_nms
    scores = np.full((1, 3, H, W), 0.5, np.float32)
    deltas = (np.random.RandomState(14).randn(1, 12, H, W) * 0.2).astype(np.float32)
    im_info = np.array([[640., 800., 1.0]], np.float32)
    head, _ = _head_tensor(ops, scores, deltas, 0)
    spec = ops.RpnLevelSpec(head, H, W, 3, 1, 16., 64, 0, 3, 0, _dev(anchors.astype(np.float32)))
    rois, probs, counts = ops.rpn_proposals([spec], 0, im_info[0], 700, 200, 0.7, 0.)
    r, p = op.generate_proposals(scores, deltas, im_info, anchors, 1. / 16, 700, 200, 0.7, 0)
    n = int(counts[0].item())
    assert n == r.shape[0]
    np.testing.assert_allclose(rois[0, :n].cpu().numpy(), r, atol=2e-3)


# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [0, 1])
def test_kps_tail(ops, dtype):
    """ConvTranspose k4s2p1 (as sub-pixel 3x3 conv) + bilinear ConvTranspose == oracle.net3d.kps_outputs_2d."""
    from oracle.net3d import Net, opts_for
    rs = np.random.RandomState(15)
    R, Cin, K, S = 3, 64, 17, 14
    x = np.maximum(rs.randn(R, Cin, S, S), 0).astype(np.float32)
    w = (rs.randn(Cin, K, 4, 4) * 0.05).astype(np.float32)
    b = (rs.randn(K) * 0.1).astype(np.float32)
    if dtype == 1:
        q = nm.q16
        x, w = q(x), q(w)
    net = Net({'kps_score_lowres_w': w, 'kps_score_lowres_b': b}, opts_for('R18'))
    ref = net.kps_outputs_2d(torch.from_numpy(x)).numpy()
    w3 = ops.deconv_k4s2_as_conv3x3(_dev(w))
    layer = ops.ConvLayer(w3, None, _dev(np.tile(b, 4)), stride=(1, 1), pads=(0, 1, 1), relu=False, dtype=dtype)
    sub = layer(ops.to_ndhwc(_dev(x), dtype), T=1)
    out = ops.kps_finalize(sub, dtype, R, 1, K, 2).cpu().numpy()
    assert out.shape == ref.shape == (R, K, 56, 56)
    err = np.abs(out - ref).max()
    print('kps tail dtype=%d err %.3e' % (dtype, err))
    assert err < (1e-4 if dtype == 0 else 3e-2)
    if dtype == 1:
        from oracle.net3d import bilinear_kernel
        up = torch.from_numpy(np.ascontiguousarray(bilinear_kernel(K, 2), np.float64))
        t64 = lambda a: torch.from_numpy(a.astype(np.float64))
        low = F.conv_transpose2d(t64(x), t64(w), t64(b), stride=2, padding=1)
        abs_low = F.conv_transpose2d(t64(np.abs(x)), t64(np.abs(w)), t64(np.abs(b)), stride=2, padding=1)
        ref64 = F.conv_transpose2d(low, up, None, stride=2, padding=1).numpy()
        abs64 = F.conv_transpose2d(abs_low, up, None, stride=2, padding=1).numpy()
        # the sub-pixel conv stores kps_score_lowres in the 16-bit format and dat_kps_finalize (elementwise.hip kps_finalize_kernel)
        # upsamples that stored blob in fp32: a second rounding, at most u16 * |lowres| under the (non-negative) bilinear taps
        extra = nm.unit_roundoff(nm.h16()) * F.conv_transpose2d(low.abs(), up, None, stride=2, padding=1).numpy()
        nm.assert_elementwise(out, ref64, abs64, Cin * 16 + 4, 'fp32', 'kps tail', extra)


def _roi_align_cases():
    from tests.test_oracle_golden import roi_align_known_answers
    return roi_align_known_answers()


@pytest.mark.parametrize('case', _roi_align_cases(), ids=lambda c: c[0])
def test_roi_align_known_answers(ops, case):
    """dat_roi_align on the hand-worked legacy-RoIAlign edge cases of tests/test_oracle_golden.py (roi smaller than a pixel, the
    max(., 1) clamp after scaling, samples at / beyond -1 and H, far-border clamping, adaptive sampling grid): exact dyadic values,
    fp32 mode -- the product against the published operator definition, not against the restated oracle."""
    name, feat, rois, pooled, scale, sampling, exp = case
    n, c, h, w = feat.shape
    fd = ops.to_ndhwc(_dev(feat.reshape(n, c, 1, h, w)), 0)
    out = ops.roi_align([fd], [scale], 0, _dev(rois), T=1, Tr=1, t0=0, pooled=pooled, sampling=sampling, k_min=2)
    got = out.cpu().numpy().transpose(0, 3, 1, 2)[:, :c]
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-4)
    if not name.startswith('adaptive'):             # (sums of <= 4 dyadic terms: exact whatever the order)
        np.testing.assert_array_equal(got, exp)


def test_conv_transpose_k4s2p1_known_answer(ops):
    """The product's ConvTranspose k4 s2 p1 (model_builder.py:848-856) -- run as a 3x3 conv that writes the four sub-pixel phases as
    channel groups (dat_deconv_k4s2_weights: channel (a * 2 + b) * K + k holds out[2 i + a, 2 j + b]) -- against the hand-worked
    definition of tests/test_oracle_golden.py: fp32 mode, small integers + 0.5, exact."""
    from tests.test_oracle_golden import conv_transpose_k4s2p1_known_answer
    x, w, b, exp = conv_transpose_k4s2p1_known_answer()
    w3 = ops.deconv_k4s2_as_conv3x3(_dev(w))                     # [4 K, Cin, 1, 3, 3], K = 1
    layer = ops.ConvLayer(w3, None, _dev(np.tile(b, 4)), stride=(1, 1), pads=(0, 1, 1), relu=False, dtype=0)
    sub = layer(ops.to_ndhwc(_dev(x), 0), T=1).cpu().numpy()    # [1, 2, 2, cstride]: channel (dy * 2 + dx) * K + k = out[2 i + dy, 2 j + dx]
    got = np.zeros((4, 4), np.float32)
    for dy in range(2):
        for dx in range(2):
            got[dy::2, dx::2] = sub[0, :, :, dy * 2 + dx]
    np.testing.assert_array_equal(got, exp[0, 0])


def test_spatial_mean_softmax(ops):
    rs = np.random.RandomState(16)
    x = rs.randn(4, 64, 1, 7, 7).astype(np.float32)
    m = ops.spatial_mean(ops.to_ndhwc(_dev(x), 0), 0, 64).cpu().numpy()
    np.testing.assert_allclose(m, x.mean(axis=(2, 3, 4)), atol=1e-5)
    z = rs.randn(11, 12).astype(np.float32)
    sm = ops.softmax_rows(_dev(z), 2).cpu().numpy()
    np.testing.assert_allclose(sm, torch.softmax(torch.from_numpy(z[:, :2]), 1).numpy(), atol=1e-6)


@pytest.mark.parametrize('T,min_size,M,R', [(1, 0, 56, 9), (3, 0, 56, 9), (1, 40, 56, 9), (1, 0, 112, 3), (1, 0, 128, 2)])
def test_heatmaps_to_keypoints_matches_the_oracle(ops, T, min_size, M, R):
    """dat_heatmaps_to_keypoints vs the ORACLE's restatement of lib/utils/keypoints.py:94-149 on top of its cv2.resize INTER_CUBIC
    restatement (oracle/resize.py, pinned by exact-rational known answers): identical cells (x, y and logit exact), probability
    to fp32 summation order.  No product code on the reference side of this comparison."""
    from oracle import resize as oresize
    rs = np.random.RandomState(11)
    K = 17 if M == 56 else 3        # (M = 112 / 128: heat maps whose separable-kernel LDS footprint exceeds the 64-KB default limit)
    maps = rs.randn(R, T * K, M, M).astype(np.float32) * 2.0
    # smooth blobs so the maximum is not a lone noise pixel
    yy, xx = np.mgrid[0:M, 0:M]
    for r in range(R):
        for c in range(T * K):
            cy, cx = rs.uniform(5, M - 5, 2)
            maps[r, c] += 6.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 18.0).astype(np.float32)
    boxes = np.zeros((R, 4 * T), dtype=np.float32)
    for t in range(T):
        x1, y1 = rs.uniform(0, 300, R), rs.uniform(0, 200, R)
        w, h = rs.uniform(0.4, 260, R), rs.uniform(0.4, 330, R)      # includes boxes below 1 px
        boxes[:, 4 * t:4 * t + 4] = np.stack([x1, y1, x1 + w, y1 + h], axis=1)
    got = ops.heatmaps_to_keypoints(_dev(maps), _dev(boxes), T, K, min_size).cpu().numpy()
    ref = np.concatenate([oresize.heatmaps_to_keypoints(maps[:, t * K:(t + 1) * K], boxes[:, 4 * t:4 * t + 4], min_size)
                          for t in range(T)], axis=-1)
    assert got.shape == ref.shape == (R, 4, T * K)
    np.testing.assert_array_equal(got[:, :3], ref[:, :3])
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize('dtype_name', ['fp32', 'bf16'])
def test_fused_stem_conv_matches_torch(ops, dtype_name):
    """dat_stem_conv: conv1 [1,7,7]/s2/p3 + AffineChannelNd + ReLU straight from the NC(T)HW fp32 clip (ResNet3D.py:258-262)."""
    import torch.nn.functional as F
    dt = ops.F32 if dtype_name == 'fp32' else ops.BF16
    g = torch.Generator().manual_seed(3)
    for (N, T, H, W) in ((1, 2, 37, 53), (2, 1, 64, 96), (1, 3, 16, 70)):
        data = torch.randn((N, 3, T, H, W), generator=g) * 50
        w = torch.randn((64, 3, 1, 7, 7), generator=g) * 0.05
        scale, bias = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
        if dtype_name == 'bf16':
            data_r, w_r = nm.q16(data), nm.q16(w)
        else:
            data_r, w_r = data, w
        ref = F.relu(F.conv3d(data_r, w_r, None, stride=(1, 2, 2), padding=(0, 3, 3)) * scale.view(1, -1, 1, 1, 1) + bias.view(1, -1, 1, 1, 1))
        layer = ops.StemConv(w.cuda(), scale.cuda(), bias.cuda(), dt, relu=True)
        y = layer(data.cuda())                       # [N*T, Ho, Wo, 64]
        Ho, Wo = ref.shape[3], ref.shape[4]
        got = y.float().cpu().view(N, T, Ho, Wo, 64).permute(0, 4, 1, 2, 3)
        err = (got - ref).abs().max().item()
        tol = 2e-3 if dtype_name == 'fp32' else 0.02 * ref.abs().max().item()
        assert err < tol, (N, T, H, W, err, tol)
        if dtype_name == 'bf16':
            _bound(got, (data_r, w_r, scale, bias, None, (2, 2), (0, 3, 3), True), 3, (1, 7, 7), 'fused stem %r' % ((N, T, H, W),))


@pytest.mark.parametrize('dtype_name', ['fp32', 'bf16'])
def test_conv_one_pixel_wide_tiles(ops, dtype_name):
    """Regression: tiles that are ONE output column wide (KW == 1 convs on maps whose height is a multiple of the tile height and
    whose width is odd, and the 4x1 stem formulation from Ho = 128 up) decode patch rows with PW == 1, where the magic-number
    division constant 2^32 / PW does not fit 32 bits."""
    import torch.nn.functional as F
    dt = ops.F32 if dtype_name == 'fp32' else ops.BF16
    tdt = ops.tdtype(dt)
    g = torch.Generator().manual_seed(8)
    for (cin, cout, k, H, W) in ((64, 64, (1, 4, 1), 131, 7), (64, 128, (1, 1, 1), 128, 5), (64, 64, (1, 1, 1), 256, 3)):
        x = torch.randn((1, cin, 2, H, W), generator=g)
        w = torch.randn((cout, cin) + k, generator=g) * (1.0 / (cin * k[1])) ** 0.5
        if dtype_name == 'bf16':
            x, w = nm.q16(x), nm.q16(w)
        ref = F.conv3d(x, w, None)
        lay = ops.ConvLayer(w.cuda(), None, None, stride=(1, 1), pads=(0, 0, 0), relu=False, dtype=dt)
        xd = x.permute(0, 2, 3, 4, 1).reshape(2, H, W, cin).to(tdt).cuda().contiguous()
        y = lay(xd, T=2).float().cpu()
        got = y.view(1, 2, ref.shape[3], ref.shape[4], -1)[..., :cout].permute(0, 4, 1, 2, 3)
        err = (got - ref).abs().max().item()
        assert err < (1e-3 if dtype_name == 'fp32' else 0.03 * ref.abs().max().item()), (cin, cout, k, H, W, err)
        if dtype_name == 'bf16':
            _bound(got, (x, w, None, None, None, (1, 1), (0, 0, 0), False), cin, k, 'one-pixel tiles %r' % ((cin, cout, k, H, W),))
    # the packed-stem formulation at a height that selects 128 x 1 tiles
    data = torch.rand((1, 3, 1, 256, 96), generator=g) * 255 - 110
    w7 = torch.randn((64, 3, 1, 7, 7), generator=g) * 0.025
    ref = F.relu(F.conv3d(nm.q16(data) if dtype_name == 'bf16' else data,
                          nm.q16(w7) if dtype_name == 'bf16' else w7, None, stride=(1, 2, 2), padding=(0, 3, 3)))
    old = ops.stem_layer(w7.cuda(), torch.ones(64).cuda(), torch.zeros(64).cuda(), dt)
    y = old(ops.stem_pack(data.cuda(), dt), T=1).float().cpu().view(1, 1, 128, 48, 64).permute(0, 4, 1, 2, 3)
    assert (y - ref).abs().max().item() < (1e-2 if dtype_name == 'fp32' else 0.02 * ref.abs().max().item())
    if dtype_name == 'bf16':
        _bound(y, (nm.q16(data), nm.q16(w7), None, None, None, (2, 2), (0, 3, 3), True), 3, (1, 7, 7), 'one-pixel tiles: packed stem')


@pytest.mark.parametrize('clips', [1, 4])
def test_full_size_layers_spot_checked(ops, clips):
    """Size-independent check at the BENCH sizes (8 x 768 x 1344 clips, R-18 FPN3D): every distinct conv layer shape runs at full
    size through the planner's own tile / split-K choice, and random output positions (all channels) are compared with a direct
    evaluation of the receptive-field dot products.  (The small-shape parity tests cannot see tile-shape-dependent bugs such as the
    one-column-tile patch decoding fixed in round 1.)

    clips = 4 is the BENCHED forward: 32 frames on the frames axis, where the planner takes other branches
    (per-frame linear strips, other split-K factors, multi-round head grids) and the temporal taps must stop at the clip borders
    (the reference pads every clip on its own, lib/modeling/ResNet3D.py:258-284) -- so the sampled positions include the corners of
    the first and the last frame of EVERY clip, whose temporal neighbours belong to another clip."""
    sys_path = __import__('sys').path
    import os
    sys_path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import bench_layers
    g = torch.Generator(device='cuda').manual_seed(12)
    cases = [(name, cin, cout, k, st, hi, wi, clips * 8, 8) for (name, cin, cout, k, st, hi, wi, cnt) in bench_layers.layer_list('R18', 8, 768, 1344, 3)]
    # the 2D heads of the benched forward: RPN conv on the centre frame of every clip's P2, keypoint-head conv on 100 rois per clip
    cases += [('conv_rpn_fpn2', 256, 256, (1, 3, 3), 1, 192, 336, clips, 1), ('kps_head_conv', 512, 512, (1, 3, 3), 1, 14, 14, 100 * clips, 1)]
    for (name, cin, cout, k, st, hi, wi, F_, T) in cases:
        pads = (k[0] // 2, k[1] // 2, k[2] // 2) if name != 'stem_k4x1' else (0, 0, 0)
        w = torch.randn((cout, cin) + tuple(k), device='cuda', generator=g) * (2.0 / (cin * k[0] * k[1] * k[2])) ** 0.5
        w = nm.q16(w)
        bias = torch.randn(cout, device='cuda', generator=g)
        layer = ops.ConvLayer(w, None, bias, stride=(st, st), pads=pads, relu=False, dtype=ops.BF16)
        x = torch.randn((F_, hi, wi, layer.cin), device='cuda', generator=g).to(nm.h16())
        y = layer(x, T=T).float()
        ho, wo = layer.out_hw(hi, wi)
        assert y.shape[0] == F_
        xf = x.float()
        w64, x64 = w.double(), x.double()
        worst = 0.0
        got_s, ref_s, abs_s = [], [], []
        idx = torch.randint(0, F_ * ho * wo, (48 if clips == 1 else 24,), device='cuda', generator=g).tolist()
        for c_ in range(F_ // T if T > 1 else min(F_, 4)):     # corners + a random interior position of the first and the last frame of every clip
            for f in ((c_ * T, c_ * T + T - 1) if T > 1 else (c_, F_ - 1 - c_)):
                base = f * ho * wo
                idx += [base, base + ho * wo - 1, base + wo - 1, base + (ho - 1) * wo,
                        base + int(torch.randint(0, ho * wo, (1,), device='cuda', generator=g).item())]
        for p_ in idx:
            f, r = divmod(p_, ho * wo)
            oh, ow = divmod(r, wo)
            lo = (f // T) * T               # temporal taps stay inside the frame's own clip
            acc = bias.clone()
            acc64, abs64 = bias.double(), bias.double().abs()
            for kt in range(k[0]):
                ft = f + kt - pads[0]
                if ft < lo or ft >= lo + T:
                    continue
                for kh in range(k[1]):
                    ih = oh * st + kh - pads[1]
                    if ih < 0 or ih >= hi:
                        continue
                    for kw in range(k[2]):
                        iw = ow * st + kw - pads[2]
                        if iw < 0 or iw >= wi:
                            continue
                        acc += w[:, :, kt, kh, kw] @ xf[ft, ih, iw, :cin]
                        acc64 += w64[:, :, kt, kh, kw] @ x64[ft, ih, iw, :cin]
                        abs64 += w64[:, :, kt, kh, kw].abs() @ x64[ft, ih, iw, :cin].abs()
            worst = max(worst, (y[f, oh, ow, :cout] - acc).abs().max().item() / max(1.0, acc.abs().max().item()))
            got_s.append(y[f, oh, ow, :cout])
            ref_s.append(acc64)
            abs_s.append(abs64)
        assert worst < 0.02, (name, clips, worst)
        nm.assert_elementwise(torch.stack(got_s), torch.stack(ref_s), torch.stack(abs_s), nm.conv_k(cin, k), nm.h16(),
                              'full size %s clips=%d' % (name, clips))


def test_rpn_proposals_at_bench_size_vs_oracle(ops):
    """GenerateProposals + NMS + collect at the BENCH level sizes (768 x 1344: 257 796 anchors over P2..P6, pre/post 1000) against
    the oracle; continuous random scores (tie-free), so the kept sets must agree box for box."""
    from oracle import proposals as op
    from oracle.anchors import generate_anchors
    rs = np.random.RandomState(31)
    H0, W0 = 768, 1344
    im_info = np.array([[H0, W0, 1.0]], np.float32)
    specs, ref_r, ref_p = [], [], []
    for lvl in range(2, 7):
        H, W = int(np.ceil(H0 / 2. ** lvl)), int(np.ceil(W0 / 2. ** lvl))
        anchors = generate_anchors(2. ** lvl, (32 * 2. ** (lvl - 2),), (0.5, 1, 2))
        scores = rs.uniform(0.001, 0.999, (1, 3, H, W)).astype(np.float32)
        deltas = (rs.randn(1, 12, H, W) * 0.3).astype(np.float32)
        head, _ = _head_tensor(ops, scores, deltas, 0)
        lg = ops.to_ncdhw(head, 0, 1, 3, 1).cpu().numpy()[:, :, 0]
        probs_dev = (1.0 / (1.0 + np.exp(-lg.astype(np.float32)))).astype(np.float32)
        r, p = op.generate_proposals(probs_dev, deltas, im_info, anchors, 1. / 2 ** lvl, 1000, 1000, 0.7, 0)
        ref_r.append(r)
        ref_p.append(p)
        specs.append(ops.RpnLevelSpec(head, H, W, 3, 1, float(2 ** lvl), 64, 0, 3, 0, _dev(anchors.astype(np.float32))))
    rois, probs, counts = ops.rpn_proposals(specs, 0, im_info[0], 1000, 1000, 0.7, 0.)
    cnt = counts.cpu().numpy()
    for i in range(5):
        assert cnt[i] == ref_r[i].shape[0], (i, cnt[i], ref_r[i].shape)
        np.testing.assert_allclose(rois[i, :cnt[i]].cpu().numpy(), ref_r[i], atol=3e-3)
    out, n_out = ops.collect_rois(rois, probs, counts, 1000)
    exp = op.collect(ref_r, ref_p, 1000)
    assert int(n_out.item()) == exp.shape[0] == 1000
    np.testing.assert_allclose(out[:1000].cpu().numpy(), exp, atol=3e-3)


def test_fused_stem_and_maxpool_at_bench_size(ops):
    """conv1 + pool1 on a full 8 x 768 x 1344 clip vs torch on the CPU (bf16 operands)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(4)
    data = torch.rand((1, 3, 8, 768, 1344), generator=g) * 255 - 110
    w = torch.randn((64, 3, 1, 7, 7), generator=g) * 0.025
    scale, bias = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    ref = F.relu(F.conv3d(nm.q16(data), nm.q16(w), None, stride=(1, 2, 2), padding=(0, 3, 3)) *
                 scale.view(1, -1, 1, 1, 1) + bias.view(1, -1, 1, 1, 1))
    y = ops.StemConv(w.cuda(), scale.cuda(), bias.cuda(), ops.BF16, relu=True)(data.cuda())
    got = y.float().cpu().view(1, 8, 384, 672, 64).permute(0, 4, 1, 2, 3)
    assert (got - ref).abs().max().item() < 0.02 * ref.abs().max().item()
    # (the frames as a batch of one-frame clips: the same conv, a smaller im2col for the float64 reference)
    _bound(got.permute(2, 1, 0, 3, 4), (nm.q16(data).permute(2, 1, 0, 3, 4), nm.q16(w), scale, bias, None, (2, 2), (0, 3, 3), True), 3,
           (1, 7, 7), 'stem at bench size')
    pool = ops.maxpool_hw(y, ops.BF16, 3, 2, 1).float().cpu().view(1, 8, 192, 336, 64).permute(0, 4, 1, 2, 3)
    ref_pool = F.max_pool3d(got, kernel_size=(1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1))
    assert (pool - ref_pool).abs().max().item() == 0.0
    # dat_stem_conv_pool: the same two layers as one kernel, conv1 never written -- bit-identical pool1
    layer = ops.StemConv(w.cuda(), scale.cuda(), bias.cuda(), ops.BF16, relu=True)
    assert torch.equal(layer.pooled(data.cuda()), ops.maxpool_hw(y, ops.BF16, 3, 2, 1))


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('shape', [(1, 1, 7, 9), (2, 3, 45, 61), (1, 2, 64, 122), (1, 1, 130, 251), (1, 2, 23, 24)])
@pytest.mark.parametrize('relu', [True, False])
def test_stem_conv_pool_fused_equals_two_kernels(ops, dtype, shape, relu):
    """dat_stem_conv_pool == dat_stem_conv + dat_maxpool_hw bit for bit on ragged sizes (tile edges in both directions, inputs
    smaller than one tile, no ReLU so that negative maxima exercise the clamped window)."""
    dt = ops.BF16 if dtype == 'bf16' else ops.F32
    n, t, h, w_ = shape
    g = torch.Generator().manual_seed(h * 1000 + w_)
    data = (torch.rand((n, 3, t, h, w_), generator=g) * 255 - 110).cuda()
    w = (torch.randn((64, 3, 1, 7, 7), generator=g) * 0.025).cuda()
    scale, bias = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) - (0.0 if relu else 3.0)).cuda()
    layer = ops.StemConv(w, scale, bias, dt, relu=relu)
    two = ops.maxpool_hw(layer(data), dt, 3, 2, 1)
    one = layer.pooled(data)
    assert one.shape == two.shape
    assert torch.equal(one, two)


def test_roi_align_at_bench_size_vs_oracle(ops):
    """RoIAlign over the P2..P5 maps of a 768 x 1344 clip (256 channels, 1000 rois, 7x7 and 14x14): 24 rois checked against the
    oracle (legacy RoIAlign, per-RoI FPN level)."""
    from oracle import proposals as op
    from oracle.roi_align import roi_align_2d
    rs = np.random.RandomState(17)
    H0, W0 = 768, 1344
    feats = [rs.randn(1, 256, 1, H0 // 2 ** l, W0 // 2 ** l).astype(np.float32) for l in range(2, 6)]
    R = 1000
    x1, y1 = rs.uniform(0, W0 * 0.8, R), rs.uniform(0, H0 * 0.8, R)
    w, h = np.exp(rs.uniform(np.log(8), np.log(900), R)), np.exp(rs.uniform(np.log(8), np.log(700), R))
    rois = np.stack([np.zeros(R), x1, y1, np.minimum(x1 + w, W0 - 1), np.minimum(y1 + h, H0 - 1)], 1).astype(np.float32)
    lvls = op.map_rois_to_fpn_levels(rois[:, 1:], 2, 5)
    assert len(np.unique(lvls)) == 4
    fds = [ops.to_ndhwc(_dev(f), 0) for f in feats]
    for pooled in (7, 14):
        out = ops.roi_align(fds, [1. / 2 ** l for l in range(2, 6)], 0, _dev(rois), T=1, Tr=1, t0=0, pooled=pooled, sampling=2)
        out = out.cpu().numpy().transpose(0, 3, 1, 2)
        for i in list(range(0, R, 50)) + [R - 1, 1, 2, 3]:
            l = int(lvls[i])
            ref = roi_align_2d(feats[l - 2][:, :, 0], rois[i:i + 1], pooled, 1. / 2 ** l, 2)[0]
            assert np.abs(out[i] - ref).max() < 1e-4, (pooled, i, l)


@pytest.mark.parametrize('dtype', [0, 1])
def test_batched_proposals_collect_and_box_results_equal_the_one_image_calls(ops, dtype):
    """Round 3: several images per forward.  dat_rpn_proposals_batch / dat_collect_rois_batch / dat_box_results_batch run the image
    as a grid dimension of the same kernels: every image's rois, scores, counts, detections and keypoint rois must be BIT-identical
    to the one-image calls (reference loop: lib/ops/generate_proposals.py:133-147; per-image post-processing
    lib/core/test.py:750-806).  Images differ in content AND in im_info (clip bounds / min-size scale)."""
    from oracle.anchors import generate_anchors
    rs = np.random.RandomState(5)
    NI = 5
    shapes = {2: (40, 56), 3: (20, 28), 4: (10, 14), 5: (5, 7), 6: (3, 4)}
    im_info = np.array([[160., 224., 1.0], [150., 200., 1.2], [160., 224., 0.9], [120., 224., 1.0], [160., 180., 1.1]], np.float32)
    heads, anchors = [], []
    for lvl in range(2, 7):
        H, W = shapes[lvl]
        an = generate_anchors(2. ** lvl, (32 * 2. ** (lvl - 2),), (0.5, 1, 2)).astype(np.float32)
        scores = rs.uniform(0.01, 0.99, (NI, 3, H, W)).astype(np.float32)
        deltas = (rs.randn(NI, 12, H, W) * 0.3).astype(np.float32)
        lg = np.log(scores / (1 - scores)).astype(np.float32)
        cat = np.concatenate([lg, deltas], axis=1)[:, :, None]                        # (NI, 15, 1, H, W)
        heads.append(ops.to_ndhwc(_dev(cat), dtype, 64))                              # [NI, H, W, 64]
        anchors.append(_dev(an))

    def specs(frame):
        return [ops.RpnLevelSpec(heads[i], shapes[l][0], shapes[l][1], 3, 1, float(2 ** l), 64, 0, 3, frame, anchors[i])
                for i, l in enumerate(range(2, 7))]
    pre, post = 600, 200
    rois_b, probs_b, counts_b = ops.rpn_proposals(specs(0), dtype, im_info, pre, post, 0.7, 4., n_images=NI, frame_stride=1)
    out_b, n_b = ops.collect_rois(rois_b, probs_b, counts_b, post)
    assert rois_b.shape == (NI, 5, post, 5) and out_b.shape == (NI * post, 5) and n_b.shape == (NI,)
    singles = []
    for i in range(NI):
        r, p, c = ops.rpn_proposals(specs(i), dtype, im_info[i], pre, post, 0.7, 4., batch_idx=float(i))
        assert torch.equal(c, counts_b[i]), (i, c, counts_b[i])
        assert torch.equal(r, rois_b[i]) and torch.equal(p, probs_b[i]), i
        o, n = ops.collect_rois(r, p, c, post)
        k = int(n.item())
        assert k == int(n_b[i].item()) and k > 20
        assert torch.equal(o[:k], out_b[i * post:i * post + k])
        assert (o[:k, 0] == i).all()
        singles.append((o, n))
    # detection post-processing over the batch: rows of image i = [i * post, (i + 1) * post)
    K = 3
    R = NI * post
    logits = rs.randn(R, K).astype(np.float32) * 2
    prob = _dev((np.exp(logits) / np.exp(logits).sum(axis=1, keepdims=True)).astype(np.float32))
    pred = _dev((rs.randn(R, K * 4) * np.tile([1.0, 1.0, 2.0, 2.0], K)).astype(np.float32))
    scales = [float(s) for s in im_info[:, 2]]
    shapes_im = [(int(round(h / s)), int(round(w / s)), 3) for h, w, s in im_info]
    args = ((10., 10., 5., 5.), float(np.float32(np.log(1000. / 16.))), 0.05, 0.5, 30, 30)
    dets_b, kp_b, nout_b = ops.box_results(out_b, n_b, prob, pred, K, 1, scales, shapes_im, *args, n_images=NI)
    assert dets_b.shape == (NI * 30, 6) and kp_b.shape == (NI * 30, 5) and nout_b.shape == (NI, 2)
    for i in range(NI):
        o, n = singles[i]
        d1, k1, n1 = ops.box_results(o, n, prob[i * post:(i + 1) * post], pred[i * post:(i + 1) * post], K, 1, scales[i],
                                     shapes_im[i], *args)
        assert torch.equal(n1, nout_b[i]), (i, n1, nout_b[i])
        k = int(n1[0].item())
        assert k > 0
        assert torch.equal(d1, dets_b[i * 30:(i + 1) * 30])
        assert torch.equal(k1[:, 1:], kp_b[i * 30:(i + 1) * 30, 1:])
        assert (kp_b[i * 30:i * 30 + k, 0] == i).all() and not kp_b[i * 30 + k:(i + 1) * 30].any()


@pytest.mark.parametrize('h,w,target,max_size,T,stride', [(72, 128, 80, 133, 2, 32), (60, 80, 80, 1333, 1, 32), (97, 53, 64, 100, 3, 0),
                                                          (720, 1280, 800, 1333, 1, 32)])
def test_device_preprocessing_is_bit_identical_to_the_host_path(ops, h, w, target, max_size, T, stride):
    """dat_preprocess_frames (uint8 BGR frames on the device -> `data`) vs the host path it replaces, utils.blob.prep_im_for_blob +
    im_list_to_blob (reference lib/utils/blob.py:40-90), and vs the independent oracle/resize.py restatement of cv2.INTER_LINEAR:
    bit-identical fp32 blobs, up- and down-scaling, padded and unpadded, clips and single frames."""
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import blob as blob_utils
    from oracle import resize as oresize
    reset_cfg()
    rs = np.random.RandomState(h + w)
    frames = rs.randint(0, 256, (2 * T, h, w, 3)).astype(np.uint8)
    scale = blob_utils.test_scale((h, w), target, max_size)
    data, (oh, ow) = ops.preprocess_frames(torch.from_numpy(frames).cuda(), T, scale, cfg.PIXEL_MEANS, stride)
    got = data.cpu().numpy()
    assert got.shape[:3] == (2, 3, T)
    for f in range(2 * T):
        ims, scales = blob_utils.prep_im_for_blob(frames[f], cfg.PIXEL_MEANS, (target,), max_size)
        assert scales[0] == scale and ims[0].shape[:2] == (oh, ow)
        ref = ims[0]
        ora = oresize.resize_linear((frames[f].astype(np.float32) - cfg.PIXEL_MEANS).astype(np.float32), fx=scale, fy=scale)
        np.testing.assert_array_equal(ref, ora)
        mine = got[f // T, :, f % T]
        np.testing.assert_array_equal(mine[:, :oh, :ow], ref.transpose(2, 0, 1))
        assert not mine[:, oh:].any() and not mine[:, :, ow:].any()
    if stride:
        assert got.shape[3] % stride == 0 and got.shape[4] % stride == 0 and got.shape[3] - oh < stride


LW_CASES = [
    # name, T, H, W (input), Cin, Cout, stride, relu, res_mode, affine: layers the weights-in-LDS 1x1 kernel (conv1x1_lw_kernel) takes
    ('k64_c64', 2, 192, 200, 64, 64, 1, True, 0, True),                     # res2_0_branch2a
    ('k256_c64', 2, 192, 200, 256, 64, 1, True, 0, True),                   # res2_x_branch2a (R-50)
    ('k512_c128', 2, 192, 200, 512, 128, 1, True, 0, True),                 # res3_x_branch2a
    ('k128_c512_sum', 2, 192, 200, 128, 512, 1, True, 1, True),             # res3_x_branch2c + Sum + ReLU: two passes of 256 channels
    ('k256_c256_up2', 2, 192, 200, 256, 256, 1, False, 2, False),           # FPN P2 lateral of R-50 + top-down Sum
    ('k512_c256_up2_parts2', 2, 128, 160, 512, 256, 1, False, 2, False),    # P3 lateral: weights 256 KB -> two cout parts (on a map too small for the K-streaming kernel, which takes it otherwise)
    ('k256_c512_s2_parts2', 2, 384, 400, 256, 512, 2, False, 0, True),      # res3_0_branch1: stride 2, two cout parts
    ('k256_c128_s2', 2, 384, 400, 256, 128, 2, True, 0, True),              # res3_0_branch2a: stride 2 (STRIDE_1X1)
    ('k256_c200_ragged', 2, 191, 201, 256, 200, 1, True, 1, True),          # Cout not a multiple of 32, ragged last tile, odd W
    ('k128_c15', 3, 190, 202, 128, 15, 1, False, 0, False),                 # an RPN-head-sized output (padded to 64 stored channels)
]


@pytest.mark.parametrize('case', LW_CASES, ids=[c[0] for c in LW_CASES])
def test_conv1x1_weights_in_lds_kernel(ops, case):
    """conv1x1_lw_kernel (round 3: HBM-bound 1x1x1 layers of R-50's res2 / res3 and the FPN laterals; ResNet3D.py:21-55, :89-101,
    FPN3D.py:111-134) against torch and -- bit for bit -- against the generic kernel (forced plan): K = 64..512, one or two
    channel passes, two cout parts, stride 2, both residual modes, Cout padding, ragged tiles."""
    name, T, H, W, Cin, Cout, stride, relu, res_mode, affine = case
    rs = np.random.RandomState(abs(hash(name)) % 1000)
    q = nm.q16
    x = q(rs.randn(1, Cin, T, H, W).astype(np.float32))
    w = q((rs.randn(Cout, Cin, 1, 1, 1) * np.sqrt(2.0 / Cin)).astype(np.float32))
    scale = rs.uniform(0.5, 1.5, Cout).astype(np.float32) if affine else None
    bias = (rs.randn(Cout) * 0.1).astype(np.float32)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = res_small = None
    if res_mode == 1:
        res = q(rs.randn(1, Cout, T, Ho, Wo).astype(np.float32))
    elif res_mode == 2:
        res_small = q(rs.randn(1, Cout, T, Ho // 2, Wo // 2).astype(np.float32))
        res = np.repeat(np.repeat(res_small, 2, axis=3), 2, axis=4)
    ref = _conv_ref(x, w, scale, bias, res, (stride, stride), (0, 0, 0), relu)
    layer = ops.ConvLayer(_dev(w), None if scale is None else _dev(scale), _dev(bias), stride=(stride, stride), pads=(0, 0, 0),
                          relu=relu, dtype=1)
    xd = ops.to_ndhwc(_dev(x), 1)
    rd = None
    if res_mode == 1:
        rd = ops.to_ndhwc(_dev(res), 1, layer.cstride)
    elif res_mode == 2:
        rd = ops.to_ndhwc(_dev(res_small), 1, layer.cstride)
    prof = ops.ConvProfiler(capacity=8)
    prof.start()
    y = layer(xd, T=T, residual=rd, res_mode=res_mode)
    rec = prof.stop()
    assert [t for t, _, _ in rec] == [2560331], 'the layer did not take the weights-in-LDS kernel: tags %r' % ([t for t, _, _ in rec],)
    try:
        assert ops.tune_plan(128, 1) == 0
        y_gen = layer(xd, T=T, residual=rd, res_mode=res_mode)
    finally:
        ops.tune_plan(0, 0)
    assert torch.equal(y, y_gen), 'differs from the generic kernel in %d elements' % int((y != y_gen).sum())
    got = ops.to_ncdhw(y, 1, 1, Cout, T).cpu().numpy()
    err = np.abs(got - ref).max()
    print('lw %s max-abs err %.3e (ref max %.2f)' % (name, err, np.abs(ref).max()))
    assert err < 3e-2 * max(1.0, np.abs(ref).max() / 4)
    _bound(got, (x, w, scale, bias, res, (stride, stride), (0, 0, 0), relu), Cin, (1, 1, 1), 'lw ' + name)
    if layer.cstride > Cout:          # the padding channels of the blob stay zero
        assert not y[..., Cout:].any()


KS_CASES = [
    # name, T, H, W (input), Cin, Cout, stride, relu, res_mode, affine: layers the K-streaming 1x1 kernel (conv1x1_ks_kernel, round 6) takes
    ('k1024_c256', 2, 192, 200, 1024, 256, 1, True, 0, True),                # res4_x_branch2a (R-50 / R-101)
    ('k2048_c512', 2, 128, 200, 2048, 512, 1, True, 0, True),                # res5_x_branch2a: two cout blocks share the input tiles
    ('k1024_c2048_s2', 2, 192, 200, 1024, 2048, 2, False, 0, True),          # res5_0_branch1: stride 2, eight cout blocks
    ('k1024_c256_up2', 2, 192, 200, 1024, 256, 1, False, 2, False),          # FPN P4 lateral + nearest-2x top-down Sum
    ('k1024_c512_sum', 2, 160, 168, 1024, 512, 1, True, 1, True),            # data gradient of a branch2c-shaped layer: Sum + ReLU epilogue
    ('k1088_c200_ragged', 2, 191, 201, 1088, 200, 1, True, 1, True),         # K not a power of two, Cout padded to 256, ragged last tile
    ('k1024_c256_mask', 2, 160, 168, 1024, 256, 1, False, 3, False),         # data gradient of res4_x_branch2c with the ReLU backward of its input fused (res_mode 3)
]


@pytest.mark.parametrize('case', KS_CASES, ids=[c[0] for c in KS_CASES])
def test_conv1x1_k_streaming_kernel(ops, case):
    """conv1x1_ks_kernel (round 6: the 1x1x1 layers whose weights do not fit LDS, K >= 1024 -- R-50's res4 / res5 `branch2a`, the res5
    shortcut, the P4 / P5 laterals; ResNet3D.py:21-55, :89-101, FPN3D.py:111-134) against torch on the same bf16 operands and -- bit for
    bit -- against the generic kernel it replaces (forced plan): stride 2, both residual modes, several cout blocks, Cout padding,
    a ragged last tile."""
    name, T, H, W, Cin, Cout, stride, relu, res_mode, affine = case
    rs = np.random.RandomState(abs(hash(name)) % 1000)
    q = nm.q16
    x = q(rs.randn(1, Cin, T, H, W).astype(np.float32))
    w = q((rs.randn(Cout, Cin, 1, 1, 1) * np.sqrt(2.0 / Cin)).astype(np.float32))
    scale = rs.uniform(0.5, 1.5, Cout).astype(np.float32) if affine else None
    bias = (rs.randn(Cout) * 0.1).astype(np.float32)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = res_small = None
    if res_mode == 1:
        res = q(rs.randn(1, Cout, T, Ho, Wo).astype(np.float32))
    elif res_mode == 2:
        res_small = q(rs.randn(1, Cout, T, Ho // 2, Wo // 2).astype(np.float32))
        res = np.repeat(np.repeat(res_small, 2, axis=3), 2, axis=4)
    elif res_mode == 3:
        res = q(rs.randn(1, Cout, T, Ho, Wo).astype(np.float32))             # the MASK: out = mask > 0 ? v : 0
    torch.set_num_threads(max(1, min(32, torch.get_num_threads())))
    ref = _conv_ref(x, w, scale, bias, None if res_mode == 3 else res, (stride, stride), (0, 0, 0), relu)
    if res_mode == 3:
        ref = np.where(res > 0, ref, 0.0).astype(np.float32)
    layer = ops.ConvLayer(_dev(w), None if scale is None else _dev(scale), _dev(bias), stride=(stride, stride), pads=(0, 0, 0),
                          relu=relu, dtype=1)
    xd = ops.to_ndhwc(_dev(x), 1)
    rd = None
    if res_mode in (1, 3):
        rd = ops.to_ndhwc(_dev(res), 1, layer.cstride)
    elif res_mode == 2:
        rd = ops.to_ndhwc(_dev(res_small), 1, layer.cstride)
    prof = ops.ConvProfiler(capacity=8)
    prof.start()
    y = layer(xd, T=T, residual=rd, res_mode=res_mode)
    rec = prof.stop()
    assert [t for t, _, _ in rec] == [2560341], 'the layer did not take the K-streaming kernel: tags %r' % ([t for t, _, _ in rec],)
    try:
        assert ops.tune_plan(128, 1) == 0
        y_gen = layer(xd, T=T, residual=rd, res_mode=res_mode)
    finally:
        ops.tune_plan(0, 0)
    assert torch.equal(y, y_gen), 'differs from the generic kernel in %d elements' % int((y != y_gen).sum())
    got = ops.to_ncdhw(y, 1, 1, Cout, T).cpu().numpy()
    err = np.abs(got - ref).max()
    print('ks %s max-abs err %.3e (ref max %.2f), %.1f us' % (name, err, np.abs(ref).max(), 1e3 * rec[0][2]))
    assert err < 3e-2 * max(1.0, np.abs(ref).max() / 4)
    _bound(got, (x, w, scale, bias, None if res_mode == 3 else res, (stride, stride), (0, 0, 0), relu, res if res_mode == 3 else None),
           Cin, (1, 1, 1), 'ks ' + name)
    if layer.cstride > Cout:          # the padding channels of the blob stay zero
        assert not y[..., Cout:].any()


@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
@pytest.mark.parametrize('h,w,target,max_size,T,stride', [
    (720, 1280, 800, 1333, 2, 32),      # the benched geometry: x 1.0414 -> 750 x 1333, padded to 768 x 1344
    (180, 320, 256, 333, 3, 0),         # a shipped 3D config's scale rule on a small frame, unpadded blob with odd width
    (97, 131, 64, 100, 1, 32),          # DOWN-scaling (x 0.66), odd source size, heavy padding
    (33, 47, 90, 150, 2, 0),            # x 2.7 up-scaling: long runs of output pixels inside one source cell, borders on every tile
    (50, 3, 60, 400, 1, 0),             # a three-pixel-wide frame (every column is a border column)
])
def test_stem_from_uint8_frames_is_bit_identical_to_the_blob_path(ops, dtype_name, h, w, target, max_size, T, stride):
    """dat_stem_conv_pool_u8 (round 6: conv1 + AffineChannelNd + ReLU + pool1 straight from the uploaded uint8 frames, the pre-processing
    arithmetic of lib/utils/blob.py:40-90 evaluated in the stem's patch loader) against dat_preprocess_frames + dat_stem_conv_pool: the
    SAME pool1, bit for bit -- up- and down-scaling, padded and unpadded blobs, border columns / rows, the last pixel of the buffer."""
    from detectandtrack_amd.core.config import cfg, reset_cfg
    from detectandtrack_amd.utils import blob as blob_utils
    reset_cfg()
    dt = ops.F32 if dtype_name == 'fp32' else ops.BF16
    rs = np.random.RandomState(h * 7 + w)
    F = 2 * T
    frames = torch.from_numpy(rs.randint(0, 256, (F, h, w, 3)).astype(np.uint8)).cuda()
    scale = blob_utils.test_scale((h, w), target, max_size)
    g = torch.Generator().manual_seed(5)
    wt = (torch.randn((64, 3, 1, 7, 7), generator=g) * 0.05).cuda()
    sc, bi = (torch.rand(64, generator=g) + 0.5).cuda(), torch.randn(64, generator=g).cuda()
    layer = ops.StemConv(wt, sc, bi, dt, relu=True)
    data, (oh, ow) = ops.preprocess_frames(frames, T, scale, cfg.PIXEL_MEANS, stride)
    ref = layer.pooled(data)
    fb = blob_utils.FrameBlob(frames, T, scale, (oh, ow), tuple(data.shape[-2:]), True, cfg.PIXEL_MEANS)
    assert tuple(fb.shape) == tuple(data.shape)
    got = layer.pooled_u8(fb)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert torch.equal(got, ref), 'differs in %d of %d elements, max %.3e' % (int((got != ref).sum()), got.numel(),
                                                                             float((got.float() - ref.float()).abs().max()))
    assert torch.equal(fb.materialise(), data)
