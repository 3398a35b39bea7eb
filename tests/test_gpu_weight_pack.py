"""The weight packers of csrc/conv_pack.hip -- per layer (ConvLayer(...).packed, ConvLayer.repack) and batched (PackBatch.run), forward
and data-gradient form, fp32 and the build's 16-bit format -- bit for bit against tests/dgrad_refs.packed_expected, padding included.
Every packed buffer is filled with 0xFF bytes before the packer runs: a slot the packer leaves unwritten reads as NaN.  The expected
value is one fp32 multiply (w * scale) and one rounding to nearest even, both IEEE operations, so there is no tolerance."""
import numpy as np
import pytest
import torch

from tests import dgrad_refs as dr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _fmt(ops, dtype):
    return 'fp32' if dtype == 'fp32' else ('fp16' if ops.L.H16 == 'fp16' else 'bf16')


def _layer(ops, w, scale, dgrad, dtype):
    dt = ops.F32 if dtype == 'fp32' else ops.BF16
    if dgrad:
        return ops.ConvLayer(None, None, None, stride=(1, 1), pads=(0, 0, 0), relu=False, dtype=dt, dgrad_of=(w, scale))
    return ops.ConvLayer(w, None, None, stride=(1, 1), pads=(0, 0, 0), relu=False, dtype=dt)


def _offset_master(w_np):
    """the master as a 4-byte-offset view of a larger fp32 buffer: contiguous, fp32, NOT 16-byte aligned"""
    n = w_np.size
    buf = torch.zeros(n + 8, dtype=torch.float32, device='cuda')
    view = buf[1:1 + n].view(w_np.shape)
    view.copy_(torch.from_numpy(w_np))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _check(ops, layer, w_np, scale_np, dgrad, dtype, what):
    fmt = _fmt(ops, dtype)
    want, d = dr.packed_expected(w_np, scale_np if dgrad else None, dgrad, fmt, cin=layer.cin)
    es = 4 if fmt == 'fp32' else 2
    assert layer.packed.numel() == d['ntap'] * d['cout_pad'] * d['cin'] * es, (what, layer.packed.numel(), d)
    torch.cuda.synchronize()
    got = dr.unpack(layer.packed, d, fmt)
    gb, wb = dr.bits(got), dr.bits(want)
    if not torch.equal(gb, wb):
        bad = (gb != wb).nonzero()
        t, co, ci = [int(v) for v in bad[0]]
        rows, cols = (w_np.shape[1], w_np.shape[0]) if dgrad else (w_np.shape[0], w_np.shape[1])
        in_pad = int(((bad[:, 1] >= rows) | (bad[:, 2] >= cols)).sum())
        raise AssertionError('%s: %d of %d packed elements differ (%d of them padding, %d NaN = never written); first at tap %d row %d '
                             'col %d: got %r, want %r' % (what, bad.shape[0], gb.numel(), in_pad, int(torch.isnan(got.float()).sum()),
                                                          t, co, ci, float(got[t, co, ci]), float(want[t, co, ci])))


@pytest.mark.parametrize('dtype', ['fp32', '16'])
@pytest.mark.parametrize('pc', dr.PACK_CASES, ids=dr.pack_case_id)
def test_per_layer_packer_is_bit_equal_to_the_expected_image(ops, pc, dtype):
    """dat_conv3d_pack_weights / _dgrad through ConvLayer: taps 1, 3, 9, 27, 49 (the tiled kernel) and 125 (the element-wise kernel,
    above 79 taps); rows and columns on tile boundaries and ragged; run lengths that are no multiple of 4 floats (no 16-byte loads)."""
    shape, dgrad = pc
    w_np, scale_np = dr.pack_master(shape)
    w, scale = torch.from_numpy(w_np).cuda(), torch.from_numpy(scale_np).cuda()
    layer = _layer(ops, w, scale, dgrad, dtype)
    layer.packed.fill_(0xFF)
    layer.repack(weights_only=True)
    _check(ops, layer, w_np, scale_np, dgrad, dtype, 'repack %s' % dr.pack_case_id(pc))
    # ... and the packing of the constructor, into a buffer the allocator hands out uninitialised: after an in-place master update
    w.mul_(0.5)
    layer2 = _layer(ops, w, scale, dgrad, dtype)
    _check(ops, layer2, w_np * np.float32(0.5), scale_np, dgrad, dtype, 'constructor %s' % dr.pack_case_id(pc))


OFFSET_CASES = [((64, 64, 1, 1, 1), False), ((64, 64, 1, 1, 1), True), ((128, 64, 1, 3, 3), False), ((128, 64, 1, 3, 3), True),
                ((64, 128, 3, 3, 3), True)]


@pytest.mark.parametrize('dtype', ['fp32', '16'])
@pytest.mark.parametrize('pc', OFFSET_CASES, ids=dr.pack_case_id)
def test_master_at_a_four_byte_offset_takes_the_scalar_loads_on_full_tiles(ops, pc, dtype):
    """A master that is a view one float into a larger buffer: friendly sizes, full tiles, but no 16-byte alignment -- pack_tile's
    scalar load branches on tiles that are NOT ragged (aligned masters reach those branches on ragged last tiles only).

    Can it occur in training?  Trainer.__init__ (training.py) lays the masters out back to back in one flat fp32 buffer, in backward
    completion order, with no alignment between them, and the workspace's device master IS that slice: a master is 16-byte aligned
    only while every weight before it has a multiple of 4 elements.  Every shipped config satisfies that (each conv / FC weight has a
    channel count or a 4 x 4 / 7 x 7 x 64 factor that makes its size a multiple of 4; biases come after all weights), but nothing
    enforces it -- a head with an odd class count in front of an odd-sized weight would hand the packer such a view."""
    shape, dgrad = pc
    w_np, scale_np = dr.pack_master(shape, seed=11)
    w, scale = _offset_master(w_np), torch.from_numpy(scale_np).cuda()
    layer = _layer(ops, w, scale, dgrad, dtype)
    assert layer.w_src.data_ptr() == w.data_ptr(), 'the layer copied the master: the view no longer reaches the packer'
    layer.packed.fill_(0xFF)
    layer.repack(weights_only=True)
    _check(ops, layer, w_np, scale_np, dgrad, dtype, 'offset master %s' % dr.pack_case_id(pc))


@pytest.mark.parametrize('dtype', ['fp32', '16'])
def test_batched_packer_is_bit_equal_to_the_expected_images(ops, dtype):
    """PackBatch.run over one table: entries of all three tile widths (64, 32 and 16 input channels a tile: <= 4, <= 9 and more taps;
    PackBatch issues one launch per tap count, so the widths meet in one run, and two different layers share each launch), forward
    and data-gradient mixed, ragged and full, the no-16-byte-loads shape and masters at a 4-byte offset."""
    specs = [(pc, False) for pc in dr.PACK_CASES if int(np.prod(pc[0][2:])) <= 63] + [(pc, True) for pc in OFFSET_CASES]
    layers, keep = [], []
    for (shape, dgrad), offset in specs:
        w_np, scale_np = dr.pack_master(shape, seed=23)
        w = _offset_master(w_np) if offset else torch.from_numpy(w_np).cuda()
        scale = torch.from_numpy(scale_np).cuda()
        layers.append(_layer(ops, w, scale, dgrad, dtype))
        keep.append((w, scale, w_np, scale_np))
    assert {l.kt * l.kh * l.kw for l in layers} == {1, 3, 9, 27, 49}
    batch = ops.PackBatch(layers)
    for (w, _, w_np, _), l in zip(keep, layers):      # an "SGD step" in place: the batch reads the masters when it runs
        w.mul_(0.75)
        w_np *= np.float32(0.75)
        l.packed.fill_(0xFF)
    batch.run()
    for ((shape, dgrad), offset), (w, scale, w_np, scale_np), l in zip(specs, keep, layers):
        _check(ops, l, w_np, scale_np, dgrad, dtype, 'batch %s%s' % (dr.pack_case_id((shape, dgrad)), ' offset' if offset else ''))
