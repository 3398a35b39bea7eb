"""The 16x16x32 MFMA shape (DAT_CONV_MFMA=1) of conv3x3_bt_kernel and of the generic kernel's 16-bit 128-channel dense 3x3 variants
against the 32x32x16 shape (DAT_CONV_MFMA=0), every case in a fresh context under both switch values:

  * every output element inside the float64 per-element bound of tests/numerics.py, under each value;
  * under each value the big-tile kernel (DAT_CONV_BT=2) bit for bit the generic kernel under the forced (256, 1) plan -- the two
    kernels always share a shape --, linear strips bit for bit the 2-D tiling;
  * the outputs under 0 and under 1 within twice that bound of each other (the shapes may sum k in a different order).

The shapes are the smallest that reach what the new code adds: ragged tiles of both tile shapes, two 256-channel blocks, a partial
channel block, several channel chunks (the double-buffered patches and the weight ring across patch borders), temporal taps with clip
borders and the rotated tap start, split-K, per-frame and whole-sequence linear strips whose border taps read the zero row.
Float64 references are computed once per case and left unchanged.  The fp16 build runs the big-tile case of
tests/test_gpu_fp16_edges.py ('big_tile_3x3') in one child process started with DAT_H16=fp16."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import numerics as nm
from tests.test_gpu_kernels import _dev, _in_fresh_context

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_TAG = 2562561            # dispatcher tag of the big-tile kernel on 16-bit tensors


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from detectandtrack_amd.ops import hip_ops
    return hip_ops


def _generic_tag(bp):
    return 128 * 10000 + bp * 10 + 1


class _Case(object):
    """Operands, layer and float64 reference of one layer shape (built once); run(env, plan, **kw) -> (output NDHWC, tags)."""

    def __init__(self, ops, name, N, T, H, W, Cin, Cout, kt, relu=False, res_mode=0, affine=False, out_t=None, seed=0):
        self.ops, self.name, self.N, self.T, self.Cout, self.out_t = ops, name, N, T, Cout, out_t
        rs = np.random.RandomState(seed + W + Cin)
        q = nm.q16
        x = q(rs.randn(N, Cin, T, H, W).astype(np.float32))
        w = q((rs.randn(Cout, Cin, kt, 3, 3) * np.sqrt(2.0 / (Cin * 9 * kt))).astype(np.float32))
        scale = rs.uniform(0.5, 1.5, Cout).astype(np.float32) if affine else None
        bias = (rs.randn(Cout) * 0.1).astype(np.float32)
        res = res_small = None
        if res_mode == 1:
            res = q(rs.randn(N, Cout, T, H, W).astype(np.float32))
        elif res_mode == 2:
            res_small = q(rs.randn(N, Cout, T, H // 2, W // 2).astype(np.float32))
            res = np.repeat(np.repeat(res_small, 2, axis=3), 2, axis=4)
        pads = (kt // 2, 1, 1)
        self.K = nm.conv_k(Cin, (kt, 3, 3))
        self.ref, self.absref = nm.conv_ref64(x, w, scale, bias, res, (1, 1), pads, relu)
        self.otn = T
        if out_t is not None:
            sl = slice(out_t[0], out_t[0] + out_t[1])
            self.ref, self.absref, self.otn = self.ref[:, :, sl], self.absref[:, :, sl], out_t[1]
        self.bound = nm.bound(self.ref, self.absref, self.K, nm.h16())
        self.layer = ops.ConvLayer(_dev(w), None if scale is None else _dev(scale), _dev(bias), stride=(1, 1), pads=pads, relu=relu, dtype=ops.BF16)
        self.x = ops.to_ndhwc(_dev(x), ops.BF16)
        self.res_mode = res_mode
        self.rd = None
        if res_mode:
            rsrc = res if res_mode == 1 else res_small
            if out_t is not None:
                rsrc = rsrc[:, :, out_t[0]:out_t[0] + out_t[1]]
            self.rd = ops.to_ndhwc(_dev(np.ascontiguousarray(rsrc)), ops.BF16, self.layer.cstride)

    def launch(self, plan=None):
        """on the CURRENT context"""
        ops = self.ops
        prof = ops.ConvProfiler(capacity=8)
        try:
            if plan is not None:
                assert ops.tune_plan(*plan) == 0
            prof.start()
            y = self.layer(self.x, T=self.T, residual=self.rd, res_mode=self.res_mode, out_t=self.out_t)
            tags = [t for t, _, _ in prof.stop()]
        finally:
            if plan is not None:
                ops.tune_plan(0, 0)
        return y, tags

    def values(self, y):
        return self.ops.to_ncdhw(y, self.ops.BF16, self.N, self.Cout, self.otn).cpu().numpy()

    def check(self, y, what):
        got = self.values(y)
        ratio = float((np.abs(got - self.ref) / self.bound).max())
        print('mfma16 %s %s (%s): worst err / bound %.3f' % (self.name, what, str(nm.h16()).replace('torch.', ''), ratio))
        nm.assert_elementwise(got, self.ref, self.absref, self.K, nm.h16(), '%s %s' % (self.name, what))
        return got

    def check_pair(self, got0, got1):
        """the two shapes against each other: twice the per-element bound"""
        d = np.abs(got0 - got1)
        ratio = float((d / (2 * self.bound)).max())
        print('mfma16 %s: |shape 0 - shape 1| worst / (2 x bound) %.3f, %d of %d elements differ' % (self.name, ratio, int((d > 0).sum()), d.size))
        assert (d <= 2 * self.bound).all(), '%s: the two MFMA shapes differ by %.3f of twice the bound' % (self.name, ratio)


def _env(mf, **more):
    e = {'DAT_CONV_MFMA': str(mf)}
    e.update(more)
    return e


BT_CASES = {
    # ragged tiles of 8 x 32 (100 x 180: 13 x 6 tiles), two 256-channel blocks, four channel chunks, the up-sampled top-down residual
    'ragged_two_channel_blocks': dict(N=1, T=3, H=100, W=180, Cin=256, Cout=512, kt=1, res_mode=2),
    # two clips of 3 frames (clip borders: frames with two valid temporal taps; the rotated tap start), two channel chunks, ragged tiles;
    # one clip would be 360 blocks, below the 384 at which DAT_CONV_BT=2 takes the big-tile kernel on 256 CUs
    'clip_borders_3x3x3': dict(N=2, T=3, H=120, W=250, Cin=128, Cout=256, kt=3, relu=True, res_mode=1, affine=True),
}


@pytest.mark.parametrize('name', sorted(BT_CASES))
def test_big_tile_kernel_both_shapes(ops, name):
    c = _Case(ops, name, seed=1, **BT_CASES[name])
    got = {}
    for mf in (0, 1):
        (y, tags), (y_gen, tags_gen) = _in_fresh_context(_env(mf, DAT_CONV_BT='2'), lambda: (c.launch(), c.launch((256, 1))))
        assert tags == [BT_TAG], 'shape %d: not the big-tile kernel: tags %r' % (mf, tags)
        assert tags_gen == [_generic_tag(256)], tags_gen
        assert torch.equal(y, y_gen), 'shape %d: the big-tile and the generic kernel differ' % mf
        got[mf] = c.check(y, 'big-tile, shape %d' % mf)
    c.check_pair(got[0], got[1])


def test_generic_kernel_partial_channel_block_both_shapes(ops):
    """64 -> 200 (the second 128-channel block holds 72 channels), two clips of four 9 x 13 frames: ragged tiles at both tile sizes and
    split-K (one chunk: the frames at the clip borders leave a split an empty or a one-patch range)."""
    c = _Case(ops, 'partial_channel_block', N=2, T=4, H=9, W=13, Cin=64, Cout=200, kt=3, relu=True, res_mode=1, affine=True, seed=2)
    for plan in ((128, 1), (128, 2), (256, 1)):
        got = {}
        for mf in (0, 1):
            y, tags = _in_fresh_context(_env(mf), lambda: c.launch(plan))
            assert tags == [_generic_tag(plan[0])], (mf, plan, tags)
            got[mf] = c.check(y, 'plan %dx%d, shape %d' % (plan + (mf,)))
        c.check_pair(got[0], got[1])


def test_linear_strips_per_frame_both_shapes(ops):
    """128 -> 256, 3x3x3 on 24 x 42 maps, the centre frame of every clip: one linear strip per frame, bit for bit the 2-D tiling."""
    c = _Case(ops, 'linear_strips', N=2, T=4, H=24, W=42, Cin=128, Cout=256, kt=3, relu=True, out_t=(2, 1), seed=3)
    got = {}
    for mf in (0, 1):
        y_lin, tags = _in_fresh_context(_env(mf, DAT_CONV_LINEAR='1'), c.launch)
        y_2d, tags2 = _in_fresh_context(_env(mf, DAT_CONV_LINEAR='0'), c.launch)
        assert tags == tags2 and len(tags) == 1 and tags[0] in (_generic_tag(128), _generic_tag(256)), (tags, tags2)
        assert torch.equal(y_lin, y_2d), 'shape %d: linear strips and 2-D tiles differ' % mf
        got[mf] = c.check(y_lin, 'strips, shape %d' % mf)
    c.check_pair(got[0], got[1])


def test_roi_head_strips_across_map_borders_both_shapes(ops):
    """256 -> 512, 1x3x3 on 100 maps of 14 x 14: strips of consecutive positions that cross map borders (taps outside the lane's own map
    read the zero row), four channel chunks."""
    c = _Case(ops, 'roi_head_strips', N=100, T=1, H=14, W=14, Cin=256, Cout=512, kt=1, relu=True, seed=4)
    got = {}
    for mf in (0, 1):
        y, tags = _in_fresh_context(_env(mf), c.launch)
        assert len(tags) == 1 and tags[0] in (_generic_tag(128), _generic_tag(256)), tags
        got[mf] = c.check(y, 'shape %d' % mf)
    c.check_pair(got[0], got[1])


def test_big_tile_3x3_of_the_fp16_edges_both_shapes(ops):
    """(1, 3, 3), 64 -> 256, four frames of 120 x 256 (tests/test_gpu_fp16_edges.py SELECT['big_tile_3x3']) in whichever build is
    loaded: 8 x 32 tiles, one chunk."""
    c = _Case(ops, 'big_tile_3x3', N=1, T=4, H=120, W=256, Cin=64, Cout=256, kt=1, affine=True, seed=5)
    got = {}
    for mf in (0, 1):
        (y, tags), (y_gen, _) = _in_fresh_context(_env(mf, DAT_CONV_BT='2'), lambda: (c.launch(), c.launch((256, 1))))
        assert tags == [BT_TAG], 'shape %d: not the big-tile kernel: tags %r' % (mf, tags)
        assert torch.equal(y, y_gen)
        got[mf] = c.check(y, 'shape %d' % mf)
    c.check_pair(got[0], got[1])


def test_fp16_build_big_tile_both_shapes():
    """The same test in the IEEE-half build (libdat_hip_f16.so): the 16-bit format belongs to the loaded library, so it runs in one
    child process started with DAT_H16=fp16, as tests/test_gpu_fp16_suite.py runs the format-generic kernel tests."""
    env = dict(os.environ, DAT_H16='fp16', PYTHONPATH=REPO)
    env.pop('DAT_LIB', None)
    cmd = [sys.executable, '-m', 'pytest', '-m', 'gpu', '-q', '-s', '-p', 'no:cacheprovider',
           'tests/test_gpu_conv_mfma16.py::test_big_tile_3x3_of_the_fp16_edges_both_shapes']
    p = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors='replace')
    print(out[-2000:])
    assert p.returncode == 0 and '1 passed' in out and '(float16)' in out, 'the fp16 child failed (exit %d):\n%s' % (p.returncode, out[-4000:])
