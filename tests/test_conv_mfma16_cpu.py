"""The two address maps the 16x16x32 MFMA shape (DAT_CONV_MFMA=1) adds to conv3x3_bt_kernel and to the generic kernel's bf16
128-channel dense 3x3 variants, restated in Python and checked without a device.

B operand: lane l of a `ds_read_b128` reads, for K32 slice s, logical 16-byte slot 4 s + (l >> 4) of patch row r0 + (l & 15), where
the patch keeps one 128-byte line per pixel and the LDS-DMA stores logical slot `phys ^ swz(row)` at physical slot `phys`
(csrc/conv_internal.h: patch_swz<1>, patch_src_slot<1>, patch_frag_addr<1>).  The LDS serves that instruction in four fixed groups of
16 lanes, one cycle each when the 16 x 4 dwords of a group fall into 64 different banks ((address / 4) mod 64).  The test enumerates
every read the kernels issue -- every tap, position group, K32 slice and patch buffer of a 16 x 16 tile, an 8 x 32 tile and a linear
strip -- and requires 64 distinct banks per group.  The swizzle of the 32x32x16 shape, (row >> 1) & 7, fails the same enumeration,
which is why the shape has its own.

A operand: the packed weights stay in the 32x32x16 fragment order (tests/dgrad_refs.pack_index); the 16x16x32 fragment of 16-row
block r16 and K32 slice s is a lane gather from two neighbouring 1-KiB fragments."""
import numpy as np
import pytest
import torch

from tests import dgrad_refs as dr

PPITCH = 128
# the lane groups of ds_read_b128 on gfx950, one LDS cycle each
GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
          [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
GROUPS += [[l + 32 for l in g] for g in GROUPS]


def swz16(row):
    """patch_swz<1>: 32-byte slot pairs move by (row >> 1) & 3"""
    return ((row >> 1) & 3) << 1


def swz32(row):
    """patch_swz<0>, the 32x32x16 kernels' swizzle"""
    return (row >> 1) & 7


def frag_addr(row, lane, s, buf_bytes, swz):
    """byte address of lane `lane`'s B fragment of K32 slice s: patch_frag_addr<1>(row, lane >> 4) ^ (s << 6), plus the buffer"""
    return buf_bytes + ((row * PPITCH + (((lane >> 4) ^ swz(row)) << 4)) ^ (s << 6))


def _banks(addr):
    return [(addr // 4 + d) % 64 for d in range(4)]


def _reads_2d(tw_log2):
    """first patch row of every (tap, 16-position group) read of a 256-position tile of 2^tw_log2 columns, and the patch size"""
    tw, th = 1 << tw_log2, 256 >> tw_log2
    pw, ph = tw + 2, th + 2
    rows = []
    for tap in range(9):
        for g in range(16):
            pos = g * 16
            r, c = pos >> tw_log2, pos & (tw - 1)
            rows.append((r + tap // 3) * pw + c + tap % 3)
    return rows, ph * pw


def _reads_linear(width):
    """a linear strip of 256 positions on maps `width` columns wide: position i reads patch row i + kh * width + kw"""
    rows = [g * 16 + (tap // 3) * width + tap % 3 for tap in range(9) for g in range(16)]
    return rows, 256 + 2 * (width + 1) + 1


def _patch_bytes(nrows):
    return (nrows * 8 + 63) // 64 * 1024          # whole 1-KiB LDS-DMA pieces


LAYOUTS = {'tile_16x16': _reads_2d(4), 'tile_8x32': _reads_2d(5), 'strip_w14': _reads_linear(14), 'strip_w42': _reads_linear(42),
           'strip_w85': _reads_linear(85)}


def _conflicts(rows, nrows, swz):
    """reads (first row, slice, buffer, group) whose 16 lanes do not touch 64 different banks"""
    bad = []
    for r0 in rows:
        for s in range(2):
            for buf in range(2):
                for gi, g in enumerate(GROUPS):
                    banks = set()
                    for l in g:
                        row = r0 + (l & 15)
                        assert row < nrows
                        banks.update(_banks(frag_addr(row, l, s, buf * _patch_bytes(nrows), swz)))
                    if len(banks) != 64:
                        bad.append((r0, s, buf, gi, len(banks)))
    return bad


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_b_fragment_reads_touch_64_banks_per_lane_group(layout):
    rows, nrows = LAYOUTS[layout]
    assert len(rows) == 9 * 16 and len(set(r % 8 for r in rows)) > 1
    bad = _conflicts(rows, nrows, swz16)
    assert not bad, '%s: %d reads with bank conflicts, e.g. (first row, slice, buffer, group, banks) %r' % (layout, len(bad), bad[:4])


def test_the_32x32x16_swizzle_is_not_conflict_free_for_this_read():
    """(row >> 1) & 7 serves 16 rows that start at a multiple of 16 -- and not every tap offset: the reason for patch_swz<1>"""
    rows, nrows = LAYOUTS['tile_16x16']
    bad = _conflicts(rows, nrows, swz32)
    assert bad and not _conflicts([0, 16, 32], nrows, swz32)


def test_every_first_row_is_conflict_free_and_the_dma_image_is_a_permutation():
    """any 16 consecutive rows (the tile shapes above do not reach every residue), and the source-side swizzle of the LDS-DMA: lane
    (row, phys) fetches logical slot phys ^ swz(row), so the read of logical slot L at phys = L ^ swz(row) finds it"""
    assert not _conflicts(list(range(64)), 64 + 16, swz16)
    for row in range(32):
        assert sorted(p ^ swz16(row) for p in range(8)) == list(range(8))
        for lane in range(64):
            for s in range(2):
                phys = ((frag_addr(row, lane, s, 0, swz16) - row * PPITCH) >> 4)
                assert 0 <= phys < 8 and phys ^ swz16(row) == 4 * s + (lane >> 4)


def a_gather_offset(r16, s, lane):
    """(old fragment: 32-row block, k-slice; byte offset inside it) of lane `lane`'s 16 bytes of the 16x16x32 A fragment (r16, s)"""
    kg = lane >> 4
    return r16 >> 1, 2 * s + (kg >> 1), 16 * (((r16 & 1) << 4) + (lane & 15) + 32 * (kg & 1))


def test_a_fragment_gather_from_the_packed_weights():
    """A[channel][k] for all 64 lanes, r16 in 0..7, s in 0..1, on an image packed in the existing fragment order: two taps, two
    64-channel chunks, 256 rows (the eight 16-row blocks of the second 128 channels are checked as well)."""
    ntap, cout_pad, cin = 2, 256, 128
    logical = torch.arange(ntap * cout_pad * cin, dtype=torch.int32).view(ntap, cout_pad, cin)       # value = its own logical index
    packed = dr.pack(logical, 'bf16').numpy()                                                        # (2-byte elements: 8 per lane)
    mb = cout_pad // 32
    for tap in range(ntap):
        for chunk in range(cin // 64):
            for base in (0, 4):                       # the wave's first 32-row block: channels 0-127 / 128-255
                for r16 in range(8):
                    for s in range(2):
                        for lane in range(64):
                            blk, ks, off = a_gather_offset(r16, s, lane)
                            frag = ((tap * (cin // 64) + chunk) * mb + base + blk) * 4 + ks
                            e0 = frag * 512 + off // 2
                            got = packed[e0:e0 + 8]
                            row = base * 32 + r16 * 16 + (lane & 15)
                            k0 = chunk * 64 + 32 * s + 8 * (lane >> 4)
                            want = logical[tap, row, k0:k0 + 8].numpy()
                            assert np.array_equal(got, want), (tap, chunk, base, r16, s, lane, got, want)
    # a load instruction (all 64 lanes of one fragment) reads four whole 256-byte runs
    for r16 in range(8):
        for s in range(2):
            offs = sorted(a_gather_offset(r16, s, l)[1] * 1024 + a_gather_offset(r16, s, l)[2] for l in range(64))
            runs = [offs[i:i + 16] for i in range(0, 64, 16)]
            assert all(r == list(range(r[0], r[0] + 256, 16)) and r[0] % 256 == 0 for r in runs), (r16, s)
