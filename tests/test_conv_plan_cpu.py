"""The launch plan of the dense conv forward (dat_conv3d_plan; csrc/conv3d_igemm.hip conv_plan), held to the rules the comments beside
it state -- on a machine without a GPU: the plan is a pure function of the knobs, the CU count and the descriptor.  Every case asks
with a NULL context and 256 compute units; a case that needs a knob asks a child process that has it in its environment."""
import pytest

from tests import conv_plan_cases as c
from tests.conv_plan_cases import BF16, BIGTILE, F32, GENERIC, PW256, PWKS, PWLW, TKS, WS64, X3, desc

SWEEP = c.sweep()


def ok_plan(d, num_cu=256):
    rc, p = c.plan(d, num_cu)
    assert rc == 0, (rc, d)
    return p


def test_fpn_p2_takes_the_big_tile_kernel_and_p3_the_generic_one():
    """FPN P2 output conv at 8 frames: 2 016 blocks of 16 x 16 positions x 256 channels = 7.9 even rounds of 256 CUs; P3's 528 blocks
    would run 3 rounds for 2.06 of work."""
    p2 = ok_plan(desc(8, 192, 336, 256, 256))
    assert (p2['family'], p2['blocks'], p2['twl'], p2['tag']) == (BIGTILE, 2016, 4, 2562561), p2
    p3 = ok_plan(desc(8, 96, 168, 256, 256))
    assert p3['family'] == GENERIC and p3['bn'] == 128 and p3['ntap'] == 9, p3


@pytest.mark.parametrize('R', [8, 32, 100])
def test_plan_frames_pins_the_split_factor_of_a_per_roi_blob(R):
    """with plan_frames = the rows of ONE image the split-K factor is the one that image gets alone, however many
    images share the blob -- on the frames of a 14 x 14 head conv and on the columns of the FC layers' [1, 1, n R, K] rows view."""
    conv1 = ok_plan(desc(R, 14, 14, 256, 256))
    fc1 = ok_plan(desc(1, 1, R, 12544, 1024, (1, 1, 1)))
    assert conv1['family'] == GENERIC and fc1['family'] == GENERIC
    for n in range(1, 9):
        p = ok_plan(desc(n * R, 14, 14, 256, 256, plan_frames=R))
        assert p['family'] == GENERIC and p['ksplit'] == conv1['ksplit'], (n, p, conv1)
        p = ok_plan(desc(1, 1, n * R, 12544, 1024, (1, 1, 1), plan_frames=R))
        assert p['family'] == GENERIC and p['ksplit'] == fc1['ksplit'], (n, p, fc1)
    # (the rule is not vacuous: without plan_frames the factor follows the grid)
    assert ok_plan(desc(8, 14, 14, 256, 256))['ksplit'] > ok_plan(desc(64, 14, 14, 256, 256))['ksplit'] >= 1


def test_masking_modes_keep_to_the_kernels_that_know_them():
    """res_mode 3 (mask) and 4 (sum + mask) live in the generic kernel and the lw / ks 1x1 kernels; plain mask layers stay off pwlw."""
    seen = set()
    layers = [desc(8, 192, 336, 256, 256), desc(8, 128, 160, 64, 256, (1, 1, 1)), desc(8, 128, 160, 64, 64),
              desc(4, 128, 160, 128, 512, (1, 1, 1)), desc(2, 96, 160, 2048, 512, (1, 1, 1))]
    assert [ok_plan(d)['family'] for d in layers] == [BIGTILE, PW256, WS64, PWLW, PWKS]
    for d in layers + SWEEP:
        for mode in (3, 4):
            if d['dtype'] == X3 and mode == 4:
                continue
            rc, p = c.plan(dict(d, res_mode=mode))
            if rc != 0:
                continue
            seen.add((mode, p['family']))
            assert p['family'] not in (BIGTILE, PW256, WS64), (mode, d, p)
            assert not (mode == 3 and p['family'] == PWLW), (d, p)
    assert {(3, PWKS), (4, PWKS), (4, PWLW), (3, GENERIC), (4, GENERIC)} <= seen, seen


@pytest.mark.parametrize('env', [{'DAT_CONV_BP': 128}, {'DAT_CONV_BP': 256}, {'DAT_CONV_KSPLIT': 2}, {'DAT_CONV_KSPLIT': 3}],
                         ids=lambda e: '%s=%d' % next(iter(e.items())))
def test_forced_plans_are_plans_of_the_generic_kernel(env):
    """DAT_CONV_BP / DAT_CONV_KSPLIT (dat_conv3d_tune_plan) force the generic kernel's tile and split-K factor.  The exceptions the model
    states: the 64-channel (Cout <= 64) and 1x1 variants have no 256-position tile, the factor never exceeds npatch_min, and a 1x1
    layer of fewer than 16 channel chunks is never split."""
    free = [c.plan(d) for d in SWEEP]
    forced = c.plans_in_child(SWEEP, env)
    n = 0
    for d, (rc0, _), (rc, p) in zip(SWEEP, free, forced):
        if rc0 != 0 and rc != 0:
            continue
        if rc != 0:
            continue                    # (a forced tile may not fit where the model's choice does)
        n += 1
        assert p['family'] == GENERIC, (d, p)
        pointwise = d['KH'] * d['KW'] == 1
        if 'DAT_CONV_BP' in env:
            want = 128 if env['DAT_CONV_BP'] == 256 and (d['Cout'] <= 64 or pointwise) else env['DAT_CONV_BP']
            assert p['bp'] == want, (d, p)
        else:
            chunks = p['npatch_min'] // (d['KT'] - 1 if d['KT'] > 1 else 1)
            want = 1 if pointwise and chunks < 16 else min(env['DAT_CONV_KSPLIT'], p['npatch_min'])
            assert p['ksplit'] == want, (d, p)
    assert n > len(SWEEP) // 2


def test_grid_rules_of_the_k_streaming_kernels_at_their_edges():
    """pwks and tks take grids of >= 3/4 block per CU (4 blocks >= 3 num_cu): one 256-position tile more or less, 256 or 304 CUs."""
    pw = lambda frames: desc(frames, 16, 16, 512, 256, (1, 1, 1))                 # one frame = one block
    tk = lambda frames: desc(frames, 16, 16, 256, 256, (3, 1, 1), T=4)
    for mk, fam in ((pw, PWKS), (tk, TKS)):
        assert ok_plan(mk(192))['family'] == fam and ok_plan(mk(192))['blocks'] == 192
        assert ok_plan(mk(188))['family'] != fam
        assert ok_plan(mk(192), 304)['family'] != fam
        assert ok_plan(mk(228), 304)['family'] == fam and ok_plan(mk(224), 304)['family'] != fam
    assert ok_plan(pw(191))['family'] != PWKS
    # DAT_CONV_TEMPORAL=2 drops the rule for tks (and only there)
    (_, t4), (_, t188), (_, p188) = c.plans_in_child([tk(4), tk(188), pw(188)], {'DAT_CONV_TEMPORAL': 2})
    assert t4['family'] == TKS and t188['family'] == TKS and p188['family'] != PWKS


def test_grid_rule_of_the_weights_in_lds_kernel_at_its_edge():
    """pwlw needs npos / 32 >= 8 num_cu / nsplit wave tiles (64 -> 128: one cout part; 256 -> 1024: four)."""
    lw = lambda frames, cin=64, cout=128: desc(frames, 16, 16, cin, cout, (1, 1, 1))
    assert ok_plan(lw(256))['family'] == PWLW and ok_plan(lw(255))['family'] == GENERIC
    assert ok_plan(lw(256), 304)['family'] == GENERIC and ok_plan(lw(304), 304)['family'] == PWLW and ok_plan(lw(303), 304)['family'] == GENERIC
    assert ok_plan(lw(64, 256, 1024))['family'] == PWLW and ok_plan(lw(63, 256, 1024))['family'] == GENERIC


def test_big_tile_grid_rules():
    """Default: >= 3.9 rounds of the CUs, evenly filled (95 %); DAT_CONV_BT=2: 2 blocks >= 3 num_cu.  64 -> 256 on 128 x 128: 64 tiles a frame."""
    bt = lambda frames: desc(frames, 128, 128, 64, 256)
    assert ok_plan(bt(6))['family'] == GENERIC
    assert ok_plan(bt(16))['family'] == BIGTILE and ok_plan(bt(16))['blocks'] == 1024       # 4.0 rounds
    assert ok_plan(bt(15))['family'] == GENERIC                                             # 3.75 rounds
    assert ok_plan(bt(17))['family'] == GENERIC                                             # 4.25 rounds: the fifth round a quarter full
    (_, b6), (_, b5), (_, b6_304) = c.plans_in_child([bt(6), bt(5)], {'DAT_CONV_BT': 2}) + c.plans_in_child([bt(6)], {'DAT_CONV_BT': 2}, 304)
    assert b6['family'] == BIGTILE and b6['blocks'] == 384 and b6['tag'] == 2562561
    assert b5['family'] == GENERIC and b6_304['family'] == GENERIC


def test_variant_rules_of_the_generic_kernel():
    for H, W in ((56, 56), (28, 28), (48, 84), (96, 168), (14, 14)):
        for cin, cout in ((128, 128), (256, 256), (512, 512)):
            p = ok_plan(desc(8, H, W, cin, cout, stride=2))
            assert (p['family'], p['bp'], p['ntap']) == (GENERIC, 128, 10), (H, W, p)     # one dense patch, 128-position tiles only
    for d in SWEEP:
        if d['KH'] == 3 and d['stride_h'] == 2:
            rc, p = c.plan(d)
            assert rc != 0 or (p['family'] == GENERIC and p['bp'] == 128), (d, p)
    p = ok_plan(desc(8, 14, 14, 256, 256, dil=2))
    assert (p['family'], p['ntap'], p['linear'], p['tag'] % 10) == (GENERIC, 19, 1, 6), p   # dilated strips; tag digit 5 + dtype
    p = ok_plan(desc(16, 14, 14, 256, 256))
    assert (p['ntap'], p['linear'], p['th_log2'], p['patch_h']) == (9, 1, 0, 1) and p['patch_w'] == p['bp'] + 2 * 15 + 1, p
    big = ok_plan(desc(70, 25, 40, 192, 128, (1, 1, 1)))                # 70 000 positions: the leaner table-driven loop
    small = ok_plan(desc(65, 25, 40, 192, 128, (1, 1, 1)))
    assert (big['family'], big['ntap'], small['family'], small['ntap']) == (GENERIC, 0, GENERIC, 1), (big, small)
    n = 0
    for rc, p in c.plans_in_child(SWEEP[:1500], {'DAT_CONV_NTAP': 0}):
        if rc == 0 and p['family'] == GENERIC:
            n += 1
            assert p['ntap'] == 0 and p['linear'] == 0 and p['mfma'] == 0, p
    assert n > 500


def test_every_plan_of_a_random_sweep_is_well_formed():
    n_ok, families = 0, set()
    for d in SWEEP:
        rc, p = c.plan(d)
        if rc != 0:
            continue
        n_ok += 1
        families.add(p['family'])
        assert 0 < p['blocks'] < 2 ** 31, (d, p)
        ho, wo = c.out_hw(d)
        oframes = d['frames'] // d['T'] * d['out_tn'] if d['out_tn'] > 0 else d['frames']
        dilated = d['KH'] > 1 and d['dil_h'] > 1
        if p['family'] != GENERIC:
            cpb, code = c.TAG_CODE[p['family']]
            assert p['tag'] == cpb * 10000 + code + d['dtype'] and d['dtype'] == BF16 and not dilated, (d, p)
            assert (p['twl'] in (4, 5)) == (p['family'] in (BIGTILE, WS64)), (d, p)
            continue
        chunks = d['Cin'] // 64 * 3 if d['dtype'] == X3 else d['Cin'] // (32 if d['dtype'] == F32 else 64)
        assert p['npatch_min'] == (d['KT'] - 1 if d['KT'] > 1 else 1) * chunks
        assert 1 <= p['ksplit'] <= p['npatch_min'], (d, p)
        assert p['bn'] == (64 if d['Cout'] <= 64 else 128) and p['bp'] in (128, 256) and 1 << (p['th_log2'] + p['tw_log2']) == p['bp'], (d, p)
        assert p['tag'] == p['bn'] * 10000 + p['bp'] * 10 + d['dtype'] + (5 if dilated else 0), (d, p)
        assert p['in_dtype'] == (F32 if d['dtype'] == F32 else BF16) and p['out_dtype'] == (BF16 if d['dtype'] == BF16 else F32)
        assert p['ntap'] in (0, 1, 9, 10, 19) and (p['ntap'] == 19) == bool(p['linear'] and dilated), (d, p)
        nbn = c.round_up(d['Cout'], p['bn']) // p['bn']
        assert p['blocks'] % (nbn * p['ksplit']) == 0
        tiles = p['blocks'] // (nbn * p['ksplit'])
        th, tw = 1 << p['th_log2'], 1 << p['tw_log2']
        dl = d['dil_h'] if dilated else 1
        if p['linear']:        # strips of bp consecutive positions: of the whole blob, or frame by frame where temporal taps differ
            per = ho * wo if d['KT'] > 1 else oframes * ho * wo
            assert tiles == (oframes if d['KT'] > 1 else 1) * -(-per // p['bp']), (d, p)
            assert p['patch_h'] == 1 and p['patch_w'] >= p['bp'] + 2 * dl * (wo + 1), (d, p)
        else:                  # the tile grid covers the map
            assert tiles == oframes * -(-ho // th) * -(-wo // tw), (d, p)
            if p['ntap'] == 10:
                need = ((th - 1) * d['stride_h'] + d['KH'], (tw - 1) * d['stride_w'] + d['KW'])
            else:
                need = (th + (d['KH'] - 1) * dl // d['stride_h'], tw + (d['KW'] - 1) * dl // d['stride_w'])
            assert (p['patch_h'], p['patch_w']) == need, (d, p)
        assert p['patch_h'] * p['patch_w'] * 128 <= 160 * 1024, (d, p)
    assert n_ok > len(SWEEP) // 2 and families >= {GENERIC, PWKS, PWLW, PW256, WS64}, (n_ok, families)


def test_the_plan_does_not_depend_on_earlier_calls():
    first = [c.plan(d) for d in SWEEP[:400]]
    assert [c.plan(d) for d in reversed(SWEEP[:400])] == first[::-1]
    assert c.plan(SWEEP[0], 304) == c.plan(SWEEP[0], 304)
    import ctypes as C
    from detectandtrack_amd import libdat
    out = libdat.ConvPlan()
    assert libdat.lib().dat_conv3d_plan(None, None, 256, C.byref(out)) != 0
    cd = libdat.ConvDesc()
    assert libdat.lib().dat_conv3d_plan(None, C.byref(cd), 0, C.byref(out)) != 0      # no context: the CU count must be given
