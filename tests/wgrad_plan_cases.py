"""The launch plan of the dense weight gradient, stated independently of csrc/train_ops.hip wgrad_plan, and the helpers of its tests
(tests/test_wgrad_plan_cpu.py, tests/test_gpu_wgrad.py).

`expect` restates what the launcher did with a layer BEFORE it became wgrad_validate / wgrad_plan / wgrad_launch (the one-function
wgrad_impl, pw_plan and dat_conv3d_wgrad_acc_batch): the family chain with the one-column refusal and the column_strip relabelling, the
pointwise tile choice, the four K-split rules and the batched one.  It is the yardstick the library's plan is held to, so it changes only
when a change MEANS to move a launch -- never to follow the library.

dat_conv3d_wgrad_plan answers without a GPU: with a NULL context it reads the DAT_WGRAD_* knobs from the environment, so a case that
needs a knob asks a child process that has it set (plans_in_child)."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
REPACK, NINE_TAP, POINTWISE, DIRECT = range(4)
KNOBS = {'DAT_WGRAD_DIRECT': 1, 'DAT_WGRAD_PW': 1, 'DAT_WGRAD_SUB': 2, 'DAT_WGRAD_KS': 0}       # name -> default


def round_up(v, m):
    return (v + m - 1) // m * m


def cdiv(a, b):
    return (a + b - 1) // b


def layer(cin, cout, k, stride, N, T, H, W, win=None, dtype=BF16, dil=1, cs_x=None, cs_g=None):
    """A weight-gradient call as hip_ops.ConvGrad makes it: the forward descriptor (Cin = the channel stride of x, "same" pads, the
    gradient's frame window when there is one clip) plus g_cstride and the real channel counts.  Channel strides: multiples of 64 unless given."""
    cs_x, cs_g = cs_x or round_up(cin, 64), cs_g or round_up(cout, 64)
    d = dict(dtype=dtype, frames=N * T, T=T, H=H, W=W, Cin=cs_x, Cout=round_up(cout, 4), out_cstride=cs_g, KT=k[0], KH=k[1], KW=k[2],
             stride_h=stride, stride_w=stride, pad_t=k[0] // 2, pad_h=k[1] // 2 * dil, pad_w=k[2] // 2 * dil, relu=0, res_mode=0,
             out_t0=0, out_tn=0, in_t0=0, in_tn=0, plan_frames=0, dil_h=dil if dil > 1 else 0, dil_w=dil if dil > 1 else 0)
    if win is not None and N == 1:
        d['out_t0'], d['out_tn'] = win
    return dict(d=d, g_cstride=cs_g, cin=cin, cout=cout)


def from_case(case, dtype=BF16):
    """A case of tests/test_gpu_wgrad.py: cin, cout, (kt, kh, kw), stride, N, T, H, W, window."""
    cin, cout, k, st, N, T, H, W, win = case
    return layer(cin, cout, tuple(k), st, N, T, H, W, win, dtype)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def dilation(d):
    return d['dil_h'] if (d['KH'] > 1 or d['KW'] > 1) and d['dil_h'] > 1 else 1


def out_hw(d):
    dl = dilation(d)
    return ((d['H'] + 2 * d['pad_h'] - dl * (d['KH'] - 1) - 1) // d['stride_h'] + 1,
            (d['W'] + 2 * d['pad_w'] - dl * (d['KW'] - 1) - 1) // d['stride_w'] + 1)


def windowed(d):
    return d['out_tn'] > 0 and d['frames'] // d['T'] == 1


def frame_range(d):
    """The frames that carry a gradient: the window of a single clip, every frame otherwise."""
    return (d['out_t0'], d['out_t0'] + d['out_tn']) if windowed(d) else (0, d['frames'])


def nine_tap_shape(d, knobs):
    return (d['KH'] == 3 and d['KW'] == 3 and d['stride_h'] == 1 and d['pad_h'] == 1 and d['pad_w'] == 1 and not knobs['DAT_WGRAD_DIRECT'] & 2
            and dilation(d) == 1)


def pointwise_shape(d, knobs):
    return (d['KT'], d['KH'], d['KW'], d['pad_t'], d['pad_h'], d['pad_w']) == (1, 1, 1, 0, 0, 0) and knobs['DAT_WGRAD_PW'] != 0


def one_column_refusal(d, knobs):
    """Spatial taps on an output map of one column and several rows: no direct kernel splits its positions (the nine-tap kernel has no split)."""
    Ho, Wo = out_hw(d)
    no_spatial_taps = d['KH'] == 1 and d['KW'] == 1 and d['pad_h'] == 0 and d['pad_w'] == 0
    return Wo == 1 and Ho > 1 and not nine_tap_shape(d, knobs) and not no_spatial_taps


def direct_eligible(L, knobs):
    d = L['d']
    Ho, Wo = out_hw(d)
    if one_column_refusal(d, knobs):
        return False
    split_range = Ho * Ho if Wo == 1 else Ho * Wo * Wo
    return (d['dtype'] == BF16 and knobs['DAT_WGRAD_DIRECT'] != 0 and d['Cin'] % 64 == 0 and L['g_cstride'] % 64 == 0 and
            d['frames'] * Ho * Wo < 2 ** 31 and d['frames'] * d['H'] * d['W'] < 2 ** 31 and split_range < 2 ** 32)


def nine_tap_plan(tiles, nchunks, sub=2, forced_ks=0, acc=False):
    """(SUB of the launched wgrad_dma9_kernel, K ranges, atomics) for a 3 x 3 stride-1 layer of `tiles` blocks per range and `nchunks` patches."""
    ks = cdiv(384, tiles) if tiles <= 96 else cdiv(768, tiles)
    if sub == 2:
        ks = 2 * (256 // tiles) if tiles <= 128 else 2
    ks = min(ks, nchunks // 4)
    if forced_ks > 0:
        ks = forced_ks
    ks = min(ks, nchunks)
    if sub == 2:
        ks &= ~1
    sub2 = sub == 2 and ks >= 2
    ks = max(ks, 1)
    return (2 if sub2 else 1), ks, bool(ks > (2 if sub2 else 1) or acc)


def pointwise_tile(L, knobs):
    """wm of the (128 wm) x (64 * 8 / wm) tile: least padded work, then least traffic, in the order 2, 1, 4; DAT_WGRAD_PW = 10 / 20 / 40 forces it."""
    if knobs['DAT_WGRAD_PW'] >= 10:
        return knobs['DAT_WGRAD_PW'] // 10
    best = None
    for wm in (2, 1, 4):
        tm, tn = 128 * wm, 64 * (8 // wm)
        nco, nci = cdiv(L['cout'], tm), cdiv(L['cin'], tn)
        key = (nco * tm * nci * tn, L['g_cstride'] * nci + L['d']['Cin'] * nco)
        if best is None or key < best[0]:
            best = (key, wm)
    return best[1]


def pointwise_ksplit(tiles, nchunks, num_cu, forced_ks=0):
    """One block per CU, at least 4 chunks of 32 positions per block; a forced value is clamped to the chunk count."""
    ks = 1 if tiles >= num_cu else num_cu // tiles
    ks = min(ks, nchunks // 4)
    if forced_ks > 0:
        ks = forced_ks
    return max(1, min(ks, nchunks))


def batched_ksplits(tiles_and_chunks, num_cu, forced_ks=0):
    """dat_conv3d_wgrad_acc_batch: the K ranges of every pointwise layer [(tiles, nchunks)] on the shared grids -- chunks per block from ~2
    blocks per CU over all layers (one per CU for a single layer), at least 4."""
    total = sum(t * c for t, c in tiles_and_chunks)
    target = (1 if len(tiles_and_chunks) == 1 else 2) * num_cu
    cpb = max(cdiv(total, target), 4)
    return [max(1, min(forced_ks if forced_ks > 0 else cdiv(c, cpb), c)) for _, c in tiles_and_chunks]


def streamed_ksplit(tiles, nchunks, min_chunks):
    """wgrad_direct_kernel (chunks of 64 positions, at least 8 per block) and wgrad_gemm_kernel (K-steps, at least 16): 1024 / tiles.  No forced value."""
    return max(1, min(1024 // tiles, nchunks // min_chunks))


def repack_geometry(d):
    """(padded frame rows, columns, all padded positions, shifted copies) of the re-packed position grid."""
    Ho, Wo = out_hw(d)
    s, dl = d['stride_h'], dilation(d)
    Hq, Wq = Ho + (d['KH'] - 1) * dl // s, Wo + (d['KW'] - 1) * dl // s
    Wq += Wq & 1
    copies = 2 if d['dtype'] == BF16 and (d['KW'] - 1) // s >= 1 else 1
    return Hq, Wq, d['frames'] // d['T'] * (d['T'] + d['KT'] - 1) * Hq * Wq, copies


def expect(L, env=None, num_cu=256, acc=False):
    """The plan of a layer the launcher accepts, as a dict of dat_wgrad_plan's fields (env: DAT_WGRAD_* name -> value)."""
    knobs = dict(KNOBS)
    knobs.update({k: int(v) for k, v in (env or {}).items()})
    d = L['d']
    Ho, Wo = out_hw(d)
    f0, f1 = frame_range(d)
    taps = d['KT'] * d['KH'] * d['KW']
    p = dict(taps=taps, ncopies=0, npack=0, strip=0, lds_bytes=0, threads=256)
    per_block = 1
    if not direct_eligible(L, knobs):
        ck = 64 if d['dtype'] == BF16 else 32
        Hq, Wq, Qtot, copies = repack_geometry(d)
        begin, end = 0, round_up(Qtot, ck)
        if windowed(d):      # whole K-steps around the window's padded positions (also when the window is the whole clip)
            begin, end = f0 * Hq * Wq // ck * ck, min(round_up(f1 * Hq * Wq, ck), end)
        p.update(family=REPACK, variant=d['dtype'], ncopies=copies, npack=1 + d['stride_h'] ** 2 * copies, tile_co=128, tile_ci=128,
                 r_begin=begin, r_end=end, nchunks=(end - begin) // ck)
        tiles = taps * cdiv(L['cout'], 128) * cdiv(L['cin'], 128)
        ks = streamed_ksplit(tiles, p['nchunks'], 16)
    elif nine_tap_shape(d, knobs):
        tiles = d['KT'] * cdiv(L['cout'], 64) * cdiv(L['cin'], 64)
        nchunks = (f1 - f0) * cdiv(d['H'], 8) * cdiv(d['W'], 8)
        per_block, ks, _ = nine_tap_plan(tiles, nchunks, 2 if knobs['DAT_WGRAD_SUB'] >= 2 else 1, knobs['DAT_WGRAD_KS'])
        p.update(family=NINE_TAP, variant=per_block, tile_co=64, tile_ci=64, r_begin=f0, r_end=f1, nchunks=nchunks,
                 threads=256 * per_block, lds_bytes=per_block * 3 * 192 * 128)
    else:
        p.update(strip=int(Wo == 1 and Ho > 1), r_begin=f0 * Ho * Wo, r_end=f1 * Ho * Wo)
        if pointwise_shape(d, knobs):
            wm = pointwise_tile(L, knobs)
            p.update(family=POINTWISE, variant=wm, tile_co=128 * wm, tile_ci=64 * (8 // wm), nchunks=cdiv(p['r_end'] - p['r_begin'], 32),
                     threads=512, lds_bytes=3 * (8 if wm == 2 else 10) * 32 * 128)
            tiles = cdiv(L['cout'], p['tile_co']) * cdiv(L['cin'], p['tile_ci'])
            ks = pointwise_ksplit(tiles, p['nchunks'], num_cu, knobs['DAT_WGRAD_KS'])
        else:
            p.update(family=DIRECT, variant=0, tile_co=128, tile_ci=128, nchunks=cdiv(p['r_end'] - p['r_begin'], 64), lds_bytes=4 * 64 * 320)
            tiles = taps * cdiv(L['cout'], 128) * cdiv(L['cin'], 128)
            ks = streamed_ksplit(tiles, p['nchunks'], 8)
    atomic = ks > per_block or acc
    p.update(n_co_tiles=cdiv(L['cout'], p['tile_co']), n_ci_tiles=cdiv(L['cin'], p['tile_ci']), tiles=tiles, ksplit=ks, atomic=int(atomic),
             memset_first=int(atomic and not acc), finish=int(not acc), blocks=tiles * ks // per_block)
    return p


# ---- the library's answer ------------------------------------------------------------------------------------------------------------
def plan(L, acc=False, num_cu=256):
    """(return code, plan dict) of dat_conv3d_wgrad_plan(NULL, ...) in this process: the environment's knobs."""
    from detectandtrack_amd import libdat
    cd, out = libdat.ConvDesc(), libdat.WgradPlan()
    for name, v in L['d'].items():
        setattr(cd, name, int(v))
    rc = libdat.lib().dat_conv3d_wgrad_plan(None, C.byref(cd), L['g_cstride'], L['cin'], L['cout'], int(acc), int(num_cu), C.byref(out))
    return rc, out.as_dict()


def acc_supported(L):
    """dat_conv3d_wgrad_acc_supported without a context: the environment's knobs."""
    from detectandtrack_amd import libdat
    cd = libdat.ConvDesc()
    for name, v in L['d'].items():
        setattr(cd, name, int(v))
    return bool(libdat.lib().dat_conv3d_wgrad_acc_supported(None, C.byref(cd), L['g_cstride']))


def plans_in_child(layers, env, num_cu=256, acc=False):
    """[(return code, plan dict)] of `layers` from a child process whose environment has `env` (knob name -> value) set."""
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update({k: str(v) for k, v in env.items()})
    p = subprocess.run([sys.executable, '-c', 'from tests import wgrad_plan_cases as c; c.child_main()'], cwd=REPO, env=e,
                       input=json.dumps({'num_cu': num_cu, 'acc': acc, 'layers': layers}).encode(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return [tuple(r) for r in json.loads(p.stdout.decode())]


def child_main():
    job = json.loads(sys.stdin.read())
    sys.stdout.write(json.dumps([plan(L, job['acc'], job['num_cu']) for L in job['layers']]))


def sweep(n=1500, seed=20240611):
    """Seeded random layers within what wgrad_validate accepts: fp32 and 16-bit, strides 1 and 2, kernels 1 x 1 x 1, 1 x 3 x 3, 3 x 1 x 1 and
    3 x 3 x 3, dilation 2 and 4 at stride 1, frame windows, several clips, maps from 1 x 1 up (one-column and one-row maps among them),
    ragged channel counts on strides padded to 64 or only to 8."""
    rnd = random.Random(seed)
    out = []
    chans = [8, 12, 64, 70, 128, 130, 200, 256, 512, 1024, 2048]
    for _ in range(n):
        k = rnd.choice([(1, 1, 1), (1, 3, 3), (3, 1, 1), (3, 3, 3)])
        stride = rnd.choice([1, 1, 2])
        dil = rnd.choice([1, 1, 2, 4]) if (k[1] == 3 and stride == 1) else 1
        T = rnd.choice([1, 2, 3, 4, 8])
        N = rnd.choice([1, 1, 1, 2, 3])
        H, W = rnd.choice([(1, 1), (1, rnd.randint(2, 40)), (rnd.randint(2, 40), 1), (rnd.randint(2, 12), 2), (2, 2), (7, 7), (9, 17), (13, 19),
                           (24, 42), (48, 84), (96, 168), (rnd.randint(1, 60), rnd.randint(1, 60))])
        cin, cout = rnd.choice(chans), rnd.choice(chans + [4, 15])
        win = (rnd.randrange(T), 1) if T > 1 and rnd.random() < 0.35 else None
        if win is not None and rnd.random() < 0.5:
            win = (win[0], rnd.randint(1, T - win[0]))
        pad = 8 if rnd.random() < 0.15 else 64
        out.append(layer(cin, cout, k, stride, N, T, H, W, win, rnd.choice([F32, BF16, BF16, BF16]), dil, round_up(cin, pad), round_up(cout, pad)))
    return out
