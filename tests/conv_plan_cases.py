"""Descriptors and helpers of the conv launch-plan tests (tests/test_conv_plan_cpu.py, tests/test_gpu_conv_plan.py).

dat_conv3d_plan answers without a GPU: with a NULL context it reads the DAT_CONV_* knobs from the environment, so a case that needs a
knob asks a child process that has it set (plans_in_child)."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, X3 = 0, 1, 2
GENERIC, BIGTILE, PW256, PWKS, TKS, PWLW, WS64 = range(7)
# the "positions" part of a special kernel's tag, and its channels per block
TAG_CODE = {BIGTILE: (256, 2560), PW256: (256, 320), PWKS: (256, 340), TKS: (256, 350), PWLW: (256, 330), WS64: (64, 9990)}
KNOBS = ('DAT_CONV_BP', 'DAT_CONV_KSPLIT', 'DAT_CONV_NTAP', 'DAT_CONV_LINEAR', 'DAT_CONV_BT', 'DAT_CONV_BT_MIN', 'DAT_CONV_WS64',
         'DAT_CONV_PWKS', 'DAT_CONV_PWLW', 'DAT_CONV_TEMPORAL', 'DAT_CONV_MFMA', 'DAT_PERSIST_PCT')


def round_up(v, m):
    return (v + m - 1) // m * m


def desc(frames, H, W, cin, cout, k=(1, 3, 3), stride=1, dtype=BF16, T=1, dil=1, res_mode=0, **over):
    """A dat_conv_desc as a dict: "same" pads, channel stride rounded up to 64 unless `over` says otherwise."""
    kt, kh, kw = k
    d = dict(dtype=dtype, frames=frames, T=T, H=H, W=W, Cin=cin, Cout=cout, out_cstride=round_up(cout, 64), KT=kt, KH=kh, KW=kw,
             stride_h=stride, stride_w=stride, pad_t=kt // 2, pad_h=kh // 2 * dil, pad_w=kw // 2 * dil, relu=1, res_mode=res_mode,
             out_t0=0, out_tn=0, in_t0=0, in_tn=0, plan_frames=0, dil_h=dil if kh > 1 else 0, dil_w=dil if kw > 1 else 0)
    d.update(over)
    return d


def out_hw(d):
    dl = d['dil_h'] if (d['KH'] > 1 or d['KW'] > 1) and d['dil_h'] > 1 else 1
    return ((d['H'] + 2 * d['pad_h'] - dl * (d['KH'] - 1) - 1) // d['stride_h'] + 1,
            (d['W'] + 2 * d['pad_w'] - dl * (d['KW'] - 1) - 1) // d['stride_w'] + 1)


def plan(d, num_cu=256):
    """(return code, plan dict) of dat_conv3d_plan(NULL, d, num_cu) in this process: the environment's knobs."""
    from detectandtrack_amd import libdat
    cd, out = libdat.ConvDesc(), libdat.ConvPlan()
    for name, v in d.items():
        setattr(cd, name, int(v))
    rc = libdat.lib().dat_conv3d_plan(None, C.byref(cd), int(num_cu), C.byref(out))
    return rc, out.as_dict()


def plans_in_child(descs, env, num_cu=256):
    """[(return code, plan dict)] of `descs` from a child process whose environment has `env` (knob name -> value) set."""
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update({k: str(v) for k, v in env.items()})
    p = subprocess.run([sys.executable, '-c', 'from tests import conv_plan_cases as c; c.child_main()'], cwd=REPO, env=e,
                       input=json.dumps({'num_cu': num_cu, 'descs': descs}).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return [tuple(r) for r in json.loads(p.stdout.decode())]


def child_main():
    job = json.loads(sys.stdin.read())
    sys.stdout.write(json.dumps([plan(d, job['num_cu']) for d in job['descs']]))


def sweep(n=3000, seed=20240607):
    """Seeded random descriptors within the ranges conv3d_fwd validates: fp32, bf16 and bf16x3, frame windows, strides 1 and 2,
    dilation, Cout from 4 to 1 024, maps from 1 x 1 to 96 x 168, every res_mode, per-RoI blobs."""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        k = rnd.choice([(1, 1, 1), (1, 3, 3), (1, 3, 3), (3, 1, 1), (3, 3, 3)])
        T = rnd.choice([1, 1, 2, 4])
        clips = rnd.choice([1, 1, 2, 3, 8, 16, 100])
        stride = rnd.choice([1, 1, 2])
        dil = rnd.choice([1, 1, 1, 2, 4]) if (k[1] == 3 and stride == 1) else 1
        H, W = rnd.choice([(1, 1), (7, 7), (14, 14), (12, 21), (24, 42), (33, 57), (48, 84), (96, 168),
                           (rnd.randint(1, 96), rnd.randint(1, 168))])
        cout = rnd.choice([4, 36, 64, 68, 128, 200, 256, 512, 1024, 4 * rnd.randint(1, 256)])
        d = desc(clips * T, H, W, 64 * rnd.choice([1, 1, 2, 3, 4, 8, 16]), cout, k, stride, rnd.choice([F32, BF16, BF16, X3]), T, dil,
                 rnd.choice([0, 0, 1, 2, 3, 4]))
        if rnd.random() < 0.2:
            d['out_cstride'] = cout                      # an unpadded channel stride
        if T > 1 and rnd.random() < 0.3:
            d['out_t0'], d['out_tn'] = T // 2, 1         # the key frame only
        if T > 1 and rnd.random() < 0.2:
            d['in_t0'], d['in_tn'] = T // 2, 1
        if clips > 1 and rnd.random() < 0.3:
            d['plan_frames'] = T * rnd.choice([1, clips // 2 or 1])
        out.append(d)
    return out
