"""The temporal-tap K-streaming kernel (conv_kt1x1_ks_kernel) on every distinct kT x 1 x 1 layer of R-18- / R-50-(2+1)D at 8 x 768 x 1344
(1 and 4 clips) next to the old dispatch, then the R-18-(2+1)D FPN3D bf16 forward against the I3D R-18 FPN3D forward (bench.py's default
leg: 4 clips per forward, 3 forwards in flight, each replayed as a captured graph) on the same box.

    python tools/probes/temporal_probe.py [layers | model]      (both by default)

The context reads DAT_CONV_TEMPORAL when it is created, so each side runs in a fresh child process of its own: layers under
DAT_CONV_TEMPORAL=2 (the kernel on every supported shape, whatever the dispatcher's grid rule) and =0; the model legs under the default (1)
and =0."""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

# stage, Cin (mid planes M), Cout, H, W at 768 x 1344 (res3 1/8, res4 1/16, res5 1/32); R-50-(2+1)D's layers are among R-18's
SHAPES = [('res3_2a', 230, 128, 96, 168), ('res3_2b', 288, 128, 96, 168), ('res4_2a', 460, 256, 48, 84), ('res4_2b', 576, 256, 48, 84),
          ('res5_2a', 921, 512, 24, 42), ('res5_2b', 1152, 512, 24, 42)]
TEMPORAL_TAGS = (1280351, 2560351)


def _timed(fn, iters=30):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def layers_child(rounds=5):
    """Per shape: `rounds` interleaved rounds of the default dispatch and of the forced plan (128 positions, no split-K: the plan the
    old dispatch picks for every layer of SHAPES, whose K per tap is < 16 chunks), each round the mean of 30 back-to-back launches."""
    import torch
    from detectandtrack_amd.ops import hip_ops as ops
    g = torch.Generator().manual_seed(1)
    out = []
    for name, cin, cout, h, w in SHAPES:
        for clips in (1, 4):
            frames = 8 * clips
            wt = (torch.randn((cout, cin, 3, 1, 1), generator=g) * (2.0 / (3 * cin)) ** 0.5).cuda()
            layer = ops.ConvLayer(wt, torch.ones(cout).cuda(), torch.zeros(cout).cuda(), pads=(1, 0, 0), relu=True, dtype=ops.BF16)
            x = torch.zeros((frames, h, w, layer.cin), dtype=ops.H16_DTYPE, device='cuda')
            x[..., :cin] = torch.randn((frames, h, w, cin), generator=g).to(ops.H16_DTYPE).cuda()
            res = torch.randn((frames, h, w, layer.cstride), generator=g).to(ops.H16_DTYPE).cuda()
            tags, t_new, t_gen = [], [], []
            for forced in (False, True):
                ops.tune_plan(128 if forced else 0, 1 if forced else 0)
                prof = ops.ConvProfiler(capacity=4)
                prof.start()
                layer(x, T=8, residual=res)
                tags.append(prof.stop()[0][0])
            for _ in range(rounds):
                ops.tune_plan(0, 0)
                t_new.append(_timed(lambda: layer(x, T=8, residual=res)))
                ops.tune_plan(128, 1)
                t_gen.append(_timed(lambda: layer(x, T=8, residual=res)))
            ops.tune_plan(0, 0)
            fl = layer.flops(frames, h, w)
            med = lambda v: sorted(v)[len(v) // 2]
            out.append(dict(name=name, cin=cin, cout=cout, clips=clips, us=med(t_new), us_min=min(t_new), gen_us=med(t_gen),
                            gen_us_min=min(t_gen), tag=tags[0], gen_tag=tags[1], tflops=fl / med(t_new) / 1e6,
                            gen_tflops=fl / med(t_gen) / 1e6))
    print('RESULT ' + json.dumps(out))


def model_child(body, seconds=20.0):
    import numpy as np
    import torch
    import bench
    from detectandtrack_amd.core.config import cfg, cfg_from_cfg, assert_and_infer_cfg, reset_cfg
    from detectandtrack_amd.core.pipeline import ClipPipeline
    from detectandtrack_amd.modeling import model_builder
    from detectandtrack_amd.utils import net as net_utils
    from detectandtrack_amd import workspace
    T, H, W, B, depth = 8, 768, 1344, 4, 3
    c = bench.model_cfg('18', T, 'bf16')
    c['MODEL']['CONV_BODY'] = body
    reset_cfg()                      # bench.build with CONV_BODY swapped
    cfg_from_cfg(c)
    assert_and_infer_cfg()
    model = model_builder.create(cfg.MODEL.TYPE, train=False)
    workspace.ResetWorkspace()
    ws = workspace.GlobalWorkspace()
    for k, v in net_utils.synthetic_params(model, cfg.RNG_SEED).items():
        ws.set_param(k, v)
    ws.CreateNet(model.net)
    ws.CreateNet(model.keypoint_net)
    clips = [torch.cat([bench.synthetic_clip(T, H, W, 10 * i + f) for f in range(B)]).contiguous().cuda() for i in range(2)]
    im_scale = min(800.0 / 720, 1333.0 / 1280)
    im_info = np.tile(np.array([[H, W, im_scale]], dtype=np.float32), (B, 1))
    im_shape = (720, 1280, 3)
    pipe = ClipPipeline(model, ws, depth, graph=1, keep_results=False)
    for i in range(2):               # capture one graph per (slot, input buffer), as bench.py primes them
        for _ in range(len(pipe.slots)):
            pipe.submit(clips[i], im_info, im_shape, resident=True)
        pipe.drain()
    for i in range(6):
        pipe.submit(clips[i % 2], im_info, im_shape, resident=True)
    pipe.drain()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for i in range(10):
            pipe.submit(clips[i % 2], im_info, im_shape, resident=True)
        pipe.drain()
        n += 10
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    print('RESULT ' + json.dumps(dict(body=body, clips_per_s=n * B / el, forwards=n, seconds=el,
                                      temporal_env=os.environ.get('DAT_CONV_TEMPORAL', '1'))))


def _child(args, env_temporal, timeout):
    env = dict(os.environ, DAT_CONV_TEMPORAL=str(env_temporal))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, cwd=REPO, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=timeout)
    txt = p.stdout.decode(errors='replace')
    if p.returncode != 0:
        raise SystemExit('child %r (DAT_CONV_TEMPORAL=%s) exited %d:\n%s' % (args, env_temporal, p.returncode, txt[-3000:]))
    return json.loads([l for l in txt.splitlines() if l.startswith('RESULT ')][-1][7:])


def main(which):
    if which in ('layers', 'all'):
        new, old = _child(['--layers-child'], 2, 900), _child(['--layers-child'], 0, 900)
        print('median (min) of 5 interleaved rounds; "generic" = the forced plan in the same process, "old" = the default dispatch of a '
              'DAT_CONV_TEMPORAL=0 process')
        print('%-8s %5s %5s %5s | %15s %8s | %15s %8s | %9s | %6s  %s' % ('layer', 'Cin', 'Cout', 'clips', 'new us', 'TFLOP/s',
                                                                         'generic us', 'TFLOP/s', 'old us', 'speed', 'tags'))
        for a, b in zip(new, old):
            print('%-8s %5d %5d %5d | %7.1f (%5.1f) %8.0f | %7.1f (%5.1f) %8.0f | %9.1f | %5.2fx  %d / %d / %d' % (
                a['name'], a['cin'], a['cout'], a['clips'], a['us'], a['us_min'], a['tflops'], a['gen_us'], a['gen_us_min'],
                a['gen_tflops'], b['us'], a['gen_us'] / a['us'], a['tag'], a['gen_tag'], b['tag']))
    if which in ('model', 'all'):
        legs = [('FPN3D.add_fpn_ResNet18_conv5_body', 1), ('FPN3D.add_fpn_ResNet18_2plus1d_conv5_body', 1),
                ('FPN3D.add_fpn_ResNet18_2plus1d_conv5_body', 0)]
        rows = [_child(['--model-child', body], env, 600) for _ in range(2) for body, env in legs]   # two alternating passes
        for r in rows:
            print('%-45s DAT_CONV_TEMPORAL=%s  %7.2f clips/s  (%d forwards of 4 clips in %.1f s)' % (
                r['body'], r['temporal_env'], r['clips_per_s'], r['forwards'], r['seconds']))


if __name__ == '__main__':
    if '--layers-child' in sys.argv:
        layers_child()
    elif '--model-child' in sys.argv:
        model_child(sys.argv[sys.argv.index('--model-child') + 1])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else 'all')
