"""The launches do what dat_conv3d_plan says: for one small layer per kernel family and per variant of the generic kernel, the tag
dat_prof_read records for the real launch is the plan's, and a plan with ksplit > 1 goes through the split-K partials and
splitk_finish_kernel.  The smallest shapes the eligibility rules admit; DAT_CONV_BT=2 / DAT_CONV_TEMPORAL=2 where the default rule
needs a workload-sized grid.  Each knob setting runs in a child process of its own (the knobs are read when a context is made)."""
import json
import os
import subprocess
import sys

import pytest

from tests.conv_plan_cases import BIGTILE, GENERIC, PW256, PWKS, PWLW, REPO, TKS, WS64

pytestmark = pytest.mark.gpu

# name: (frames, T, H, W, cin, cout, kernel, stride, dilation), and what the plan must say: family, then (ntap, linear) of the generic kernel
CASES = {
    '': {
        'pwks': ((192, 1, 16, 16, 512, 256, (1, 1, 1), 1, 1), PWKS, None),            # 49 152 positions: 192 blocks on 256 CUs
        'pwlw': ((256, 1, 16, 16, 64, 128, (1, 1, 1), 1, 1), PWLW, None),             # 65 536 positions: 8 wave tiles per CU
        'pw256': ((2, 1, 4, 8, 64, 256, (1, 1, 1), 1, 1), PW256, None),               # 32 positions per frame
        'ws64': ((2, 1, 32, 32, 64, 64, (1, 3, 3), 1, 1), WS64, None),
        'generic_tap0': ((70, 1, 25, 40, 192, 128, (1, 1, 1), 1, 1), GENERIC, (0, 0)),  # a 1x1 of 70 000 positions
        'generic_tap1': ((2, 1, 25, 40, 192, 128, (1, 1, 1), 1, 1), GENERIC, (1, 0)),
        'generic_tap9': ((2, 1, 32, 32, 128, 128, (1, 3, 3), 1, 1), GENERIC, (9, 0)),
        'generic_tap10': ((2, 1, 32, 32, 128, 128, (1, 3, 3), 2, 1), GENERIC, (10, 0)),
        'generic_tap19': ((8, 1, 14, 14, 128, 128, (1, 3, 3), 1, 2), GENERIC, (19, 1)),
        'generic_strips': ((16, 1, 14, 14, 128, 128, (1, 3, 3), 1, 1), GENERIC, (9, 1)),
        'generic_splitk': ((8, 4, 12, 21, 512, 512, (3, 3, 3), 1, 1), GENERIC, (9, 1)),  # 2 clips of 4 frames
    },
    'DAT_CONV_BT=2': {'bigtile': ((6, 1, 128, 128, 64, 256, (1, 3, 3), 1, 1), BIGTILE, None)},      # 384 blocks = 1.5 per CU
    'DAT_CONV_TEMPORAL=2': {'tks': ((4, 4, 16, 16, 64, 256, (3, 1, 1), 1, 1), TKS, None)},
}


def _child(setting):
    """Runs the cases of one knob setting on the GPU; prints {name: [plan, recorded tags, output all written, scratch bytes]}."""
    import torch
    from detectandtrack_amd.ops import hip_ops as ops
    out = {}
    for name, ((frames, T, H, W, cin, cout, k, stride, dil), _, _) in CASES[setting].items():
        ops.drop_ctx()          # a fresh context per case: its scratch starts empty
        g = torch.Generator(device='cuda').manual_seed(cin + cout)
        w = torch.randn((cout, cin) + k, device='cuda', generator=g) * (2.0 / (cin * k[0] * k[1] * k[2])) ** 0.5
        layer = ops.ConvLayer(w, None, torch.zeros(cout, device='cuda'), stride=(stride, stride), pads=(k[0] // 2, k[1] // 2 * dil, k[2] // 2 * dil),
                              relu=True, dtype=ops.BF16, dilation=dil)
        x = torch.randn((frames, H, W, cin), device='cuda', generator=g).to(ops.tdtype(ops.BF16))
        plan = layer.plan(frames, T, H, W)
        ho, wo = layer.out_hw(H, W)
        y = torch.full((frames, ho, wo, layer.cstride), float('nan'), dtype=x.dtype, device='cuda')
        prof = ops.ConvProfiler(capacity=8)
        prof.start()
        layer(x, T=T, out=y)
        tags = [t for t, _, _ in prof.stop()]
        torch.cuda.synchronize()
        out[name] = [plan, tags, not bool(torch.isnan(y[..., :cout].float()).any()), ops.ws_info()[1], frames * ho * wo * cout * 4]
    print('PLANS ' + json.dumps(out))


@pytest.mark.parametrize('setting', list(CASES), ids=lambda s: s or 'default')
def test_launches_record_the_tag_of_their_plan(setting):
    env = {k: v for k, v in os.environ.items() if not k.startswith('DAT_CONV_')}
    if setting:
        env.update([setting.split('=')])
    code = 'import sys; sys.path.insert(0, %r); from tests.test_gpu_conv_plan import _child; _child(%r)' % (REPO, setting)
    p = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = p.stdout.decode(errors='replace')
    assert p.returncode == 0, text[-4000:]
    got = json.loads([l for l in text.splitlines() if l.startswith('PLANS ')][-1][6:])
    bf16_build = os.environ.get('DAT_H16', 'bf16') == 'bf16'
    for name, (_, family, variant) in CASES[setting].items():
        plan, tags, written, ws_bytes, out_f32_bytes = got[name]
        print(name, plan, tags)
        assert tags == [plan['tag']], (name, plan, tags)
        assert written, '%s: the launch left output elements unwritten' % name
        if family != TKS or bf16_build:         # (the fp16 build keeps kT x 1 x 1 layers on the generic kernel)
            assert plan['family'] == family, (name, plan)
        if variant is not None:
            assert (plan['ntap'], plan['linear']) == variant, (name, plan)
        if plan['family'] == GENERIC and plan['ksplit'] > 1:
            # the conv kernel of a split plan writes fp32 partials to the context's scratch only: y is splitk_finish_kernel's work
            assert ws_bytes >= plan['ksplit'] * out_f32_bytes, (name, plan, ws_bytes)
    if not setting:
        splits = [n for n in CASES[''] if got[n][0]['ksplit'] > 1]
        assert 'generic_splitk' in splits, splits
