"""Times the headline step's largest 3x3 layers on the two kernels that know both MFMA shapes (conv3x3_bt_kernel, conv3d_igemm_kernel
<bf16,128,256 / 128,128, 9 taps>) under the context's DAT_CONV_MFMA value (0 = 32x32x16, 1 = 16x16x32; read when the context is created, so
one process per value), on random data: HIP-event time per launch, the shader clock the kernels' own clock stamps give under the conv
profiler (100 MHz x shader cycles / real-time ticks, summed over the blocks' first lanes), and their product, shader cycles per launch.
A higher clock at about equal cycles is what DESIGN.md section 3.1 expects of the 16x16x32 shape."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from detectandtrack_amd.ops import hip_ops as ops  # noqa: E402

# name, Cin, Cout, kT, frames (4 clips of 8), H, W
SHAPES = [('fpn_P2_output', 256, 256, 3, 32, 192, 336), ('conv_rpn_fpn2', 256, 256, 1, 32, 192, 336), ('fpn_P3_output', 256, 256, 3, 32, 96, 168),
          ('res3_branch2b', 128, 128, 3, 32, 96, 168), ('res4_branch2b', 256, 256, 3, 32, 48, 84)]


def main():
    g = torch.Generator().manual_seed(1)
    mf = os.environ.get('DAT_CONV_MFMA', 'default')
    for name, cin, cout, kt, frames, h, w in SHAPES:
        wt = (torch.randn((cout, cin, kt, 3, 3), generator=g) * (2.0 / (cin * 9 * kt)) ** 0.5).cuda()
        x = torch.randn((frames, h, w, cin), generator=g).to(ops.H16_DTYPE).cuda()
        layer = ops.ConvLayer(wt, torch.ones(cout).cuda(), torch.zeros(cout).cuda(), stride=(1, 1), pads=(kt // 2, 1, 1), relu=True, dtype=ops.BF16)
        for _ in range(3):
            layer(x, T=8)
        torch.cuda.synchronize()
        prof = ops.ConvProfiler(capacity=64)
        prof.start()
        for _ in range(10):
            layer(x, T=8)
        rec = prof.stop()
        ms = sum(m for _, _, m in rec) / len(rec)
        fl = rec[0][1]
        print('DAT_CONV_MFMA=%s %-14s %3d -> %3d kT %d %dx%d: tag %7d  %8.1f us  %6.0f TFLOP/s  shader clock %6.0f MHz  %7.0f k cycles'
              % (mf, name, cin, cout, kt, h, w, rec[0][0], ms * 1e3, fl / ms / 1e9, prof.shader_mhz, ms * prof.shader_mhz))
        del x, layer
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
