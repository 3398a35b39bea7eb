"""Where a block of the unrolled-tap conv kernels spends its life: runs four benched 3x3 layers of the headline step (4 clips) on a
-DDAT_CONV_TRACE build of csrc/conv3d_igemm.hip, named by DAT_LIB.  That build stamps s_memtime at kernel entry, after the barrier that
publishes the first patch, after the last tap, after the last store is issued and after s_waitcnt vmcnt(0); the launcher synchronises
after every launch and prints the mean per block to stderr ('TRACE unrolled ...').  Each layer runs four times; profiles/persist/README.md
quotes the fourth.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -DDAT_CONV_TRACE -c conv3d_igemm.hip -o trace.o   # then link it in place of conv3d_igemm.o
    DAT_LIB=/path/to/trace/libdat_hip.so python tools/probes/conv_phase_probe.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from detectandtrack_amd.ops import hip_ops as ops  # noqa: E402

# name (tap-steps per block), Cin, Cout, kT, frames, T, H, W
SHAPES = [('res3_branch2b_54', 128, 128, 3, 32, 8, 96, 168), ('conv_fcn2-8_72', 512, 512, 1, 400, 1, 14, 14),
          ('fpn_res3_1_sum_108', 256, 256, 3, 32, 8, 96, 168), ('conv_fcn1_36', 256, 512, 1, 400, 1, 14, 14)]


def main():
    g = torch.Generator().manual_seed(1)
    for name, cin, cout, kt, frames, T, h, w in SHAPES:
        wt = (torch.randn((cout, cin, kt, 3, 3), generator=g) * (2.0 / (cin * 9 * kt)) ** 0.5).cuda()
        x = torch.randn((frames, h, w, cin), generator=g).to(ops.H16_DTYPE).cuda()
        layer = ops.ConvLayer(wt, torch.ones(cout).cuda(), torch.zeros(cout).cuda(), stride=(1, 1), pads=(kt // 2, 1, 1), relu=True, dtype=ops.BF16)
        for i in range(4):
            sys.stderr.write('LAYER %s rep %d\n' % (name, i))
            sys.stderr.flush()
            layer(x, T=T)
            torch.cuda.synchronize()
        del x, layer
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
