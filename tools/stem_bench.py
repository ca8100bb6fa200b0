#!/usr/bin/env python
"""The two stem kernels alone (batch 64, 416x416): forward (fp32 output with fused statistics, as in training) and weight
gradient; algorithmic bytes = the 32-channel fp32 tensor written / read once plus the frames.  VD_STEM_MFMA=0: VALU forward.
Then the backward of the stem cell, fp32 and bf16 tensors: vd_bn_bwd_apply + vd_stem_wgrad against the fused vd_stem_wgrad_bn
(VD_STEM_BN_VEC=0 / 1: its one-element / 16-byte loads) and vd_bn_bwd_apply alone.
usage: python tools/stem_bench.py [batch] [size]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from viddet_amd import ops
from viddet_amd import lib as L

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
S = int(sys.argv[2]) if len(sys.argv) > 2 else 416
x = torch.randn(B, 3, S, S, device="cuda")
w = torch.randn(32, 3, 3, 3, device="cuda") * 0.2
wp = torch.zeros(32, 32, device="cuda")
ops.pack_weight_fwd(w, wp, 32)
out = torch.empty(B, S, S, 32, device="cuda")
nb = L.load().vd_stem_conv_blocks(B, S, S)
part = torch.empty(nb, 64, device="cuda")
dz = torch.randn(B, S, S, 32, device="cuda")
dwp = torch.empty(32, 32, device="cuda")
ws = torch.empty(max(16, L.load().vd_stem_wgrad_ws_bytes(B, S, S)), dtype=torch.uint8, device="cuda")


def timeit(fn, it=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it


gb = (B * S * S * 32 * 4 + B * 3 * S * S * 4) / 1e9
tf = timeit(lambda: ops.stem_conv(x, wp, out, stats_part=part))
tw = timeit(lambda: ops.stem_wgrad(x, dz, dwp, ws))
print("stem forward %.3f ms (%.2f TB/s)   stem weight gradient %.3f ms (%.2f TB/s)   [%.2f GB each]" % (tf, gb / tf, tw, gb / tw, gb))

# The backward of the stem cell behind dy, in one process: the two-launch pair (vd_bn_bwd_apply into dz, vd_stem_wgrad on it),
# the fused launch (vd_stem_wgrad_bn: dz computed from z and dy in the kernel) and vd_bn_bwd_apply alone, the streaming
# yardstick.  Bytes: pair = z + dy read, dz written and read back, frames; fused = z + dy, frames.  min of three blocks of 20.
for dt, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
    M_ = B * S * S
    z, dy, dzs = out.to(dt), dz.to(dt), torch.empty(B, S, S, 32, dtype=dt, device="cuda")
    sc, sh = torch.rand(32, device="cuda") + 0.5, torch.randn(32, device="cuda")
    mu, iv = torch.randn(32, device="cuda") * 0.3, torch.rand(32, device="cuda") + 0.5
    sums2 = torch.randn(64, dtype=torch.float64, device="cuda") * M_ * 0.1
    esz = z.element_size()
    t_bytes, f_bytes = M_ * 32 * esz / 1e9, B * 3 * S * S * 4 / 1e9

    def pair():
        ops.bn_bwd_apply(z, dy, sc, sh, mu, iv, sums2, float(M_), M_, 32, dzs)
        ops.stem_wgrad(x, dzs, dwp, ws)

    fused = lambda: ops.stem_wgrad_bn(x, z, dy, sc, sh, mu, iv, sums2, float(M_), dwp, ws)
    apply_ = lambda: ops.bn_bwd_apply(z, dy, sc, sh, mu, iv, sums2, float(M_), M_, 32, dzs)
    pair()
    ref = dwp.clone()
    fused()
    torch.cuda.synchronize()
    assert torch.equal(ref, dwp), "fused weight gradient differs from the two-launch pair"
    tp, tfu, ta = [min(timeit(f) for _ in range(3)) for f in (pair, fused, apply_)]
    print("stem backward %s: pair %.3f ms (%.2f TB/s of %.2f GB)   fused %.3f ms (%.2f TB/s of %.2f GB)   fused / pair %.3f   "
          "bn_bwd_apply alone %.3f ms (%.2f TB/s of %.2f GB)" %
          (name, tp, (4 * t_bytes + f_bytes) / tp, 4 * t_bytes + f_bytes, tfu, (2 * t_bytes + f_bytes) / tfu, 2 * t_bytes + f_bytes,
           tfu / tp, ta, 3 * t_bytes / ta, 3 * t_bytes))
