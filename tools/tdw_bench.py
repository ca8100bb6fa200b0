"""Times the temporal-conv kernels (vd_tdw.hip) alone on the row shapes of the (2+1)-D backbone, and one BatchNorm apply /
backward-apply launch on the same rows in the same session as the yardstick: all four are pure streams.

    python tools/tdw_bench.py [--batch 16] [--k 3] [--size 416] [--reps 20] [--out profiles/tdw_bench.json]

Reports achieved TB/s on ideal bytes: forward 2 tensors (3 with the residual), backward 3 (dy, x, dx); the BatchNorm apply 2,
its backward-apply 3."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viddet_amd import lib as L      # noqa: E402
from viddet_amd import ops           # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _ in range(3):                                   # three blocks of `reps` launches: the spread is the run-to-run figure
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        best.append(e0.elapsed_time(e1) / reps * 1e-3)
    return min(best), max(best)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    lib = L.load()
    B, K = a.batch, a.k
    rows = []
    # (channels, divisor) of the stem, then of the five stages of Darknet3D
    for C_, div in ((32, 1), (64, 2), (128, 4), (256, 8), (512, 16), (1024, 32)):
        hw = (a.size // div) ** 2
        M = B * K * hw
        x = torch.randn(M, C_, device='cuda')
        res, y, dy, dx = torch.randn_like(x), torch.empty_like(x), torch.randn_like(x), torch.empty_like(x)
        w, dw = torch.randn(3 * C_, device='cuda'), torch.empty(3 * C_, device='cuda')
        ws = torch.empty(ops.tdw_bwd_ws_bytes(B, K, hw, C_), dtype=torch.uint8, device='cuda')
        am = torch.zeros(L.AMAX_FLOATS, device='cuda')
        sc, sh = torch.rand(C_, device='cuda') + 0.5, torch.randn(C_, device='cuda')
        mean, inv = torch.randn(C_, device='cuda'), torch.rand(C_, device='cuda') + 0.5
        sums2 = torch.zeros(2 * C_, dtype=torch.float64, device='cuda')
        tb = 4.0 * M * C_ / 1e12
        cases = [
            ("tdw_fwd", 2, lambda: ops.tdw_fwd(x, w, None, y, B, K, hw, C_, am)),
            ("tdw_fwd+res", 3, lambda: ops.tdw_fwd(x, w, res, y, B, K, hw, C_, am)),
            ("tdw_bwd", 3, lambda: ops.tdw_bwd(dy, x, w, dx, dw, B, K, hw, C_, ws)),
            ("tdw_bwd dx only", 2, lambda: ops.tdw_bwd(dy, x, w, dx, None, B, K, hw, C_, None)),
            ("bn_apply", 2, lambda: ops.bn_apply_leaky(x, sc, sh, None, y, M, C_, amax_out=am)),
            ("bn_bwd_apply", 3, lambda: ops.bn_bwd_apply(x, dy, sc, sh, mean, inv, sums2, float(M), M, C_, dx, amax_out=am)),
        ]
        for name, nt, fn in cases:
            lo, hi = timed(fn, a.reps)
            rows.append(dict(kernel=name, rows=M, C=C_, us_min=lo * 1e6, us_max=hi * 1e6, tbps=nt * tb / lo, tbps_low=nt * tb / hi))
            print("%-16s rows %9d x C %4d: %8.1f us (%.1f max)  %.2f TB/s" % (name, M, C_, lo * 1e6, hi * 1e6, nt * tb / lo), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(batch=B, k=K, size=a.size, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
