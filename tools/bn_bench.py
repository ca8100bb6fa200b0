#!/usr/bin/env python
"""Achieved HBM rate of the BatchNorm apply / backward-apply kernels alone (no side-stream neighbour), on the activation
shapes of the batch-64 416x416 training step, beside two yardsticks from outside the library on the same shapes in the same
run: torch.Tensor.copy_ (1 read + 1 write, the traffic of apply) and torch.add(a, b, out=c) (2 reads + 1 write, the traffic
of apply with a residual and of bwd_apply).  Rates are algorithmic bytes over event time.

usage: python tools/bn_bench.py [--json] [--storage fp32 bf16] [--iters N]
VD_BN_STREAM=0 times the one-vector-per-trip kernels (the switch is read once per process: run twice to compare)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from viddet_amd import lib as L
from viddet_amd import ops

SHAPES = [(64 * 208 * 208, 64), (64 * 104 * 104, 128), (64 * 52 * 52, 256), (64 * 26 * 26, 512), (64 * 13 * 13, 1024),
          (64 * 208 * 208, 32), (64 * 52 * 52, 128)]


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


def bench_shape(M, C, dt, it):
    x = torch.randn(M, C, device="cuda").to(dt)
    dy = torch.randn(M, C, device="cuda").to(dt)
    y = torch.empty_like(x)
    sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
    mu, iv = torch.randn(C, device="cuda"), torch.rand(C, device="cuda") + 0.5
    sums2 = torch.randn(2 * C, device="cuda", dtype=torch.float64)
    gb = M * C * x.element_size() / 1e9
    runs = [("copy", 2, lambda: y.copy_(x)),
            ("add", 3, lambda: torch.add(x, dy, out=y)),
            ("apply", 2, lambda: ops.bn_apply_leaky(x, sc, sh, None, y, M, C)),
            ("apply_res", 3, lambda: ops.bn_apply_leaky(x, sc, sh, dy, y, M, C)),
            ("bwd_apply", 3, lambda: ops.bn_bwd_apply(x, dy, sc, sh, mu, iv, sums2, float(M), M, C, y))]
    if dt == torch.float32:          # as the model calls them: publishing the max-abs of the output (the bf16 entries have no slots)
        slot = torch.zeros(L.AMAX_FLOATS, device="cuda")
        runs += [("apply_amax", 2, lambda: ops.bn_apply_leaky(x, sc, sh, None, y, M, C, amax_out=slot)),
                 ("bwd_apply_amax", 3, lambda: ops.bn_bwd_apply(x, dy, sc, sh, mu, iv, sums2, float(M), M, C, y, amax_out=slot))]
    r = {"M": M, "C": C, "MB": round(gb * 1e3, 1)}
    for name, streams, fn in runs:
        t = timeit(fn, it)
        r[name + "_us"] = round(t * 1e3, 1)
        r[name + "_TBps"] = round(streams * gb / t, 3)
    # each kernel as a fraction of the yardstick with its traffic
    r["apply_vs_copy"] = round(r["apply_TBps"] / r["copy_TBps"], 3)
    r["apply_res_vs_add"] = round(r["apply_res_TBps"] / r["add_TBps"], 3)
    r["bwd_apply_vs_add"] = round(r["bwd_apply_TBps"] / r["add_TBps"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true", help="one JSON document on stdout instead of the table")
    ap.add_argument("--storage", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    doc = {"device": torch.cuda.get_device_name(0), "VD_BN_STREAM": os.environ.get("VD_BN_STREAM", "1"), "iters": a.iters}
    for st in a.storage:
        rows = [bench_shape(M, C, torch.bfloat16 if st == "bf16" else torch.float32, a.iters) for M, C in SHAPES]
        keys = ["copy", "add", "apply", "apply_res", "bwd_apply"] + (["apply_amax", "bwd_apply_amax"] if st == "fp32" else [])
        doc[st] = {"shapes": rows, "sum_ms": {k: round(sum(r[k + "_us"] for r in rows) / 1e3, 3) for k in keys}}
        if a.json:
            continue
        print("storage %s (VD_BN_STREAM=%s)" % (st, doc["VD_BN_STREAM"]))
        for r in rows:
            print("M %8d C %4d %6.1f MB | copy %.2f add %.2f TB/s | apply %.1f us %.2f TB/s (%.2f of copy) | apply+res %.1f us "
                  "%.2f TB/s (%.2f of add) | bwd_apply %.1f us %.2f TB/s (%.2f of add)" %
                  (r["M"], r["C"], r["MB"], r["copy_TBps"], r["add_TBps"], r["apply_us"], r["apply_TBps"], r["apply_vs_copy"],
                   r["apply_res_us"], r["apply_res_TBps"], r["apply_res_vs_add"], r["bwd_apply_us"], r["bwd_apply_TBps"],
                   r["bwd_apply_vs_add"]))
        print("sum ms: " + ", ".join("%s %.3f" % kv for kv in doc[st]["sum_ms"].items()))
    if a.json:
        print(json.dumps(doc))


if __name__ == "__main__":
    main()
