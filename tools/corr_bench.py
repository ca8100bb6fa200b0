"""Times the correlation join's launches alone at full size (B = 16 windows, k = 3, 416 x 416, d in {0, 4}): the three
route shapes (early) and the three tip shapes (late), forward and backward in fp32 and on bf16 tensors; prints time,
TF/s and GB/s on algorithmic bytes.  Then one early and one late d = 4 training step against the 'cat' join network of
the same position (ms / step), in fp32 or (--storage bf16) bf16 storage.

  python tools/corr_bench.py [--batch 16] [--size 416] [--reps 20] [--no-steps] [--storage bf16]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def launches(B, K, size, reps):
    from viddet_amd import lib as L
    lib = L.load()
    rows = []
    shapes = [("route%d" % i, c, size // dv) for i, (c, dv) in enumerate([(256, 8), (512, 16), (1024, 32)])] + \
             [("tip%d" % i, 2 * c, size // dv) for i, (c, dv) in enumerate([(512, 32), (256, 16), (128, 8)])]
    for d in (0, 4):
        D2 = (2 * d + 1) ** 2
        for name, C, h in shapes:
            Cc = K * C + (K - 1) * D2
            ldy = -(-Cc // 64) * 64
            x = torch.randn(B * K, h, h, C, device='cuda')
            y = torch.empty(B, h, h, ldy, device='cuda')
            dx = torch.empty_like(x)
            xb, yb = x.bfloat16(), y.bfloat16()
            dxb = torch.empty_like(xb)
            s = L.stream_ptr()
            flops = 2.0 * B * h * h * (K - 1) * D2 * C
            byt = 4.0 * B * h * h * (K * C + ldy)
            for kind, fn, f, b_ in (
                    ("fwd", lambda: lib.vd_corr_fwd(x.data_ptr(), y.data_ptr(), B, K, h, h, C, d, ldy, s), flops, byt),
                    ("bwd", lambda: lib.vd_corr_bwd(y.data_ptr(), x.data_ptr(), dx.data_ptr(), B, K, h, h, C, d, ldy, s),
                     2 * flops, byt + 4.0 * B * K * h * h * C),
                    ("fwd_bf16", lambda: lib.vd_corr_fwd_bf16(xb.data_ptr(), yb.data_ptr(), B, K, h, h, C, d, ldy, s), flops,
                     byt / 2),
                    ("bwd_bf16", lambda: lib.vd_corr_bwd_bf16(yb.data_ptr(), xb.data_ptr(), dxb.data_ptr(), B, K, h, h, C, d, ldy, s),
                     2 * flops, (byt + 4.0 * B * K * h * h * C) / 2)):
                ms = _time(fn, reps)
                rows.append(dict(d=d, shape=name, C=C, hw=h, kind=kind, ms=round(ms, 4), tflops=round(f / ms / 1e9, 2),
                                 gbs=round(b_ / ms / 1e6, 1)))
                print(json.dumps(rows[-1]), flush=True)
    return rows


def steps(B, K, size, reps, storage='fp32'):
    import numpy as np
    from viddet_amd.model import yolo3_darknet53
    from oracle import yolo as Y
    out = {}
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((B, K, 3, size, size)).astype(np.float32)).cuda()
    gt = np.full((B, 2, 4), -1.0)
    gid = np.full((B, 2, 1), -1.0)
    gt[:, 0] = [40., 60., 200., 300.]
    gid[:, 0] = 1.0
    tg = [torch.from_numpy(np.asarray(t, dtype=np.float32)).cuda()
          for t in Y.prefetch_targets(size, size, [size // 32, size // 16, size // 8], gt, gid, 30)]
    gtt = torch.from_numpy(gt.astype(np.float32)).cuda()
    for pos in ("early", "late"):
        for label, kw in (("corr_d4", dict(corr_pos=pos, corr_d=4)), ("cat", dict(k_join_type="cat", k_join_pos=pos))):
            net = yolo3_darknet53(["c%d" % i for i in range(30)], k=K, **kw)
            net.initialize(init="he", seed=1)
            net.set_storage(storage)

            def step():
                net(x, gtt, *tg)
                net.backward()
                net.sgd_step(1e-4, 0.9, 5e-4, B)

            for _ in range(2):
                step()
            out["%s_%s" % (pos, label)] = round(_time(step, reps), 2)
            print(json.dumps({"step": "%s_%s" % (pos, label), "storage": storage, "ms": out["%s_%s" % (pos, label)]}), flush=True)
            del net
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--storage", default="fp32", choices=["fp32", "bf16"], help="storage of the timed training steps")
    a = ap.parse_args()
    if not a.no_launches:
        launches(a.batch, a.k, a.size, a.reps)
    if not a.no_steps:
        steps(a.batch, a.k, a.size, max(3, a.reps // 4), a.storage)


if __name__ == "__main__":
    main()
