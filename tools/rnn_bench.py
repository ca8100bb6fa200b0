"""Times the bidirectional ConvGRU of temporal windows (--rnn_pos) at full size (B = 16 windows, k = 3, 416 x 416).

The gate kernels alone on the three `late` state shapes (2c channels at 13 / 26 / 52 squared) and the `out` shape: time and
GB/s on the bytes each launch moves (forward with a state: 8 Ch floats per row, backward: 16), beside one BatchNorm-apply
launch on the same rows (the project's yardstick for a streaming pass).  Then one training step of the late / max network
with and without rnn_pos late, and of rnn_pos out (ms / step), and with --split the step's time by launch family (every
launch timed alone on one stream, Program.run_timed).

`--trace-steps late|out|none` runs four training steps of one variant and nothing else: the program to put behind
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR --`, whose output tools/summarize_rocprof.py and
tools/step_gaps.py read.

The gate_bwd timing repeats the in-place kernel on the same I / H, so after the first call its inputs are gradients of
gradients (small values): a bandwidth figure, not the arithmetic of a real step.

  python tools/rnn_bench.py [--batch 16] [--size 416] [--reps 20] [--no-steps] [--no-launches] [--split]
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


def launches(B, K, size, reps, classes=30):
    from viddet_amd import lib as L
    lib = L.load()
    A = 3 * (5 + classes)
    shapes = [("late%d" % i, 2 * c, size // dv) for i, (c, dv) in enumerate([(512, 32), (256, 16), (128, 8)])] + \
             [("out2", -(-A // 32) * 32, size // 8)]
    for name, Ch, h in shapes:
        hw, M = h * h, B * h * h
        I = torch.randn(B * K, hw, 3 * Ch, device='cuda')
        H = torch.randn(M, 3 * Ch, device='cuda')
        hp, hn, dh = torch.rand(M, Ch, device='cuda'), torch.empty(M, Ch, device='cuda'), torch.randn(M, Ch, device='cuda')
        dy = torch.randn(B * K, hw, Ch, device='cuda')
        bias = torch.zeros(3 * Ch, device='cuda')
        ones, zeros = torch.ones(Ch, device='cuda'), torch.zeros(Ch, device='cuda')
        s = L.stream_ptr()
        for kind, fn, byt in (
                ("gate_fwd", lambda: lib.vd_gru_gate_fwd(I.data_ptr(), H.data_ptr(), bias.data_ptr(), hp.data_ptr(), hn.data_ptr(), B, K, 1,
                                                         hw, Ch, s), 4.0 * M * Ch * 8),
                ("gate_bwd", lambda: lib.vd_gru_gate_bwd(I.data_ptr(), H.data_ptr(), 1, bias.data_ptr(), hp.data_ptr(), dy.data_ptr(), 0.5,
                                                         dh.data_ptr(), 1, B, K, 1, hw, Ch, s), 4.0 * M * Ch * 16),
                ("bn_apply", lambda: lib.vd_bn_apply_leaky(hp.data_ptr(), ones.data_ptr(), zeros.data_ptr(), None, hn.data_ptr(), M, Ch,
                                                           0.1, None, s), 4.0 * M * Ch * 2)):
            ms = _time(fn, reps)
            print(json.dumps(dict(shape=name, Ch=Ch, hw=h, rows=M, kind=kind, ms=round(ms, 4), gbs=round(byt / ms / 1e6, 1))), flush=True)


def steps(B, K, size, reps, split, classes=30, only=None):
    import numpy as np
    from viddet_amd.model import yolo3_darknet53
    from oracle import yolo as Y
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((B, K, 3, size, size)).astype(np.float32)).cuda()
    gt = np.full((B, 2, 4), -1.0)
    gid = np.full((B, 2, 1), -1.0)
    gt[:, 0] = [40., 60., 200., 300.]
    gid[:, 0] = 1.0
    tg = [torch.from_numpy(np.asarray(t, dtype=np.float32)).cuda()
          for t in Y.prefetch_targets(size, size, [size // 32, size // 16, size // 8], gt, gid, classes)]
    gtt = torch.from_numpy(gt.astype(np.float32)).cuda()
    variants = (("late_max", dict()), ("late_max_rnn_late", dict(rnn_pos="late")), ("max_rnn_out", dict(rnn_pos="out")))
    if only is not None:
        variants = [v for v in variants if v[1].get("rnn_pos") == (None if only == "none" else only)]
    for label, kw in variants:
        net = yolo3_darknet53(["c%d" % i for i in range(classes)], k=K, k_join_type="max", k_join_pos="late", **kw)
        net.initialize(init="he", seed=1)

        def step():
            net(x, gtt, *tg)
            net.backward()
            net.sgd_step(1e-4, 0.9, 5e-4, B)

        for _ in range(2):
            step()
        if only is not None:
            for _ in range(4):
                step()
            torch.cuda.synchronize()
            continue
        print(json.dumps({"step": label, "ms": round(_time(step, reps), 2)}), flush=True)
        if split and kw:
            tp = net._last_train
            fam = {}
            for seg in tp['fwd'] + tp['bwd']:
                names = {r[0] for r in seg.recs if r[0]}
                for fname, meta, e0, e1 in seg.run_timed(names):
                    torch.cuda.synchronize()
                    kind = (meta or {}).get('kind', '')
                    gru = fname.startswith('vd_gru') or '.rnn.' in str((meta or {}).get('node', ''))
                    key = ("gru:" if gru else "") + (fname if not kind else "%s/%s" % (fname, kind))
                    fam[key] = fam.get(key, 0.0) + e0.elapsed_time(e1)
            tot = sum(fam.values())
            for key, ms in sorted(fam.items(), key=lambda kv: -kv[1])[:16]:
                print(json.dumps({"step": label, "family": key, "ms": round(ms, 3), "share": round(ms / tot, 4)}), flush=True)
            print(json.dumps({"step": label, "serial_sum_ms": round(tot, 2),
                              "gru_ms": round(sum(v for k_, v in fam.items() if k_.startswith("gru:")), 2)}), flush=True)
        del net
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--split", action="store_true", help="the rnn steps' time by launch family (each launch timed alone)")
    ap.add_argument("--trace-steps", default=None, choices=["late", "out", "none"])
    a = ap.parse_args()
    if a.trace_steps:
        return steps(a.batch, a.k, a.size, 0, False, only=a.trace_steps)
    if not a.no_launches:
        launches(a.batch, a.k, a.size, a.reps)
    if not a.no_steps:
        steps(a.batch, a.k, a.size, max(3, a.reps // 4), a.split)


if __name__ == "__main__":
    main()
