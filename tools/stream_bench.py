#!/usr/bin/env python
"""Developer tool: streaming detection (net.detect_video) against the windowed path on the same clip.

One clip of T frames at --size, --classes classes, window K with step 1, chunks of --chunk output frames.  Per variant
(join position x precision) it times, in ONE process and in alternating blocks,

  stream    net.detect_video(frames, chunk)             - the per-frame prefix once per frame, joins off the feature ring
  windowed  net(windows) at batch `chunk` on the T windows the window rule builds from the same clip (gathered on the device
            before the clock starts) - what the project offered before detect_video

and reports the median of --blocks blocks as frames/s (host clock around work that ends in a device synchronise), the
per-phase device times of the streaming programs (events around the prefix and the suffix replays), and for every ring join
launch its time and TB/s on ideal bytes (K frames read + one written) beside vd_temporal_pool(_bf16) at the same shape on a
materialised window.  Needs a GPU: there is no fallback.  Prints one JSON line per variant.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch


def _sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def join_launches(net, sp, bf16, reps=20):
    """every ring-join record of the suffix program, timed alone, beside the windowed kernel on a gathered copy"""
    from viddet_amd import lib as L
    from viddet_amd.model import PoolNode
    lib, out = L.load(), []
    esz = 2 if bf16 else 4
    for n in net.nodes:
        if not isinstance(n, PoolNode) or n.type == 2:
            continue
        ring, y, slots = sp['sb']['ring:' + n.src], sp['sb'][n.dst], sp['slots']
        Bc, inner, S = y.shape[0], y[0].numel(), ring.shape[0]
        win = ring[slots.long()].contiguous()
        idx = lib.vd_temporal_pool_idx_bf16 if bf16 else lib.vd_temporal_pool_idx
        f_idx = lambda: idx(ring.data_ptr(), slots.data_ptr(), y.data_ptr(), S, Bc, n.K, inner, n.type, L.stream_ptr())
        if bf16:
            f_win = lambda: lib.vd_temporal_pool_bf16(win.data_ptr(), y.data_ptr(), Bc, n.K, inner, n.type, L.stream_ptr())
        else:
            f_win = lambda: lib.vd_temporal_pool(win.data_ptr(), y.data_ptr(), None, Bc, n.K, inner, n.type, L.stream_ptr())
        ideal = float(esz) * Bc * inner * (n.K + 1)
        ms_i, ms_w = _event_ms(f_idx, reps), _event_ms(f_win, reps)
        out.append(dict(join=n.name, inner=inner, ms_idx=round(ms_i, 4), tbps_idx=round(ideal / ms_i / 1e9, 3),
                        ms_windowed=round(ms_w, 4), tbps_windowed=round(ideal / ms_w / 1e9, 3)))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--joins", default="early,late")
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/stream_bench.py needs an MI355X: a timing taken elsewhere says nothing")
    from viddet_amd.model import yolo3_darknet53
    from viddet_amd.stream import ring_size, stream_window_slots
    T, K, chunk = a.frames, a.window, a.chunk
    g = torch.Generator(device="cuda").manual_seed(3)
    frames = torch.randn(T, 3, a.size, a.size, device="cuda", generator=g)
    widx = torch.from_numpy(stream_window_slots(T, K, 1)).cuda()
    for jp in a.joins.split(","):
        net = yolo3_darknet53(["c%d" % i for i in range(a.classes)], k=K, k_join_type="max", k_join_pos=jp)
        net.initialize(init="he", obj_bias=-2.0)
        for prec in a.precisions.split(","):
            net.set_precision(prec)

            def stream():
                return net.detect_video(frames, step=1, chunk=chunk)

            def windowed():
                for t0 in range(0, T, chunk):
                    net(frames[widx[t0:t0 + chunk]])

            for f in (stream, windowed):                           # plans, tuning, code objects
                f()
                f()
            ts, tw = [], []
            for _ in range(a.blocks):                              # alternating blocks in one process
                ts.append(_sync_time(stream))
                tw.append(_sync_time(windowed))
            sp = net._programs[('stream_bf16' if prec == 'bf16' else 'stream', chunk, a.size, a.size, ring_size(K, 1, chunk))]
            res = dict(variant="max %s %s" % (jp, prec), frames=T, size=a.size, classes=a.classes, K=K, chunk=chunk,
                       stream_fps=round(T / statistics.median(ts), 1), windowed_fps=round(T / statistics.median(tw), 1),
                       ratio=round(statistics.median(tw) / statistics.median(ts), 3),
                       stream_s=[round(t, 4) for t in ts], windowed_s=[round(t, 4) for t in tw],
                       prefix_ms_per_run=round(_event_ms(sp['pre'].run, 5), 3), suffix_ms_per_run=round(_event_ms(sp['suf'].run, 5), 3),
                       stream_stats=net.stream_stats, joins=join_launches(net, sp, prec == 'bf16'))
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        del net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
