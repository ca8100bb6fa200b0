#!/usr/bin/env python
"""Developer tool: the resize of raw video frames on the device (net.set_device_resize) against the host's
imresize in front of the same detector.

Per source size (360x480, 720x1280) and target (416, 608), in ONE process:

  host      viddet_amd.video.imresize(frame, interp=9) ms per frame on one core (median of --host_reps calls)
  kernel    vd_resize_u8_nchw ms per launch at batch --chunk (device events) and GB/s on the bytes the operator has to move
            (source uint8 read once + fp32 planes written)
  detect    net.detect_video frames/s end to end on a clip of --frames raw frames: `host` resizes every frame with imresize
            (what YOLO3VideoInferenceTransform does) and hands the resized uint8 clip over, `device` hands the raw clip to a
            net with set_device_resize on; alternating blocks, median of --blocks (host clock around work that ends in a
            device synchronise)

Needs a GPU: there is no fallback.  Prints one JSON line per (source, target).
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


def host_ms(frame, size, reps):
    from viddet_amd.video import imresize
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        imresize(frame, size, size, interp=9)
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def kernel_ms(raw, size, reps=50):
    from viddet_amd import lib as L
    from viddet_amd.video import resize_tables
    n, h0, w0, _ = raw.shape
    used, *tabs = resize_tables(h0, w0, size, size, 9)
    iy, wy, ix, wx = [torch.from_numpy(t).cuda() for t in tabs]
    out = torch.empty(n, 3, size, size, device="cuda")
    lib = L.load()

    def run():
        L.check(lib.vd_resize_u8_nchw(raw.data_ptr(), out.data_ptr(), None, n, h0, w0, size, size, iy.data_ptr(), wy.data_ptr(),
                                      iy.shape[1], ix.data_ptr(), wx.data_ptr(), ix.shape[1], L.stream_ptr()), "vd_resize_u8_nchw")
    ms = _event_ms(run, reps)
    nbytes = raw.numel() + out.numel() * 4
    return used, iy.shape[1], ix.shape[1], ms, nbytes / ms / 1e6


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--host_reps", type=int, default=5)
    ap.add_argument("--sources", default="360x480,720x1280")
    ap.add_argument("--targets", default="416,608")
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/resize_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    from viddet_amd.model import yolo3_darknet53
    from viddet_amd.video import imresize
    torch.set_num_threads(1)
    net = yolo3_darknet53(["c%d" % i for i in range(a.classes)])
    net.initialize(init="he", obj_bias=-2.0)
    net.set_precision(a.precision)
    rng = np.random.default_rng(3)
    for size in [int(s) for s in a.targets.split(",")]:
        for src in a.sources.split(","):
            h0, w0 = [int(s) for s in src.split("x")]
            clip = rng.integers(0, 256, (a.frames, h0, w0, 3), dtype=np.uint8)
            used, ty, tx, k_ms, k_gbps = kernel_ms(torch.from_numpy(clip[:a.chunk]).cuda(), size)

            def host():
                net.set_device_resize(None)
                x = np.stack([imresize(f, size, size, interp=9) for f in clip])
                return net.detect_video(torch.from_numpy(x), chunk=a.chunk)

            def device():
                net.set_device_resize(size, size)
                return net.detect_video(torch.from_numpy(clip), chunk=a.chunk)

            for f in (host, device):                               # plans, tuning, code objects, tap tables
                f()
            th, td = [], []
            for _ in range(a.blocks):                              # alternating blocks in one process
                th.append(_sync_time(host))
                td.append(_sync_time(device))
            net.set_device_resize(None)
            res = dict(source=[h0, w0], target=size, interp=used, Ty=ty, Tx=tx, precision=a.precision, frames=a.frames, chunk=a.chunk,
                       host_imresize_ms_per_frame=round(host_ms(clip[0], size, a.host_reps), 2),
                       kernel_ms_per_launch=round(k_ms, 4), kernel_frames=a.chunk, kernel_gbps=round(k_gbps, 1),
                       detect_host_resize_fps=round(a.frames / statistics.median(th), 1),
                       detect_device_resize_fps=round(a.frames / statistics.median(td), 1),
                       ratio=round(statistics.median(th) / statistics.median(td), 2),
                       host_s=[round(t, 4) for t in th], device_s=[round(t, 4) for t in td])
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
