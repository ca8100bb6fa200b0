#!/usr/bin/env python
"""Developer tool: NV12 frames converted inside the device resize (net.set_device_resize(source='nv12'))
against packed RGB frames through the RGB kernel, in front of the same detector.

Per source size (360x480, 720x1280) and target (416, 608), in ONE process:

  kernel    vd_resize_nv12_nchw ms per launch at batch --chunk (device events) and GB/s on the bytes it has to move (both
            planes read once + fp32 planes written), beside vd_resize_u8_nchw on nv12_to_rgb of the same frames (3 bytes per
            pixel read + the same planes written), alternating
  detect    net.detect_video frames/s end to end on a clip of --frames frames handed over on the HOST: `nv12` the NV12
            clip under source='nv12', `rgb` the converted RGB clip under source='rgb' (twice the bytes to upload; the
            host conversion itself is NOT in the timed region); alternating blocks, median of --blocks (host clock
            around work that ends in a device synchronise)

Needs a GPU: there is no fallback.  Prints one JSON line per (source, target).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from tools.resize_probe import _event_ms, _sync_time


def kernel_ms(nv, rgb, size, coef, reps=50, rounds=3):
    """(interp, Ty, Tx, nv12 ms, nv12 GB/s, rgb ms, rgb GB/s): the two launches on the same frames, alternating, median"""
    from viddet_amd import lib as L
    from viddet_amd.video import resize_tables
    n, h0, w0, _ = rgb.shape
    used, *tabs = resize_tables(h0, w0, size, size, 9)
    iy, wy, ix, wx = [torch.from_numpy(t).cuda() for t in tabs]
    out = torch.empty(n, 3, size, size, device="cuda")
    lib = L.load()

    def run_nv12():
        L.check(lib.vd_resize_nv12_nchw(nv.data_ptr(), nv.numel(), nv.shape[1] * w0, w0, h0 * w0, out.data_ptr(), None, n, h0, w0,
                                        size, size, iy.data_ptr(), wy.data_ptr(), iy.shape[1], ix.data_ptr(), wx.data_ptr(),
                                        ix.shape[1], *coef, L.stream_ptr()), "vd_resize_nv12_nchw")

    def run_rgb():
        L.check(lib.vd_resize_u8_nchw(rgb.data_ptr(), out.data_ptr(), None, n, h0, w0, size, size, iy.data_ptr(), wy.data_ptr(),
                                      iy.shape[1], ix.data_ptr(), wx.data_ptr(), ix.shape[1], L.stream_ptr()), "vd_resize_u8_nchw")
    tn, tr = [], []
    for _ in range(rounds):
        tn.append(_event_ms(run_nv12, reps))
        tr.append(_event_ms(run_rgb, reps))
    mn, mr = statistics.median(tn), statistics.median(tr)
    return used, iy.shape[1], ix.shape[1], mn, (nv.numel() + out.numel() * 4) / mn / 1e6, mr, (rgb.numel() + out.numel() * 4) / mr / 1e6


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--sources", default="360x480,720x1280")
    ap.add_argument("--targets", default="416,608")
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--yuv_matrix", default="bt601")
    ap.add_argument("--yuv_range", default="limited")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/nv12_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    from viddet_amd.model import yolo3_darknet53
    from viddet_amd.video import nv12_matrix, nv12_to_rgb
    coef = nv12_matrix(a.yuv_matrix, a.yuv_range)
    torch.set_num_threads(1)
    net = yolo3_darknet53(["c%d" % i for i in range(a.classes)])
    net.initialize(init="he", obj_bias=-2.0)
    net.set_precision(a.precision)
    rng = np.random.default_rng(3)
    for size in [int(s) for s in a.targets.split(",")]:
        for src in a.sources.split(","):
            h0, w0 = [int(s) for s in src.split("x")]
            nv = torch.from_numpy(rng.integers(0, 256, (a.frames, h0 * 3 // 2, w0), dtype=np.uint8))
            rgb = torch.from_numpy(nv12_to_rgb(nv.numpy(), a.yuv_matrix, a.yuv_range))
            used, ty, tx, n_ms, n_gbps, r_ms, r_gbps = kernel_ms(nv[:a.chunk].cuda(), rgb[:a.chunk].cuda(), size, coef)

            def from_nv12():
                net.set_device_resize(size, size, source="nv12", matrix=a.yuv_matrix, range=a.yuv_range)
                return net.detect_video(nv, chunk=a.chunk)

            def from_rgb():
                net.set_device_resize(size, size)
                return net.detect_video(rgb, chunk=a.chunk)

            res_n, res_r = from_nv12(), from_rgb()                 # plans, tuning, code objects, tap tables
            torch.cuda.synchronize()
            same = all(torch.equal(x, y) for x, y in zip(res_n, res_r))
            tn, tr = [], []
            for _ in range(a.blocks):                              # alternating blocks in one process
                tn.append(_sync_time(from_nv12))
                tr.append(_sync_time(from_rgb))
            net.set_device_resize(None)
            res = dict(source=[h0, w0], target=size, interp=used, Ty=ty, Tx=tx, precision=a.precision, frames=a.frames, chunk=a.chunk,
                       matrix=a.yuv_matrix, range=a.yuv_range, kernel_frames=a.chunk,
                       nv12_kernel_ms_per_launch=round(n_ms, 4), nv12_kernel_gbps=round(n_gbps, 1),
                       rgb_kernel_ms_per_launch=round(r_ms, 4), rgb_kernel_gbps=round(r_gbps, 1),
                       kernel_ratio_rgb_over_nv12=round(r_ms / n_ms, 2),
                       detect_nv12_fps=round(a.frames / statistics.median(tn), 1),
                       detect_rgb_fps=round(a.frames / statistics.median(tr), 1),
                       detect_ratio_nv12_over_rgb=round(statistics.median(tr) / statistics.median(tn), 2),
                       detections_identical=same,
                       nv12_s=[round(t, 4) for t in tn], rgb_s=[round(t, 4) for t in tr])
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
