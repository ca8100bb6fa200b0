#!/usr/bin/env python
"""Developer tool: the overlay on the device (vd_overlay, ops.overlay) against its host definition on the same
frames and rows.

In ONE process, on --frames (16) random frames of every --sizes (360x480,720x1280) with --dets (10,100) drifting, tracked rows
per frame and as many ground-truth rows, at every --trail (0,8), as RGB and as NV12:

  host     overlay_host seconds per frame, on the first --host_frames frames
  device   vd_overlay ms per call out of place and in place, each of its launches alone (vd_overlay_stages), Tensor.copy_ of
           the same frames beside it - device events around --reps replays of the call captured into a graph, so that the
           device and not the host's argument checks is timed; the eager call is reported beside them - and GB/s on the bytes
           moved: the out-of-place form and the copy read and write every byte of the frames once
  video    the call as a share of net.detect_video(track=...) on a --video_frames (64) clip of the first size at --data_shape

alternating blocks, median of --blocks; the device result is compared with the host's on the host's frames on the way: that it
is equal is the pass condition, no speed is asked for.  Needs a GPU: there is no fallback.  Prints one JSON line per
measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from seq_nms_probe import _event_ms

STAGES = (("primitives", 1), ("paint", 2))


def _graph_ms(fn, reps):
    """device time of fn: captured once into a graph and replayed, so that the host's share of a call (argument checks, the
    ctypes call) does not pace the device"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return _event_ms(g.replay, reps)


def rows_of(F, n, size, seed=3):
    """n objects drifting over F frames of size = (H0, W0): (ids, scores (F,n,1), bboxes (F,n,4), track (F,n), gt (F,n,5))"""
    rng = np.random.default_rng(seed)
    h0, w0 = size
    c = rng.uniform(0.1, 0.9, (n, 2)) * (w0, h0)
    wh = rng.uniform(0.04, 0.25, (n, 2)) * (w0, h0)
    vel = rng.uniform(-0.01, 0.01, (n, 2)) * (w0, h0)
    t = np.arange(F)[:, None, None]
    p = c[None] + vel[None] * t
    box = np.concatenate([p - wh / 2, p + wh / 2], axis=-1).astype(np.float32)
    ids = np.broadcast_to(rng.integers(0, 20, n).astype(np.float32)[None, :, None], (F, n, 1)).copy()
    scores = np.broadcast_to(np.sort(rng.uniform(0.5, 1.0, n).astype(np.float32))[::-1][None, :, None], (F, n, 1)).copy()
    track = np.broadcast_to(np.arange(n, dtype=np.int32)[None], (F, n)).copy()
    gt = np.concatenate([box + 3.0, ids], axis=-1).astype(np.float32)
    return ids, scores, box, track, gt


def probe(a, size, n, L, fmt):
    from viddet_amd import lib as Lb, ops
    from viddet_amd.overlay import overlay_host
    from viddet_amd.video import rgb_to_nv12
    F = a.frames
    rgb = np.random.default_rng(1).integers(0, 256, (F,) + size + (3,), dtype=np.uint8)
    frames = rgb if fmt == "rgb" else rgb_to_nv12(rgb)
    ids, scores, box, track, gt = rows_of(F, n, size)
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, box)]
    kw = dict(track=torch.from_numpy(track).cuda(), gt=torch.from_numpy(gt).cuda(), trail=L, fmt=fmt)
    src = torch.from_numpy(frames).cuda()
    out, work = torch.empty_like(src), src.clone()
    ws = torch.empty(Lb.OVERLAY_WS_PER_ROW * F * 2 * n, dtype=torch.uint8, device="cuda")
    oop = lambda stages=None: ops.overlay(src, *dv, out=out, ws=ws, stages=stages, **kw)
    inp = lambda: ops.overlay(work, *dv, out=work, ws=ws, **kw)
    copy = lambda: out.copy_(src)
    hf = min(a.host_frames, F)
    th, t_call, t_oop, t_inp, t_copy = [], [], [], [], []
    per = {name: [] for name, _ in STAGES}
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t0 = time.perf_counter()
        want = overlay_host(frames[:hf], ids[:hf], scores[:hf], box[:hf], track[:hf], gt[:hf], trail=L, fmt=fmt)
        th.append((time.perf_counter() - t0) / hf)
        t_call.append(_event_ms(oop, a.reps))                      # as a caller sees it: the host's share included
        t_oop.append(_graph_ms(oop, a.reps))
        t_inp.append(_graph_ms(inp, a.reps))
        t_copy.append(_graph_ms(copy, a.reps))
        for name, bit in STAGES:                                   # the workspace holds a whole call's records
            per[name].append(_graph_ms(lambda: oop(bit), a.reps))
    got, painted = oop()
    torch.cuda.synchronize()
    # (frame f < hf of the call has the same trail as in the host's shorter call: trails only reach back)
    same = bool(np.array_equal(got[:hf].cpu().numpy(), want[0]) and np.array_equal(painted[:hf].cpu().numpy(), want[1])
                and np.array_equal(work[:hf].cpu().numpy(), want[0]))
    med = statistics.median
    nbytes = frames.nbytes
    gbs = lambda ms: round(2.0 * nbytes / (ms * 1e-3) / 1e9, 1)
    px = float(painted.float().mean())
    return dict(what="overlay", fmt=fmt, size="%dx%d" % size, frames=F, rows_per_frame=n, gt_rows_per_frame=n, trail=L,
                painted_share=round(px / (size[0] * size[1]), 4), host_frames=hf,
                host_median_s_per_frame=round(med(th), 4), eager_call_median_ms=round(med(t_call), 4),
                out_of_place_ms_per_call=[round(t, 4) for t in t_oop], out_of_place_median_ms=round(med(t_oop), 4),
                in_place_median_ms=round(med(t_inp), 4), copy_median_ms=round(med(t_copy), 4),
                launch_median_ms={name: round(med(v), 4) for name, v in per.items()},
                out_of_place_gb_s=gbs(med(t_oop)), copy_gb_s=gbs(med(t_copy)),
                out_of_place_over_copy=round(med(t_oop) / med(t_copy), 2), in_place_over_copy=round(med(t_inp) / med(t_copy), 2),
                same_result=same)


def video(a, size):
    """the overlay's share of detect_video(track=...) on one clip at the first size, resized to --data_shape on the device"""
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["class%d" % i for i in range(20)])
    net.initialize(init="he", obj_bias=0.0)
    net.set_device_resize(a.data_shape, a.data_shape)
    x = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (a.video_frames,) + size + (3,), dtype=np.uint8)).cuda()
    trk = dict(method="sort")
    plain = lambda: net.detect_video(x, chunk=8, track=trk)
    drawn = lambda: net.detect_video(x, chunk=8, track=trk, overlay=dict(thresh=0.3))
    tp, td = [], []
    for _ in range(a.blocks):
        tp.append(_event_ms(plain, 1))
        td.append(_event_ms(drawn, 1))
    med = statistics.median
    painted = net.last_overlay[1].float().mean().item() if net.last_overlay is not None else 0.0
    return dict(what="video", size="%dx%d" % size, frames=a.video_frames, data_shape=a.data_shape,
                detect_video_median_ms=round(med(tp), 3), with_overlay_median_ms=round(med(td), 3),
                overlay_share=round((med(td) - med(tp)) / med(td), 4), painted_pixels_per_frame=round(painted, 1))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="360x480,720x1280", help="source sizes H0xW0, one probe each")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--dets", default="10,100", help="rows (and ground-truth rows) per frame, one probe each")
    ap.add_argument("--trail", default="0,8", help="frames a trail reaches back, one probe each")
    ap.add_argument("--formats", default="rgb,nv12")
    ap.add_argument("--host_frames", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--video_frames", type=int, default=64)
    ap.add_argument("--data_shape", type=int, default=416)
    ap.add_argument("--no_video", action="store_true", help="skip the detect_video part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/overlay_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    results = []

    def emit(d):
        results.append(d)
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for fmt in a.formats.split(","):
        for size in sizes:
            for n in [int(s) for s in a.dets.split(",")]:
                for L in [int(s) for s in a.trail.split(",")]:
                    emit(probe(a, size, n, L, fmt))
    if not a.no_video:
        emit(video(a, sizes[0]))
    if not all(d.get("same_result", True) for d in results):
        raise SystemExit("the device's result differs from overlay_host's")


if __name__ == "__main__":
    main()
