#!/usr/bin/env python
"""Developer tool: the VID motion metric with its matching on the device (detect_yolo3.py --metrics vid --device_metric,
DESIGN.md 25) against the host metric on the same detections.

In ONE process, on SyntheticTracks at --clips (64) x --frames (64) with about --dets (10,300) synthetic detections per image
(noisy copies of the ground truth and clutter, distinct scores):

  host     VIDDetectionMetric.get() seconds
  device   DeviceVIDDetectionMetric.get() seconds, split into pack / upload / launch (device events) / download / AP
  kernel   vd_vid_match ms per launch (device events, --reps launches) on the first chunk of that set

alternating blocks, median of --blocks; the two results are compared on the way.  Needs a GPU: there is no fallback.
Prints one JSON line per detection count.
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


def detections(ds, per_image, seed=1):
    """about per_image rows [sid, label, score, x1, y1, x2, y2] per image: up to three noisy copies of every ground truth,
    clutter for the rest"""
    rng = np.random.default_rng(seed)
    w, h = ds.frame_size
    rows = []
    for sid in ds.get_sample_ids():
        lab = ds.get_label(sid)
        n = int(rng.integers(max(1, per_image - per_image // 5), per_image + per_image // 5 + 1))
        k = min(n, 3 * len(lab))
        if k:
            g = lab[rng.integers(0, len(lab), k)]
            s = np.stack([g[:, 2] - g[:, 0] + 1, g[:, 3] - g[:, 1] + 1] * 2, axis=1)
            box = g[:, :4] + rng.normal(0, 0.08, (k, 4)) * s
            cls = np.where(rng.random(k) < 0.85, g[:, 4], rng.integers(0, ds.num_class, k))
            rows.append(np.concatenate([np.full((k, 1), sid), cls[:, None], np.zeros((k, 1)), box], axis=1))
        if n > k:
            xy = rng.uniform(0, (w - 20, h - 20), (n - k, 2))
            wh = np.exp(rng.uniform(np.log(10.0), np.log(250.0), (n - k, 2)))
            rows.append(np.concatenate([np.full((n - k, 1), sid), rng.integers(0, ds.num_class, (n - k, 1)), np.zeros((n - k, 1)),
                                        xy, xy + wh], axis=1))
    rows = np.concatenate(rows)
    rows[:, 2] = 0.06 + 0.93 * (rng.permutation(len(rows)) + 0.5) / len(rows)
    return [[int(r[0]), int(r[1])] + r[2:].tolist() for r in rows]


def _event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def probe(a, ds, per_image):
    from viddet_amd import ops
    from viddet_amd.device_vid_metric import DeviceVIDDetectionMetric, pack_images
    from viddet_amd.vid_metric import AREA_RANGES, MOTION_RANGES, VIDDetectionMetric
    res = detections(ds, per_image)
    host, dev = VIDDetectionMetric(ds), DeviceVIDDetectionMetric(ds)
    host._results, dev._results = res, res

    def run(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.get()
        return time.perf_counter() - t0, out

    run(dev)                                                       # code objects, pinned-memory pools
    th, td, parts = [], [], []
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t, oh = run(host)
        th.append(t)
        t, od = run(dev)
        td.append(t)
        parts.append(dict(dev.timings))
    same = oh == od and np.array_equal(host.ap, dev.ap)
    chunks, _ = pack_images(ds, res)
    det, gt = chunks[0]
    B, N, M, C = det.shape[0], det.shape[1], gt.shape[1], len(ds.classes)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    args = (up(det), up(gt), up(MOTION_RANGES), up(AREA_RANGES), 0.5, 10.0, i32(B, N), i32(B, N), i32(B, N), i32(B, 4), i32(B),
            i32(C), i32(16, C))
    k_ms = _event_ms(lambda: ops.vid_match(*args), a.reps)
    med = lambda key: round(statistics.median(p[key] for p in parts), 5)
    return dict(clips=a.clips, frames=a.frames, images=len(ds), detections=len(res), detections_per_image=round(len(res) / len(ds), 1),
                chunks=len(chunks), host_get_s=[round(t, 4) for t in th], device_get_s=[round(t, 4) for t in td],
                host_get_median_s=round(statistics.median(th), 4), device_get_median_s=round(statistics.median(td), 4),
                device_split_s=dict(pack=med("pack"), upload=med("upload"), launch=med("launch"), download=med("download"), ap=med("ap")),
                kernel=dict(B=B, N=N, M=M, ms_per_launch=round(k_ms, 4)), same_result=bool(same))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,300", help="detections per image, one probe each")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/vid_metric_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("vid", num_videos=a.clips, frames_per_video=a.frames)
    ds.motion_ious
    for n in [int(s) for s in a.dets.split(",")]:
        line = json.dumps(probe(a, ds, n))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
