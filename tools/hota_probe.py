#!/usr/bin/env python
"""Developer tool: the HOTA tracking metric with its matching on the device (vd_hota_match, ops.hota_match, DeviceHOTAMetric,
DESIGN.md 35) against the host metric on the same tracked detections.

In ONE process, on SyntheticTracks at --clips (64) x --frames (64) with about --dets (10,100) synthetic detections per frame
(tools/seq_nms_probe.py's), linked by ops.track at every --max_age (0,7):

  metric   HOTAMetric.get() seconds against DeviceHOTAMetric.get() seconds, the latter split into pack / upload / launch /
           download / summary (its `timings`); the two results compared in every character
  kernel   vd_hota_match ms per launch over ALL clips at once (device events, --reps calls), its outputs compared with
           hota_match_host's bit for bit, and vd_mot_match on the same rows beside it
  quality  tools/track_probe.py's quality case - the ground truth at score 0.9, boxes jittered by --jitter (4 %) of their size,
           --drop (10 %) of the rows left out - linked by `iou` at sigma_iou 0.5, by `iou` at 0.3 and by `sort` (0.3), each at
           max_age 1 and 7: HOTA, DetA, AssA, LocA beside the MOT metric's MOTA and IDF1 of the same rows
  dense    the assignment at its widest: 128 label rows against 128 prediction rows a frame, crowded -
           hota_match_host ms per frame against vd_hota_match ms per launch (the frames run side by side)

alternating blocks, median of --blocks; that the device's result equals the host's is the pass condition, no speed is asked for.
Needs a GPU: there is no fallback.  Prints one JSON line per measurement.
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

from mot_probe import _results
from seq_nms_probe import _event_ms, clip_arrays


def _same_bits(got, want):
    return all(np.array_equal(np.ascontiguousarray(g).view(np.int32), np.ascontiguousarray(w).view(np.int32)) for g, w in zip(got, want))


def probe(a, ds, per_image, max_age):
    from viddet_amd import ops
    from viddet_amd.device_hota_metric import DeviceHOTAMetric, dense_ids
    from viddet_amd.hota_metric import HOTAMetric, hota_match_host
    from viddet_amd.mot_metric import masked_track, pack_clips
    ids, scores, bboxes = clip_arrays(ds, per_image)
    F, N = bboxes.shape[:2]
    T, C = a.frames, len(ds.classes)
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    track = ops.track(*dv, clip_start=cs, num_class=C, sigma_h=0.0, t_min=1, max_age=max_age)[0].cpu().numpy()
    results = _results(ds, ids, scores, bboxes, track)
    host, dev = HOTAMetric(ds), DeviceHOTAMetric(ds)
    host._results, dev._results = results, results
    arrays, pcs = pack_clips(ds, results)
    G = arrays[0].shape[1]
    # the launches alone: on the ids as the metric class sends them, dense per clip
    sent = list(arrays)
    sent[2], num_gt = dense_ids(arrays[2], pcs)
    sent[6], num_pred = dense_ids(masked_track(arrays[3], arrays[4], arrays[6], C), pcs)
    A, P = max(1, max(num_gt)), max(1, max(num_pred))
    da = [torch.from_numpy(x).cuda() for x in sent]
    dcs = torch.tensor(pcs, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.hota_ws_bytes(len(pcs) - 1, A, P), dtype=torch.uint8, device="cuda")
    call = lambda: ops.hota_match(*da, num_gt_id=A, num_track=P, clip_start=dcs, num_class=C, ws=ws)
    mot_ws = torch.empty(4 * F * (G + arrays[5].shape[1]), dtype=torch.uint8, device="cuda")
    mot_call = lambda: ops.mot_match(*da, clip_start=dcs, num_class=C, ws=mot_ws)
    dev.get()                                                      # code objects, the pinned pool
    th, td, kernel, mot_kernel, parts = [], [], [], [], []
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t0 = time.perf_counter()
        want = host.get()
        th.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        got = dev.get()
        td.append(time.perf_counter() - t0)
        parts.append(dict(dev.timings))
        kernel.append(_event_ms(call, a.reps))
        mot_kernel.append(_event_ms(mot_call, a.reps))
    records = [r.cpu().numpy() for r in call()]
    same = want == got and host.summary == dev.summary and _same_bits(records, hota_match_host(*sent, clip_start=pcs, num_class=C))
    med = statistics.median
    s = host.summary["all"]
    return dict(what="hota", clips=a.clips, frames=T, label_rows_per_frame=G, rows_per_frame=arrays[5].shape[1], classes=C, max_age=max_age,
                detections_per_frame=round(float((ids >= 0).sum()) / F, 1), GT=s["GT"], PRED=s["PRED"], TP_at_0_5=s["TP"][9],
                gt_ids_per_clip=A, track_ids_per_clip=P, workspace_bytes=int(ws.numel()),
                HOTA=round(s["HOTA"], 4), DetA=round(s["DetA"], 4), AssA=round(s["AssA"], 4), LocA=round(s["LocA"], 4),
                host_get_s=[round(t, 4) for t in th], host_median_get_s=round(med(th), 4),
                device_get_s=[round(t, 4) for t in td], device_median_get_s=round(med(td), 4),
                device_parts_median_s={k: round(med([p[k] for p in parts]), 5) for k in parts[0]},
                kernel_ms_per_launch=[round(t, 4) for t in kernel], kernel_median_ms_per_launch=round(med(kernel), 4),
                mot_kernel_median_ms_per_launch=round(med(mot_kernel), 4), same_result=bool(same))


def quality(a, ds, method, sigma_iou, max_age):
    """tools/track_probe.py's quality case (its generator, its seed) linked by `method` and scored by both tracking metrics"""
    from viddet_amd import ops
    from viddet_amd.device_hota_metric import DeviceHOTAMetric
    from viddet_amd.hota_metric import HOTAMetric
    from viddet_amd.mot_metric import MOTMetric
    rng = np.random.default_rng(7)
    T = ds.frames_per_video
    labels = [ds.get_label(sid) for sid in ds.get_sample_ids()]
    N = max(1, max(len(l) for l in labels))
    F = len(labels)
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    for t, l in enumerate(labels):
        keep = l[rng.uniform(size=len(l)) >= a.drop]
        wh = np.stack([keep[:, 2] - keep[:, 0], keep[:, 3] - keep[:, 1]] * 2, axis=1)
        box = keep[:, :4] + rng.normal(0.0, a.jitter, (len(keep), 4)) * wh
        n = len(keep)
        ids[t, :n, 0], scores[t, :n, 0], bboxes[t, :n] = keep[:, 4], 0.9, box
    link = ops.track if method == "iou" else ops.track_sort
    track = link(*[torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)], clip_start=list(range(0, F + 1, T)),
                 num_class=len(ds.classes), sigma_iou=sigma_iou, max_age=max_age)[0].cpu().numpy()
    results = _results(ds, ids, scores, bboxes, track)
    host, dev, mot = HOTAMetric(ds), DeviceHOTAMetric(ds), MOTMetric(ds)
    host._results, dev._results, mot._results = results, results, results
    same = host.get() == dev.get() and host.summary == dev.summary
    mot.get()
    s, m = dev.summary["all"], mot.summary["all"]
    return dict(what="quality", method=method, sigma_iou=sigma_iou, max_age=max_age, clips=ds.num_videos, frames=T, jitter=a.jitter,
                drop=a.drop, GT=s["GT"], PRED=s["PRED"], gt_tracks=s["gt_tracks"], pred_tracks=s["pred_tracks"],
                HOTA=round(s["HOTA"], 4), DetA=round(s["DetA"], 4), AssA=round(s["AssA"], 4), LocA=round(s["LocA"], 4),
                AssRe=round(s["AssRe"], 4), AssPr=round(s["AssPr"], 4), MOTA=round(m["MOTA"], 4), IDF1=round(m["IDF1"], 4),
                IDSW=m["IDSW"], Frag=m["Frag"], same_result=bool(same))


def dense(a, G=128, N=128, clips=4, frames=8):
    """the assignment at its widest, which no SyntheticTracks set reaches: G label rows and N prediction rows a frame whose boxes
    crowd one corner of the frame (many admissible pairs a row), ids that persist over the clip"""
    from viddet_amd import ops
    from viddet_amd.hota_metric import hota_match_host
    rng = np.random.default_rng(5)
    F = clips * frames

    def boxes(n):
        c, wh = rng.uniform(50, 250, (F, n, 2)), rng.uniform(60, 100, (F, n, 2))
        return np.concatenate([c - wh / 2, c + wh / 2], axis=2).astype(np.float32)

    arrays = (boxes(G), np.zeros((F, G), np.int32), np.stack([rng.permutation(G) for _ in range(F)]).astype(np.int32),
              np.zeros((F, N, 1), np.float32), np.full((F, N, 1), 0.9, np.float32), boxes(N),
              np.stack([rng.permutation(N) for _ in range(F)]).astype(np.int32))
    cs = list(range(0, F + 1, frames))
    da = [torch.from_numpy(x).cuda() for x in arrays]
    dcs = torch.tensor(cs, dtype=torch.int32, device="cuda")
    call = lambda: ops.hota_match(*da, num_gt_id=G, num_track=N, clip_start=dcs, num_class=1)
    mot_call = lambda: ops.mot_match(*da, clip_start=dcs, num_class=1)
    th, kernel, mot_kernel = [], [], []
    for _ in range(a.blocks):
        t0 = time.perf_counter()
        want = hota_match_host(*arrays, clip_start=cs, num_class=1)
        th.append(time.perf_counter() - t0)
        kernel.append(_event_ms(call, a.reps))
        mot_kernel.append(_event_ms(mot_call, a.reps))
    got = [r.cpu().numpy() for r in call()]
    med = statistics.median
    return dict(what="dense", clips=clips, frames=frames, label_rows_per_frame=G, rows_per_frame=N, matched=int((want[0] >= 0).sum()),
                host_s=[round(t, 4) for t in th], host_median_ms_per_frame=round(1e3 * med(th) / F, 3),
                kernel_ms_per_launch=[round(t, 4) for t in kernel], kernel_median_ms_per_launch=round(med(kernel), 4),
                mot_kernel_median_ms_per_launch=round(med(mot_kernel), 4), same_result=bool(_same_bits(got, want)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one probe each")
    ap.add_argument("--max_age", default="0,7", help="one probe each")
    ap.add_argument("--quality_max_age", default="1,7", help="the quality table, one row each per tracker")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=0.04, help="quality: sigma of the box noise, as a share of the box's size")
    ap.add_argument("--drop", type=float, default=0.1, help="quality: the share of ground-truth rows left out")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/hota_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("vid", num_videos=a.clips, frames_per_video=a.frames)
    results = []

    def emit(d):
        results.append(d)
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for n in [int(s) for s in a.dets.split(",")]:
        for m in [int(s) for s in a.max_age.split(",")]:
            emit(probe(a, ds, n, m))
    for m in [int(s) for s in a.quality_max_age.split(",")]:
        for method, sigma_iou in (("iou", 0.5), ("iou", 0.3), ("sort", 0.3)):
            emit(quality(a, ds, method, sigma_iou, m))
    emit(dense(a))
    if not all(d["same_result"] for d in results):
        raise SystemExit("the device's result differs from the host's")


if __name__ == "__main__":
    main()
