#!/usr/bin/env python
"""Developer tool: Seq-NMS on the device (vd_seq_nms, ops.seq_nms) against its host definition on the same
detections.

In ONE process, on SyntheticTracks at --clips (64) x --frames (64) with about --dets (10,100) synthetic detections per frame
(noisy copies of the ground truth and clutter, as tools/vid_metric_probe.py makes them):

  host     seq_nms_host seconds per clip, on the first --host_clips clips (the loop is Python: all 64 would take minutes)
  device   vd_seq_nms ms per call over ALL clips at once (device events, --reps calls), and the three launches apart:
           link table / rounds / sort, from calls that stop after one, two and three launches
  share    the call as a share of net.detect_video on one --frames clip at --size (416): detect_video with and without
           seq_nms=True, wall time around a synchronize

alternating blocks, median of --blocks; the device result is compared with the host's on the host's clips on the way.  Needs a
GPU: there is no fallback.  Prints one JSON line per measurement.
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


def clip_arrays(ds, per_image, seed=1):
    """(ids (F,N,1), scores (F,N,1), bboxes (F,N,4)) float32, frames in (clip, frame) order, rows by score descending as the
    network's NMS leaves them, -1 rows behind; N = the fullest frame's rows"""
    from vid_metric_probe import detections
    rows = detections(ds, per_image, seed)
    at = {sid: i for i, sid in enumerate(ds.get_sample_ids())}
    per = [[] for _ in at]
    for r in rows:
        per[at[r[0]]].append(r[1:])
    N = max(len(p) for p in per)
    if N > 128:
        raise SystemExit("a frame holds %d rows, vd_seq_nms takes 128" % N)
    F = len(per)
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    for t, p in enumerate(per):
        p.sort(key=lambda r: -r[1])
        for i, r in enumerate(p):
            ids[t, i, 0], scores[t, i, 0], bboxes[t, i] = r[0], r[1], r[2:6]
    return ids, scores, bboxes


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
    from viddet_amd.seq_nms import seq_nms_host
    ids, scores, bboxes = clip_arrays(ds, per_image)
    F, N = bboxes.shape[:2]
    T, C = a.frames, len(ds.classes)
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    ws = torch.empty(48 * F * N, dtype=torch.uint8, device="cuda")
    dcs = torch.tensor(cs, dtype=torch.int32, device="cuda")
    call = lambda stages=None: ops.seq_nms(*dv, clip_start=dcs, num_class=C, ws=ws, stages=stages)
    hc = min(a.host_clips, a.clips)
    head = [x[:hc * T] for x in (ids, scores, bboxes)]
    th, full, s1, s3 = [], [], [], []
    stats = {}
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t0 = time.perf_counter()
        want = seq_nms_host(*head, clip_start=cs[:hc + 1], num_class=C, stats=stats)
        th.append((time.perf_counter() - t0) / hc)
        full.append(_event_ms(call, a.reps))
        s1.append(_event_ms(lambda: call(1), a.reps))
        s3.append(_event_ms(lambda: call(3), a.reps))
    got = call()
    torch.cuda.synchronize()
    same = all(np.array_equal(g[:hc * T].cpu().numpy(), w) for g, w in zip(got, want))
    med = statistics.median
    return dict(what="seq_nms", clips=a.clips, frames=T, rows_per_frame=N, classes=C,
                detections_per_frame=round(float((ids >= 0).sum()) / F, 1), host_clips=hc,
                host_rounds_per_clip=round(stats["rounds"] / hc, 1), host_s_per_clip=[round(t, 4) for t in th],
                host_median_s_per_clip=round(med(th), 4), device_ms_per_call=[round(t, 4) for t in full],
                device_median_ms_per_call=round(med(full), 4), device_median_ms_per_clip=round(med(full) / a.clips, 5),
                launches_ms=dict(link=round(med(s1), 4), rounds=round(med(s3) - med(s1), 4), sort=round(med(full) - med(s3), 4)),
                same_result=bool(same))


def share(a, ds):
    """one clip through net.detect_video (random weights: the rows the untrained heads let through) with and without Seq-NMS"""
    from viddet_amd import ops
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(ds.classes, k=3, k_join_type="max", k_join_pos="early")
    net.initialize(init="he", obj_bias=-2.0)
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(a.frames, 3, a.size, a.size, generator=g).cuda()

    def run(seq):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = net.detect_video(x, chunk=8, seq_nms=seq)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    run(None), run(True)                                           # plans, tuning, code objects
    tp, ts = [], []
    for _ in range(a.blocks):
        tp.append(run(None)[0])
        ts.append(run(True)[0])
    plain = [t.clone() for t in run(None)[1]]
    C = len(ds.classes)
    k_ms = _event_ms(lambda: ops.seq_nms(*plain, num_class=C), a.reps)
    med = statistics.median
    return dict(what="detect_video", frames=a.frames, size=a.size, rows_per_frame=int(plain[0].shape[1]),
                detections_per_frame=round(float((plain[0] >= 0).sum()) / a.frames, 1),
                plain_s=[round(t, 4) for t in tp], with_seq_nms_s=[round(t, 4) for t in ts], plain_median_s=round(med(tp), 4),
                with_seq_nms_median_s=round(med(ts), 4), seq_nms_ms_per_call=round(k_ms, 4),
                seq_nms_share_of_plain=round(k_ms / 1e3 / med(tp), 5))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one probe each")
    ap.add_argument("--host_clips", type=int, default=1)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no_share", action="store_true", help="skip the detect_video part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/seq_nms_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("vid", num_videos=a.clips, frames_per_video=a.frames)

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for n in [int(s) for s in a.dets.split(",")]:
        emit(probe(a, ds, n))
    if not a.no_share:
        emit(share(a, ds))


if __name__ == "__main__":
    main()
