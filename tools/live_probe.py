#!/usr/bin/env python
"""Developer tool: a live video session (net.open_video) against net.detect_video on the same clip.

In ONE process, on one clip of --frames (64) random frames at --size (416), K = 3 (max join, early), random weights:

  throughput  frames/s of detect_video(clip, chunk) and of a session fed --push (1) frame(s) at a time and flushed, at every
              --chunks (8,1): wall time around a synchronize
  latency     seconds per session.push (a synchronize behind each), median and maximum over the clip: a push that completes
              a launch group pays for it, the others only copy their frame
  tracker     vd_track_push ms per push of 1 and of 8 frames (a TrackState over the clip's detections, device events over whole
              passes) beside vd_track on the whole clip

alternating blocks, median of --blocks.  The session's tensors are compared with detect_video's, and the online tracker's rows,
decided by finalize_tracks, with vd_track's, on the way: that they are equal is the pass condition, no speed is asked for.
Needs a GPU: there is no fallback.  Prints one JSON line per measurement."""
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

import torch

from seq_nms_probe import _event_ms

med = statistics.median


def _session_clip(session, x, push, times=None):
    outs, rows = [], []
    for a in range(0, x.shape[0], push):
        if times is not None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        outs.append(session.push(x[a:a + push])[1:])
        if times is not None:
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        rows.append(session.last_rows)
    outs.append(session.flush()[1:])
    rows.append(session.last_rows)
    return [torch.cat(t) for t in zip(*outs)] + [torch.cat(rows)]


def throughput(a, net, x, chunk):
    T = x.shape[0]
    session = net.open_video(chunk=chunk)

    def whole():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = net.detect_video(x, chunk=chunk)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, list(out) + [net.last_rows]

    def live(times=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = _session_clip(session, x, a.push, times)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    whole(), live()                                                # plans, tuning, code objects
    tw, tl, lat = [], [], []
    for _ in range(a.blocks):                                      # alternating blocks in one process
        tw.append(whole()[0])
        tl.append(live()[0])
    for _ in range(a.blocks):
        per = []
        live(per)
        lat.append(per)
    want, got = whole()[1], live()[1]
    same = all(torch.equal(g, w) for g, w in zip(got, want)) and session.stream_stats == net.stream_stats
    return dict(what="session", frames=T, size=a.size, K=3, chunk=chunk, push=a.push,
                detect_video_s=[round(t, 4) for t in tw], session_s=[round(t, 4) for t in tl],
                detect_video_frames_per_s=round(T / med(tw), 1), session_frames_per_s=round(T / med(tl), 1),
                push_median_ms=round(1e3 * med([med(p) for p in lat]), 3), push_max_ms=round(1e3 * med([max(p) for p in lat]), 3),
                same_result=bool(same))


def tracker(a, net, x):
    from viddet_amd import ops
    from viddet_amd.track import finalize_tracks
    plain = [t.clone() for t in net.detect_video(x, chunk=8)]
    T, N = plain[2].shape[:2]
    C = net.num_class
    state = ops.TrackState(1, N, C)
    parts = {p: [[t[i:i + p].contiguous() for t in plain] for i in range(0, T, p)] for p in (1, 8)}

    def clip(p):
        state.reset()
        return [state.push(*f) for f in parts[p]]

    ms = {p: [] for p in parts}
    full = []
    for _ in range(a.blocks):
        for p in parts:
            ms[p].append(_event_ms(lambda: clip(p), a.reps) / len(parts[p]))
        full.append(_event_ms(lambda: ops.track(*plain, num_class=C), a.reps))
    want = ops.track(*plain, num_class=C)
    same = True
    for p in parts:
        online = [torch.cat(t).cpu().numpy() for t in zip(*clip(p))]
        final = finalize_tracks(*online)
        same = same and all(torch.equal(torch.from_numpy(f), w.cpu()) for f, w in zip(final, want))
    return dict(what="tracker", frames=T, rows_per_frame=N, detections_per_frame=round(float((plain[0] >= 0).sum()) / T, 1),
                push1_ms_per_push=round(med(ms[1]), 4), push8_ms_per_push=round(med(ms[8]), 4),
                push1_ms_per_clip=round(med(ms[1]) * len(parts[1]), 4), push8_ms_per_clip=round(med(ms[8]) * len(parts[8]), 4),
                vd_track_ms_per_clip=round(med(full), 4), same_result=bool(same))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--chunks", default="8,1", help="one probe each")
    ap.add_argument("--push", type=int, default=1, help="frames per session.push")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/live_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(30)], k=3, k_join_type="max", k_join_pos="early")
    net.initialize(init="he", obj_bias=-2.0)
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    x = torch.randn(a.frames, 3, a.size, a.size, generator=torch.Generator().manual_seed(3)).cuda()
    results = []

    def emit(d):
        results.append(d)
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for chunk in [int(s) for s in a.chunks.split(",")]:
        emit(throughput(a, net, x, chunk))
    emit(tracker(a, net, x))
    if not all(d["same_result"] for d in results):
        raise SystemExit("the session's result differs from detect_video's")


if __name__ == "__main__":
    main()
