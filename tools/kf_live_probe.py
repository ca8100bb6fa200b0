#!/usr/bin/env python
"""Developer tool: SORT and BYTE carried from push to push on the device (vd_track_kf_push, ops.KalmanTrackState)
beside the offline kernels on the same detections, and a live session that carries BYTE beside net.detect_video(track=byte).

In ONE process:

  tracker  on SyntheticTracks, one clip of --frames (64) frames with about --dets (10,100) synthetic detections per frame
           (tools/seq_nms_probe.py's; their scores are drawn, so both of BYTE's associations have rows), for `sort` and `byte` at
           their default parameters: vd_track_kf_push ms per push of 1 and of 8 frames and summed over the clip (a
           KalmanTrackState over the clip's detections, a reset() included in each pass; device events over whole passes) beside
           vd_track_sort / vd_track_byte on the whole clip
  session  one clip of --frames random frames at --size (416), K = 3 (max join, early), random weights: frames/s of
           detect_video(clip, chunk 8, track=byte) and of a session with track={'method': 'byte', 'online': True} fed --push (1)
           frame(s) at a time and flushed: wall time around a synchronize

alternating blocks, median of --blocks.  The online rows, decided by finalize_tracks, are compared with the offline kernel's
result and with detect_video's last_tracks / last_track_boxes on the way: that they are equal is the pass condition, no speed is
asked for.  Needs a GPU: there is no fallback.  Prints one JSON line per measurement."""
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

from seq_nms_probe import _event_ms, clip_arrays

med = statistics.median
DECIDE = ("sigma_h", "t_min")


def _bits(a, b):
    return all(torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32)) for x, y in zip(a, b))


def _final(rows, decide):
    from viddet_amd.track import finalize_tracks
    final = finalize_tracks(*[r.cpu().numpy() for r in rows[:3]], tbox=rows[3].cpu().numpy(), **decide)
    return [torch.from_numpy(f) for f in final]


def tracker(a, ds, per_image, method):
    from viddet_amd import ops
    if method == "sort":
        from viddet_amd.sort import DEFAULTS
    else:
        from viddet_amd.byte import DEFAULTS
    T, C = a.frames, len(ds.classes)
    ids, scores, bboxes = [torch.from_numpy(x[:T]).cuda() for x in clip_arrays(ds, per_image)]
    N = bboxes.shape[1]
    okw = {k: v for k, v in DEFAULTS.items() if k not in DECIDE}
    state = ops.KalmanTrackState(1, N, C, method=method, **okw)
    parts = {p: [[t[i:i + p].contiguous() for t in (ids, scores, bboxes)] for i in range(0, T, p)] for p in (1, 8)}
    link = ops.track_sort if method == "sort" else ops.track_byte
    offline = lambda: link(ids, scores, bboxes, num_class=C, **DEFAULTS)

    def clip(p):
        state.reset()
        return [state.push(*f) for f in parts[p]]

    ms = {p: [] for p in parts}
    full = []
    for _ in range(a.blocks):                                      # alternating blocks in one process
        for p in parts:
            ms[p].append(_event_ms(lambda: clip(p), a.reps) / len(parts[p]))
        full.append(_event_ms(offline, a.reps))
    want = offline()
    same = True
    for p in parts:
        rows = [torch.cat(t) for t in zip(*clip(p))]
        same = same and _bits(_final(rows, {k: DEFAULTS[k] for k in DECIDE}), want)
    return dict(what="tracker", method=method, frames=T, rows_per_frame=N, classes=C, max_age=DEFAULTS["max_age"],
                detections_per_frame=round(float((ids >= 0).sum()) / T, 1), kept_rows=int((want[0] >= 0).sum()),
                push1_ms_per_push=round(med(ms[1]), 4), push8_ms_per_push=round(med(ms[8]), 4),
                push1_ms_per_clip=round(med(ms[1]) * len(parts[1]), 4), push8_ms_per_clip=round(med(ms[8]) * len(parts[8]), 4),
                offline_ms_per_clip=round(med(full), 4), offline_kernel="vd_track_" + method, same_result=bool(same))


def session(a):
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(30)], k=3, k_join_type="max", k_join_pos="early")
    net.initialize(init="he", obj_bias=-2.0)
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    x = torch.randn(a.frames, 3, a.size, a.size, generator=torch.Generator().manual_seed(3)).cuda()
    T, chunk = x.shape[0], 8
    sc = net.detect_video(x, chunk=chunk)[1]
    sd = float(sc[sc >= 0].median())                               # untrained heads score low: the split at the rows' median
    trk = dict(method="byte", sigma_l=0.0, sigma_d=sd, sigma_new=sd, sigma_h=0.0, clip=a.size)
    live_session = net.open_video(chunk=chunk, track=dict(trk, online=True))

    def whole():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.detect_video(x, chunk=chunk, track=trk)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, list(net.last_tracks) + [net.last_track_boxes]

    def live():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = []
        for i in range(0, T, a.push):
            live_session.push(x[i:i + a.push])
            rows.append(live_session.last_tracks + (live_session.last_track_boxes,))
        live_session.flush()
        rows.append(live_session.last_tracks + (live_session.last_track_boxes,))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, [torch.cat(t) for t in zip(*rows)]

    whole(), live()                                                # plans, tuning, code objects
    tw, tl = [], []
    for _ in range(a.blocks):                                      # alternating blocks in one process
        tw.append(whole()[0])
        tl.append(live()[0])
    want, rows = whole()[1], live()[1]
    same = _bits(_final(rows, live_session.track_decide), want)
    return dict(what="session", method="byte", frames=T, size=a.size, K=3, chunk=chunk, push=a.push,
                rows_per_frame=int(rows[0].shape[1]), candidate_rows=int((rows[0] >= 0).sum()), kept_rows=int((want[0] >= 0).sum()),
                detect_video_s=[round(t, 4) for t in tw], session_s=[round(t, 4) for t in tl],
                detect_video_frames_per_s=round(T / med(tw), 1), session_frames_per_s=round(T / med(tl), 1), same_result=bool(same))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one probe each")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--push", type=int, default=1, help="session: frames per push")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip_session", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/kf_live_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("vid", num_videos=1, frames_per_video=a.frames)
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
        for method in ("sort", "byte"):
            emit(tracker(a, ds, n, method))
    if not a.skip_session:
        emit(session(a))
    if not all(d["same_result"] for d in results):
        raise SystemExit("the online rows, decided at the clip's end, differ from the offline result")


if __name__ == "__main__":
    main()
