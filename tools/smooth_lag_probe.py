#!/usr/bin/env python
"""Developer tool: fixed-lag smoothing of track boxes in live sessions on the device (vd_track_smooth_push, ops.SmoothLagState,
DESIGN.md 40) beside the fixed-interval smoother on the same rows, a live session with and without the option, and what a lag
buys in box quality.

In ONE process:

  kernel   on SyntheticTracks, one clip of --frames (64) frames with about --dets (10,100) synthetic detections per frame
           (tools/seq_nms_probe.py's), linked by the online SORT tracker at max_age 7: vd_track_smooth_push ms per push of 1
           and of 8 frames and summed over the clip, at lag 1, 4 and 15 (a SmoothLagState over the clip's rows, the flush
           included in each pass; device events over whole passes) beside vd_track_smooth on the whole clip
  session  one clip of --frames random frames at --size (416), K = 3 (max join, early), random weights: frames/s of a session
           with track=byte online fed --push (1) frame(s) at a time and flushed, without the option and with smooth={'lag': 4}:
           wall time around a synchronize
  quality  tools/track_probe.py's jittered case (the ground truth jittered by --jitter, a share --drop of the rows left out,
           16 clips side by side as 16 streams of one launch, SORT online at max_age 7): LocA / HOTA / MOTP / COCO AP on the
           plain boxes, at lag 0, 1, 2, 4, 8 and 15, and on the full smoother's boxes

alternating blocks, median of --blocks.  The device's rows are compared with smooth_lag_host (kernel: the clip fed all at once
and a frame at a time) on the way: that they are equal is the pass condition, no speed or quality is asked for.  Needs a GPU:
there is no fallback.  Prints one JSON line per measurement."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from seq_nms_probe import _event_ms, clip_arrays

med = statistics.median
LAGS = (1, 4, 15)
QUALITY_LAGS = (0, 1, 2, 4, 8, 15)


def _same(got, want):
    return bool(np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and
                np.array_equal(got[1].cpu().numpy(), want[1]))


def kernel(a, ds, per_image):
    from viddet_amd import ops
    from viddet_amd.smooth_lag import smooth_lag_host
    T, C = a.frames, len(ds.classes)
    ids, scores, bboxes = [torch.from_numpy(x[:T]).cuda() for x in clip_arrays(ds, per_image)]
    N = bboxes.shape[1]
    track = ops.KalmanTrackState(1, N, C, method="sort", max_age=7).push(ids, scores, bboxes)[0]
    rows = (ids, scores, bboxes, track)
    parts = {p: [[t[i:i + p].contiguous() for t in rows] for i in range(0, T, p)] for p in (1, 8)}
    states = {lag: ops.SmoothLagState(1, N, C, lag=lag) for lag in LAGS}
    offline = lambda: ops.smooth(ids, scores, bboxes, track, num_class=C, max_gap=7)

    def clip(lag, p):
        st = states[lag]
        outs = [st.push(*f)[1:] for f in parts[p]]
        outs.append(st.flush()[1:])
        return outs

    ms = {(lag, p): [] for lag in LAGS for p in parts}
    full = []
    for _ in range(a.blocks):                                      # alternating blocks in one process
        for lag, p in ms:
            ms[lag, p].append(_event_ms(lambda: clip(lag, p), a.reps) / len(parts[p]))
        full.append(_event_ms(offline, a.reps))
    same = True
    host = [t.cpu().numpy() for t in rows]
    for lag in LAGS:
        want = smooth_lag_host(None, *host, C, lag, 7, flush=True)[2:]
        for p in parts:
            same = same and _same([torch.cat(t) for t in zip(*clip(lag, p))], want)
    slen = offline()[1]
    out = dict(what="kernel", frames=T, rows_per_frame=N, classes=C, max_gap=7,
               detections_per_frame=round(float((ids >= 0).sum()) / T, 1), members=int((slen > 0).sum()),
               offline_ms_per_clip=round(med(full), 4), offline_kernel="vd_track_smooth", same_result=bool(same))
    for lag in LAGS:
        out["lag_%d" % lag] = dict(push1_ms_per_push=round(med(ms[lag, 1]), 4), push8_ms_per_push=round(med(ms[lag, 8]), 4),
                                   push1_ms_per_clip=round(med(ms[lag, 1]) * len(parts[1]), 4),
                                   push8_ms_per_clip=round(med(ms[lag, 8]) * len(parts[8]), 4))
    return out


def session(a):
    from viddet_amd.model import yolo3_darknet53
    from viddet_amd.smooth_lag import smooth_lag_host
    net = yolo3_darknet53(["c%d" % i for i in range(30)], k=3, k_join_type="max", k_join_pos="early")
    net.initialize(init="he", obj_bias=-2.0)
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    x = torch.randn(a.frames, 3, a.size, a.size, generator=torch.Generator().manual_seed(3)).cuda()
    T, chunk, lag = x.shape[0], 8, 4
    sc = net.detect_video(x, chunk=chunk)[1]
    sd = float(sc[sc >= 0].median())                               # untrained heads score low: the split at the rows' median
    trk = dict(method="byte", online=True, sigma_l=0.0, sigma_d=sd, sigma_new=sd, sigma_h=0.0, clip=a.size)
    sessions = dict(plain=net.open_video(chunk=chunk, track=trk), lagged=net.open_video(chunk=chunk, track=trk, smooth={"lag": lag}))

    def live(s):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = []
        for i in range(0, T, a.push):
            out = s.push(x[i:i + a.push])
            rows.append(out[1:] + (s.last_tracks[0], s.last_pre_smooth, s.last_smooth))
        out = s.flush()
        rows.append(out[1:] + (s.last_tracks[0], s.last_pre_smooth, s.last_smooth))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, rows

    for s in sessions.values():
        live(s)                                                    # plans, tuning, code objects
    ts = {k: [] for k in sessions}
    for _ in range(a.blocks):                                      # alternating blocks in one process
        for k, s in sessions.items():
            ts[k].append(live(s)[0])
    ids, scores, sbox, track, pre, slen = [torch.cat(t) for t in zip(*live(sessions["lagged"])[1])]
    want = smooth_lag_host(None, ids.cpu().numpy(), scores.cpu().numpy(), pre.cpu().numpy(), track.cpu().numpy(), 30, lag, 7,
                           flush=True)[2:]
    return dict(what="session", method="byte", lag=lag, frames=T, size=a.size, K=3, chunk=chunk, push=a.push,
                rows_per_frame=int(ids.shape[1]), smoothed_rows=int((slen >= 2).sum()),
                plain_s=[round(t, 4) for t in ts["plain"]], lagged_s=[round(t, 4) for t in ts["lagged"]],
                plain_frames_per_s=round(T / med(ts["plain"]), 1), lagged_frames_per_s=round(T / med(ts["lagged"]), 1),
                same_result=_same((sbox, slen), want))


def quality(a, ds):
    """tools/track_probe.py's case - the ground truth, jittered and thinned - as one stream per clip through the online SORT
    tracker and the fixed-lag smoother: the tracking and detection metrics on the plain boxes, at every lag, and on the
    fixed-interval smoother's boxes"""
    from viddet_amd import ops
    from viddet_amd.coco_metric import COCODetectionMetric
    from viddet_amd.hota_metric import HOTAMetric
    from viddet_amd.mot_metric import MOTMetric
    from viddet_amd.smooth_lag import smooth_lag_host
    from viddet_amd.track import finalize_tracks
    rng = np.random.default_rng(7)
    T, V, C = ds.frames_per_video, ds.num_videos, len(ds.classes)
    sids = list(ds.get_sample_ids())
    labels = [ds.get_label(sid) for sid in sids]
    N = max(1, max(len(l) for l in labels))
    F = len(labels)
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    for t, l in enumerate(labels):
        keep = l[rng.uniform(size=len(l)) >= a.drop]
        wh = np.stack([keep[:, 2] - keep[:, 0], keep[:, 3] - keep[:, 1]] * 2, axis=1)
        n = len(keep)
        ids[t, :n, 0], scores[t, :n, 0], bboxes[t, :n] = keep[:, 4], 0.9, keep[:, :4] + rng.normal(0.0, a.jitter, (n, 4)) * wh
    dv = [torch.from_numpy(x.reshape((V, T) + x.shape[1:])).cuda() for x in (ids, scores, bboxes)]     # a stream per clip
    online = ops.KalmanTrackState(V, N, C, method="sort", max_age=7).push(*dv)
    track = online[0]
    final = np.concatenate([finalize_tracks(*[o[v].cpu().numpy() for o in online[:3]])[0] for v in range(V)])
    on = ids[..., 0] >= 0

    def lagged(lag):
        st = ops.SmoothLagState(V, N, C, lag=lag)
        first, rest = st.push(*dv, track)[1:], st.flush()[1:]
        return [torch.cat(t, dim=1) for t in zip(first, rest)]

    def metrics(boxes):
        hota, mot = HOTAMetric(ds), MOTMetric(ds, iou_thresh=0.5)
        with tempfile.TemporaryDirectory() as tmp:
            coco = COCODetectionMetric(ds, os.path.join(tmp, "coco"), use_time=False, cleanup=True, data_shape=None)
            for t, sid in enumerate(sids):
                k = on[t]
                args = ([[boxes[t, k]]], [[ids[t, k, 0]]], [[scores[t, k, 0]]], None, None, None)
                hota.update(*args, sid=sid, tracks=[[final[t, k]]])
                mot.update(*args, sid=sid, tracks=[[final[t, k]]])
                coco.update(*args, sid=sid)
            text = coco.get()[1][0]
            del coco                                               # its clean-up, while the directory is still there
        out = {}
        for metric, keys in ((hota, ("LocA", "HOTA")), (mot, ("MOTP",))):
            table = dict(zip(*metric.get()))
            out.update({key: round(float(table[key]), 4) for key in keys if key in table})
        m = re.search(r"IoU=0\.50:0\.95 \| area=\s*all \| maxDets=100 \] = (-?[\d.]+)", text)
        out["AP"] = float(m.group(1)) if m else None
        return out

    table = dict(plain=metrics(bboxes))
    same = True
    for lag in QUALITY_LAGS:
        got = lagged(lag)
        table["lag_%d" % lag] = metrics(got[0].cpu().numpy().reshape(F, N, 4))
        want = smooth_lag_host(None, *[x[:T] for x in (ids, scores, bboxes)], track[0].cpu().numpy(), C, lag, 7, flush=True)[2:]
        same = same and _same((got[0][0], got[1][0]), want)        # the first stream against the definition
    full = ops.smooth(*[t.reshape((F,) + tuple(t.shape[2:])) for t in dv], track.reshape(F, N),
                      clip_start=list(range(0, F + 1, T)), num_class=C, max_gap=7)
    table["full"] = metrics(full[0].cpu().numpy())
    return dict(what="quality", clips=V, frames=T, jitter=a.jitter, drop=a.drop, max_age=7, rows=int(on.sum()),
                rows_tracked=int((final >= 0).sum()), table=table, same_result=bool(same))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one probe each")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--push", type=int, default=1, help="session: frames per push")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=0.04, help="quality: sigma of the box noise, as a share of the box's size")
    ap.add_argument("--drop", type=float, default=0.1, help="quality: the share of ground-truth rows left out")
    ap.add_argument("--quality_clips", type=int, default=16)
    ap.add_argument("--skip_session", action="store_true")
    ap.add_argument("--no_quality", action="store_true", help="skip the quality part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/smooth_lag_probe.py needs an MI355X: a timing taken elsewhere says nothing")
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
        emit(kernel(a, ds, n))
    if not a.skip_session:
        emit(session(a))
    if not a.no_quality:
        emit(quality(a, SyntheticTracks("vid", num_videos=a.quality_clips, frames_per_video=a.frames)))
    if not all(d["same_result"] for d in results):
        raise SystemExit("the device's rows differ from smooth_lag_host's")


if __name__ == "__main__":
    main()
