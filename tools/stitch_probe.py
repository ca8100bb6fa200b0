#!/usr/bin/env python
"""Developer tool: the stitching pass on the device (vd_track_stitch, ops.stitch) against its host definition on the
same tracked detections.

In ONE process, on SyntheticTracks at --clips (64) x --frames (64) with about --dets (10,100) synthetic detections per frame
(tools/seq_nms_probe.py's), linked by ops.track_sort and by ops.track_byte at --max_age (1):

  host     stitch_host seconds per clip, on the first --host_clips clips
  device   vd_track_stitch ms per call over ALL clips at once (device events, --reps calls)
  widest   the all-against-all case: --wide_tracks (512) tracks of one row at one place, 128 a frame, so that every tail reaches
           every head of every later frame - the longest the assignment loop runs
  quality  on tools/track_probe.py's jittered case - the ground-truth rows at score 0.9 with boxes jittered by --jitter (4 %) of
           their size - with an occlusion run of 8 to 24 frames cut out of every object, linked by ops.track_sort at max_age 1
           and 7: MOTMetric (IDF1, id switches) and HOTAMetric (AssA, HOTA) on the tracker's ids against the stitched ones

alternating blocks, median of --blocks; the device result is compared with the host's on the host's clips on the way: that it
is equal is the pass condition, no speed or quality is asked for.  Needs a GPU: there is no fallback.  Prints one JSON line per
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

from seq_nms_probe import _event_ms, clip_arrays


def _same(got, want):
    return bool(all(np.array_equal(got[k], want[k]) for k in (0, 1, 3, 4)) and
                np.array_equal(np.ascontiguousarray(got[2]).view(np.int32), np.ascontiguousarray(want[2]).view(np.int32)))


def probe(a, ds, per_image, method):
    from viddet_amd import lib as L, ops
    from viddet_amd.stitch import stitch_host
    ids, scores, bboxes = clip_arrays(ds, per_image)
    F, N = bboxes.shape[:2]
    T, C = a.frames, len(ds.classes)
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    dcs = torch.tensor(cs, dtype=torch.int32, device="cuda")
    link = ops.track_sort if method == "sort" else ops.track_byte
    track = link(*dv, clip_start=dcs, num_class=C, max_age=a.max_age)[0]
    ws = torch.empty(L.TRACK_STITCH_WS_PER_ROW * F * N, dtype=torch.uint8, device="cuda")
    kw = dict(num_class=C, max_gap=a.max_gap, sigma_iou=a.sigma_iou)
    call = lambda: ops.stitch(*dv, track, clip_start=dcs, ws=ws, **kw)
    hc = min(a.host_clips, a.clips)
    head = [x[:hc * T] for x in (ids, scores, bboxes)] + [track.cpu().numpy()[:hc * T]]
    th, full = [], []
    stats = {}
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t0 = time.perf_counter()
        want = stitch_host(*head, clip_start=cs[:hc + 1], stats=stats, **kw)
        th.append((time.perf_counter() - t0) / hc)
        full.append(_event_ms(call, a.reps))
    got = [g.cpu().numpy() for g in call()]
    same = _same([g[:hc * T] for g in got[:3]] + [g[:hc] for g in got[3:]], want)
    med = statistics.median
    return dict(what="stitch", tracker=method, clips=a.clips, frames=T, rows_per_frame=N, classes=C, max_age=a.max_age,
                max_gap=a.max_gap, sigma_iou=a.sigma_iou, detections_per_frame=round(float((ids >= 0).sum()) / F, 1), host_clips=hc,
                host_tracks_per_clip=round(sum(stats["tracks"]) / hc, 1), host_pairs_per_clip=round(sum(stats["pairs"]) / hc, 1),
                host_links_per_clip=round(sum(stats["links"]) / hc, 1), links_all_clips=int(got[3].sum()),
                most_links_in_a_clip=int(got[3].max()), overflow_all_clips=int(got[4].sum()),
                host_s_per_clip=[round(t, 4) for t in th], host_median_s_per_clip=round(med(th), 4),
                device_ms_per_call=[round(t, 4) for t in full], device_median_ms_per_call=round(med(full), 4),
                device_median_ms_per_clip=round(med(full) / a.clips, 5), same_result=bool(same))


def wide_case(K):
    """K tracks of one row, 128 a frame, all of one class at one place (a jitter of a pixel tells their IoUs apart): every tail
    reaches every head of every later frame"""
    n = min(K, 128)
    F = -(-K // n)
    rng = np.random.default_rng(11)
    ids, scores = np.zeros((F, n, 1), np.float32), np.full((F, n, 1), 0.9, np.float32)
    xy = rng.uniform(0.0, 1.0, (F, n, 2))
    bboxes = np.concatenate([xy, xy + 40.0], axis=2).astype(np.float32)
    track = np.arange(F * n, dtype=np.int32).reshape(F, n)
    ids.reshape(-1)[K:], scores.reshape(-1)[K:], track.reshape(-1)[K:] = -1, -1, -1
    return ids, scores, bboxes, track


def widest(a):
    """the all-against-all case: one clip, one workgroup, the longest the assignment loop runs"""
    from viddet_amd import ops
    from viddet_amd.stitch import stitch_host
    case = wide_case(a.wide_tracks)
    dv = [torch.from_numpy(x).cuda() for x in case]
    kw = dict(max_gap=a.max_gap, sigma_iou=a.sigma_iou)
    call = lambda: ops.stitch(*dv, **kw)
    stats = {}
    t0 = time.perf_counter()
    want = stitch_host(*case, stats=stats, **kw)
    th = time.perf_counter() - t0
    full = [_event_ms(call, a.reps) for _ in range(a.blocks)]
    got = [g.cpu().numpy() for g in call()]
    return dict(what="widest", tracks=stats["tracks"][0], frames=case[3].shape[0], pairs=stats["pairs"][0], links=stats["links"][0],
                host_s=round(th, 4), device_ms_per_call=[round(t, 4) for t in full],
                device_median_ms_per_call=round(statistics.median(full), 4), same_result=_same(got, want))


def quality(a, ds, max_age):
    """tools/track_probe.py's case - the ground truth, jittered - with an occlusion of 8 to 24 frames cut out of every object,
    through SORT and the pass: the identity metrics on the tracker's ids and on the stitched ones"""
    from viddet_amd import ops
    from viddet_amd.hota_metric import HOTAMetric
    from viddet_amd.mot_metric import MOTMetric
    from viddet_amd.stitch import stitch_host
    rng = np.random.default_rng(7)
    T, V, C = ds.frames_per_video, ds.num_videos, len(ds.classes)
    sids = list(ds.get_sample_ids())
    labels = [ds.get_label(sid) for sid in sids]
    hidden = set()                                                 # (clip, ground-truth track, frame)
    for v in range(V):
        for g in np.unique(np.concatenate([l[:, 5] for l in labels[v * T:(v + 1) * T]])):
            n = int(rng.integers(8, 25))
            s = int(rng.integers(1, max(2, T - n)))
            hidden.update((v, int(g), t) for t in range(s, s + n))
    N = max(1, max(len(l) for l in labels))
    F = len(labels)
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    for t, l in enumerate(labels):
        keep = l[[(t // T, int(g), t % T) not in hidden for g in l[:, 5]]] if len(l) else l
        wh = np.stack([keep[:, 2] - keep[:, 0], keep[:, 3] - keep[:, 1]] * 2, axis=1)
        box = keep[:, :4] + rng.normal(0.0, a.jitter, (len(keep), 4)) * wh
        n = len(keep)
        ids[t, :n, 0], scores[t, :n, 0], bboxes[t, :n] = keep[:, 4], 0.9, box
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    track = ops.track_sort(*dv, clip_start=cs, num_class=C, max_age=max_age)[0]
    kw = dict(clip_start=cs, num_class=C, max_gap=a.max_gap, sigma_iou=a.sigma_iou)
    got = [g.cpu().numpy() for g in ops.stitch(*dv, track, **kw)]
    track = track.cpu().numpy()
    same = _same(got, stitch_host(ids, scores, bboxes, track, **kw))
    on = ids[..., 0] >= 0

    def metrics(tr):
        hota, mot = HOTAMetric(ds), MOTMetric(ds, iou_thresh=0.5)
        for t, sid in enumerate(sids):
            k = on[t]
            args = ([[bboxes[t, k]]], [[ids[t, k, 0]]], [[scores[t, k, 0]]], None, None, None)
            hota.update(*args, sid=sid, tracks=[[tr[t, k]]])
            mot.update(*args, sid=sid, tracks=[[tr[t, k]]])
        out = {}
        for metric, keys in ((mot, ("IDF1", "IDSW", "MOTA")), (hota, ("AssA", "HOTA", "DetA"))):
            table = dict(zip(*metric.get()))
            out.update({key: float(table[key]) for key in keys if key in table})
        return out

    return dict(what="quality", clips=V, frames=T, jitter=a.jitter, occlusion="8..24 frames of every object", max_age=max_age,
                max_gap=a.max_gap, sigma_iou=a.sigma_iou, rows=int(on.sum()), tracks=int(sum(len(np.unique(c[c >= 0])) for c in np.split(track, V))),
                links=int(got[3].sum()), table=dict(tracker=metrics(track), stitched=metrics(got[0])), same_result=bool(same))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one probe each")
    ap.add_argument("--trackers", default="sort,byte", help="the tracker that links the rows, one probe each")
    ap.add_argument("--max_age", type=int, default=1, help="the tracker's max_age in the timing part")
    ap.add_argument("--max_gap", type=int, default=30)
    ap.add_argument("--sigma_iou", type=float, default=0.3)
    ap.add_argument("--host_clips", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wide_tracks", type=int, default=512, help="widest: the tracks of the all-against-all case")
    ap.add_argument("--jitter", type=float, default=0.04, help="quality: sigma of the box noise, as a share of the box's size")
    ap.add_argument("--quality_max_age", default="1,7")
    ap.add_argument("--quality_clips", type=int, default=16)
    ap.add_argument("--no_quality", action="store_true", help="skip the quality part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/stitch_probe.py needs an MI355X: a timing taken elsewhere says nothing")
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
        for method in a.trackers.split(","):
            emit(probe(a, ds, n, method))
    emit(widest(a))
    if not a.no_quality:
        qds = SyntheticTracks("vid", num_videos=a.quality_clips, frames_per_video=a.frames)
        for m in [int(s) for s in a.quality_max_age.split(",")]:
            emit(quality(a, qds, m))
    if not all(d.get("same_result", True) for d in results):
        raise SystemExit("the device's result differs from stitch_host's")


if __name__ == "__main__":
    main()
