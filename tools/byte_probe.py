#!/usr/bin/env python
"""Developer tool: BYTE on the device (vd_track_byte, ops.track_byte) against its host definition and beside SORT
(vd_track_sort) on the same detections: what the second association costs, and what it buys.

In ONE process, on SyntheticTracks at --clips (64) x --frames (64) with about --dets (10,100) synthetic detections per frame
(tools/seq_nms_probe.py's; their scores are drawn, so both associations have rows), at every --max_age (1,7):

  host     byte_host seconds per clip, on the first --host_clips clips
  device   vd_track_byte ms per call over ALL clips at once (device events, --reps calls), and vd_track_sort on the same rows at
           the same sigma_l, sigma_iou and max_age (it sees the high and the low rows in ONE assignment)
  quality  a case built on tools/track_probe.py's - the ground-truth rows at score 0.9 with boxes jittered by --jitter (4 %) of
           their size and --drop (10 %) of the rows dropped - in which a seeded share --dip (30 %) of each object's rows has its
           score lowered below sigma_d (to 0.15 ... 0.45) in runs of 1 to 3 frames, and two clutter boxes a frame scored
           0.15 ... 0.45 are added; linked by `byte` and by `sort` at sigma_l 0.1 and at sigma_l = sigma_d 0.5 (the same
           sigma_iou and max_age), scored by MOTMetric and HOTAMetric

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

from mot_probe import _results
from seq_nms_probe import _event_ms, clip_arrays
from sort_probe import _same


def probe(a, ds, per_image, max_age):
    from viddet_amd import lib as L, ops
    from viddet_amd.byte import DEFAULTS, byte_host
    ids, scores, bboxes = clip_arrays(ds, per_image)
    F, N = bboxes.shape[:2]
    T, C = a.frames, len(ds.classes)
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    ws = torch.empty(L.TRACK_SORT_WS_PER_ROW * F * N + L.TRACK_SORT_WS_PER_CLIP * a.clips, dtype=torch.uint8, device="cuda")
    dcs = torch.tensor(cs, dtype=torch.int32, device="cuda")
    call = lambda: ops.track_byte(*dv, clip_start=dcs, num_class=C, max_age=max_age, ws=ws)
    sort_call = lambda: ops.track_sort(*dv, clip_start=dcs, num_class=C, max_age=max_age, sigma_l=DEFAULTS["sigma_l"],
                                       sigma_iou=DEFAULTS["sigma_iou"], ws=ws)
    hc = min(a.host_clips, a.clips)
    head = [x[:hc * T] for x in (ids, scores, bboxes)]
    th, full, sort_full = [], [], []
    stats = {}
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t0 = time.perf_counter()
        want = byte_host(*head, clip_start=cs[:hc + 1], num_class=C, max_age=max_age, stats=stats)
        th.append((time.perf_counter() - t0) / hc)
        full.append(_event_ms(call, a.reps))
        sort_full.append(_event_ms(sort_call, a.reps))
    got = call()
    torch.cuda.synchronize()
    med = statistics.median
    sc = scores[ids >= 0]
    return dict(what="track_byte", clips=a.clips, frames=T, rows_per_frame=N, classes=C, max_age=max_age,
                detections_per_frame=round(float((ids >= 0).sum()) / F, 1),
                high_rows_per_frame=round(float((sc >= DEFAULTS["sigma_d"]).sum()) / F, 1),
                low_rows_per_frame=round(float(((sc >= DEFAULTS["sigma_l"]) & (sc < DEFAULTS["sigma_d"])).sum()) / F, 1), host_clips=hc,
                host_most_active=int(stats["active"].max()), host_tracks_per_clip=round(sum(stats["tracks"]) / hc, 1),
                host_first_pairs_per_frame=round(float(stats["first"][:hc * T].mean()), 2),
                host_second_pairs_per_frame=round(float(stats["second"][:hc * T].mean()), 2),
                host_s_per_clip=[round(t, 4) for t in th], host_median_s_per_clip=round(med(th), 4),
                device_ms_per_call=[round(t, 4) for t in full], device_median_ms_per_call=round(med(full), 4),
                device_median_ms_per_clip=round(med(full) / a.clips, 5),
                vd_track_sort_ms_per_call=[round(t, 4) for t in sort_full], vd_track_sort_median_ms_per_call=round(med(sort_full), 4),
                same_result=_same(got, want, hc * T))


def dipped_case(a, ds):
    """tools/track_probe.py's jittered, thinned ground truth with score dips per object and two low-score clutter boxes a frame"""
    rng = np.random.default_rng(7)
    T = ds.frames_per_video
    labels = [ds.get_label(sid) for sid in ds.get_sample_ids()]
    F = len(labels)
    N = max(1, max(len(l) for l in labels)) + 2
    extent = max(float(l[:, :4].max()) for l in labels if len(l))
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    run = {}                                                       # (clip, ground-truth track) -> (the frame its last dip ends before, its score)
    dips = 0
    for t, l in enumerate(labels):
        clip, frame = divmod(t, T)
        rows = []
        for r in l[rng.uniform(size=len(l)) >= a.drop]:
            wh = np.array([r[2] - r[0], r[3] - r[1]] * 2)
            key = (clip, int(r[5]))
            end, s = run.get(key, (0, 0.9))
            # a run starts with probability dip / 2 and lasts 1 to 3 frames, 2 on average: a share of about `dip` of the rows;
            # the frame behind a run and a clip's first frame stay high
            if frame > end and rng.uniform() < a.dip / 2.0:
                end, s = frame + int(rng.integers(1, 4)), float(rng.uniform(0.15, 0.45))
                run[key] = (end, s)
            score = s if frame < end else 0.9
            dips += score < 0.5
            rows.append((score, r[4], r[:4] + rng.normal(0.0, a.jitter, 4) * wh))
        for _ in range(2):                                         # clutter
            xy, wh = rng.uniform(0.0, extent * 0.8, 2), rng.uniform(extent * 0.05, extent * 0.2, 2)
            rows.append((float(rng.uniform(0.15, 0.45)), float(rng.integers(0, len(ds.classes))), np.concatenate([xy, xy + wh])))
        rows.sort(key=lambda r: -r[0])                             # by score descending, as the network's NMS leaves them
        for i, (s, c, b) in enumerate(rows):
            ids[t, i, 0], scores[t, i, 0], bboxes[t, i] = c, s, b
    return ids, scores, bboxes, int(dips)


def quality(a, ds, max_age):
    from viddet_amd import ops
    from viddet_amd.byte import DEFAULTS, byte_host
    from viddet_amd.hota_metric import HOTAMetric
    from viddet_amd.mot_metric import MOTMetric
    ids, scores, bboxes, dips = dipped_case(a, ds)
    F, T = len(ids), ds.frames_per_video
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    kw = dict(clip_start=cs, num_class=len(ds.classes), max_age=max_age)
    got = ops.track_byte(*dv, **kw)
    stats = {}
    same = _same(got, byte_host(ids, scores, bboxes, stats=stats, **kw), F)
    out = dict(what="quality", clips=ds.num_videos, frames=T, max_age=max_age, jitter=a.jitter, drop=a.drop, dip=a.dip,
               dipped_rows=dips, clutter_rows=2 * F, second_pairs=int(stats["second"].sum()), same_result=same)
    si = DEFAULTS["sigma_iou"]
    links = dict(byte=got[0], sort_at_sigma_l_0_1=ops.track_sort(*dv, sigma_l=DEFAULTS["sigma_l"], sigma_iou=si, **kw)[0],
                 sort_at_sigma_l_sigma_d=ops.track_sort(*dv, sigma_l=DEFAULTS["sigma_d"], sigma_iou=si, **kw)[0])
    for name, track in links.items():
        results = _results(ds, ids, scores, bboxes, track.cpu().numpy())
        mot, hota = MOTMetric(ds), HOTAMetric(ds)
        mot._results, hota._results = results, results
        mot.get(), hota.get()
        s, h = mot.summary["all"], hota.summary["all"]
        out[name] = dict(MOTA=round(s["MOTA"], 4), IDF1=round(s["IDF1"], 4), IDSW=s["IDSW"], Frag=s["Frag"], TP=s["TP"], FN=s["FN"],
                         FP=s["FP"], MT=s["MT"], PT=s["PT"], ML=s["ML"], HOTA=round(h["HOTA"], 4), DetA=round(h["DetA"], 4),
                         AssA=round(h["AssA"], 4))
    out["GT"], out["ground_truth_tracks"] = s["GT"], s["gt_tracks"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one probe each")
    ap.add_argument("--max_age", default="1,7", help="one probe each")
    ap.add_argument("--host_clips", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=0.04, help="quality: sigma of the box noise, as a share of the box's size")
    ap.add_argument("--drop", type=float, default=0.1, help="quality: the share of ground-truth rows left out")
    ap.add_argument("--dip", type=float, default=0.3, help="quality: the share of an object's rows whose score is lowered below sigma_d")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/byte_probe.py needs an MI355X: a timing taken elsewhere says nothing")
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

    ages = [int(s) for s in a.max_age.split(",")]
    for n in [int(s) for s in a.dets.split(",")]:
        for m in ages:
            emit(probe(a, ds, n, m))
    for m in ages:
        emit(quality(a, ds, m))
    if not all(d.get("same_result", True) for d in results):
        raise SystemExit("the device's result differs from byte_host's")


if __name__ == "__main__":
    main()
