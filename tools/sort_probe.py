#!/usr/bin/env python
"""Developer tool: SORT on the device (vd_track_sort, ops.track_sort) against its host definition and beside the
IOU tracker (vd_track) on the same detections.

In ONE process, on SyntheticTracks at --clips (64) x --frames (64) with about --dets (10,100) synthetic detections per frame
(tools/seq_nms_probe.py's), at every --max_age (1,7):

  host     sort_host seconds per clip, on the first --host_clips clips
  device   vd_track_sort ms per call over ALL clips at once (device events, --reps calls), and vd_track on the same rows
  share    the call as a share of net.detect_video on one --frames clip at --size (416): detect_video with and without
           track={'method': 'sort'}, wall time around a synchronize
  quality  tools/track_probe.py's case - the ground-truth rows at score 0.9 with boxes jittered by --jitter (4 %) of their size
           and --drop (10 %) of the rows dropped - linked by either method and scored by MOTMetric: MOTA, IDF1, id switches,
           fragmentations of `iou` (at its own sigma_iou 0.5 and at SORT's 0.3) against `sort`

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


def _same(got, want, rows):
    ok = all(np.array_equal(g[:rows].cpu().numpy(), w) for g, w in zip(got[:3], want[:3]))
    g, w = got[3][:rows].cpu().numpy(), want[3]
    nan = np.isnan(w)
    return bool(ok and np.isnan(g[nan]).all() and np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan]))


def probe(a, ds, per_image, max_age):
    from viddet_amd import lib as L, ops
    from viddet_amd.sort import sort_host
    ids, scores, bboxes = clip_arrays(ds, per_image)
    F, N = bboxes.shape[:2]
    T, C = a.frames, len(ds.classes)
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    ws = torch.empty(L.TRACK_SORT_WS_PER_ROW * F * N + L.TRACK_SORT_WS_PER_CLIP * a.clips, dtype=torch.uint8, device="cuda")
    dcs = torch.tensor(cs, dtype=torch.int32, device="cuda")
    call = lambda: ops.track_sort(*dv, clip_start=dcs, num_class=C, max_age=max_age, ws=ws)
    iou_call = lambda: ops.track(*dv, clip_start=dcs, num_class=C, max_age=max_age, ws=ws)
    hc = min(a.host_clips, a.clips)
    head = [x[:hc * T] for x in (ids, scores, bboxes)]
    th, full, iou_full = [], [], []
    stats = {}
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t0 = time.perf_counter()
        want = sort_host(*head, clip_start=cs[:hc + 1], num_class=C, max_age=max_age, stats=stats)
        th.append((time.perf_counter() - t0) / hc)
        full.append(_event_ms(call, a.reps))
        iou_full.append(_event_ms(iou_call, a.reps))
    got = call()
    torch.cuda.synchronize()
    med = statistics.median
    return dict(what="track_sort", clips=a.clips, frames=T, rows_per_frame=N, classes=C, max_age=max_age,
                detections_per_frame=round(float((ids >= 0).sum()) / F, 1), host_clips=hc,
                host_most_active=int(stats["active"].max()), host_tracks_per_clip=round(sum(stats["tracks"]) / hc, 1),
                host_s_per_clip=[round(t, 4) for t in th], host_median_s_per_clip=round(med(th), 4),
                device_ms_per_call=[round(t, 4) for t in full], device_median_ms_per_call=round(med(full), 4),
                device_median_ms_per_clip=round(med(full) / a.clips, 5),
                vd_track_ms_per_call=[round(t, 4) for t in iou_full], vd_track_median_ms_per_call=round(med(iou_full), 4),
                same_result=_same(got, want, hc * T))


def quality(a, ds, max_age):
    """tools/track_probe.py's quality case, linked by either method, scored by the MOT metric"""
    from viddet_amd import ops
    from viddet_amd.mot_metric import MOTMetric
    from viddet_amd.sort import sort_host
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
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    kw = dict(clip_start=cs, num_class=len(ds.classes), max_age=max_age)
    got = ops.track_sort(*dv, **kw)
    same = _same(got, sort_host(ids, scores, bboxes, **kw), F)
    out = dict(what="quality", clips=ds.num_videos, frames=T, max_age=max_age, jitter=a.jitter, drop=a.drop, same_result=same)
    links = dict(iou=ops.track(*dv, **kw)[0], iou_at_0_3=ops.track(*dv, sigma_iou=0.3, **kw)[0], sort=got[0])
    for name, track in links.items():
        metric = MOTMetric(ds)
        metric._results = _results(ds, ids, scores, bboxes, track.cpu().numpy())
        metric.get()
        s = metric.summary["all"]
        out[name] = dict(MOTA=round(s["MOTA"], 4), IDF1=round(s["IDF1"], 4), IDSW=s["IDSW"], Frag=s["Frag"], TP=s["TP"], FN=s["FN"],
                         FP=s["FP"], MT=s["MT"], PT=s["PT"], ML=s["ML"])
    out["GT"], out["ground_truth_tracks"] = s["GT"], s["gt_tracks"]
    return out


def share(a, ds):
    """one clip through net.detect_video (random weights: the rows the untrained heads let through) with and without SORT"""
    from viddet_amd import ops
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(ds.classes, k=3, k_join_type="max", k_join_pos="early")
    net.initialize(init="he", obj_bias=-2.0)
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(a.frames, 3, a.size, a.size, generator=g).cuda()

    def run(track):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = net.detect_video(x, chunk=8, track=track)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    sort = dict(method="sort")
    run(None), run(sort)                                           # plans, tuning, code objects
    tp, ts = [], []
    for _ in range(a.blocks):
        tp.append(run(None)[0])
        ts.append(run(sort)[0])
    plain = [t.clone() for t in run(None)[1]]
    C = len(ds.classes)
    k_ms = {m: _event_ms(lambda: ops.track_sort(*plain, num_class=C, max_age=m), a.reps) for m in (1, 7)}
    i_ms = {m: _event_ms(lambda: ops.track(*plain, num_class=C, max_age=m), a.reps) for m in (1, 7)}
    med = statistics.median
    return dict(what="detect_video", frames=a.frames, size=a.size, rows_per_frame=int(plain[0].shape[1]),
                detections_per_frame=round(float((plain[0] >= 0).sum()) / a.frames, 1),
                plain_s=[round(t, 4) for t in tp], with_sort_s=[round(t, 4) for t in ts], plain_median_s=round(med(tp), 4),
                with_sort_median_s=round(med(ts), 4), track_sort_ms_per_call={str(m): round(v, 4) for m, v in k_ms.items()},
                vd_track_ms_per_call={str(m): round(v, 4) for m, v in i_ms.items()},
                track_sort_share_of_plain={str(m): round(v / 1e3 / med(tp), 5) for m, v in k_ms.items()})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one probe each")
    ap.add_argument("--max_age", default="1,7", help="one probe each")
    ap.add_argument("--host_clips", type=int, default=2)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=0.04, help="quality: sigma of the box noise, as a share of the box's size")
    ap.add_argument("--drop", type=float, default=0.1, help="quality: the share of ground-truth rows left out")
    ap.add_argument("--no_share", action="store_true", help="skip the detect_video part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/sort_probe.py needs an MI355X: a timing taken elsewhere says nothing")
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
    for m in [0] + ages:
        emit(quality(a, ds, m))
    if not a.no_share:
        emit(share(a, ds))
    if not all(d.get("same_result", True) for d in results):
        raise SystemExit("the device's result differs from sort_host's")


if __name__ == "__main__":
    main()
