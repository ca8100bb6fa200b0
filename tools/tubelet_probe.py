#!/usr/bin/env python
"""Developer tool: the tubelet pass on the device (vd_tubelet, ops.tubelet) against its host definition on the same
tracked detections.

In ONE process, on SyntheticTracks at --clips (64) x --frames (64) with about --dets (10,100) synthetic detections per frame
(tools/seq_nms_probe.py's), linked by ops.track at every --max_age (2,7):

  host     tubelet_host seconds per clip, on the first --host_clips clips
  device   vd_tubelet ms per call over ALL clips at once (device events, --reps calls), each of its launches alone
           (vd_tubelet_stages), and vd_track on the same rows beside it
  share    the call as a share of net.detect_video on one --frames clip at --size (416): detect_video with track alone and with
           track and tubelet, wall time around a synchronize
  quality  on tools/track_probe.py's ground truth - boxes jittered by --jitter (4 %) of their size, --drop (10 %) of the rows
           left out - with scores drawn per row and --clutter random boxes per frame with lower scores: the host VID and VOC
           metrics on the plain rows against the rows after the pass, for avg / max / None, with and without filling, and how
           many of the rows left out a fill restores (same class, IoU >= 0.5 to the row)

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

STAGES = (("clear", 1), ("members", 2), ("chain", 4), ("frames", 8))


def probe(a, ds, per_image, max_age):
    from viddet_amd import lib as L, ops
    from viddet_amd.tubelet import tubelet_host
    ids, scores, bboxes = clip_arrays(ds, per_image)
    F, N = bboxes.shape[:2]
    T, C = a.frames, len(ds.classes)
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    dcs = torch.tensor(cs, dtype=torch.int32, device="cuda")
    ws_t = torch.empty(L.TRACK_WS_PER_ROW * F * N, dtype=torch.uint8, device="cuda")
    link = lambda: ops.track(*dv, clip_start=dcs, num_class=C, max_age=max_age, ws=ws_t)
    track = link()[0]
    ws = torch.empty(L.TUBELET_WS_PER_ROW * F * N, dtype=torch.uint8, device="cuda")
    call = lambda stages=None: ops.tubelet(*dv, track, clip_start=dcs, num_class=C, max_gap=max_age, ws=ws, stages=stages)
    hc = min(a.host_clips, a.clips)
    head = [x[:hc * T] for x in (ids, scores, bboxes)] + [track.cpu().numpy()[:hc * T]]
    th, full, trk = [], [], []
    per = {name: [] for name, _ in STAGES}
    stats = {}
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t0 = time.perf_counter()
        want = tubelet_host(*head, clip_start=cs[:hc + 1], num_class=C, max_gap=max_age, stats=stats)
        th.append((time.perf_counter() - t0) / hc)
        full.append(_event_ms(call, a.reps))
        trk.append(_event_ms(link, a.reps))
        for name, bit in STAGES:                                   # the workspace holds a whole call's tables
            per[name].append(_event_ms(lambda: call(bit), a.reps))
    got = call()
    torch.cuda.synchronize()
    same = all(np.array_equal(g[:hc * T].cpu().numpy(), w) for g, w in zip(got, want))
    med = statistics.median
    return dict(what="tubelet", clips=a.clips, frames=T, rows_per_frame=N, classes=C, max_age=max_age, max_gap=max_age,
                detections_per_frame=round(float((ids >= 0).sum()) / F, 1), host_clips=hc,
                host_tracks_per_clip=round(sum(stats["tracks"]) / hc, 1), host_filled_per_clip=round(sum(stats["filled"]) / hc, 1),
                host_dropped_per_clip=round(sum(stats["dropped"]) / hc, 1),
                filled_all_clips=int((got[3] == -2).sum()), dropped_all_clips=int(got[5].sum()),
                host_s_per_clip=[round(t, 4) for t in th], host_median_s_per_clip=round(med(th), 4),
                device_ms_per_call=[round(t, 4) for t in full], device_median_ms_per_call=round(med(full), 4),
                device_median_ms_per_clip=round(med(full) / a.clips, 5),
                launch_median_ms={name: round(med(v), 4) for name, v in per.items()},
                track_median_ms_per_call=round(med(trk), 4), same_result=bool(same))


def _iou(a, b):
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def quality(a, ds):
    """the ground truth, jittered and thinned, with drawn scores and clutter, through the tracker and the pass: the host VID
    and VOC metrics ahead of the pass and after it"""
    from viddet_amd import ops
    from viddet_amd.metrics import VOCMApMetric
    from viddet_amd.tubelet import tubelet_host
    from viddet_amd.vid_metric import VIDDetectionMetric
    rng = np.random.default_rng(7)
    T, V, C = ds.frames_per_video, ds.num_videos, len(ds.classes)
    sids = list(ds.get_sample_ids())
    labels = [ds.get_label(sid) for sid in sids]
    sizes = [ds.image_size(sid) for sid in sids]
    F = len(labels)
    N = min(128, max(len(l) for l in labels) + a.clutter + 8)      # room for fills
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    left_out = []                                                  # (frame, class, box) of the rows the thinning took
    for t, l in enumerate(labels):
        on = rng.uniform(size=len(l)) >= a.drop
        keep = l[on]
        left_out += [(t, int(r[4]), r[:4]) for r in l[~on]]
        wh = np.stack([keep[:, 2] - keep[:, 0], keep[:, 3] - keep[:, 1]] * 2, axis=1)
        box = keep[:, :4] + rng.normal(0.0, a.jitter, (len(keep), 4)) * wh
        w, h = sizes[t]
        xy = rng.uniform(0, 0.7, (a.clutter, 2)) * [w, h]
        noise = np.concatenate([xy, xy + rng.uniform(0.1, 0.3, (a.clutter, 2)) * [w, h]], axis=1)
        rows = [(c, s, b) for c, s, b in zip(keep[:, 4], rng.uniform(0.2, 1.0, len(keep)), box)]
        rows += [(c, s, b) for c, s, b in zip(rng.integers(0, C, a.clutter), rng.uniform(0.05, 0.6, a.clutter), noise)]
        rows.sort(key=lambda r: -r[1])
        for i, (c, s, b) in enumerate(rows[:N]):
            ids[t, i, 0], scores[t, i, 0], bboxes[t, i] = c, s, b
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    track = ops.track(*dv, clip_start=cs, num_class=C, max_age=a.quality_max_age)[0]

    def metrics(i_, s_, b_):
        vid = VIDDetectionMetric(ds, iou_thresh=0.5)
        voc = VOCMApMetric(iou_thresh=0.5, class_names=ds.classes)
        for t, sid in enumerate(sids):
            on = i_[t, :, 0] >= 0
            vid.update([[b_[t, on]]], [[i_[t, on, 0]]], [[s_[t, on, 0]]], None, None, None, sid=sid)
            voc.update([b_[t, on]], [i_[t, on, 0]], [s_[t, on, 0]], [labels[t][:, :4]], [labels[t][:, 4]])
        vid.get()
        cell = np.asarray(vid.ap[0][0], dtype=np.float64)
        return round(float(np.mean(cell[cell >= 0])), 4), round(float(voc.get()[1][-1]), 4)

    out = dict(what="quality", clips=V, frames=T, jitter=a.jitter, drop=a.drop, clutter=a.clutter, max_age=a.quality_max_age,
               rows=int((ids >= 0).sum()), rows_left_out=len(left_out), rows_per_frame=N, table={}, same_result=True)
    out["table"]["plain"] = dict(zip(("vid_map", "voc_map"), metrics(ids, scores, bboxes)))
    track_h = track.cpu().numpy()
    for rescore in ("avg", "max", None):
        for gap in (0, a.quality_max_age):
            for drop in (False, True):
                kw = dict(clip_start=cs, num_class=C, rescore=rescore, max_gap=gap, drop_untracked=drop)
                got = [g.cpu().numpy() for g in ops.tubelet(*dv, track, **kw)]
                if rescore == "avg" and not drop:                  # the host's result on the way (the whole set: slow)
                    want = tubelet_host(ids, scores, bboxes, track_h, **kw)
                    out["same_result"] &= all(np.array_equal(g, w) for g, w in zip(got, want))
                restored = 0
                if gap:
                    for t, c, b in left_out:
                        fills = np.nonzero((got[3][t] == -2) & (got[0][t, :, 0] == c))[0]
                        restored += int(any(_iou(b, got[2][t, i]) >= 0.5 for i in fills))
                vid_map, voc_map = metrics(got[0], got[1], got[2])
                out["table"]["%s_gap%d%s" % (rescore, gap, "_drop" if drop else "")] = dict(
                    vid_map=vid_map, voc_map=voc_map, rows=int((got[0] >= 0).sum()), filled=int((got[3] == -2).sum()),
                    dropped=int(got[5].sum()), restored=restored)
    return out


def share(a, ds):
    """one clip through net.detect_video (random weights: the rows the untrained heads let through) with the tracker alone and
    with the pass behind it"""
    from viddet_amd import ops
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(ds.classes, k=3, k_join_type="max", k_join_pos="early")
    net.initialize(init="he", obj_bias=-2.0)
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(a.frames, 3, a.size, a.size, generator=g).cuda()
    trk = dict(max_age=2)

    def run(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = net.detect_video(x, chunk=8, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    run(), run(track=trk), run(track=trk, tubelet=True)            # plans, tuning, code objects
    tp, tt, tu = [], [], []
    for _ in range(a.blocks):
        tp.append(run()[0])
        tt.append(run(track=trk)[0])
        tu.append(run(track=trk, tubelet=True)[0])
    pre, links = net.last_pre_tubelet, net.last_tracks[0]
    C = len(ds.classes)
    k_ms = _event_ms(lambda: ops.tubelet(*pre, links, num_class=C), a.reps)
    med = statistics.median
    return dict(what="detect_video", frames=a.frames, size=a.size, rows_per_frame=int(pre[0].shape[1]),
                detections_per_frame=round(float((pre[0] >= 0).sum()) / a.frames, 1),
                plain_s=[round(t, 4) for t in tp], with_track_s=[round(t, 4) for t in tt], with_tubelet_s=[round(t, 4) for t in tu],
                plain_median_s=round(med(tp), 4), with_track_median_s=round(med(tt), 4), with_tubelet_median_s=round(med(tu), 4),
                tubelet_ms_per_call=round(k_ms, 4), tubelet_share_of_plain=round(k_ms / 1e3 / med(tp), 5))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one probe each")
    ap.add_argument("--max_age", default="2,7", help="the tracker's max_age and the pass's max_gap, one probe each")
    ap.add_argument("--host_clips", type=int, default=2)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=0.04, help="quality: sigma of the box noise, as a share of the box's size")
    ap.add_argument("--drop", type=float, default=0.1, help="quality: the share of ground-truth rows left out")
    ap.add_argument("--clutter", type=int, default=2, help="quality: random boxes per frame, scored in [0.05, 0.6)")
    ap.add_argument("--quality_max_age", type=int, default=7)
    ap.add_argument("--quality_clips", type=int, default=16)
    ap.add_argument("--no_share", action="store_true", help="skip the detect_video part")
    ap.add_argument("--no_quality", action="store_true", help="skip the quality part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/tubelet_probe.py needs an MI355X: a timing taken elsewhere says nothing")
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
    if not a.no_quality:
        emit(quality(a, SyntheticTracks("vid", num_videos=a.quality_clips, frames_per_video=a.frames)))
    if not a.no_share:
        emit(share(a, ds))
    if not all(d.get("same_result", True) for d in results):
        raise SystemExit("the device's result differs from tubelet_host's")


if __name__ == "__main__":
    main()
