#!/usr/bin/env python
"""Developer tool: the smoothing pass on the device (vd_track_smooth, ops.smooth) against its host definition on the
same tracked detections.

In ONE process, on SyntheticTracks at --clips (64) x --frames (64) with about --dets (10,100) synthetic detections per frame
(tools/seq_nms_probe.py's), linked by ops.track_sort at every --max_age (1,7), the pass's max_gap being the tracker's max_age:

  host     smooth_host seconds per clip, on the first --host_clips clips
  device   vd_track_smooth ms per call over ALL clips at once (device events, --reps calls), each of its launches alone
           (vd_track_smooth_stages), and vd_tubelet on the same rows beside it
  quality  on tools/track_probe.py's jittered case - the ground-truth rows at score 0.9 with boxes jittered by --jitter (4 %) of
           their size and --drop (10 %) of the rows left out - linked by ops.track_sort at --quality_max_age: HOTAMetric (HOTA,
           LocA), MOTMetric (MOTP) and COCODetectionMetric (AP, AP75) on the plain boxes against the smoothed ones, and the mean
           IoU of a row's box with the ground-truth box it was made from

alternating blocks, median of --blocks; the device result is compared with the host's on the host's clips on the way: that it
is equal is the pass condition, no speed or quality is asked for.  Needs a GPU: there is no fallback.  Prints one JSON line per
measurement.
"""
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

STAGES = (("clear", 1), ("members", 2), ("links", 4), ("segments", 8))


def _same(got, want):
    return bool(np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]))


def probe(a, ds, per_image, max_age):
    from viddet_amd import lib as L, ops
    from viddet_amd.smooth import smooth_host
    ids, scores, bboxes = clip_arrays(ds, per_image)
    F, N = bboxes.shape[:2]
    T, C = a.frames, len(ds.classes)
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    dcs = torch.tensor(cs, dtype=torch.int32, device="cuda")
    track = ops.track_sort(*dv, clip_start=dcs, num_class=C, max_age=max_age)[0]
    ws = torch.empty(L.TRACK_SMOOTH_WS_PER_ROW * F * N, dtype=torch.uint8, device="cuda")
    ws_t = torch.empty(L.TUBELET_WS_PER_ROW * F * N, dtype=torch.uint8, device="cuda")
    call = lambda stages=None: ops.smooth(*dv, track, clip_start=dcs, num_class=C, max_gap=max_age, ws=ws, stages=stages)
    tube = lambda: ops.tubelet(*dv, track, clip_start=dcs, num_class=C, max_gap=max_age, ws=ws_t)
    hc = min(a.host_clips, a.clips)
    head = [x[:hc * T] for x in (ids, scores, bboxes)] + [track.cpu().numpy()[:hc * T]]
    th, full, tub = [], [], []
    per = {name: [] for name, _ in STAGES}
    stats = {}
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t0 = time.perf_counter()
        want = smooth_host(*head, clip_start=cs[:hc + 1], num_class=C, max_gap=max_age, stats=stats)
        th.append((time.perf_counter() - t0) / hc)
        full.append(_event_ms(call, a.reps))
        tub.append(_event_ms(tube, a.reps))
        for name, bit in STAGES:                                   # the workspace holds a whole call's tables
            per[name].append(_event_ms(lambda: call(bit), a.reps))
    got = call()
    torch.cuda.synchronize()
    slen = got[1].cpu().numpy()
    same = _same([g[:hc * T].cpu().numpy() for g in got], want)
    med = statistics.median
    return dict(what="smooth", clips=a.clips, frames=T, rows_per_frame=N, classes=C, max_age=max_age, max_gap=max_age,
                detections_per_frame=round(float((ids >= 0).sum()) / F, 1), host_clips=hc,
                host_segments_per_clip=round(sum(stats["segments"]) / hc, 1), host_members_per_clip=round(sum(stats["members"]) / hc, 1),
                members_all_clips=int((slen > 0).sum()), smoothed_all_clips=int((slen >= 2).sum()), longest_segment=int(slen.max()),
                host_s_per_clip=[round(t, 4) for t in th], host_median_s_per_clip=round(med(th), 4),
                device_ms_per_call=[round(t, 4) for t in full], device_median_ms_per_call=round(med(full), 4),
                device_median_ms_per_clip=round(med(full) / a.clips, 5),
                launch_median_ms={name: round(med(v), 4) for name, v in per.items()},
                tubelet_median_ms_per_call=round(med(tub), 4), same_result=bool(same))


def _iou_rows(a, b):
    iw = np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0])
    ih = np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
    return inter / ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter)


def quality(a, ds):
    """tools/track_probe.py's case - the ground truth, jittered and thinned - through SORT and the pass: the tracking and
    detection metrics on the plain boxes and on the smoothed ones"""
    from viddet_amd import ops
    from viddet_amd.coco_metric import COCODetectionMetric
    from viddet_amd.hota_metric import HOTAMetric
    from viddet_amd.mot_metric import MOTMetric
    from viddet_amd.smooth import smooth_host
    rng = np.random.default_rng(7)
    T, V, C = ds.frames_per_video, ds.num_videos, len(ds.classes)
    sids = list(ds.get_sample_ids())
    labels = [ds.get_label(sid) for sid in sids]
    N = max(1, max(len(l) for l in labels))
    F = len(labels)
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    truth = np.zeros((F, N, 4), np.float64)
    for t, l in enumerate(labels):
        keep = l[rng.uniform(size=len(l)) >= a.drop]
        wh = np.stack([keep[:, 2] - keep[:, 0], keep[:, 3] - keep[:, 1]] * 2, axis=1)
        box = keep[:, :4] + rng.normal(0.0, a.jitter, (len(keep), 4)) * wh
        n = len(keep)
        ids[t, :n, 0], scores[t, :n, 0], bboxes[t, :n], truth[t, :n] = keep[:, 4], 0.9, box, keep[:, :4]
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    track = ops.track_sort(*dv, clip_start=cs, num_class=C, max_age=a.quality_max_age)[0]
    got = [g.cpu().numpy() for g in ops.smooth(*dv, track, clip_start=cs, num_class=C, max_gap=a.quality_max_age)]
    track = track.cpu().numpy()
    same = _same(got, smooth_host(ids, scores, bboxes, track, clip_start=cs, num_class=C, max_gap=a.quality_max_age))
    on = ids[..., 0] >= 0

    def metrics(boxes):
        hota, mot = HOTAMetric(ds), MOTMetric(ds, iou_thresh=0.5)
        with tempfile.TemporaryDirectory() as tmp:
            coco = COCODetectionMetric(ds, os.path.join(tmp, "coco"), use_time=False, cleanup=True, data_shape=None)
            for t, sid in enumerate(sids):
                k = on[t]
                args = ([[boxes[t, k]]], [[ids[t, k, 0]]], [[scores[t, k, 0]]], None, None, None)
                hota.update(*args, sid=sid, tracks=[[track[t, k]]])
                mot.update(*args, sid=sid, tracks=[[track[t, k]]])
                coco.update(*args, sid=sid)
            text = coco.get()[1][0]
            del coco                                               # its clean-up, while the directory is still there
        out = {}
        for metric, keys in ((hota, ("HOTA", "LocA")), (mot, ("MOTP", "MOTA"))):
            table = dict(zip(*metric.get()))
            out.update({key: float(table[key]) for key in keys if key in table})
        for key, pat in (("AP", r"IoU=0\.50:0\.95 \| area=\s*all \| maxDets=100 \] = (-?[\d.]+)"),
                         ("AP75", r"IoU=0\.75\s*\| area=\s*all \| maxDets=100 \] = (-?[\d.]+)")):
            m = re.search(pat, text)
            out[key] = float(m.group(1)) if m else None
        out["mean_iou_with_truth"] = round(float(_iou_rows(boxes[on].astype(np.float64), truth[on]).mean()), 4)
        return out

    return dict(what="quality", clips=V, frames=T, jitter=a.jitter, drop=a.drop, max_age=a.quality_max_age, rows=int(on.sum()),
                rows_tracked=int((track >= 0).sum()), rows_smoothed=int((got[1] >= 2).sum()),
                table=dict(plain=metrics(bboxes), smoothed=metrics(got[0])), same_result=bool(same))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one probe each")
    ap.add_argument("--max_age", default="1,7", help="the tracker's max_age and the pass's max_gap, one probe each")
    ap.add_argument("--host_clips", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=0.04, help="quality: sigma of the box noise, as a share of the box's size")
    ap.add_argument("--drop", type=float, default=0.1, help="quality: the share of ground-truth rows left out")
    ap.add_argument("--quality_max_age", type=int, default=7)
    ap.add_argument("--quality_clips", type=int, default=16)
    ap.add_argument("--no_quality", action="store_true", help="skip the quality part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/smooth_probe.py needs an MI355X: a timing taken elsewhere says nothing")
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
    if not all(d.get("same_result", True) for d in results):
        raise SystemExit("the device's result differs from smooth_host's")


if __name__ == "__main__":
    main()
