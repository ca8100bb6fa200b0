#!/usr/bin/env python
"""Developer tool: the tracker on the device (vd_track, ops.track) against its host definition on the same
detections.

In ONE process, on SyntheticTracks at --clips (64) x --frames (64) with about --dets (10,100) synthetic detections per frame
(tools/seq_nms_probe.py's), at every --max_age (0,7):

  host     track_host seconds per clip, on the first --host_clips clips
  device   vd_track ms per call over ALL clips at once (device events, --reps calls)
  share    the call as a share of net.detect_video on one --frames clip at --size (416): detect_video with and without
           track=True, wall time around a synchronize
  quality  on the ground-truth rows at score 0.9 with boxes jittered by --jitter (4 %) of their size and --drop (10 %) of the
           rows dropped: the ground-truth tracks that come out in more than one piece (fragmented) and the id switches (two
           consecutive kept rows of one ground-truth track with different ids), on the device, equal to the host's

alternating blocks, median of --blocks; the device result is compared with the host's on the host's clips on the way: that it
is equal is the pass condition, no speed is asked for.  Needs a GPU: there is no fallback.  Prints one JSON line per measurement.
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


def probe(a, ds, per_image, max_age):
    from viddet_amd import lib as L, ops
    from viddet_amd.track import track_host
    ids, scores, bboxes = clip_arrays(ds, per_image)
    F, N = bboxes.shape[:2]
    T, C = a.frames, len(ds.classes)
    cs = list(range(0, F + 1, T))
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    ws = torch.empty(L.TRACK_WS_PER_ROW * F * N, dtype=torch.uint8, device="cuda")
    dcs = torch.tensor(cs, dtype=torch.int32, device="cuda")
    call = lambda: ops.track(*dv, clip_start=dcs, num_class=C, max_age=max_age, ws=ws)
    hc = min(a.host_clips, a.clips)
    head = [x[:hc * T] for x in (ids, scores, bboxes)]
    th, full = [], []
    stats = {}
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t0 = time.perf_counter()
        want = track_host(*head, clip_start=cs[:hc + 1], num_class=C, max_age=max_age, stats=stats)
        th.append((time.perf_counter() - t0) / hc)
        full.append(_event_ms(call, a.reps))
    got = call()
    torch.cuda.synchronize()
    same = all(np.array_equal(g[:hc * T].cpu().numpy(), w) for g, w in zip(got, want))
    med = statistics.median
    return dict(what="track", clips=a.clips, frames=T, rows_per_frame=N, classes=C, max_age=max_age,
                detections_per_frame=round(float((ids >= 0).sum()) / F, 1), host_clips=hc,
                host_most_active=int(stats["active"].max()), host_tracks_per_clip=round(sum(stats["tracks"]) / hc, 1),
                host_s_per_clip=[round(t, 4) for t in th], host_median_s_per_clip=round(med(th), 4),
                device_ms_per_call=[round(t, 4) for t in full], device_median_ms_per_call=round(med(full), 4),
                device_median_ms_per_clip=round(med(full) / a.clips, 5), same_result=bool(same))


def quality(a, ds, max_age):
    """the ground truth, jittered and thinned, through the tracker: how many ground-truth tracks break, how many ids switch"""
    from viddet_amd import ops
    from viddet_amd.track import track_host
    rng = np.random.default_rng(7)
    T, V = ds.frames_per_video, ds.num_videos
    labels = [ds.get_label(sid) for sid in ds.get_sample_ids()]
    N = max(1, max(len(l) for l in labels))
    F = len(labels)
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    truth = -np.ones((F, N), np.int64)
    for t, l in enumerate(labels):
        keep = l[rng.uniform(size=len(l)) >= a.drop]
        wh = np.stack([keep[:, 2] - keep[:, 0], keep[:, 3] - keep[:, 1]] * 2, axis=1)
        box = keep[:, :4] + rng.normal(0.0, a.jitter, (len(keep), 4)) * wh
        n = len(keep)
        ids[t, :n, 0], scores[t, :n, 0], bboxes[t, :n], truth[t, :n] = keep[:, 4], 0.9, box, keep[:, 5]
    cs = list(range(0, F + 1, T))
    kw = dict(clip_start=cs, num_class=len(ds.classes), max_age=max_age)
    got = ops.track(*[torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)], **kw)
    want = track_host(ids, scores, bboxes, **kw)
    same = all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    track = got[0].cpu().numpy()
    gt_tracks = fragmented = switches = unassigned = 0
    for v in range(V):
        tr, gt = track[v * T:(v + 1) * T], truth[v * T:(v + 1) * T]
        for g in np.unique(gt[gt >= 0]):
            seq = tr[gt == g]                                      # row-major: in frame order, one row per frame
            unassigned += int((seq < 0).sum())
            seq = seq[seq >= 0]
            gt_tracks += 1
            fragmented += int(len(np.unique(seq)) != 1 or (tr[gt == g] < 0).any())
            switches += int((seq[1:] != seq[:-1]).sum())
    return dict(what="quality", clips=V, frames=T, max_age=max_age, jitter=a.jitter, drop=a.drop, rows=int((truth >= 0).sum()),
                ground_truth_tracks=gt_tracks, fragmented=fragmented, id_switches=switches, rows_without_track=unassigned,
                same_result=bool(same))


def share(a, ds):
    """one clip through net.detect_video (random weights: the rows the untrained heads let through) with and without the tracker"""
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

    run(None), run(True)                                           # plans, tuning, code objects
    tp, ts = [], []
    for _ in range(a.blocks):
        tp.append(run(None)[0])
        ts.append(run(True)[0])
    plain = [t.clone() for t in run(None)[1]]
    C = len(ds.classes)
    k_ms = {m: _event_ms(lambda: ops.track(*plain, num_class=C, max_age=m), a.reps) for m in (0, 7)}
    med = statistics.median
    return dict(what="detect_video", frames=a.frames, size=a.size, rows_per_frame=int(plain[0].shape[1]),
                detections_per_frame=round(float((plain[0] >= 0).sum()) / a.frames, 1),
                plain_s=[round(t, 4) for t in tp], with_track_s=[round(t, 4) for t in ts], plain_median_s=round(med(tp), 4),
                with_track_median_s=round(med(ts), 4), track_ms_per_call={str(m): round(v, 4) for m, v in k_ms.items()},
                track_share_of_plain={str(m): round(v / 1e3 / med(tp), 5) for m, v in k_ms.items()})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one probe each")
    ap.add_argument("--max_age", default="0,7", help="one probe each")
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
        raise SystemExit("tools/track_probe.py needs an MI355X: a timing taken elsewhere says nothing")
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
    if not a.no_share:
        emit(share(a, ds))
    if not all(d.get("same_result", True) for d in results):
        raise SystemExit("the device's result differs from track_host's")


if __name__ == "__main__":
    main()
