#!/usr/bin/env python
"""Developer tool: appearance association on the device (vd_roi_embed, vd_track_sort_app) against its host
definitions and beside SORT (vd_track_sort) on the same detections.

In ONE process, on SyntheticTracks:

  separation  --clips (16) clips of --frames (64) frames of 64 x 64, the ground-truth rows at score 0.9 with boxes jittered by
              --jitter (4 %) of their size and --drop (10 %) of the rows left out (tools/track_probe.py's case); descriptors
              from a net on those frames - UNTRAINED weights (He initialisation): the backbone is a random projection, what it
              separates says nothing of a trained one - through ops.roi_embed on extract_features' stride-8 map; the distribution
              of cos_q / 2**20 over same-track and different-track pairs of adjacent frames
  quality     the same rows linked by ops.track_sort and by ops.track_sort_app with those descriptors, scored by MOTMetric: id
              switches, fragmentations, MOTA
  device      vd_roi_embed ms per chunk (8 frames x 100 rows on a 52 x 52 x 256 map, the stride-8 route at 416 x 416), and
              vd_track_sort_app against vd_track_sort ms per call over --tclips (64) clips at about --dets (10,100) rows per frame
  share       the two calls as a share of net.detect_video on one 64-frame clip at --size (416): detect_video with
              track={'method': 'sort'} with and without `appearance`, wall time around a synchronize

alternating blocks, median of --blocks; every device result is compared with the host definition on the way: that they are
equal is the pass condition, no speed or quality is asked for.  Needs a GPU: there is no fallback.  Prints one JSON line per
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

med = statistics.median


def _quantiles(v):
    v = np.asarray(v, np.float64)
    if not len(v):
        return dict(n=0)
    q = np.quantile(v, [0.05, 0.25, 0.5, 0.75, 0.95])
    return dict(n=int(len(v)), mean=round(float(v.mean()), 4), q05=round(float(q[0]), 4), q25=round(float(q[1]), 4),
                median=round(float(q[2]), 4), q75=round(float(q[3]), 4), q95=round(float(q[4]), 4))


def noisy_rows(a, ds):
    """tools/track_probe.py's quality case and, per row, the ground-truth track it came from (-1 on an empty row)"""
    rng = np.random.default_rng(7)
    labels = [ds.get_label(sid) for sid in ds.get_sample_ids()]
    N = max(1, max(len(l) for l in labels))
    F = len(labels)
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    gt = -np.ones((F, N), np.int64)
    for t, l in enumerate(labels):
        keep = l[rng.uniform(size=len(l)) >= a.drop]
        wh = np.stack([keep[:, 2] - keep[:, 0], keep[:, 3] - keep[:, 1]] * 2, axis=1)
        n = len(keep)
        ids[t, :n, 0], scores[t, :n, 0] = keep[:, 4], 0.9
        bboxes[t, :n] = keep[:, :4] + rng.normal(0.0, a.jitter, (n, 4)) * wh
        gt[t, :n] = keep[:, 5]
    return ids, scores, bboxes, gt


def separation_and_quality(a, emit):
    from viddet_amd import ops
    from viddet_amd.appearance import app_sort_host, cos_q_matrix, embed_host
    from viddet_amd.data import SyntheticTracks
    from viddet_amd.mot_metric import MOTMetric
    from viddet_amd.model import yolo3_darknet53
    ds = SyntheticTracks("vid", num_videos=a.clips, frames_per_video=a.frames, size=(64, 64))
    T = a.frames
    ids, scores, bboxes, gt = noisy_rows(a, ds)
    net = yolo3_darknet53(ds.classes)
    net.initialize(init="he")
    dids, dbx = torch.from_numpy(ids).cuda(), torch.from_numpy(bboxes).cuda()
    embs, same_embed = [], True
    for v in range(a.clips):
        x = torch.from_numpy(ds.video_frames(v)).cuda().permute(0, 3, 1, 2).float() / 127.5 - 1.0
        f = net.extract_features(x.contiguous())[0].permute(0, 2, 3, 1).contiguous()     # NHWC, stride 8
        rows = slice(v * T, (v + 1) * T)
        e = ops.roi_embed(f, dids[rows], dbx[rows], 8)
        if v < a.host_clips:
            same_embed &= bool(np.array_equal(e.cpu().numpy(), embed_host(f.cpu().numpy(), ids[rows], bboxes[rows], 8)))
        embs.append(e)
    emb = torch.cat(embs)
    he = emb.cpu().numpy()
    same_t, diff_t = [], []
    for v in range(a.clips):
        for t in range(v * T, (v + 1) * T - 1):
            r0, r1 = np.nonzero(gt[t] >= 0)[0], np.nonzero(gt[t + 1] >= 0)[0]
            if len(r0) and len(r1):
                c = cos_q_matrix(he[t, r0], he[t + 1, r1])[0] / float(1 << 20)
                eq = gt[t, r0][:, None] == gt[t + 1, r1][None, :]
                same_t += c[eq].tolist()
                diff_t += c[~eq].tolist()
    emit(dict(what="separation", weights="untrained (He initialisation)", clips=a.clips, frames=T, size=64, level=8,
              rows_with_descriptor=int(he.any(axis=2).sum()), rows=int((ids >= 0).sum()), same_track=_quantiles(same_t),
              different_track=_quantiles(diff_t), same_result=same_embed))
    cs = list(range(0, len(ids) + 1, T))
    for max_age in (1, 7):
        kw = dict(clip_start=cs, num_class=len(ds.classes), max_age=max_age)
        dv = [dids, torch.from_numpy(scores).cuda(), dbx]
        plain = ops.track_sort(*dv, **kw)
        out = dict(what="quality", weights="untrained (He initialisation)", clips=a.clips, frames=T, max_age=max_age,
                   jitter=a.jitter, drop=a.drop)
        links = dict(sort=plain[0])
        same = True
        for sa in a.sigma_app:
            got = ops.track_sort_app(*dv, emb, sigma_app=sa, **kw)
            hc = min(a.host_clips, a.clips) * T
            want = app_sort_host(ids[:hc], scores[:hc], bboxes[:hc], he[:hc], sigma_app=sa, **dict(kw, clip_start=cs[:hc // T + 1]))
            same &= _same(got, want, hc)
            links["sort_app_%g" % sa] = got[0]
        out["same_result"] = same
        for name, track in links.items():
            metric = MOTMetric(ds)
            metric._results = _results(ds, ids, scores, bboxes, track.cpu().numpy())
            metric.get()
            s = metric.summary["all"]
            out[name] = dict(MOTA=round(s["MOTA"], 4), IDF1=round(s["IDF1"], 4), IDSW=s["IDSW"], Frag=s["Frag"], TP=s["TP"], FN=s["FN"],
                             FP=s["FP"])
        emit(out)


def device(a, emit):
    from viddet_amd import lib as L, ops
    from viddet_amd.appearance import app_sort_host, embed_host
    from viddet_amd.data import SyntheticTracks
    rng = np.random.RandomState(3)
    # the descriptor: one chunk of 8 frames x 100 rows on the stride-8 route of a 416 x 416 input
    f = torch.randn(8, 52, 52, 256, device="cuda")
    f = torch.where(f > 0, f, 0.1 * f)
    lo = rng.uniform(0, 300, (8, 100, 2))
    bx = torch.from_numpy(np.concatenate([lo, lo + rng.uniform(8, 116, (8, 100, 2))], axis=2).astype(np.float32)).cuda()
    rid = torch.zeros(8, 100, 1, device="cuda")
    out = torch.empty(8, 100, 256, dtype=torch.int8, device="cuda")
    t_embed = [_event_ms(lambda: ops.roi_embed(f, rid, bx, 8, out=out), a.reps * 4) for _ in range(a.blocks)]
    same = bool(np.array_equal(out[:1].cpu().numpy(), embed_host(f[:1].cpu().numpy(), rid[:1].cpu().numpy(), bx[:1].cpu().numpy(), 8)))
    emit(dict(what="roi_embed", frames=8, rows_per_frame=100, map="52x52x256 fp32", ms_per_chunk=[round(t, 4) for t in t_embed],
              median_ms_per_chunk=round(med(t_embed), 4), same_result=same))
    ds = SyntheticTracks("vid", num_videos=a.tclips, frames_per_video=a.frames)
    T, C = a.frames, len(ds.classes)
    for per_image in a.dets:
        ids, scores, bboxes = clip_arrays(ds, per_image)
        F, N = bboxes.shape[:2]
        proto = rng.randint(-110, 111, (32, 256))
        emb = np.clip(proto[rng.randint(0, 32, (F, N))] + rng.randint(-10, 11, (F, N, 256)), -127, 127).astype(np.int8)
        cs = list(range(0, F + 1, T))
        dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
        demb = torch.from_numpy(emb).cuda()
        dcs = torch.tensor(cs, dtype=torch.int32, device="cuda")
        ws = torch.empty(L.TRACK_SORT_WS_PER_ROW * F * N + L.TRACK_SORT_APP_WS_PER_CLIP * a.tclips, dtype=torch.uint8, device="cuda")
        for max_age in (1, 7):
            sort_call = lambda: ops.track_sort(*dv, clip_start=dcs, num_class=C, max_age=max_age, ws=ws)
            app_call = lambda: ops.track_sort_app(*dv, demb, clip_start=dcs, num_class=C, max_age=max_age, ws=ws)
            ts, ta = [], []
            for _ in range(a.blocks):                              # alternating blocks in one process
                ts.append(_event_ms(sort_call, a.reps))
                ta.append(_event_ms(app_call, a.reps))
            hc = min(a.host_clips, a.tclips)
            want = app_sort_host(ids[:hc * T], scores[:hc * T], bboxes[:hc * T], emb[:hc * T], clip_start=cs[:hc + 1], num_class=C,
                                 max_age=max_age)
            got = app_call()
            torch.cuda.synchronize()
            emit(dict(what="track_sort_app", clips=a.tclips, frames=T, rows_per_frame=N, max_age=max_age,
                      detections_per_frame=round(float((ids >= 0).sum()) / F, 1), vd_track_sort_ms_per_call=[round(t, 4) for t in ts],
                      vd_track_sort_app_ms_per_call=[round(t, 4) for t in ta], vd_track_sort_median_ms=round(med(ts), 4),
                      vd_track_sort_app_median_ms=round(med(ta), 4), same_result=_same(got, want, hc * T)))


def share(a, emit):
    from viddet_amd import ops
    from viddet_amd.data import SyntheticTracks
    from viddet_amd.model import yolo3_darknet53
    ds = SyntheticTracks("vid", num_videos=1, frames_per_video=a.frames)
    net = yolo3_darknet53(ds.classes, k=3, k_join_type="max", k_join_pos="early")
    net.initialize(init="he", obj_bias=-2.0)
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    x = torch.randn(a.frames, 3, a.size, a.size, generator=torch.Generator().manual_seed(3)).cuda()

    def run(track):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = net.detect_video(x, chunk=8, track=track)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    sort, app = dict(method="sort"), dict(method="sort", appearance=True)
    run(None), run(sort), run(app)                                 # plans, tuning, code objects
    tp, ts, ta = [], [], []
    for _ in range(a.blocks):
        tp.append(run(None)[0])
        ts.append(run(sort)[0])
        ta.append(run(app)[0])
    plain = [t.clone() for t in run(app)[1]]
    emb, C = net.last_embeddings, len(ds.classes)
    k_sort = _event_ms(lambda: ops.track_sort(*plain, num_class=C), a.reps)
    k_app = _event_ms(lambda: ops.track_sort_app(*plain, emb, num_class=C), a.reps)
    emit(dict(what="detect_video", weights="untrained (He initialisation)", frames=a.frames, size=a.size, k=3,
              rows_per_frame=int(plain[0].shape[1]), detections_per_frame=round(float((plain[0] >= 0).sum()) / a.frames, 1),
              plain_s=[round(t, 4) for t in tp], with_sort_s=[round(t, 4) for t in ts], with_appearance_s=[round(t, 4) for t in ta],
              plain_median_s=round(med(tp), 4), with_sort_median_s=round(med(ts), 4), with_appearance_median_s=round(med(ta), 4),
              track_sort_ms=round(k_sort, 4), track_sort_app_ms=round(k_app, 4),
              appearance_share_of_sort_run=round((med(ta) - med(ts)) / med(ts), 5)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--tclips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dets", default="10,100", help="detections per frame, one timing each")
    ap.add_argument("--sigma_app", default="0.8,0.5", help="one quality run each")
    ap.add_argument("--host_clips", type=int, default=2)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=0.04, help="sigma of the box noise, as a share of the box's size")
    ap.add_argument("--drop", type=float, default=0.1, help="the share of ground-truth rows left out")
    ap.add_argument("--no_share", action="store_true", help="skip the detect_video part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/appearance_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    a.dets = [int(s) for s in a.dets.split(",")]
    a.sigma_app = [float(s) for s in a.sigma_app.split(",")]
    results = []

    def emit(d):
        results.append(d)
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    separation_and_quality(a, emit)
    device(a, emit)
    if not a.no_share:
        share(a, emit)
    if not all(d.get("same_result", True) for d in results):
        raise SystemExit("a device result differs from its host definition")


if __name__ == "__main__":
    main()
