#!/usr/bin/env python
"""Developer tool: camera-motion compensation on the device (vd_motion.hip, ops.motion_*).

In ONE process:

  sig      vd_motion_sig ms per launch on --frames (16) frames of every --sizes (360x480,720x1280), RGB and NV12, at --cell, and
           GB/s on the bytes it reads (the luma's source bytes: all of RGB, the Y plane of NV12) beside Tensor.copy_ of the same
           frames (which reads and writes every byte) - device events around --reps replays of the call captured into a graph
  match    vd_motion_match ms per call on the last size's signatures at --radii (4,8,16)
  video    net.detect_video(track=sort) with and without gmc on a --video_frames (64) clip of the first size at --data_shape
  gate     the distribution of sad_best / sad_zero on SyntheticPan's frames (exact translates) and on SyntheticVideo's
           uncorrelated frames: what the gate separates
  quality  MOTA, IDF1, id switches and HOTA on SyntheticPan's ground truth, jittered and thinned as tools/track_probe.py does
           it, through every tracker with and without gmc (the motion estimated on the device from the clips' frames)

alternating blocks, median of --blocks; every device result is compared with the definition's on the way: that it is equal is
the pass condition, no speed or quality is asked for.  Needs a GPU: there is no fallback.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from overlay_probe import _graph_ms
from seq_nms_probe import _event_ms

med = statistics.median


def sig_probe(a, size, fmt):
    from viddet_amd import motion as M, ops
    from viddet_amd.video import rgb_to_nv12
    rgb = np.random.default_rng(1).integers(0, 256, (a.frames,) + size + (3,), dtype=np.uint8)
    frames = rgb if fmt == "rgb" else rgb_to_nv12(rgb)
    src = torch.from_numpy(frames).cuda()
    dst = torch.empty_like(src)
    out = ops.motion_signature(src, cell=a.cell, fmt=fmt)
    run = lambda: ops.motion_signature(src, cell=a.cell, fmt=fmt, out=out)
    copy = lambda: dst.copy_(src)
    t_sig, t_copy = [], []
    for _ in range(a.blocks):
        t_sig.append(_graph_ms(run, a.reps))
        t_copy.append(_graph_ms(copy, a.reps))
    torch.cuda.synchronize()
    same = bool(np.array_equal(out[:2].cpu().numpy(), M.signature_host(frames[:2], a.cell, fmt)))
    read = a.frames * size[0] * size[1] * (3 if fmt == "rgb" else 1)
    return dict(what="sig", fmt=fmt, size="%dx%d" % size, frames=a.frames, cell=a.cell, ms_per_launch=[round(t, 4) for t in t_sig],
                median_ms=round(med(t_sig), 4), read_gb_s=round(read / (med(t_sig) * 1e-3) / 1e9, 1), copy_median_ms=round(med(t_copy), 4),
                copy_gb_s=round(2.0 * frames.nbytes / (med(t_copy) * 1e-3) / 1e9, 1), same_result=same), out


def match_probe(a, sig, size, radius):
    from viddet_amd import motion as M, ops
    ws = torch.empty(8 * sig.shape[0] * (2 * radius + 1) ** 2, dtype=torch.uint8, device="cuda")
    run = lambda: ops.motion_match(sig, radius=radius, cell=a.cell, ws=ws)
    ts = [_graph_ms(run, a.reps) for _ in range(a.blocks)]
    got = run()
    torch.cuda.synchronize()
    want = M.match_host(sig[:3].cpu().numpy(), radius=radius, cell=a.cell)
    same = bool(np.array_equal(got[0][:3].cpu().numpy(), want[0]) and np.array_equal(got[1][:3].cpu().numpy(), want[1]))
    return dict(what="match", size="%dx%d" % size, frames=int(sig.shape[0]), cell=a.cell, radius=radius, grid="%dx%d" % tuple(sig.shape[1:]),
                median_ms=round(med(ts), 4), ms_per_call=[round(t, 4) for t in ts], same_result=same)


def video(a, size):
    from viddet_amd.data import SyntheticPan
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["class%d" % i for i in range(20)])
    net.initialize(init="he", obj_bias=0.0)
    net.set_device_resize(a.data_shape, a.data_shape)
    ds = SyntheticPan("vid", num_videos=1, frames_per_video=a.video_frames, size=(size[1], size[0]), pan=a.pan, cell=a.cell)
    x = torch.from_numpy(ds.video_frames(0)).cuda()
    plain = lambda: net.detect_video(x, chunk=8, track=dict(method="sort"))
    gmc = lambda: net.detect_video(x, chunk=8, track=dict(method="sort", gmc=dict(cell=a.cell)))
    tp, tg = [], []
    for _ in range(a.blocks):
        tp.append(_event_ms(plain, 1))
        tg.append(_event_ms(gmc, 1))
    same = bool(np.array_equal(np.cumsum(net.last_motion[0].cpu().numpy(), axis=0), -ds.camera_path(0)))
    return dict(what="video", size="%dx%d" % size, frames=a.video_frames, data_shape=a.data_shape, detect_video_sort_median_ms=round(med(tp), 3),
                with_gmc_median_ms=round(med(tg), 3), gmc_share=round((med(tg) - med(tp)) / med(tg), 4), same_result=same)


def _device_motion(a, frames, radius=8):
    from viddet_amd import ops
    sig = ops.motion_signature(torch.from_numpy(frames).cuda(), cell=a.cell)
    return ops.motion_match(sig, radius=radius, gate=1.0, cell=a.cell)


def gate(a):
    """sad_best / sad_zero at gate 1.0 (nothing refused): translates of one canvas against frames without a common motion"""
    from viddet_amd.data import SyntheticPan, SyntheticVideo
    out = {}
    for name, ds in (("pan", SyntheticPan("vid", num_videos=a.clips, frames_per_video=a.clip_frames, pan=a.pan, cell=a.cell)),
                     ("uncorrelated", SyntheticVideo("vid", num_videos=a.clips, frames_per_video=a.clip_frames))):
        r = []
        for v in range(ds.num_videos):
            sad = _device_motion(a, ds.video_frames(v))[1].cpu().numpy()[1:]
            r += (sad[:, 0] / np.maximum(sad[:, 1], 1)).tolist()
        out[name] = dict(min=round(min(r), 4), median=round(med(r), 4), max=round(max(r), 4), pairs=len(r))
    return dict(what="gate", cell=a.cell, radius=8, ratio=out)


def quality(a):
    from viddet_amd import motion as M, ops
    from viddet_amd.data import SyntheticPan
    from viddet_amd.hota_metric import hota_match_host, hota_summary
    from viddet_amd.mot_metric import masked_track, mot_match_host, mot_summary
    ds = SyntheticPan("vid", num_videos=a.clips, frames_per_video=a.clip_frames, pan=a.pan, cell=a.cell)
    rng = np.random.default_rng(7)
    T, V = ds.frames_per_video, ds.num_videos
    labels = [ds.get_label(sid) for sid in ds.get_sample_ids()]
    F, N = len(labels), max(1, max(len(l) for l in labels))
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    gt_boxes, gt_cls, gt_id = -np.ones((F, N, 4), np.float32), -np.ones((F, N), np.int32), -np.ones((F, N), np.int32)
    for t, l in enumerate(labels):
        g = len(l)
        gt_boxes[t, :g], gt_cls[t, :g], gt_id[t, :g] = l[:, :4], l[:, 4], l[:, 5]
        keep = l[rng.uniform(size=len(l)) >= a.drop]
        wh = np.stack([keep[:, 2] - keep[:, 0], keep[:, 3] - keep[:, 1]] * 2, axis=1)
        n = len(keep)
        ids[t, :n, 0], scores[t, :n, 0], bboxes[t, :n] = keep[:, 4], 0.9, keep[:, :4] + rng.normal(0.0, a.jitter, (n, 4)) * wh
    cs = list(range(0, F + 1, T))
    cum, same = [], True
    for v in range(V):
        motion, _, c = _device_motion(a, ds.video_frames(v))
        same &= bool(np.array_equal(np.cumsum(motion.cpu().numpy(), axis=0), -ds.camera_path(v)))
        cum.append(c)
    dv = [torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)]
    stab = ops.motion_shift(dv[0], dv[2], torch.cat(cum), 1.0, 1.0, -1)
    same &= bool(np.array_equal(stab.cpu().numpy(), M.stabilise_host(ids, bboxes, -np.concatenate(
        [np.diff(ds.camera_path(v), axis=0, prepend=0) for v in range(V)]), cs, 1.0, 1.0), equal_nan=True))
    C = len(ds.classes)
    rows = []
    for name, link in (("iou", ops.track), ("sort", ops.track_sort), ("byte", ops.track_byte)):
        for on, bx in ((False, dv[2]), (True, stab)):
            track = link(dv[0], dv[1], bx, clip_start=cs, num_class=C)[0].cpu().numpy()
            tr = masked_track(ids, scores, track, C)
            mot = mot_summary(mot_match_host(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, tr, cs, C), gt_id, tr, cs)["all"]
            hota = hota_summary(hota_match_host(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, tr, cs, C), gt_id, tr, cs)["all"]
            rows.append(dict(tracker=name, gmc=on, MOTA=round(mot["MOTA"], 4), IDF1=round(mot["IDF1"], 4), IDSW=int(mot["IDSW"]),
                             HOTA=round(hota["HOTA"], 4)))
    return dict(what="quality", clips=V, frames=T, pan=a.pan, jitter=a.jitter, drop=a.drop, rows=rows, same_result=same)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="360x480,720x1280", help="source sizes H0xW0")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--formats", default="rgb,nv12")
    ap.add_argument("--cell", type=int, default=4)
    ap.add_argument("--radii", default="4,8,16")
    ap.add_argument("--pan", type=int, default=24)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--clip_frames", type=int, default=32)
    ap.add_argument("--jitter", type=float, default=0.03)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--video_frames", type=int, default=64)
    ap.add_argument("--data_shape", type=int, default=416)
    ap.add_argument("--no_video", action="store_true", help="skip the detect_video part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/motion_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    results = []

    def emit(d):
        results.append(d)
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    sig = None
    for fmt in a.formats.split(","):
        for size in sizes:
            d, sig = sig_probe(a, size, fmt)
            emit(d)
    for radius in [int(r) for r in a.radii.split(",")]:
        emit(match_probe(a, sig, sizes[-1], radius))
    if not a.no_video:
        emit(video(a, sizes[0]))
    emit(gate(a))
    emit(quality(a))
    if not all(d.get("same_result", True) for d in results):
        raise SystemExit("a device result differs from the definition's")


if __name__ == "__main__":
    main()
