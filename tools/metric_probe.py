#!/usr/bin/env python
"""Developer tool: the VOC mAP matching on the device (train_yolov3.py --device_metric) against the host metric
behind the same validation loop.

In ONE process, at --size (416) / --batch (64) / --classes (20):

  host      VOCMApMetric.update ms per image on one core (median over the images of one batch of real detections)
  kernel    vd_voc_match ms per launch (device events) on that batch; update_device (upload + launch) ms per batch
  validate  wall time of train_yolov3.py's validate() over --batches batches of SyntheticDetection with either metric,
            alternating blocks, median of --blocks (host clock; validate() ends in the metric's get(), which has read the
            device's results); the two results are compared on the way

Needs a GPU: there is no fallback.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch


def _event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def probe(a):
    import train_yolov3 as T
    from viddet_amd import ops
    from viddet_amd.data import Loader, SyntheticDetection, YOLO3VideoInferenceTransform
    from viddet_amd.metrics import DeviceVOCMApMetric, VOCMApMetric
    from viddet_amd.model import yolo3_darknet53
    T.FLAGS = T.parse_flags([])
    ds = SyntheticDetection("synthetic", num_samples=a.batch * a.batches, num_class=a.classes)
    net = yolo3_darknet53(ds.classes)
    net.initialize(init="he", seed=1)
    loader = Loader(ds, YOLO3VideoInferenceTransform(a.size, a.size, device_normalize=True), a.batch, train=False, last_batch="keep")
    try:
        # one batch of the network's own detections for the two micro-timings
        net.set_nms(nms_thresh=0.45, nms_topk=400)
        batch = next(iter(loader))
        ids, scores, bboxes = [t.clone() for t in net(torch.from_numpy(batch[0]).cuda())]
        label = batch[-2]
        torch.cuda.synchronize()
        h_ids, h_scores, h_boxes = ids.cpu().numpy(), scores.cpu().numpy(), np.clip(bboxes.cpu().numpy(), 0, a.size)
        host = VOCMApMetric(0.5, ds.classes)
        ts = []
        with np.errstate(all="ignore"):
            for j in range(len(h_ids)):
                t0 = time.perf_counter()
                host.update([h_boxes[j]], [h_ids[j]], [h_scores[j]], [label[j][..., :4]], [label[j][..., 4:5]], None)
                ts.append(time.perf_counter() - t0)
        B, N = h_ids.shape[:2]
        gt = torch.from_numpy(np.ascontiguousarray(label, np.float32)).cuda()
        rec = (torch.empty((B, N), dtype=torch.int32, device="cuda"), torch.empty((B, N), device="cuda"),
               torch.empty((B, N), dtype=torch.int8, device="cuda"))
        counts = torch.zeros((2, a.classes), dtype=torch.int32, device="cuda")
        f = lambda t: t.reshape(B, -1).contiguous()
        k_ms = _event_ms(lambda: ops.voc_match(f(ids), f(scores), bboxes.contiguous(), gt, float(a.size), 0.5, *rec, counts[0],
                                               counts[1]), a.reps)
        dev = DeviceVOCMApMetric(0.5, ds.classes)
        u_ms = _event_ms(lambda: dev.update_device(ids, scores, bboxes, label, clip=a.size), 20)
        res = dict(size=a.size, batch=a.batch, classes=a.classes, batches=a.batches, N=int(N), M=int(label.shape[1]),
                   detections_per_image=round(float((h_ids >= 0).sum()) / B, 1),
                   host_update_ms_per_image=round(1e3 * statistics.median(ts), 4),
                   kernel_ms_per_launch=round(k_ms, 4), update_device_ms_per_batch=round(u_ms, 4))

        def run(metric):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with np.errstate(all="ignore"):
                out = T.validate(net, loader, metric, a.size)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        mh, md = VOCMApMetric(0.5, ds.classes), DeviceVOCMApMetric(0.5, ds.classes)
        run(mh), run(md)                                           # plans, tuning, code objects
        th, td = [], []
        for _ in range(a.blocks):                                  # alternating blocks in one process
            t, oh = run(mh)
            th.append(t)
            t, od = run(md)
            td.append(t)
        same = oh[0] == od[0] and np.array_equal(np.asarray(oh[1]), np.asarray(od[1]), equal_nan=True)
        images = a.batch * a.batches
        res["validate"] = dict(images=images, host_s=[round(t, 4) for t in th], device_s=[round(t, 4) for t in td],
                               host_ms_per_image=round(1e3 * statistics.median(th) / images, 4),
                               device_ms_per_image=round(1e3 * statistics.median(td) / images, 4),
                               ratio=round(statistics.median(th) / statistics.median(td), 3), same_result=bool(same),
                               mAP=None if np.isnan(od[1][-1]) else float(od[1][-1]))
    finally:
        loader.close()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/metric_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    line = json.dumps(probe(a))
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
