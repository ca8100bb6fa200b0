#!/usr/bin/env python
"""Developer tool: the COCO detection metric with its matching on the device (detect_yolo3.py --metrics coco --device_metric,
DESIGN.md 26) against the host metric on the same detections.

In ONE process, on SyntheticDetection('coco') (80 classes) with --images (2000) images and about --dets (10,100) synthetic
detections per image (noisy copies of the ground truth and clutter, scores from a ladder so that ties occur):

  host     COCODetectionMetric.get() seconds
  device   DeviceCOCODetectionMetric.get() seconds, split into pack / upload / launch (device events) / download / accumulate
  kernel   vd_coco_match ms per launch (device events, --reps launches) on the first chunk of that set

alternating blocks, median of --blocks; the two results are compared on the way.  Needs a GPU: there is no fallback.
Prints one JSON line per detection count.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch


class LabelSet:
    """SyntheticDetection's labels, drawn once (the metric asks for the rows of every sample at every get())"""

    def __init__(self, ds):
        self.classes, self.sample_ids, self._ds = ds.classes, ds.sample_ids, ds
        self._labels = [ds[i][1] for i in range(len(ds))]

    def __len__(self):
        return len(self._labels)

    def sample_path(self, idx):
        return self._ds.sample_path(idx)

    def image_size(self, sid):
        return self._ds.image_size(sid)

    def get_label(self, sid):
        return self._labels[sid]


def detections(ds, per_image, seed=1):
    """per image (sid, boxes (n,4) xyxy, labels (n,), scores (n,)), n about per_image: up to three noisy copies of every ground
    truth, clutter for the rest"""
    rng = np.random.default_rng(seed)
    out = []
    for sid in ds.sample_ids:
        w, h = ds.image_size(sid)
        lab = ds.get_label(sid)
        n = int(rng.integers(max(1, per_image - per_image // 5), per_image + per_image // 5 + 1))
        k = min(n, 3 * len(lab))
        g = lab[rng.integers(0, len(lab), k)]
        s = np.stack([g[:, 2] - g[:, 0] + 1, g[:, 3] - g[:, 1] + 1] * 2, axis=1)
        box = g[:, :4] + rng.normal(0, 0.05, (k, 4)) * s
        cls = np.where(rng.random(k) < 0.85, g[:, 4], rng.integers(0, len(ds.classes), k))
        xy = rng.uniform(0, (w - 20, h - 20), (n - k, 2))
        wh = np.exp(rng.uniform(np.log(10.0), np.log(250.0), (n - k, 2)))
        box = np.concatenate([box, np.concatenate([xy, xy + wh], axis=1)])
        cls = np.concatenate([cls, rng.integers(0, len(ds.classes), n - k)])
        out.append((sid, box, cls.astype(np.float64), 0.06 + 0.93 * rng.integers(0, 200, n) / 200))
    return out


def _event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def probe(a, ds, per_image):
    from viddet_amd import ops
    from viddet_amd.coco_metric import AREA_RNG, IOU_THRS, COCODetectionMetric
    from viddet_amd.device_coco_metric import DeviceCOCODetectionMetric, pack_images
    host, dev = COCODetectionMetric(ds, None), DeviceCOCODetectionMetric(ds, None)
    for m in (host, dev):
        for sid, box, cls, score in detections(ds, per_image):
            m.update([box[None]], [cls[None]], [score[None]], sid=sid)

    def run(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.get()
        return time.perf_counter() - t0, out

    host.ground_truth(), dev.ground_truth()                        # built once per metric, outside the timed blocks
    run(dev)                                                       # code objects, pinned-memory pools
    th, td, parts = [], [], []
    for _ in range(a.blocks):                                      # alternating blocks in one process
        t, oh = run(host)
        th.append(t)
        t, od = run(dev)
        td.append(t)
        parts.append(dict(dev.timings))
    he, de = host._coco_eval, dev._coco_eval
    same = oh == od and all(np.array_equal(he.eval[k], de.eval[k]) for k in ("precision", "recall"))
    chunks = pack_images(de.imgIds, de.images)
    det, gt = chunks[0]
    B, N, M, K = det.shape[0], det.shape[1], gt.shape[1], len(ds.classes)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    args = (up(det), up(gt), up(IOU_THRS), up(AREA_RNG), i32(B, N), i32(B, N, 4), i32(K, 4))
    k_ms = _event_ms(lambda: ops.coco_match(*args), a.reps)
    med = lambda key: round(statistics.median(p[key] for p in parts), 5)
    ndet = sum(len(d) for d, _ in de.images)
    return dict(images=len(ds), detections=ndet, detections_per_image=round(ndet / len(ds), 1), chunks=len(chunks),
                host_get_s=[round(t, 4) for t in th], device_get_s=[round(t, 4) for t in td],
                host_get_median_s=round(statistics.median(th), 4), device_get_median_s=round(statistics.median(td), 4),
                device_split_s=dict(pack=med("pack"), upload=med("upload"), launch=med("launch"), download=med("download"),
                                    accumulate=med("accumulate")),
                kernel=dict(B=B, N=N, M=M, K=K, ms_per_launch=round(k_ms, 4)), AP=round(float(he.stats[0]), 4), same_result=bool(same))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--dets", default="10,100", help="detections per image, one probe each")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/coco_metric_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    warnings.simplefilter("ignore")
    from viddet_amd.data import SyntheticDetection
    ds = LabelSet(SyntheticDetection("coco", num_samples=a.images))
    for n in [int(s) for s in a.dets.split(",")]:
        line = json.dumps(probe(a, ds, n))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
