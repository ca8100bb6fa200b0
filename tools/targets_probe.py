#!/usr/bin/env python
"""Developer tool: the YOLO prefetch targets on the device (train_yolov3.py --device_targets) against the host
generator in front of the same training step.

For each --shapes entry `size:classes:batch` (default 416:80:64 and 608:285:32), in ONE process:

  host      viddet_amd.targets.prefetch_targets ms per sample on one core (median of --host_reps samples) and the bytes a step
            uploads on either path: the five dense columns + gt, or the label rows
  kernel    vd_yolo_targets ms per call (both launches, device events) on one loader batch and GB/s on the bytes it writes;
            the upload + call as targets_on_device runs them, ms per batch
  loop      frames/s of train_yolov3.py's loop (loader batch -> device -> forward, backward, SGD step) over --batches batches,
            the host loader against the device_targets loader, for num_workers 0 and --workers; alternating blocks, median of
            --blocks (host clock around work that ends in a device synchronise)

Needs a GPU: there is no fallback.  Prints one JSON line per shape.
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


def host_ms(labels, size, classes, reps):
    from viddet_amd.targets import prefetch_targets
    ts = []
    for i in range(reps):
        lab = labels[i % len(labels)][np.newaxis]
        t0 = time.perf_counter()
        prefetch_targets(size, size, lab[..., :4], lab[..., 4:5], classes)
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def kernel_ms(labels, size, classes, reps=50):
    from viddet_amd import ops
    from viddet_amd.device_targets import num_rows, targets_on_device
    N, M, _ = labels.shape
    P = num_rows(size, size)
    gt = torch.from_numpy(np.ascontiguousarray(labels[..., :4])).cuda()
    ids = torch.from_numpy(np.ascontiguousarray(labels[..., 4])).cuda()
    out = [torch.empty((N, P, c), dtype=torch.float32, device="cuda") for c in (1, 2, 2, 2, classes)]
    ms = _event_ms(lambda: ops.yolo_targets(gt, ids, 1, None, N, M, classes, size, size, *out), reps)
    written = sum(o.numel() for o in out) * 4
    whole = _event_ms(lambda: targets_on_device(labels, size, size, classes), 10)
    return ms, written / ms / 1e6, whole, written


def probe(a, size, classes, batch):
    from viddet_amd.data import Loader, SyntheticDetection, YOLO3VideoTrainTransform
    from viddet_amd.device_targets import targets_on_device
    from viddet_amd.model import yolo3_darknet53
    from viddet_amd.video import Rng
    h0, w0 = [int(s) for s in a.source.split("x")]
    ds = SyntheticDetection("synthetic", num_samples=batch * a.batches, size=(w0, h0), num_class=classes)
    net = yolo3_darknet53(["c%d" % i for i in range(classes)])
    net.initialize(init="he", seed=1)

    def loader(device_targets, workers):
        tf = YOLO3VideoTrainTransform(size, size, classes, Rng.seeded(1), device_targets=device_targets)
        return Loader(ds, tf, batch, train=True, shuffle=True, seed=1, num_workers=workers)

    def epoch(ld, device_targets):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in ld:
            x = torch.from_numpy(b[0]).cuda()
            if device_targets:
                tg = targets_on_device(b[1], size, size, classes)
                net(x, *tg)
            else:
                dv = [torch.from_numpy(c).cuda() for c in b[1:]]
                net(x, dv[5], *dv[0:5])
            net.backward()
            net.sgd_step(1e-4, 0.9, 5e-4, batch)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    hb, db = next(iter(loader(False, 0))), next(iter(loader(True, 0)))
    k_ms, k_gbps, whole_ms, written = kernel_ms(db[1], size, classes)
    res = dict(target=size, classes=classes, batch=batch, batches=a.batches, M=int(db[1].shape[1]),
               host_prefetch_targets_ms_per_sample=round(host_ms(db[1], size, classes, a.host_reps), 3),
               upload_bytes_per_step_host=int(sum(c.nbytes for c in hb[1:])), upload_bytes_per_step_device=int(db[1].nbytes),
               kernel_ms_per_call=round(k_ms, 4), kernel_bytes_written=int(written), kernel_gbps=round(k_gbps, 1),
               upload_and_call_ms_per_batch=round(whole_ms, 3))
    frames = batch * a.batches
    for workers in (0, a.workers):
        lh, ld = loader(False, workers), loader(True, workers)
        try:
            epoch(lh, False), epoch(ld, True)                      # plans, tuning, code objects, worker start-up
            th, td = [], []
            for _ in range(a.blocks):                              # alternating blocks in one process
                th.append(epoch(lh, False))
                td.append(epoch(ld, True))
        finally:
            lh.close(), ld.close()
        res["loop_workers%d" % workers] = dict(
            host_fps=round(frames / statistics.median(th), 1), device_fps=round(frames / statistics.median(td), 1),
            ratio=round(statistics.median(th) / statistics.median(td), 2),
            host_s=[round(t, 3) for t in th], device_s=[round(t, 3) for t in td])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default="360x480")
    ap.add_argument("--shapes", default="416:80:64,608:285:32", help="comma list of size:classes:batch")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--host_reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/targets_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    torch.set_num_threads(1)
    for shape in a.shapes.split(","):
        size, classes, batch = [int(v) for v in shape.split(":")]
        line = json.dumps(probe(a, size, classes, batch))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
