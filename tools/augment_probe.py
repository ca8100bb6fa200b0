#!/usr/bin/env python
"""Developer tool: the training augmentation with its pixels on the device (train_yolov3.py --device_augment)
against the host transform in front of the same training step.

For --source (360x480) frames and a --size (416) target, in ONE process:

  host      YOLO3VideoTrainTransform ms per sample on one core, with and without device_augment (the decisions alone);
            median of --host_reps samples, the same seeds for both
  kernel    vd_augment_u8_nchw ms per launch on one loader batch of --batch samples (device events) and GB/s on the bytes the
            operator has to move (source uint8 read once + fp32 planes written); the packed upload + launch as
            augment_on_device runs them, ms per batch
  loop      frames/s of train_yolov3.py's loop (loader batch -> device -> forward, backward, SGD step) over --batches batches,
            the host loader against the device_augment loader, for num_workers 0 and --workers; alternating blocks, median of
            --blocks (host clock around work that ends in a device synchronise)

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


def host_ms(ds, size, classes, reps, device_augment):
    from viddet_amd.data import YOLO3VideoTrainTransform
    from viddet_amd.video import Rng
    tf = YOLO3VideoTrainTransform(size, size, classes, Rng.seeded(1), device_augment=device_augment)
    ts = []
    for i in range(reps):
        sample = ds[i % len(ds)]
        t0 = time.perf_counter()
        tf(*sample)
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts)


def kernel_ms(batch, reps=50):
    from viddet_amd import ops
    from viddet_amd.augment import augment_on_device
    buf, lay = batch.packed()
    dev = torch.from_numpy(buf).cuda()
    sec = {name: dev[off:] for name, (off, _, _) in lay.items()}
    out = torch.empty((batch.N * batch.K, 3, batch.H, batch.W), dtype=torch.float32, device="cuda")

    def run():
        ops.augment_u8_nchw(sec["raw"], sec["src_off"], sec["src_hw"], sec["color"], sec["idx_y"], sec["w_y"], batch.Ty,
                            sec["idx_x"], sec["w_x"], batch.Tx, sec["fill"], out, batch.N, batch.K, batch.H, batch.W)
    ms = _event_ms(run, reps)
    nbytes = batch.raw.size + out.numel() * 4
    whole = _event_ms(lambda: augment_on_device(batch), 10)
    return ms, nbytes / ms / 1e6, whole


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default="360x480")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--host_reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/augment_probe.py needs an MI355X: a timing taken elsewhere says nothing")
    from viddet_amd.augment import augment_on_device
    from viddet_amd.data import Loader, SyntheticDetection, YOLO3VideoTrainTransform
    from viddet_amd.model import yolo3_darknet53
    from viddet_amd.video import Rng
    torch.set_num_threads(1)
    h0, w0 = [int(s) for s in a.source.split("x")]
    ds = SyntheticDetection("synthetic", num_samples=a.batch * a.batches, size=(w0, h0), num_class=a.classes)
    net = yolo3_darknet53(["c%d" % i for i in range(a.classes)])
    net.initialize(init="he", seed=1)

    def loader(device_augment, workers):
        tf = YOLO3VideoTrainTransform(a.size, a.size, a.classes, Rng.seeded(1), device_augment=device_augment)
        return Loader(ds, tf, a.batch, train=True, shuffle=True, seed=1, num_workers=workers)

    def epoch(ld, device_augment):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for batch in ld:
            x = augment_on_device(batch[0]) if device_augment else torch.from_numpy(batch[0]).cuda()
            dv = [torch.from_numpy(b).cuda() for b in batch[1:]]
            net(x, dv[5], *dv[0:5])
            net.backward()
            net.sgd_step(1e-4, 0.9, 5e-4, a.batch)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    first = next(iter(loader(True, 0)))[0]
    k_ms, k_gbps, whole_ms = kernel_ms(first)
    res = dict(source=[h0, w0], target=a.size, batch=a.batch, batches=a.batches, Ty=first.Ty, Tx=first.Tx,
               host_transform_ms_per_sample=round(host_ms(ds, a.size, a.classes, a.host_reps, False), 2),
               host_decisions_ms_per_sample=round(host_ms(ds, a.size, a.classes, a.host_reps, True), 2),
               kernel_ms_per_launch=round(k_ms, 4), kernel_gbps=round(k_gbps, 1), upload_and_launch_ms_per_batch=round(whole_ms, 3))
    frames = a.batch * a.batches
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
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
