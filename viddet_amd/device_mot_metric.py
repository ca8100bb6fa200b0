"""The MOT tracking metric with the per-frame matching on the device (detect_yolo3.py --track --metrics mot --device_metric,
DESIGN.md 33).

`MOTMetric.get()` matches every frame in NumPy.  `DeviceMOTMetric.get()` packs the clips as the host class does (padded to the
largest G and N present), uploads them in chunks of whole clips (pinned, one copy per chunk), launches vd_mot_match
(viddet_amd/csrc/vd_mot_eval.hip) once per chunk, downloads every chunk's records in ONE copy and hands them to the accumulation
the host class uses (mot_metric.mot_summary): the counts, the float64 sums and the identity pairing stay on the host.

This module imports NumPy only; torch is imported where a device tensor is touched.
"""
import time

import numpy as np

from .mot_metric import MOTMetric, format_summary, masked_track, mot_summary, pack_clips

CHUNK_BYTES = 32 << 20          # the padded rows of one upload


def clip_chunks(clip_start, G, N, chunk_bytes=CHUNK_BYTES):
    """[(first clip, end clip)]: runs of whole clips whose rows - 24 bytes a label row, 28 a prediction row - stay within
    chunk_bytes (a clip that is larger alone is a chunk of its own)"""
    per_frame = 24 * G + 28 * N
    out, lo = [], 0
    V = len(clip_start) - 1
    while lo < V:
        hi = lo + 1
        while hi < V and (clip_start[hi + 1] - clip_start[lo]) * per_frame <= chunk_bytes:
            hi += 1
        out.append((lo, hi))
        lo = hi
    return out


class DeviceMOTMetric(MOTMetric):
    """MOTMetric whose per-frame matching runs in vd_mot_match.  update() is inherited (host rows); get() returns what the host
    class returns, equal in every character.  `timings` holds the seconds of the last get(): pack, upload, launch (both by
    device events), enqueue, download, summary."""

    def __init__(self, dataset, iou_thresh=0.5, agnostic=False, chunk_bytes=CHUNK_BYTES):
        super().__init__(dataset, iou_thresh, agnostic)
        self.chunk_bytes = int(chunk_bytes)
        self.timings = {}

    def get(self):
        import torch
        from . import ops
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceMOTMetric needs the GPU: vd_mot_match has no host fallback (MOTMetric is the host metric)")
        t0 = time.perf_counter()
        arrays, cs = pack_clips(self.dataset, self._results)
        F, G, N = arrays[0].shape[0], arrays[0].shape[1], arrays[5].shape[1]
        chunks = clip_chunks(cs, G, N, self.chunk_bytes)
        t1 = time.perf_counter()
        dev = torch.device("cuda", torch.cuda.current_device())
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * len(chunks) + 1)]
        outs = []
        if ev:
            ev[0].record()
        for k, (lo, hi) in enumerate(chunks):
            a, b = cs[lo], cs[hi]
            f = b - a
            # every array is 4 bytes an element: one int32 buffer, the clip offsets (from 0) first, padded to 16 bytes
            offs = np.zeros(-(-(hi - lo + 1) // 4) * 4, dtype=np.int32)
            offs[:hi - lo + 1] = np.asarray(cs[lo:hi + 1], dtype=np.int32) - a
            order = (0, 5, 1, 2, 3, 4, 6)                                       # the two box arrays first: they stay 16-byte aligned
            parts = [offs] + [np.ascontiguousarray(arrays[i][a:b]).reshape(-1).view(np.int32) for i in order]
            host = torch.from_numpy(np.concatenate(parts)).pin_memory()
            buf = host.to(dev, non_blocking=True)                               # ONE upload per chunk
            ev[2 * k + 1].record()
            at, views = len(offs), [None] * 7
            for i in order:
                x = arrays[i]
                n = f * int(np.prod(x.shape[1:]))
                views[i] = buf[at:at + n].view(torch.float32 if x.dtype == np.float32 else torch.int32).view(f, *x.shape[1:])
                at += n
            out = ops.mot_match(*views, clip_start=buf[:hi - lo + 1], num_class=self._num_class(), iou_thresh=self._iou_thresh,
                                agnostic=self._agnostic)
            ev[2 * k + 2].record()
            outs.append(torch.cat([o.view(torch.int32).reshape(-1) for o in out]))
        t2 = time.perf_counter()
        raw = torch.cat(outs).cpu().numpy() if outs else np.zeros(0, np.int32)  # ONE download
        t3 = time.perf_counter()
        up = sum(ev[2 * k].elapsed_time(ev[2 * k + 1]) for k in range(len(chunks))) * 1e-3
        launch = sum(ev[2 * k + 1].elapsed_time(ev[2 * k + 2]) for k in range(len(chunks))) * 1e-3
        match, flags = np.empty((F, G), np.int32), np.empty((F, G), np.int32)
        miou, adm = np.empty((F, G), np.float32), np.empty((F, G, 4), np.uint32)
        at = 0
        for lo, hi in chunks:
            a, b = cs[lo], cs[hi]
            n = (b - a) * G
            match[a:b] = raw[at:at + n].reshape(-1, G)
            miou[a:b] = raw[at + n:at + 2 * n].view(np.float32).reshape(-1, G)
            flags[a:b] = raw[at + 2 * n:at + 3 * n].reshape(-1, G)
            adm[a:b] = raw[at + 3 * n:at + 7 * n].view(np.uint32).reshape(-1, G, 4)
            at += 7 * n
        self.summary = mot_summary((match, miou, flags, adm), arrays[2],
                                   masked_track(arrays[3], arrays[4], arrays[6], self._num_class()), cs)
        t4 = time.perf_counter()
        self.timings = dict(pack=t1 - t0, upload=up, launch=launch, enqueue=t2 - t1, download=t3 - t2, summary=t4 - t3)
        return format_summary(self.summary["all"])
