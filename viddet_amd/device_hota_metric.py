"""The HOTA tracking metric with the per-frame matching on the device (detect_yolo3.py --track --metrics hota --device_metric,
DESIGN.md 35).

`HOTAMetric.get()` matches every frame in NumPy.  `DeviceHOTAMetric.get()` packs the clips as the host class does (padded to the
largest G and N present), ranks every clip's ids so that they are dense (np.unique: the matching reads ids only for equality),
uploads the clips in chunks of whole clips (pinned, one copy per chunk), launches vd_hota_match
(viddet_amd/csrc/vd_hota_eval.hip) once per chunk, downloads every chunk's records in ONE copy and hands them to the
accumulation the host class uses (hota_metric.hota_summary): the counts and the float64 sums stay on the host.

A chunk holds at most CHUNK_BYTES of padded rows and its workspace - per clip 8 * A * P + 4 * A + 4 * P bytes with A, P the
largest numbers of ground-truth ids and of track ids of a clip in the chunk - at most WS_BYTES; a clip that is beyond either
alone is a chunk of its own for the rows and refused for the workspace.

This module imports NumPy only; torch is imported where a device tensor is touched.
"""
import time

import numpy as np

from .hota_metric import HOTAMetric, format_summary, hota_summary
from .mot_metric import MAX_GT_ID, masked_track, pack_clips

CHUNK_BYTES = 32 << 20          # the padded rows of one upload
WS_BYTES = 256 << 20            # the workspace of one launch group


def dense_ids(table, clip_start):
    """table (F,K) of ids, -1 or below: none -> (the ids of every clip replaced by their rank among the clip's ids >= 0, int32,
    the others -1; the number of ids of every clip)"""
    table = np.asarray(table)
    out = np.full(table.shape, -1, dtype=np.int32)
    counts = []
    for t0, t1 in zip(clip_start[:-1], clip_start[1:]):
        part = table[t0:t1]
        on = part >= 0
        ids, rank = np.unique(part[on], return_inverse=True)
        out[t0:t1][on] = rank
        counts.append(len(ids))
    return out, counts


def clip_chunks(clip_start, G, N, num_gt, num_pred, chunk_bytes=CHUNK_BYTES, ws_bytes=WS_BYTES):
    """[(first clip, end clip, A, P)]: runs of whole clips whose rows - 24 bytes a label row, 28 a prediction row - stay within
    chunk_bytes (a clip that is larger alone is a chunk of its own) and whose workspace, clips * (8 * A * P + 4 * A + 4 * P) at
    the run's largest A = max(1, num_gt) and P = max(1, num_pred), stays within ws_bytes.  ValueError naming the clip whose
    workspace is beyond ws_bytes alone."""
    per_frame = 24 * G + 28 * N
    need = lambda v, a, p: v * (8 * a * p + 4 * a + 4 * p)
    out, lo = [], 0
    V = len(clip_start) - 1
    while lo < V:
        A, P = max(1, num_gt[lo]), max(1, num_pred[lo])
        if need(1, A, P) > ws_bytes:
            raise ValueError("DeviceHOTAMetric: clip %d holds %d ground-truth tracks and %d prediction tracks, its workspace of %d "
                             "bytes is beyond the %d taken" % (lo, num_gt[lo], num_pred[lo], need(1, A, P), ws_bytes))
        hi = lo + 1
        while hi < V and (clip_start[hi + 1] - clip_start[lo]) * per_frame <= chunk_bytes:
            a, p = max(A, num_gt[hi]), max(P, num_pred[hi])
            if need(hi + 1 - lo, a, p) > ws_bytes:
                break
            A, P, hi = a, p, hi + 1
        out.append((lo, hi, A, P))
        lo = hi
    return out


class DeviceHOTAMetric(HOTAMetric):
    """HOTAMetric whose per-frame matching runs in vd_hota_match.  update() is inherited (host rows); get() returns what the host
    class returns, equal in every character.  `timings` holds the seconds of the last get(): pack, upload, launch (both by
    device events), enqueue, download, summary."""

    def __init__(self, dataset, agnostic=False, chunk_bytes=CHUNK_BYTES, ws_bytes=WS_BYTES):
        super().__init__(dataset, agnostic)
        self.chunk_bytes = int(chunk_bytes)
        self.ws_bytes = int(ws_bytes)
        self.timings = {}

    def get(self):
        import torch
        from . import ops
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceHOTAMetric needs the GPU: vd_hota_match has no host fallback (HOTAMetric is the host metric)")
        t0 = time.perf_counter()
        arrays, cs = pack_clips(self.dataset, self._results)
        F, G, N = arrays[0].shape[0], arrays[0].shape[1], arrays[5].shape[1]
        track = masked_track(arrays[3], arrays[4], arrays[6], self._num_class())
        dense_gt, num_gt = dense_ids(arrays[2], cs)                              # pack_clips keeps them inside [0, 1024)
        dense_track, num_pred = dense_ids(track, cs)
        assert max(num_gt + [0]) <= MAX_GT_ID
        sent = list(arrays)
        sent[2], sent[6] = dense_gt, dense_track
        chunks = clip_chunks(cs, G, N, num_gt, num_pred, self.chunk_bytes, self.ws_bytes)
        t1 = time.perf_counter()
        dev = torch.device("cuda", torch.cuda.current_device())
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * len(chunks) + 1)]
        outs = []
        if ev:
            ev[0].record()
        for k, (lo, hi, A, P) in enumerate(chunks):
            a, b = cs[lo], cs[hi]
            f = b - a
            # every array is 4 bytes an element: one int32 buffer, the clip offsets (from 0) first, padded to 16 bytes
            offs = np.zeros(-(-(hi - lo + 1) // 4) * 4, dtype=np.int32)
            offs[:hi - lo + 1] = np.asarray(cs[lo:hi + 1], dtype=np.int32) - a
            order = (0, 5, 1, 2, 3, 4, 6)                                       # the two box arrays first: they stay 16-byte aligned
            parts = [offs] + [np.ascontiguousarray(sent[i][a:b]).reshape(-1).view(np.int32) for i in order]
            host = torch.from_numpy(np.concatenate(parts)).pin_memory()
            buf = host.to(dev, non_blocking=True)                               # ONE upload per chunk
            ev[2 * k + 1].record()
            at, views = len(offs), [None] * 7
            for i in order:
                x = sent[i]
                n = f * int(np.prod(x.shape[1:]))
                views[i] = buf[at:at + n].view(torch.float32 if x.dtype == np.float32 else torch.int32).view(f, *x.shape[1:])
                at += n
            out = ops.hota_match(*views, num_gt_id=A, num_track=P, clip_start=buf[:hi - lo + 1], num_class=self._num_class(),
                                 agnostic=self._agnostic)
            ev[2 * k + 2].record()
            outs.append(torch.cat([o.view(torch.int32).reshape(-1) for o in out]))
        t2 = time.perf_counter()
        raw = torch.cat(outs).cpu().numpy() if outs else np.zeros(0, np.int32)  # ONE download
        t3 = time.perf_counter()
        up = sum(ev[2 * k].elapsed_time(ev[2 * k + 1]) for k in range(len(chunks))) * 1e-3
        launch = sum(ev[2 * k + 1].elapsed_time(ev[2 * k + 2]) for k in range(len(chunks))) * 1e-3
        match, mscore = np.empty((F, G), np.int32), np.empty((F, G), np.int32)
        msim = np.empty((F, G), np.float32)
        at = 0
        for lo, hi, _, _ in chunks:
            a, b = cs[lo], cs[hi]
            n = (b - a) * G
            match[a:b] = raw[at:at + n].reshape(-1, G)
            msim[a:b] = raw[at + n:at + 2 * n].view(np.float32).reshape(-1, G)
            mscore[a:b] = raw[at + 2 * n:at + 3 * n].reshape(-1, G)
            at += 3 * n
        self.summary = hota_summary((match, msim, mscore), arrays[2], track, cs)
        t4 = time.perf_counter()
        self.timings = dict(pack=t1 - t0, upload=up, launch=launch, enqueue=t2 - t1, download=t3 - t2, summary=t4 - t3)
        return format_summary(self.summary["all"])
