"""The COCO detection metric with the per-image matching on the device (detect_yolo3.py --metrics coco --device_metric,
DESIGN.md 26).

`COCODetectionMetric.get()` matches every image in NumPy (coco_metric.match_image).  `DeviceCOCODetectionMetric.get()` packs the
same per-image rows into padded float64 arrays, uploads them chunk by chunk (pinned, one copy per chunk), launches
vd_coco_match (viddet_amd/csrc/vd_coco_eval.hip) once per chunk, downloads every chunk's integer records in ONE copy and hands
them to the host class's own accumulation (coco_metric.accumulate_records): the set-wide sort, the cumulative sums,
precision and recall stay on the host.

This module imports NumPy only; torch is imported where a device tensor is touched.
"""
import time

import numpy as np

from .coco_metric import AREA_RNG, COCODetectionMetric, COCOEval, DET_W, GT_W, IOU_THRS
from .lib import COCO_MATCH_MAX_DET as MAX_DET, COCO_MATCH_MAX_GT as MAX_GT

CHUNK_BYTES = 32 << 20          # padded det + gt rows of one upload


def pack_images(img_ids, images, chunk_bytes=CHUNK_BYTES):
    """images: per image (det (n,6), gt (m,8)) as coco_metric.image_rows gives them, img_ids: their sample ids.  ->
    [(det (b,N,6), gt (b,M,8))] over the images in order, each chunk padded to its own widest image (padded rows: category -1,
    the rest 0) and at most chunk_bytes large (one image is always taken)."""
    ndet = np.array([len(d) for d, _ in images], dtype=np.int64)
    ngt = np.array([len(g) for _, g in images], dtype=np.int64)
    for i in np.nonzero(ndet > MAX_DET)[0]:
        raise ValueError("DeviceCOCODetectionMetric: sample id %s holds %d detections, vd_coco_match takes at most %d"
                         % (img_ids[i], ndet[i], MAX_DET))
    for i in np.nonzero(ngt > MAX_GT)[0]:
        raise ValueError("DeviceCOCODetectionMetric: sample id %s holds %d label rows, vd_coco_match takes at most %d"
                         % (img_ids[i], ngt[i], MAX_GT))
    chunks, lo = [], 0
    while lo < len(images):
        hi, N, M = lo, 0, 0
        while hi < len(images):
            n, m = max(N, int(ndet[hi])), max(M, int(ngt[hi]))
            if hi > lo and (hi + 1 - lo) * (n * DET_W + m * GT_W) * 8 > chunk_bytes:
                break
            hi, N, M = hi + 1, n, m
        det = np.zeros((hi - lo, N, DET_W))
        gt = np.zeros((hi - lo, M, GT_W))
        det[..., 5] = -1.0
        gt[..., 5] = -1.0
        for i in range(lo, hi):
            det[i - lo, :ndet[i]] = images[i][0]
            gt[i - lo, :ngt[i]] = images[i][1]
        chunks.append((det, gt))
        lo = hi
    return chunks


def unpack_records(chunks, images, raw, K, A=4):
    """raw: the one downloaded int32 array - npig (K,A), then per chunk rec_rank (b,N) and rec_bits (b,N,A) - -> (ranks, bits
    per image without the padded rows, npig)"""
    npig = raw[:K * A].reshape(K, A).astype(np.int64)
    at, ranks, bits, i = K * A, [], [], 0
    for det, _ in chunks:
        b, N = det.shape[0], det.shape[1]
        rank = raw[at:at + b * N].reshape(b, N)
        bit = raw[at + b * N:at + b * N * (1 + A)].reshape(b, N, A)
        at += b * N * (1 + A)
        for j in range(b):
            n = len(images[i][0])
            ranks.append(rank[j, :n].astype(np.int64)), bits.append(bit[j, :n].astype(np.int64))
            i += 1
    return ranks, bits, npig


class DeviceCOCODetectionMetric(COCODetectionMetric):
    """COCODetectionMetric whose per-image matching runs in vd_coco_match.  update() is inherited (host rows); get() returns
    what the host class returns.  `timings` holds the seconds of the last get(): pack, upload, launch (device events),
    download, accumulate."""

    def __init__(self, dataset, save_prefix, use_time=True, cleanup=False, score_thresh=0.05, data_shape=None,
                 chunk_bytes=CHUNK_BYTES):
        super().__init__(dataset, save_prefix, use_time, cleanup, score_thresh, data_shape)
        self.chunk_bytes = int(chunk_bytes)
        self.chunks = 0

    def _evaluator(self, gt, results):
        return COCOEval(gt, results, match=self._match_device)

    def _match_device(self, img_ids, images, K):
        import torch
        from . import ops
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceCOCODetectionMetric needs the GPU: vd_coco_match has no host fallback "
                               "(COCODetectionMetric is the host metric)")
        A = len(AREA_RNG)
        t0 = time.perf_counter()
        chunks = pack_images(img_ids, images, self.chunk_bytes)
        head = np.concatenate([np.asarray(IOU_THRS, np.float64), np.asarray(AREA_RNG, np.float64).reshape(-1)])   # NumPy's values
        t1 = time.perf_counter()
        dev = torch.device("cuda", torch.cuda.current_device())
        counts = torch.zeros(K * A, dtype=torch.int32, device=dev)
        ev_ = [torch.cuda.Event(enable_timing=True) for _ in range(2 * len(chunks) + 1)]
        outs = []
        ev_[0].record()
        for k, (det, gt) in enumerate(chunks):
            b, N, M = det.shape[0], det.shape[1], gt.shape[1]
            host = torch.from_numpy(np.concatenate([head, det.reshape(-1), gt.reshape(-1)])).pin_memory()
            buf = host.to(dev, non_blocking=True)                               # ONE upload per chunk
            ev_[2 * k + 1].record()
            out = torch.empty(b * N * (1 + A), dtype=torch.int32, device=dev)
            nh, nd = len(head), b * N * DET_W
            ops.coco_match(buf[nh:nh + nd].view(b, N, DET_W), buf[nh + nd:].view(b, M, GT_W), buf[0:10], buf[10:nh].view(A, 2),
                           out[:b * N].view(b, N), out[b * N:].view(b, N, A), counts.view(K, A))
            ev_[2 * k + 2].record()
            outs.append(out)
        t2 = time.perf_counter()
        raw = torch.cat([counts] + outs).cpu().numpy()                          # ONE download
        t3 = time.perf_counter()
        up = sum(ev_[2 * k].elapsed_time(ev_[2 * k + 1]) for k in range(len(chunks))) * 1e-3
        launch = sum(ev_[2 * k + 1].elapsed_time(ev_[2 * k + 2]) for k in range(len(chunks))) * 1e-3
        self.timings = dict(pack=t1 - t0, upload=up, launch=launch, enqueue=t2 - t1, download=t3 - t2)
        self.chunks = len(chunks)
        return unpack_records(chunks, images, raw, K, A)
