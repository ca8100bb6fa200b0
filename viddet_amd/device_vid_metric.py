"""The VID motion metric with the per-image matching on the device (detect_yolo3.py --metrics vid --device_metric).

`VIDDetectionMetric.get()` matches every image in NumPy.  `DeviceVIDDetectionMetric.get()` packs the collected detections
and the dataset's label rows per image into padded float64 arrays, uploads them chunk by chunk (pinned, one copy per
chunk), launches vd_vid_match (viddet_amd/csrc/vd_vid_eval.hip) once per chunk, downloads every chunk's integer records in
ONE copy and hands them to the same AP code as the host class (vid_metric.ap_cells): the set-wide sort, the cumulative
sums and AP stay on the host.

This module imports NumPy only; torch is imported where a device tensor is touched.
"""
import time

import numpy as np

from .lib import VID_MATCH_MAX_DET as MAX_DET, VID_MATCH_MAX_GT as MAX_GT
from .vid_metric import VIDDetectionMetric, _rows, ap_sorted, check_dataset, check_ranges, class_groups, empty_weights

CHUNK_BYTES = 32 << 20          # padded det + gt rows of one upload


def pack_images(dataset, results, agnostic=False, chunk_bytes=CHUNK_BYTES):
    """-> (chunks, all_motion_iou): chunks = [(det (b,N,6), gt (b,M,6))] over the dataset's images in get_sample_ids() order,
    each padded to its own widest image (padded rows: label -1) and at most chunk_bytes large; det rows are label, score,
    x1, y1, x2, y2 in the order update() collected them, gt rows x1, y1, x2, y2, label, motion_iou.  Detections of sample ids
    the dataset does not hold are dropped, as the reference never visits them."""
    ids = check_dataset(dataset, None, None)
    pos = {sid: i for i, sid in enumerate(ids)}
    dt = np.array(results, dtype=np.float64).reshape(-1, 7)
    img = np.array([pos.get(int(s), -1) for s in dt[:, 0]], dtype=np.int64)
    dt, img = dt[img >= 0], img[img >= 0]
    by_img = np.argsort(img, kind="stable")
    dt, img = dt[by_img], img[by_img]
    ndet = np.bincount(img, minlength=len(ids))
    first = np.concatenate(([0], np.cumsum(ndet)))
    slot = np.arange(len(img)) - first[img]                                   # the row inside its image
    if agnostic:
        dt[:, 1] = 0.0
    motion = dataset.motion_ious
    labels, all_motion = [], []
    for sid in ids:
        rows = _rows(dataset.get_label(sid), 6).copy()
        miou = np.asarray(motion[str(sid)], dtype=np.float64)
        all_motion.append(miou)
        rows[:, 5] = miou[:len(rows)]
        if agnostic:
            rows[:, 4] = 0.0
        labels.append(rows)
    ngt = np.array([len(r) for r in labels], dtype=np.int64)
    for i in np.nonzero(ndet > MAX_DET)[0]:
        raise ValueError("DeviceVIDDetectionMetric: sample id %d holds %d detections, vd_vid_match takes at most %d"
                         % (ids[i], ndet[i], MAX_DET))
    for i in np.nonzero(ngt > MAX_GT)[0]:
        raise ValueError("DeviceVIDDetectionMetric: sample id %d holds %d label rows, vd_vid_match takes at most %d"
                         % (ids[i], ngt[i], MAX_GT))
    chunks, lo = [], 0
    while lo < len(ids):
        hi, N, M = lo, 0, 0
        while hi < len(ids):
            n, m = max(N, int(ndet[hi])), max(M, int(ngt[hi]))
            if hi > lo and (hi + 1 - lo) * (n + m) * 48 > chunk_bytes:
                break
            hi, N, M = hi + 1, n, m
        det = np.full((hi - lo, N, 6), -1.0)
        gt = np.full((hi - lo, M, 6), -1.0)
        sel = slice(first[lo], first[hi])
        det[img[sel] - lo, slot[sel]] = dt[sel][:, [1, 2, 3, 4, 5, 6]]
        for i in range(lo, hi):
            gt[i - lo, :ngt[i]] = labels[i]
        chunks.append((det, gt))
        lo = hi
    return chunks, (np.concatenate(all_motion) if all_motion else np.zeros(0))


def ap_from_records(chunks, records, npos, nout, all_motion_iou, motion_ranges, C):
    """The host half: chunks as pack_images gives them, records = per chunk (rec_gt, rec_tp, rec_fp (b,N), img_nig (b,4),
    img_ngt (b,)) as vd_vid_match writes them, npos (C,), nout (16,C) -> ap (4,4,C).  The float64 fp values are formed as the
    reference writes them (img_nig / float(img_ngt), empty_weight from all motion IoUs), the rows ordered as the host metric
    orders them - by score descending, ties by image, then by row - and vid_metric.ap_sorted does the rest."""
    ew = np.array(empty_weights(all_motion_iou, motion_ranges))
    conf, lab, img, row, tpb, fpb, frac = [], [], [], [], [], [], []
    base = 0
    for (det, _), (rec_gt, rec_tp, rec_fp, img_nig, img_ngt) in zip(chunks, records):
        b, n = rec_gt.shape
        keep = rec_gt != -2
        bi, ri = np.nonzero(keep)
        conf.append(det[..., 1][keep]), lab.append(det[..., 0][keep].astype(int))
        img.append(bi + base), row.append(ri)
        tpb.append(rec_tp[keep].astype(np.int64)), fpb.append(rec_fp[keep].astype(np.int64) & 0xffffffff)
        with np.errstate(invalid="ignore", divide="ignore"):
            f = np.where(img_ngt[:, None] > 0, img_nig / img_ngt[:, None].astype(np.float64), 0.0)       # :265-266
        frac.append(f[bi])
        base += b
    cat = lambda parts, empty: np.concatenate(parts) if parts else empty
    conf, lab, img, row = cat(conf, np.zeros(0)), cat(lab, np.zeros(0, int)), cat(img, np.zeros(0, int)), cat(row, np.zeros(0, int))
    tpb, fpb, frac = cat(tpb, np.zeros(0, np.int64)), cat(fpb, np.zeros(0, np.int64)), cat(frac, np.zeros((0, 4)))
    s = np.lexsort((row, img, -conf))
    lab, tpb, fpb, frac = lab[s], tpb[s], fpb[s], frac[s]
    ap = np.zeros((4, 4, C))
    npos = np.asarray(npos, np.float64)
    groups = class_groups(lab, C)
    for c in range(16):
        mi = c // 4
        code = (fpb >> (2 * c)) & 3
        fp = np.where(code == 1, 1.0, np.where(code == 2, ew[mi], np.where(code == 3, frac[:, mi], 0.0)))
        tp = ((tpb >> c) & 1).astype(np.float64)
        ap[mi, c % 4] = ap_sorted(tp, fp, lab, C, npos - np.asarray(nout[c], np.float64), groups)
    return ap


class DeviceVIDDetectionMetric(VIDDetectionMetric):
    """VIDDetectionMetric whose per-image matching runs in vd_vid_match.  update() is inherited (host rows); get() returns
    what the host class returns.  `timings` holds the seconds of the last get(): pack, upload, launch, download, ap
    (upload and launch by device events)."""

    def __init__(self, dataset, conf_score_thresh=0.05, iou_thresh=0.5, class_map=None, agnostic=False, offset=None,
                 chunk_bytes=CHUNK_BYTES):
        super().__init__(dataset, conf_score_thresh, iou_thresh, class_map, agnostic, offset)
        self.chunk_bytes = int(chunk_bytes)
        self.timings = {}

    def _evaluate(self):
        import torch
        from . import ops
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceVIDDetectionMetric needs the GPU: vd_vid_match has no host fallback (VIDDetectionMetric is the host metric)")
        mr, ar = check_ranges(self._motion_ranges, self._area_ranges)
        C = 1 if self._agnostic else len(self.dataset.wn_classes)
        t0 = time.perf_counter()
        chunks, all_motion = pack_images(self.dataset, self._results, self._agnostic, self.chunk_bytes)
        t1 = time.perf_counter()
        dev = torch.device("cuda", torch.cuda.current_device())
        counts = torch.zeros(17 * C, dtype=torch.int32, device=dev)            # npos (C), nout (16,C)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * len(chunks) + 1)]
        outs = []
        ev[0].record()
        for k, (det, gt) in enumerate(chunks):
            b, N, M = det.shape[0], det.shape[1], gt.shape[1]
            host = torch.from_numpy(np.concatenate([mr.reshape(-1), ar.reshape(-1), det.reshape(-1), gt.reshape(-1)])).pin_memory()
            buf = host.to(dev, non_blocking=True)                               # ONE upload per chunk
            ev[2 * k + 1].record()
            out = torch.empty(b * (3 * N + 5), dtype=torch.int32, device=dev)
            at = [0]

            def take(*shape):
                n = int(np.prod(shape))
                t = out[at[0]:at[0] + n].view(*shape)
                at[0] += n
                return t

            d_det, d_gt = buf[16:16 + b * N * 6].view(b, N, 6), buf[16 + b * N * 6:].view(b, M, 6)
            ops.vid_match(d_det, d_gt, buf[0:8].view(4, 2), buf[8:16].view(4, 2), self._iou_thresh, 10.0, take(b, N), take(b, N),
                          take(b, N), take(b, 4), take(b), counts[:C], counts[C:].view(16, C))
            ev[2 * k + 2].record()
            outs.append(out)
        t2 = time.perf_counter()
        raw = torch.cat([counts] + outs).cpu().numpy()                          # ONE download
        t3 = time.perf_counter()
        up = sum(ev[2 * k].elapsed_time(ev[2 * k + 1]) for k in range(len(chunks))) * 1e-3
        launch = sum(ev[2 * k + 1].elapsed_time(ev[2 * k + 2]) for k in range(len(chunks))) * 1e-3
        npos, nout = raw[:C], raw[C:17 * C].reshape(16, C)
        at, records = 17 * C, []
        for det, _ in chunks:
            b, N = det.shape[0], det.shape[1]
            parts = []
            for shape in ((b, N), (b, N), (b, N), (b, 4), (b,)):
                n = int(np.prod(shape))
                parts.append(raw[at:at + n].reshape(shape))
                at += n
            records.append(tuple(parts))
        ap = ap_from_records(chunks, records, npos, nout, all_motion, mr, C)
        t4 = time.perf_counter()
        self.timings = dict(pack=t1 - t0, upload=up, launch=launch, enqueue=t2 - t1, download=t3 - t2, ap=t4 - t3)
        return ap
