"""VOC mAP with the per-image matching on the device (train_yolov3.py --device_metric).

`VOCMApMetric.update` walks every image and every class of it in NumPy.  `DeviceVOCMApMetric.update_device` hands the network's
output tensors and the batch's label rows to vd_voc_match (viddet_amd/csrc/vd_eval.hip): one workgroup per image writes, for
every detection row, its class, its score and the code 1 / 0 / -1 (true positive / false positive / ignored) the host loop
would have appended, and adds the class's ground-truth counts.  Nothing comes back to the host before `get()`: one download of
the compact records, which are then filed into the inherited `_npos` / `_scores` / `_hits` dictionaries in the order the host
metric would have produced - images by sample id, inside an image by class, score descending, row.  AP itself (a sort and two
cumulative sums per class, once per validation) is the inherited host code.

This module imports NumPy only; torch is imported where a device tensor is touched.
"""
import numpy as np

from .lib import VOC_MATCH_MAX_DET as MAX_DET, VOC_MATCH_MAX_GT as MAX_GT
from .metrics import VOCMApMetric, VOCMApMetricTemporal


def check_shapes(N, M, label_w):
    """ValueError, by argument, for what vd_voc_match does not take"""
    if label_w not in (5, 6):
        raise ValueError("update_device: labels must end in 5 [x1, y1, x2, y2, id] or 6 [+ difficult] columns, got %d" % label_w)
    if N > MAX_DET:
        raise ValueError("update_device: N=%d detections per image (ids / scores / bboxes), vd_voc_match takes at most %d"
                         % (N, MAX_DET))
    if M > MAX_GT:
        raise ValueError("update_device: M=%d label rows per image (labels), vd_voc_match takes at most %d" % (M, MAX_GT))


def file_records(metric, sample_ids, rec_cls, rec_score, rec_hit, npos, ndiff):
    """Compact records -> metric._npos / _scores / _hits, as VOCMApMetric.update would have filled them image by image.
    sample_ids: (I,) the images' order keys (a stable sort: equal ids keep their order here); rec_cls / rec_score / rec_hit:
    lists of (b,N) arrays whose images, concatenated, are the I images (N may differ between the arrays; rows with
    rec_cls < 0 are no detection); npos / ndiff (C,): non-difficult / difficult ground-truth rows per class."""
    sid = np.asarray(sample_ids).reshape(-1)
    pos = np.empty(len(sid), np.int64)
    pos[np.argsort(sid, kind="stable")] = np.arange(len(sid))
    img, row, first = [], [], 0
    for c in rec_cls:
        b, n = c.shape
        img.append(np.repeat(pos[first:first + b], n))
        row.append(np.tile(np.arange(n), b))
        first += b
    assert first == len(sid), "file_records: %d images in the records, %d sample ids" % (first, len(sid))
    cat = lambda parts, dt: np.concatenate([np.asarray(p).reshape(-1) for p in parts]) if parts else np.zeros(0, dt)
    img, row = cat(img, np.int64), cat(row, np.int64)
    cls, score, hit = cat(rec_cls, np.int32), cat(rec_score, np.float32), cat(rec_hit, np.int8)
    keep = cls >= 0
    img, row, cls, score, hit = img[keep], row[keep], cls[keep], score[keep], hit[keep]
    # the host's order: image, class (np.union1d is sorted), then the stable argsort of -score (NaN last, ties by row)
    order = np.lexsort((row, -score, cls, img))
    cls, score, hit = cls[order], score[order], hit[order]
    npos, ndiff = np.asarray(npos).reshape(-1), np.asarray(ndiff).reshape(-1)
    for c in np.nonzero((npos > 0) | (ndiff > 0))[0]:            # a class with ground truth: counted, and its score list exists
        metric._npos[int(c)] += int(npos[c])
        metric._scores[int(c)]
    for c in np.unique(cls):
        sel = cls == c
        metric._npos[int(c)] += 0
        metric._scores[int(c)].extend(score[sel].tolist())
        metric._hits[int(c)].extend(hit[sel].tolist())


class DeviceVOCMApMetric(VOCMApMetric):
    """VOCMApMetric whose per-image matching runs in vd_voc_match.  `update_device` per batch, then (under data parallelism)
    `gather()` once, then `get()`.  `update()` is the inherited host path.  num_labels: the number of label ids the model can
    emit, where a class_map makes it differ from len(class_names)."""

    def __init__(self, iou_thresh=0.5, class_names=None, class_map=None, num_labels=None):
        super().__init__(iou_thresh, class_names, class_map)
        self.num_labels = int(num_labels) if num_labels is not None else max(
            [self.num] + ([int(v) + 1 for v in class_map] if class_map is not None else []))

    def reset(self):
        super().reset()
        self._dev = []                 # per update_device call: (sample ids, rec_cls, rec_score, rec_hit) - the last three on the device
        self._counts = None            # (2, num_labels) int32 on the device: npos, ndiff
        self._host = []                # the same records once downloaded (or received from other ranks)
        self._host_counts = None
        self._next_id = 0

    # ---- the device side -------------------------------------------------------------------------------------------------
    def _labels_to_device(self, labels, device):
        """(.., M, 5|6) label rows -> a contiguous fp32 device tensor; the class_map is applied to the host ids first, by the
        host metric's expression (so class_map[-1] is what a padded row becomes, as there)"""
        import torch
        if hasattr(labels, "is_cuda"):
            if self.class_map is not None:
                raise TypeError("update_device: with a class_map the labels must be the loader's host array (the map is applied "
                                "before the upload)")
            if not labels.is_cuda or labels.dtype != torch.float32:
                raise TypeError("update_device: a labels tensor must be fp32 on the device, got %s on %s" % (labels.dtype, labels.device))
            return labels.contiguous()
        lab = np.ascontiguousarray(labels, dtype=np.float32)
        if self.class_map is not None:
            lab = lab.copy()
            ids = lab[..., 4].reshape(-1)
            lab[..., 4] = np.array([self.class_map[int(l)] for l in ids], np.float32).reshape(lab.shape[:-1])
        # pinned and asynchronous: a pageable upload would wait for the stream, i.e. for the forward pass in front of it
        return torch.from_numpy(lab).pin_memory().to(device, non_blocking=True)

    def update_device(self, ids, scores, bboxes, labels, clip=None, sample_ids=None):
        """ids (B,N,1), scores (B,N,1), bboxes (B,N,4): the device tensors net(...) returns; labels (B,M,5|6): the loader's fp32
        array or a device tensor; clip: the detections are clipped to [0, clip] first (None: not); sample_ids (B,): the images'
        positions in the evaluation set (None: call order).  One upload, one launch on the current stream; no download and no
        synchronisation.  The inputs are not kept."""
        if bboxes.dim() != 3 or bboxes.shape[-1] != 4:
            raise ValueError("update_device: bboxes must be (B,N,4), got %r" % (tuple(bboxes.shape),))
        B, N = int(bboxes.shape[0]), int(bboxes.shape[1])
        lshape = tuple(labels.shape)
        if len(lshape) != 3 or lshape[0] != B:
            raise ValueError("update_device: labels must be (B,M,5|6) with B=%d, got %r" % (B, lshape))
        check_shapes(N, lshape[1], lshape[2])
        if ids.numel() != B * N or scores.numel() != B * N:
            raise ValueError("update_device: ids %r and scores %r must hold one value per row of bboxes %r"
                             % (tuple(ids.shape), tuple(scores.shape), tuple(bboxes.shape)))
        self._match(ids, scores, bboxes, self._labels_to_device(labels, bboxes.device), clip, self._sample_ids(sample_ids, B))

    def _sample_ids(self, sample_ids, B):
        if sample_ids is None:
            sid = np.arange(self._next_id, self._next_id + B, dtype=np.int64)
        else:
            sid = np.array(sample_ids, dtype=np.int64).reshape(-1)
            if len(sid) != B:
                raise ValueError("update_device: %d sample_ids for %d images" % (len(sid), B))
        self._next_id += B
        return sid

    def _match(self, ids, scores, bboxes, gt, clip, sid):
        """the launch: gt (B,M,5|6) is on the device, its class_map applied"""
        import torch
        from . import ops
        B, N = int(bboxes.shape[0]), int(bboxes.shape[1])
        dev = bboxes.device
        f32 = lambda t, shape: t.detach().to(torch.float32).reshape(shape).contiguous()
        if self._counts is None:
            self._counts = torch.zeros((2, self.num_labels), dtype=torch.int32, device=dev)
        rec_cls = torch.empty((B, N), dtype=torch.int32, device=dev)
        rec_score = torch.empty((B, N), dtype=torch.float32, device=dev)
        rec_hit = torch.empty((B, N), dtype=torch.int8, device=dev)
        ops.voc_match(f32(ids, (B, N)), f32(scores, (B, N)), f32(bboxes, (B, N, 4)), gt.contiguous(),
                      -1.0 if clip is None else float(clip), self.iou_thresh, rec_cls, rec_score, rec_hit, self._counts[0],
                      self._counts[1])
        self._dev.append((sid, rec_cls, rec_score, rec_hit))

    def _download(self):
        """every pending device record -> self._host, in ONE device-to-host copy"""
        if not self._dev:
            return
        import torch
        raw = lambda t: t.reshape(-1).view(torch.uint8)
        parts = [raw(self._counts)]
        for _, c, s, h in self._dev:
            parts += [raw(c), raw(s), raw(h)]
        buf = torch.cat(parts).cpu().numpy()
        at = [0]

        def take(shape, dt):
            n = int(np.prod(shape)) * np.dtype(dt).itemsize
            a = buf[at[0]:at[0] + n].copy().view(dt).reshape(shape)
            at[0] += n
            return a

        self.add_records(None, [], [], [], *take((2, self.num_labels), np.int32).astype(np.int64))
        for sid, c, _, _ in self._dev:
            shp = tuple(c.shape)
            self._host.append((sid, take(shp, np.int32), take(shp, np.float32), take(shp, np.int8)))
        self._dev, self._counts = [], None

    # ---- the host side ---------------------------------------------------------------------------------------------------
    def add_records(self, sample_ids, rec_cls, rec_score, rec_hit, npos, ndiff):
        """Records that are on the host already (what vd_voc_match writes, from wherever): one (B,N) array each, or lists of
        them with sample_ids over all their images; npos / ndiff (num_labels,) are added to the counts."""
        if isinstance(rec_cls, np.ndarray):
            rec_cls, rec_score, rec_hit = [rec_cls], [rec_score], [rec_hit]
        first = 0
        sid = np.zeros(0, np.int64) if sample_ids is None else np.asarray(sample_ids, dtype=np.int64).reshape(-1)
        for c, s, h in zip(rec_cls, rec_score, rec_hit):
            self._host.append((sid[first:first + c.shape[0]], np.asarray(c), np.asarray(s), np.asarray(h)))
            first += c.shape[0]
        counts = np.stack([np.asarray(npos, np.int64).reshape(-1), np.asarray(ndiff, np.int64).reshape(-1)])
        self._host_counts = counts if self._host_counts is None else self._host_counts + counts

    def gather(self, group=None):
        """Under data parallelism: every rank's records (sample ids, rec_cls, rec_score, rec_hit, counts), exchanged once as
        host objects and merged - rank by rank, then (in get()) by sample id with a stable sort, as update_metric_sharded merges
        host records, duplicates included.  Every rank then holds the single-process metric, and no image was matched twice.
        Call it once, after the last update_device.  -> the number of images."""
        from . import dist as vdist
        return self._merge(vdist.all_gather_objects(self._export(), group))

    def _export(self):
        """this rank's records and counts as host objects (the pending device records come down first)"""
        self._download()
        return self._host, self._host_counts

    def _merge(self, parts):
        """parts: one _export() per rank, in rank order -> they replace this metric's records; the number of images"""
        self._host = [rec for recs, _ in parts for rec in recs]
        counts = [c for _, c in parts if c is not None]
        self._host_counts = sum(counts[1:], counts[0]) if counts else None
        return int(sum(len(r[0]) for r in self._host))

    def _file(self):
        self._download()
        if self._host_counts is None:
            return
        sid = np.concatenate([r[0] for r in self._host]) if self._host else np.zeros(0, np.int64)
        file_records(self, sid, [r[1] for r in self._host], [r[2] for r in self._host], [r[3] for r in self._host],
                     self._host_counts[0], self._host_counts[1])
        self._host, self._host_counts = [], None

    def get(self):
        """One download, the records filed in the host metric's order, then the inherited AP code"""
        self._file()
        return super().get()


class DeviceVOCMApMetricTemporal(VOCMApMetricTemporal):
    """VOCMApMetricTemporal over DeviceVOCMApMetric: update_device takes (B,t,N,.) outputs and (B,t,M,.) labels and files image
    (b, j) under frame offset j."""

    def __init__(self, t, iou_thresh=0.5, class_names=None, class_map=None, num_labels=None):
        self.t = int(t)
        self._per_t = [DeviceVOCMApMetric(iou_thresh, class_names, class_map, num_labels) for _ in range(self.t)]
        self.class_names = self._per_t[0].class_names

    def update_device(self, ids, scores, bboxes, labels, clip=None, sample_ids=None):
        if bboxes.dim() != 4 or bboxes.shape[1] != self.t or bboxes.shape[-1] != 4:
            raise ValueError("update_device: bboxes must be (B,%d,N,4), got %r" % (self.t, tuple(bboxes.shape)))
        lshape = tuple(labels.shape)
        if len(lshape) != 4 or lshape[:2] != tuple(bboxes.shape[:2]):
            raise ValueError("update_device: labels must be (B,%d,M,5|6) with B=%d, got %r" % (self.t, bboxes.shape[0], lshape))
        check_shapes(int(bboxes.shape[2]), lshape[2], lshape[3])
        B, N = int(bboxes.shape[0]), int(bboxes.shape[2])
        if ids.numel() != B * self.t * N or scores.numel() != B * self.t * N:
            raise ValueError("update_device: ids %r and scores %r must hold one value per row of bboxes %r"
                             % (tuple(ids.shape), tuple(scores.shape), tuple(bboxes.shape)))
        gt = self._per_t[0]._labels_to_device(labels, bboxes.device)        # one upload for the t offsets, class_map applied
        ids, scores = ids.reshape(B, self.t, N), scores.reshape(B, self.t, N)
        for j, m in enumerate(self._per_t):
            m._match(ids[:, j], scores[:, j], bboxes[:, j], gt[:, j], clip, m._sample_ids(sample_ids, B))

    def gather(self, group=None):
        """ONE exchange for the t frame offsets: every rank's t record sets travel together"""
        from . import dist as vdist
        parts = vdist.all_gather_objects([m._export() for m in self._per_t], group)
        return [m._merge([p[j] for p in parts]) for j, m in enumerate(self._per_t)][0]
