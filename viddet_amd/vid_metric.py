"""The ImageNet VID motion metric: mAP split by object motion (slow / medium / fast) and by object area.

Restates /root/reference/metrics/imgnetvid.py in float64 NumPy, operation for operation:
  gt_thresholds    parse_set :28-31          the IoU a ground truth asks for (below 0.5 for small boxes)
  box_overlap      boxoverlap :288-309       = the `+1` IoU inside vid_eval_motion :170-179
  motion_ious      datasets/imgnetvid.py:758-783 (generate_motion_ious)
  vid_ap           vid_ap :40-65
  calculate_ap     calculate_ap :312-354
  vid_eval_motion  vid_eval_motion :68-285
  VIDDetectionMetric :357-472

Stated departures:
  * the reference's `np.argsort(-conf)` (:120, :334) is not stable; here both are stable (ties by row), so equal scores
    have a defined order.  The golden fixture's scores are pairwise distinct.
  * `class_map is not None` raises NotImplementedError: the reference filters the boxes by the map but not `thr` /
    `motion_iou` (:204-211 against :218-219), so its rows misalign.
  * `offset` other than None / 0 raises NotImplementedError (it selects a frame of a --mult_out window, which is not built).
  * an empty result list returns (['mAP'], ['0.0']): what the reference's `try` (:392-397) intends; as written it dies
    on the attribute `self._img_ids`, which nothing sets.

This module imports NumPy only.
"""
import warnings

import numpy as np

MOTION_RANGES = [[0.0, 1.0], [0.0, 0.7], [0.7, 0.9], [0.9, 1.0]]                                       # :382
AREA_RANGES = [[0, 1e5 * 1e5], [0, 50 * 50], [50 * 50, 150 * 150], [150 * 150, 1e5 * 1e5]]             # :383


def _rows(a, width):
    """an (n, >= width) float64 array of label rows (an empty one has no second axis to keep)"""
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(len(a), -1) if a.size else np.zeros((0, width))


def gt_thresholds(boxes, iou_thr=0.5, pixel_tolerance=10):
    """parse_set :28-31: (n,>=4) boxes -> (n,) the IoU each ground truth asks for"""
    boxes = _rows(boxes, 4)
    w = boxes[:, 2] - boxes[:, 0] + 1
    h = boxes[:, 3] - boxes[:, 1] + 1
    with np.errstate(invalid="ignore", divide="ignore"):
        thr = (w * h) / ((w + pixel_tolerance) * (h + pixel_tolerance))
        thr[thr > iou_thr] = iou_thr
    return thr


def box_overlap(bb, bbgt):
    """boxoverlap :288-309: the IoU of two boxes whose corners are pixel indices (width = x2 - x1 + 1)"""
    ov = 0
    iw = np.min((bb[2], bbgt[2])) - np.max((bb[0], bbgt[0])) + 1
    ih = np.min((bb[3], bbgt[3])) - np.max((bb[1], bbgt[1])) + 1
    if iw > 0 and ih > 0:
        intersect = iw * ih
        ua = (bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) + (bbgt[2] - bbgt[0] + 1.) * (bbgt[3] - bbgt[1] + 1.) - intersect
        ov = intersect / ua
    return ov


def overlaps(bboxes, gt_bboxes):
    """vid_eval_motion :165-180 for one image: (n,4) x (m,4) -> (n,m), the same float64 operations in the same order
    (`iw * ih` is formed once; max / min propagate NaN as np.max / np.min of a pair do)"""
    bb = np.asarray(bboxes, dtype=np.float64).reshape(-1, 4)[:, None, :]
    gt = np.asarray(gt_bboxes, dtype=np.float64).reshape(-1, 4)[None, :, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        iw = np.minimum(bb[..., 2], gt[..., 2]) - np.maximum(bb[..., 0], gt[..., 0]) + 1
        ih = np.minimum(bb[..., 3], gt[..., 3]) - np.maximum(bb[..., 1], gt[..., 1]) + 1
        ua = (bb[..., 2] - bb[..., 0] + 1.) * (bb[..., 3] - bb[..., 1] + 1.) + \
             (gt[..., 2] - gt[..., 0] + 1.) * (gt[..., 3] - gt[..., 1] + 1.) - iw * ih
        ov = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), ov, 0.0)


def motion_ious(clip_labels):
    """datasets/imgnetvid.py:758-783 for one clip.  clip_labels: per frame an (n,>=6) array x1,y1,x2,y2,cls,track.
    -> per frame a list: for every box with track id >= 0 the np.mean of its IoU with the same track's (first) box in the
    frames t-10 .. t+10 except t, inside the clip; NaN where the track has no neighbour (np.mean([]), warning suppressed);
    [0.0] for a frame without such boxes."""
    video = [_rows(f, 6) for f in clip_labels]
    out = []
    for frame in range(len(video)):
        frame_ious = []
        for box_idx in range(len(video[frame])):
            trk_id = video[frame][box_idx][5]
            if trk_id > -1:
                ious = []
                for i in range(-10, 11):
                    frame_c = frame + i
                    if 0 <= frame_c < len(video) and i != 0:
                        for c_box_idx in range(len(video[frame_c])):
                            if trk_id == video[frame_c][c_box_idx][5]:
                                ious.append(box_overlap(video[frame][box_idx], video[frame_c][c_box_idx]))
                                break
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)           # np.mean([]): nan, kept
                    frame_ious.append(float(np.mean(ious)))
        out.append(frame_ious if frame_ious else [0.0])
    return out


def vid_ap(rec, prec):
    """vid_ap :40-65: precision integrated over recall"""
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    # :57-58 `for i in range(mpre.size - 1, 0, -1): mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])` is the running maximum
    # from the right; a maximum rounds nothing, so the accumulate gives the loop's values bit for bit (NaN propagates alike)
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def class_groups(obj_labels, num_classes):
    """per class the positions of its rows, ascending: what `obj_labels == c` selects (:345-346), found for all classes by
    one stable sort"""
    by_class = np.argsort(obj_labels, kind="stable")
    cuts = np.searchsorted(obj_labels[by_class], np.arange(num_classes + 1))
    return [by_class[cuts[c]:cuts[c + 1]] for c in range(num_classes)]


def ap_sorted(tp_all, fp_all, obj_labels, num_classes, npos, groups=None):
    """calculate_ap :342-354 on rows that are already in the order of the set-wide sort by score (groups:
    class_groups(obj_labels, num_classes), where the caller has them already)"""
    cur_ap = np.zeros(num_classes)
    if groups is None:
        groups = class_groups(obj_labels, num_classes)
    for c in range(num_classes):
        fp = np.cumsum(fp_all[groups[c]])
        tp = np.cumsum(tp_all[groups[c]])
        if npos[c] <= 0:
            cur_ap[c] = -1
        else:
            rec = tp / npos[c]
            prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
            cur_ap[c] = vid_ap(rec, prec)
    return cur_ap


def _cat(cells, gt_img_ids, dtype):
    """the reference's np.array(list_of_ragged)[gt_img_ids] (:329-332, old-NumPy object arrays): concatenate in gt_img_ids
    order, skipping None"""
    parts = [cells[i] for i in gt_img_ids if cells[i] is not None]
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def calculate_ap(tp_cell, fp_cell, gt_img_ids, obj_labels_cell, obj_confs_cell, classname_map, npos):
    """calculate_ap :312-354.  The four `_cell` arguments are indexable by image id (None: no detections)."""
    tp_all = _cat(tp_cell, gt_img_ids, np.float64)
    fp_all = _cat(fp_cell, gt_img_ids, np.float64)
    obj_labels = _cat(obj_labels_cell, gt_img_ids, np.int64)
    confs = _cat(obj_confs_cell, gt_img_ids, np.float64)
    sorted_inds = np.argsort(-confs, kind="stable")                           # :334, stable here
    return ap_sorted(tp_all[sorted_inds], fp_all[sorted_inds], obj_labels[sorted_inds], len(classname_map), npos)


def check_ranges(motion_ranges, area_ranges):
    mr, ar = np.asarray(motion_ranges, np.float64), np.asarray(area_ranges, np.float64)
    if mr.shape != (4, 2) or ar.shape != (4, 2):
        raise ValueError("the VID metric is built for 4 motion and 4 area ranges (16 cells), got %r and %r" % (mr.shape, ar.shape))
    return mr, ar


def group_detections(dt, agnostic=False):
    """vid_eval_motion :93-130: result rows [img_id, label, score, x1, y1, x2, y2] -> {img_id: (labels, confs, bboxes)},
    every image's rows by score descending (stable: ties keep the order of `dt`)"""
    dt = np.array(dt, dtype=np.float64).reshape(-1, 7)
    img_ids, obj_labels = dt[:, 0].astype(int), dt[:, 1].astype(int)
    obj_confs, obj_bboxes = dt[:, 2].astype(float), dt[:, 3:].astype(float)
    out = {}
    if len(img_ids):
        by_img = np.argsort(img_ids, kind="stable")
        img_ids, obj_labels, obj_confs, obj_bboxes = img_ids[by_img], obj_labels[by_img], obj_confs[by_img], obj_bboxes[by_img]
        cuts = np.nonzero(np.diff(img_ids))[0] + 1
        for lo, hi in zip(np.concatenate(([0], cuts)), np.concatenate((cuts, [len(img_ids)]))):
            s = np.argsort(-obj_confs[lo:hi], kind="stable") + lo
            out[int(img_ids[lo])] = (obj_labels[s] * 0 if agnostic else obj_labels[s], obj_confs[s], obj_bboxes[s])
    return out


def match_image(labels, bboxes, gt_labels, gt_bboxes, gt_thr, gt_motion, motion_ranges, area_ranges):
    """vid_eval_motion :213-266 for one image, every cell at once.  labels (n,), bboxes (n,4): the detections by score
    descending; gt_labels (m,), gt_bboxes (m,4), gt_thr (m,), gt_motion (m,).  ->
      kmax (n,) the matched ground-truth row or -1;
      tp (16,n) 0/1; fp_code (16,n) 0 = 0, 1 = 1, 2 = empty_weight, 3 = the image's ignored fraction (cell = 4*motion + area);
      ig_motion (4,m), ig_area (4,m).
    Why once is enough: `kmax` depends on `ov`, `gt_thr`, the labels and `gt_detected`, and none of them on the cell - the
    reference rebuilds `gt_detected` from zeros in every cell and fills it by the same rule.  The cell enters afterwards
    only: which matched rows count as tp, and what an unmatched detection costs."""
    n, m = len(labels), len(gt_labels)
    ov = overlaps(bboxes, gt_bboxes)
    gt_motion = np.asarray(gt_motion, np.float64)[:m] if m else np.zeros(0)
    gt_area = (gt_bboxes[:, 3] - gt_bboxes[:, 1] + 1) * (gt_bboxes[:, 2] - gt_bboxes[:, 0] + 1) if m else np.zeros(0)        # :222
    with np.errstate(invalid="ignore"):
        ig_motion = np.stack([(gt_motion < r[0]) | (gt_motion > r[1]) for r in motion_ranges])                               # :219
        ig_area = np.stack([(gt_area < r[0]) | (gt_area > r[1]) for r in area_ranges])                                       # :223
    kmax = np.full(n, -1, np.int64)
    gt_detected = np.zeros(m, bool)
    with np.errstate(invalid="ignore"):
        ok = (ov >= gt_thr[None, :]) & (labels[:, None] == gt_labels[None, :])
        for j in range(n):                                                    # the greedy: score order, :232-249
            cand = np.where(ok[j] & ~gt_detected, ov[j], -np.inf)
            if m and cand.max() > -1:                                         # `ov > ovmax` from -1; argmax = the first maximum
                kmax[j] = int(cand.argmax())
                gt_detected[kmax[j]] = True
        # :243-246, over ALL ground truths whatever their class, from -1
        big = lambda mask: np.where(mask[:, None, :] & ~np.isnan(ov)[None], ov[None], -1.0).max(axis=2, initial=-1.0)
        ovmax_ig, ovmax_nig = big(ig_motion), big(~ig_motion)                 # (4,n)
        bb_area = (bboxes[:, 3] - bboxes[:, 1] + 1) * (bboxes[:, 2] - bboxes[:, 0] + 1)                                      # :253
        gate = np.stack([(bb_area < r[0]) | (bb_area > r[1]) for r in area_ranges])                                          # :254 (4,n)
    tp = np.zeros((16, n))
    fp_code = np.zeros((16, n), np.int64)
    hit = kmax >= 0
    for mi in range(4):
        rule = np.where(ovmax_nig[mi] > ovmax_ig[mi], 1, np.where(ovmax_ig[mi] > ovmax_nig[mi], 0, 2 if m == 0 else 3))      # :258-266
        for ai in range(4):
            c = 4 * mi + ai
            tp[c, hit] = (~ig_motion[mi, kmax[hit]] & ~ig_area[ai, kmax[hit]]).astype(np.float64)                            # :250
            fp_code[c] = np.where(hit | gate[ai], 0, rule)
    return kmax, tp, fp_code, ig_motion, ig_area


def empty_weights(all_motion_iou, motion_ranges):
    """:196-199: the share of ALL motion IoUs of the set inside the range (NaN is in none)"""
    a = np.asarray(all_motion_iou, np.float64)
    with np.errstate(invalid="ignore"):
        return [int(np.sum((a >= r[0]) & (a <= r[1]))) / float(len(a)) for r in motion_ranges]


def fp_values(fp_code, motion_index, empty_weight, ignored_fraction):
    """the float64 fp of :258-266 from its code"""
    return np.where(fp_code == 1, 1.0, np.where(fp_code == 2, empty_weight[motion_index],
                                                np.where(fp_code == 3, ignored_fraction[motion_index], 0.0)))


def check_dataset(dataset, class_map, offset):
    if class_map is not None:
        raise NotImplementedError("VIDDetectionMetric: class_map is not built (the reference filters the boxes by the map "
                                  "but not their thresholds and motion IoUs, metrics/imgnetvid.py:204-219)")
    if offset not in (None, 0):
        raise NotImplementedError("VIDDetectionMetric: offset=%r selects a frame of a --mult_out window, which is not built" % (offset,))
    ids = list(dataset.get_sample_ids())
    if ids and isinstance(ids[0], list):
        raise NotImplementedError("VIDDetectionMetric: window sample ids (--mult_out) are not built")
    return [int(i) for i in ids]


def vid_eval_motion(dataset, dt, motion_ranges, area_ranges, iou_threshold=0.5, class_map=None, agnostic=False, offset=None):
    """vid_eval_motion :68-285 -> ap (4, 4, C): average precision per motion range, area range and class (-1: the cell
    holds no ground truth of the class).

    The reference repeats the greedy matching loop for each of the 16 cells; here an image is matched ONCE (match_image)
    and the 16 cells are derived from that match.  That is equal because nothing the match reads depends on the cell:
    the overlaps, the thresholds, the labels and the `gt_detected` flags (reset in every cell, refilled by the same rule)
    are the same 16 times, so `kmax` is.  The cell decides only whether a matched row counts as a true positive, the area
    gate and the motion rule of an unmatched detection, and which ground truths leave `npos`."""
    gt_img_ids = check_dataset(dataset, class_map, offset)
    mr, ar = check_ranges(motion_ranges, area_ranges)
    C = 1 if agnostic else len(dataset.wn_classes)
    dets = group_detections(dt, agnostic)
    motion_iou = dataset.motion_ious
    ew = empty_weights(np.concatenate([np.asarray(motion_iou[str(k)], np.float64) for k in gt_img_ids]), mr)
    npos = np.zeros(C)
    nout = np.zeros((16, C))
    tp_all, fp_all, lab_all, conf_all = [], [], [], []
    for img_id in gt_img_ids:
        boxes = _rows(dataset.get_label(img_id), 6)
        gt_labels = boxes[:, 4].astype(int) * (0 if agnostic else 1)
        gt_thr = gt_thresholds(boxes, iou_threshold, 10)
        for x in gt_labels:
            npos[x] += 1                                                      # :157-158
        labels, confs, bboxes = dets.get(img_id, (np.zeros(0, int), np.zeros(0), np.zeros((0, 4))))
        _, tp, code, ig_m, ig_a = match_image(labels, bboxes, gt_labels, boxes[:, :4], gt_thr, motion_iou[str(img_id)], mr, ar)
        m = len(gt_labels)
        frac = [int(ig_m[i].sum()) / float(m) if m else 0.0 for i in range(4)]                                              # :265-266
        for mi in range(4):
            for ai in range(4):
                np.add.at(nout[4 * mi + ai], gt_labels[ig_m[mi] | ig_a[ai]], 1.0)                                        # :271-276
        if len(labels):
            tp_all.append(tp)
            fp_all.append(np.stack([fp_values(code[c], c // 4, ew, frac) for c in range(16)]))
            lab_all.append(labels)
            conf_all.append(confs)
    return ap_cells(tp_all, fp_all, lab_all, conf_all, npos, nout, C)


def ap_cells(tp_all, fp_all, lab_all, conf_all, npos, nout, C):
    """:278-283 for the 16 cells: per-image (16,n) tp / fp and (n,) labels / scores in gt_img_ids order -> ap (4,4,C).  The
    set-wide sort (:334) does not depend on the cell and is done once."""
    ap = np.zeros((4, 4, C))
    cat = lambda parts, axis, empty: np.concatenate(parts, axis=axis) if parts else empty
    tp, fp = cat(tp_all, 1, np.zeros((16, 0))), cat(fp_all, 1, np.zeros((16, 0)))
    labels, confs = cat(lab_all, 0, np.zeros(0, int)), cat(conf_all, 0, np.zeros(0))
    s = np.argsort(-confs, kind="stable")
    labels = labels[s]
    groups = class_groups(labels, C)
    for c in range(16):
        ap[c // 4, c % 4] = ap_sorted(tp[c][s], fp[c][s], labels, C, np.asarray(npos, np.float64) - nout[c], groups)
    return ap


class VIDDetectionMetric:
    """VIDDetectionMetric :357-472: collects [sid, label, score, x1, y1, x2, y2] rows in update(); get() evaluates them
    against the dataset's labels (`get_sample_ids`, `get_label`, `motion_ious`, `wn_classes`, `classes`)."""

    def __init__(self, dataset, conf_score_thresh=0.05, iou_thresh=0.5, class_map=None, agnostic=False, offset=None):
        check_dataset(dataset, class_map, offset)
        self.name = "ImgNetVIDMeanAP"
        self.dataset = dataset
        self._results = []
        self._conf_score_thresh = conf_score_thresh
        self._iou_thresh = iou_thresh
        self._class_map = class_map
        self._agnostic = agnostic
        self._offset = offset
        self._motion_ranges = [list(r) for r in MOTION_RANGES]
        self._area_ranges = [list(r) for r in AREA_RANGES]
        self.ap = None                                    # (4,4,C) of the last get()

    def reset(self):
        self._results = []

    def update(self, pred_bboxes, pred_labels, pred_scores, gt_bboxes=None, gt_ids=None, gt_difficults=None, sid=None,
               *args, **kwargs):
        """:429-472: pred_bboxes (B,N,4), pred_labels (B,N), pred_scores (B,N) (arrays or lists of per-image arrays) of the
        image(s) with sample id `sid`; rows with label < 0 and rows with score < conf_score_thresh are dropped.  The ground
        truth arguments are not read: get() takes it from the dataset."""
        as_numpy = lambda a: np.concatenate([np.asarray(x) for x in a], axis=0) if isinstance(a, (list, tuple)) else np.asarray(a)
        for pred_bbox, pred_label, pred_score in zip(*[as_numpy(x) for x in [pred_bboxes, pred_labels, pred_scores]]):
            valid_pred = np.where(pred_label.flat >= 0)[0]
            pred_bbox = pred_bbox[valid_pred, :].astype(np.float64)
            pred_label = pred_label.flat[valid_pred].astype(int)
            pred_score = pred_score.flat[valid_pred].astype(np.float64)
            for bbox, label, score in zip(pred_bbox, pred_label, pred_score):
                if score < self._conf_score_thresh:
                    continue
                self._results.append([sid, int(label), score] + bbox[:4].tolist())

    def _evaluate(self):
        return vid_eval_motion(self.dataset, self._results, self._motion_ranges, self._area_ranges,
                               iou_threshold=self._iou_thresh, class_map=self._class_map, agnostic=self._agnostic,
                               offset=self._offset)

    def get(self):
        """:388-426 -> names, values: the summary block (mean AP of the 16 cells), then one '{:.1f}' per class of cell
        (all motions, all areas) - or the single 'agnostic' entry"""
        if not self._results:
            return ['mAP', ], ['0.0', ]
        ap = self.ap = self._evaluate()
        names, values = [], []
        names.append('~~~~ Summary metrics ~~~~\n')
        info_str = ''
        for motion_index, motion_range in enumerate(self._motion_ranges):
            for area_index, area_range in enumerate(self._area_ranges):
                info_str += 'motion [{0:.1f} {1:.1f}], area [{2} {3} {4} {5}]\n'.format(
                    motion_range[0], motion_range[1], np.sqrt(area_range[0]), np.sqrt(area_range[0]),
                    np.sqrt(area_range[1]), np.sqrt(area_range[1]))
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)          # np.mean([]) of a cell without ground truth: nan
                    mean = np.mean([ap[motion_index][area_index][i] for i in range(len(ap[motion_index][area_index]))
                                    if ap[motion_index][area_index][i] >= 0])
                info_str += 'Mean AP@{:.1f} = {:.4f}\n\n'.format(self._iou_thresh, mean)
        values.append(info_str)
        if self._agnostic:
            names.append('agnostic')
            values.append('{:.1f}'.format(100 * ap[0, 0, 0]))
            return names, values
        for cls_ind, cls_name in enumerate(self.dataset.classes):
            names.append(cls_name)
            values.append('{:.1f}'.format(100 * ap[0, 0, cls_ind]))
        return names, values
