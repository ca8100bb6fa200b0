"""NumPy restatement of vd_vid_match's record format (include/viddet_hip.h), written out with loops over the
detections in score order - independent of viddet_amd.vid_metric.match_image - plus the cases and the array-backed dataset
the VID metric tests share."""
import os

import numpy as np

from viddet_amd.vid_metric import AREA_RANGES, MOTION_RANGES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vid_golden.npz")
MR = np.array(MOTION_RANGES, np.float64)
AR = np.array(AREA_RANGES, np.float64)


def _overlap(bb, g):
    """(4,) x (m,4) -> (m,): vid_eval_motion :170-179"""
    with np.errstate(invalid="ignore", divide="ignore"):
        iw = np.minimum(bb[2], g[:, 2]) - np.maximum(bb[0], g[:, 0]) + 1
        ih = np.minimum(bb[3], g[:, 3]) - np.maximum(bb[1], g[:, 1]) + 1
        ua = (bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) + (g[:, 2] - g[:, 0] + 1.) * (g[:, 3] - g[:, 1] + 1.) - iw * ih
        return np.where((iw > 0) & (ih > 0), iw * ih / ua, 0.0)


def match_records(det, gt, motion_ranges=MR, area_ranges=AR, iou_thresh=0.5, pixel_tolerance=10.0, C=1):
    """det (B,N,6) label, score, x1, y1, x2, y2; gt (B,M,6) x1, y1, x2, y2, label, motion_iou (label < 0: padded)
    -> rec_gt, rec_tp, rec_fp (B,N), img_nig (B,4), img_ngt (B,), npos (C,), nout (16,C), all int32"""
    det, gt = np.asarray(det, np.float64), np.asarray(gt, np.float64)
    B, N, M = det.shape[0], det.shape[1], gt.shape[1]
    rec_gt = np.full((B, N), -2, np.int32)
    rec_tp = np.zeros((B, N), np.uint32)
    rec_fp = np.zeros((B, N), np.uint32)
    img_nig, img_ngt = np.zeros((B, 4), np.int32), np.zeros(B, np.int32)
    npos, nout = np.zeros(C, np.int32), np.zeros((16, C), np.int32)
    err = lambda: np.errstate(invalid="ignore", divide="ignore")
    for b in range(B):
        g = gt[b]
        gvalid = g[:, 4] >= 0
        gcls = np.where(gvalid, np.where(gvalid, g[:, 4], 0).astype(np.int64), -1)
        with err():
            w, h = g[:, 2] - g[:, 0] + 1, g[:, 3] - g[:, 1] + 1
            thr = (w * h) / ((w + pixel_tolerance) * (h + pixel_tolerance))
            thr[thr > iou_thresh] = iou_thresh
            area = (g[:, 3] - g[:, 1] + 1) * (g[:, 2] - g[:, 0] + 1)
            ig_m = np.stack([(g[:, 5] < r[0]) | (g[:, 5] > r[1]) for r in motion_ranges])
            ig_a = np.stack([(area < r[0]) | (area > r[1]) for r in area_ranges])
        img_ngt[b] = gvalid.sum()
        img_nig[b] = (ig_m & gvalid).sum(axis=1)
        for k in np.nonzero(gvalid & (gcls < C))[0]:
            npos[gcls[k]] += 1
            for c in range(16):
                nout[c, gcls[k]] += int(ig_m[c // 4, k] | ig_a[c % 4, k])
        d = det[b]
        dvalid = d[:, 0] >= 0
        rows = np.nonzero(dvalid)[0]
        order = rows[np.argsort(-d[rows, 1], kind="stable")]
        detected = np.zeros(M, bool)
        for j in order:
            cls, bb = int(d[j, 0]), d[j, 2:6]
            ov = _overlap(bb, g)
            with err():
                cand = gvalid & ~detected & (gcls == cls) & (ov >= thr)       # ov >= thr >= ... > -1: any candidate beats ovmax = -1
                kmax = int(np.argmax(np.where(cand, ov, -np.inf))) if cand.any() else -1      # strict >: the first maximum
                seen = gvalid & ~np.isnan(ov)                                 # `ov > x` is false for a NaN
                ig = [np.max(ov[seen & ig_m[r]], initial=-1.0) for r in range(4)]
                nig = [np.max(ov[seen & ~ig_m[r]], initial=-1.0) for r in range(4)]
            rec_gt[b, j] = kmax
            if kmax >= 0:
                detected[kmax] = True
                for c in range(16):
                    if not ig_m[c // 4, kmax] and not ig_a[c % 4, kmax]:
                        rec_tp[b, j] |= np.uint32(1 << c)
                continue
            with err():
                bb_area = (bb[3] - bb[1] + 1) * (bb[2] - bb[0] + 1)
            for c in range(16):
                mi, ai = c // 4, c % 4
                if bb_area < area_ranges[ai][0] or bb_area > area_ranges[ai][1]:
                    code = 0
                elif nig[mi] > ig[mi]:
                    code = 1
                elif ig[mi] > nig[mi]:
                    code = 0
                else:
                    code = 2 if img_ngt[b] == 0 else 3
                rec_fp[b, j] |= np.uint32(code << (2 * c))
    return rec_gt, rec_tp.view(np.int32), rec_fp.view(np.int32), img_nig, img_ngt, npos, nout


def random_case(B, N, M, C, seed, one_class=False, size=400.0):
    """(det (B,N,6), gt (B,M,6)) that exercise every branch: labels in [0, C), ground truths of every size class (a few of
    zero area: thr = 0) and motion IoU (a few NaN), detections near ground truths of their own and of other classes (so that
    several compete for one row) and far from all, distinct scores, padded rows in the middle of both lists."""
    rng = np.random.default_rng([seed, B, N, M, C])
    gt = np.full((B, M, 6), -1.0)
    det = np.full((B, N, 6), -1.0)
    scores = rng.permutation(B * max(N, 1)).reshape(B, max(N, 1))[:, :N] / float(B * max(N, 1)) * 0.9 + 0.05
    for b in range(B):
        side = np.exp(rng.uniform(np.log(4.0), np.log(250.0), (M, 2)))
        xy = rng.uniform(0, size - 1, (M, 2))
        g = np.concatenate([xy, np.minimum(xy + side, size - 1)], axis=1)
        zero = rng.random(M) < 0.04
        g[zero, 2:4] = g[zero, 0:2] - 1                                       # w = h = 0: thr = 0
        gt[b, :, :4] = g
        gt[b, :, 4] = 0 if one_class else rng.integers(0, C, M)
        gt[b, :, 5] = rng.choice([0.3, 0.65, 0.7, 0.8, 0.9, 0.95, 1.0, np.nan], M)
        gt[b, rng.random(M) < 0.15, 4] = -1.0                                 # padded rows anywhere
        if b == B - 1 and B > 1:
            gt[b, :, 4] = -1.0                                                # an image without ground truth
        for j in range(N):
            if M and rng.random() < 0.75:
                k = int(rng.integers(0, M))
                s = g[k, 2:4] - g[k, 0:2] + 1
                box = g[k] + rng.normal(0, 1, 4) * np.concatenate([s, s]) * rng.choice([0.0, 0.03, 0.1, 0.3])
                cls = gt[b, k, 4] if rng.random() < 0.8 and gt[b, k, 4] >= 0 else (0 if one_class else rng.integers(0, C))
            else:
                xy1 = rng.uniform(0, size - 1, 2)
                box = np.concatenate([xy1, xy1 + np.exp(rng.uniform(np.log(4.0), np.log(250.0), 2))])
                cls = 0 if one_class else rng.integers(0, C)
            det[b, j, 0], det[b, j, 1], det[b, j, 2:6] = cls, scores[b, j], box
        det[b, rng.random(N) < 0.1, 0] = -1.0
    return det, gt


class ArrayDataset:
    """What VIDDetectionMetric reads of a dataset, from arrays: sample ids (I,), label rows (R,7) sid, x1, y1, x2, y2, cls,
    track, and per sample id the motion IoU list"""

    def __init__(self, sample_ids, labels, motion, num_class):
        self._ids = [int(s) for s in sample_ids]
        self._labels = {s: np.zeros((0, 6)) for s in self._ids}
        labels = np.asarray(labels, np.float64).reshape(-1, 7)
        for s in self._ids:
            self._labels[s] = labels[labels[:, 0] == s][:, 1:7]
        self.motion_ious = motion
        self.classes = ["class%d" % i for i in range(num_class)]
        self.wn_classes = list(self.classes)

    def get_sample_ids(self):
        return list(self._ids)

    def get_label(self, sid):
        return self._labels[int(sid)].copy()


def dataset_from_case(det, gt, C):
    """a packed case as a dataset + result rows: what DeviceVIDDetectionMetric would pack back into (det, gt) up to the
    position of the padded rows"""
    B = det.shape[0]
    labels, motion, results = [], {}, []
    for b in range(B):
        rows = gt[b][gt[b, :, 4] >= 0]
        labels += [[b + 1] + r[:5].tolist() + [float(i)] for i, r in enumerate(rows)]
        motion[str(b + 1)] = rows[:, 5].tolist() if len(rows) else [0.0]
        results += [[b + 1, int(r[0]), r[1]] + r[2:6].tolist() for r in det[b][det[b, :, 0] >= 0]]
    return ArrayDataset(range(1, B + 1), labels, motion, C), results


def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return load_golden_arrays({k: z[k] for k in z.files})


def load_golden_arrays(g):
    counts = g["motion_counts"]
    cuts = np.concatenate(([0], np.cumsum(counts)))
    motion = {str(int(s)): g["motion_values"][cuts[i]:cuts[i + 1]].tolist() for i, s in enumerate(g["sample_ids"])}
    ds = ArrayDataset(g["sample_ids"], g["labels"], motion, int(g["num_class"]))
    return g, ds


def golden_results(g):
    return [[int(r[0]), int(r[1]), float(r[2])] + r[3:7].tolist() for r in g["dets"]]
