"""The COCO bbox evaluation written out with dicts and loops, one statement per statement of the algorithm DESIGN.md 26 fixes
(loadRes, computeIoU, evaluateImg, accumulate, summarize, and the wrapper's get()).  It shares no code with
viddet_amd/coco_metric.py and is slow on purpose; tests/test_coco_metric_cpu.py holds the vectorised metric against it, and
tests/test_coco_metric_gpu.py the device path against the metric."""
import copy
from collections import defaultdict

import numpy as np


def iou_one(d, g, crowd):
    dx, dy, dw, dh = [float(v) for v in d]
    gx, gy, gw, gh = [float(v) for v in g]
    w = min(dx + dw, gx + gw) - max(dx, gx)
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if w <= 0 or h <= 0:
        return 0.0
    i = w * h
    u = dw * dh if crowd else dw * dh + gw * gh - i
    return i / u


class Eval:
    def __init__(self, gt, results):
        self.iouThrs = np.linspace(.5, 0.95, 10)
        self.recThrs = np.linspace(0, 1, 101)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.imgIds = sorted(im['id'] for im in gt['images'])
        self.catIds = sorted(c['id'] for c in gt['categories'])
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for a in copy.deepcopy(gt['annotations']):
            if a['image_id'] in self.imgIds and a['category_id'] in self.catIds:
                a['ignore'] = 'iscrowd' in a and a['iscrowd']
                self._gts[a['image_id'], a['category_id']].append(a)
        for n, r in enumerate(copy.deepcopy(results)):                         # loadRes
            assert r['image_id'] in self.imgIds
            r['area'] = r['bbox'][2] * r['bbox'][3]
            r['id'] = n + 1
            r['iscrowd'] = 0
            if r['category_id'] in self.catIds:
                self._dts[r['image_id'], r['category_id']].append(r)
        self.evalImgs, self.ious, self.eval, self.stats = [], {}, {}, []

    def computeIoU(self, imgId, catId):
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in inds]
        if len(dt) > self.maxDets[-1]:
            dt = dt[0:self.maxDets[-1]]
        if len(dt) == 0 or len(gt) == 0:
            return []
        return np.array([[iou_one(d['bbox'], g['bbox'], int(g['iscrowd'])) for g in gt] for d in dt])

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            if g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1]):
                g['_ignore'] = 1
            else:
                g['_ignore'] = 0
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        ious = self.ious[imgId, catId][:, gtind] if len(self.ious[imgId, catId]) > 0 else self.ious[imgId, catId]
        T, G, D = len(self.iouThrs), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gtIg = np.array([g['_ignore'] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(self.iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {'dtMatches': dtm, 'dtScores': [d['score'] for d in dt], 'gtIgnore': gtIg, 'dtIgnore': dtIg,
                'dtRows': [d.get('row') for d in dt]}

    def evaluate(self):
        for imgId in self.imgIds:
            for catId in self.catIds:
                self.ious[imgId, catId] = self.computeIoU(imgId, catId)
        self.evalImgs = [self.evaluateImg(imgId, catId, areaRng, self.maxDets[-1])
                         for catId in self.catIds for areaRng in self.areaRng for imgId in self.imgIds]

    def accumulate(self):
        T, R, K, A, M = len(self.iouThrs), len(self.recThrs), len(self.catIds), len(self.areaRng), len(self.maxDets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        I0 = len(self.imgIds)
        for k in range(K):
            Nk = k * A * I0
            for a in range(A):
                Na = a * I0
                for m, maxDet in enumerate(self.maxDets):
                    E = [self.evalImgs[Nk + Na + i] for i in range(I0)]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                    inds = np.argsort(-dtScores, kind='mergesort')
                    dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    gtIg = np.concatenate([e['gtIgnore'] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp, fp = np.array(tp), np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,)).tolist()
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = pr.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, self.recThrs, side='left')
                        try:
                            for ri, pi in enumerate(inds):
                                q[ri] = pr[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
        self.eval = {'precision': precision, 'recall': recall}

    def summarize(self):
        def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
            iStr = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
            titleStr = 'Average Precision' if ap == 1 else 'Average Recall'
            typeStr = '(AP)' if ap == 1 else '(AR)'
            iouStr = '{:0.2f}:{:0.2f}'.format(self.iouThrs[0], self.iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
            aind = [i for i, aRng in enumerate(self.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(self.maxDets) if mDet == maxDets]
            if ap == 1:
                s = self.eval['precision']
                if iouThr is not None:
                    s = s[np.where(iouThr == self.iouThrs)[0]]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval['recall']
                if iouThr is not None:
                    s = s[np.where(iouThr == self.iouThrs)[0]]
                s = s[:, :, aind, mind]
            mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
            lines.append(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
            return mean_s

        lines = []
        stats = np.zeros((12,))
        stats[0] = _summarize(1)
        stats[1] = _summarize(1, iouThr=.5, maxDets=self.maxDets[2])
        stats[2] = _summarize(1, iouThr=.75, maxDets=self.maxDets[2])
        stats[3] = _summarize(1, areaRng='small', maxDets=self.maxDets[2])
        stats[4] = _summarize(1, areaRng='medium', maxDets=self.maxDets[2])
        stats[5] = _summarize(1, areaRng='large', maxDets=self.maxDets[2])
        stats[6] = _summarize(0, maxDets=self.maxDets[0])
        stats[7] = _summarize(0, maxDets=self.maxDets[1])
        stats[8] = _summarize(0, maxDets=self.maxDets[2])
        stats[9] = _summarize(0, areaRng='small', maxDets=self.maxDets[2])
        stats[10] = _summarize(0, areaRng='medium', maxDets=self.maxDets[2])
        stats[11] = _summarize(0, areaRng='large', maxDets=self.maxDets[2])
        self.stats = stats
        return '\n'.join(lines) + '\n'


def get_strings(ev, classes):
    """the wrapper's get() from an evaluated and accumulated Eval"""
    import warnings
    names, values = ['~~~~ Summary metrics ~~~~\n'], [ev.summarize().strip()]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for k, c in enumerate(classes):
            p = ev.eval['precision'][0:10, :, k, 0, 2]
            names.append(c)
            values.append('{:.1f}'.format(100 * np.mean(p[p > -1])))
        p = ev.eval['precision'][0:10, :, :, 0, 2]
        names.append('~~~~ MeanAP @ IoU=[0.50,0.95] ~~~~\n')
        values.append('{:.1f}'.format(100 * np.mean(p[p > -1])))
    return names, values


def run(gt, results):
    ev = Eval(gt, results)
    ev.evaluate()
    ev.accumulate()
    return ev


# ---- what both test files share -------------------------------------------------------------------------------------------
class ListDataset:
    """a dataset from plain lists, with what COCODetectionMetric and coco_ground_truth read"""

    def __init__(self, classes, labels, size=(640, 480), ids=None):
        self.classes = list(classes)
        self._labels = [np.asarray(l, dtype=np.float64).reshape(-1, 5) for l in labels]
        self.sample_ids = list(range(len(labels))) if ids is None else list(ids)
        self._size = size

    def __len__(self):
        return len(self._labels)

    def sample_path(self, idx):
        return "img%d.jpg" % idx

    def image_size(self, sid):
        return self._size

    def get_label(self, sid):
        return self._labels[self.sample_ids.index(sid)]


def seeded_predictions(ds, seed, per_image_extra=4, score_steps=12):
    """per sample of a SyntheticDetection-like set (xyxy boxes, labels, scores): its ground truths jittered, some with another
    class, plus random boxes; the scores come from a short ladder, so many are equal"""
    rng = np.random.default_rng(seed)
    out = []
    for idx, sid in enumerate(ds.sample_ids):
        w, h = ds.image_size(sid)
        lab = np.asarray(ds[idx][1], dtype=np.float64)
        boxes, labels = [], []
        for r in lab:
            for _ in range(int(rng.integers(0, 3))):
                s = np.array([r[2] - r[0], r[3] - r[1]] * 2)
                boxes.append(r[:4] + rng.normal(0, 0.06, 4) * s)
                labels.append(int(r[4]) if rng.random() < 0.8 else int(rng.integers(0, len(ds.classes))))
        for _ in range(per_image_extra):
            xy = rng.uniform(0, (0.7 * w, 0.7 * h))
            boxes.append(np.concatenate([xy, xy + rng.uniform(3, (0.3 * w, 0.3 * h))]))
            labels.append(int(rng.integers(0, len(ds.classes))))
        scores = 0.06 + 0.9 * rng.integers(0, score_steps, len(boxes)) / score_steps
        out.append((sid, np.array(boxes).reshape(-1, 4), np.array(labels, dtype=np.float64), scores))
    return out


# ---- per-image records (the format of coco_metric.match_image and vd_coco_match) from the loops above -----------------------
def records(det, gt, K):
    """det (n,6) x, y, w, h, score, category, gt (m,8) x, y, w, h, area, category, annotation id, iscrowd of ONE image ->
    rank (n,), bits (n,4), npig (K,4), read off evaluateImg's arrays"""
    gtd = {'images': [{'id': 0}], 'categories': [{'id': k} for k in range(K)],
           'annotations': [{'image_id': 0, 'id': int(g[6]), 'bbox': [float(v) for v in g[:4]], 'area': float(g[4]),
                            'category_id': int(g[5]), 'iscrowd': int(g[7])} for g in gt if 0 <= g[5] < K]}
    res = [{'image_id': 0, 'category_id': int(d[5]), 'bbox': [float(v) for v in d[:4]], 'score': float(d[4]), 'row': i}
           for i, d in enumerate(det) if 0 <= d[5] < K]
    ev = Eval(gtd, res)
    ev.evaluate()
    rank = np.full(len(det), -1, np.int64)
    bits = np.zeros((len(det), 4), np.int64)
    npig = np.zeros((K, 4), np.int64)
    for k in range(K):
        for a in range(4):
            e = ev.evalImgs[k * 4 + a]
            if e is None:
                continue
            npig[k, a] = np.count_nonzero(e['gtIgnore'] == 0)
            for j, row in enumerate(e['dtRows']):
                rank[row] = j
                for t in range(10):
                    if e['dtMatches'][t, j] != 0:
                        bits[row, a] |= 1 << t
                    if e['dtIgnore'][t, j]:
                        bits[row, a] |= 1 << (10 + t)
    return rank, bits, npig


def random_image(rng, n, m, K, first_id=1, pad=0.0, one_category=False):
    """an image on an integer grid: ground truths with duplicates (tied IoUs), crowds, areas exactly on the range boundaries;
    detections that copy ground truths exactly, shifted by a pixel or two, or as their upper half (IoU exactly 0.5), and
    clutter; scores from a ladder of 8 (ties); `pad`: the share of rows turned into padded ones (category -1), anywhere"""
    gt = np.zeros((m, 8))
    for i in range(m):
        if i and rng.random() < 0.2:
            gt[i] = gt[rng.integers(0, i)]                                      # the same box again
        else:
            w, h = [(32, 32), (96, 96), (int(rng.integers(2, 30)) * 2, int(rng.integers(2, 30)) * 2)][min(2, int(rng.integers(0, 8)))]
            gt[i, :4] = [int(rng.integers(0, 100)), int(rng.integers(0, 100)), w, h]
            gt[i, 4] = w * h
            gt[i, 5] = 0 if one_category else int(rng.integers(0, K))
            gt[i, 7] = float(rng.random() < 0.15)
        gt[i, 6] = first_id + i
    det = np.zeros((n, 6))
    for i in range(n):
        kind = int(rng.integers(0, 5)) if m else 4
        if kind < 4:
            g = gt[rng.integers(0, m)]
            det[i, :4] = g[:4]
            det[i, 5] = g[5] if rng.random() < 0.85 or one_category else int(rng.integers(0, K))
            if kind == 1:
                det[i, :2] += rng.integers(-2, 3, 2)
            elif kind == 2:
                det[i, 3] = g[3] / 2
            elif kind == 3:
                det[i, :4] += rng.integers(-3, 4, 4)
                det[i, 2:4] = np.maximum(det[i, 2:4], 1)
        else:
            det[i, :4] = [int(rng.integers(0, 100)), int(rng.integers(0, 100)), int(rng.integers(1, 60)), int(rng.integers(1, 60))]
            det[i, 5] = 0 if one_category else int(rng.integers(0, K))
        det[i, 4] = 0.1 + 0.1 * int(rng.integers(0, 8))
    if pad:
        det[rng.random(n) < pad, 5] = -1
        gt[rng.random(m) < pad, 5] = -1
    return det, gt


def edge_images():
    """[(name, det, gt, K)]: the small images at which the matching can go wrong"""
    rng = np.random.default_rng(11)
    out = []
    d, g = random_image(rng, 6, 4, 3)
    out += [("no detections", np.zeros((0, 6)), g, 3), ("no ground truth", d, np.zeros((0, 8)), 3),
            ("neither", np.zeros((0, 6)), np.zeros((0, 8)), 3)]
    out.append(("one detection", *random_image(rng, 1, 3, 1), 1))
    out.append(("padded rows", *random_image(rng, 40, 20, 5, pad=0.3), 5))
    out.append(("five categories: 0 and 4 share a wavefront", *random_image(rng, 70, 30, 5), 5))
    out.append(("three categories: one wavefront idle", *random_image(rng, 30, 12, 3), 3))
    out.append(("annotation id 0", *random_image(rng, 12, 5, 2, first_id=0), 2))
    out.append(("130 detections of one category", *random_image(rng, 130, 20, 5, one_category=True), 5))
    out.append(("a tile larger than the staging buffer", *random_image(rng, 120, 90, 2), 2))
    # by hand: two equal ground truths (ids 0, 1); an IoU of exactly 0.5; a crowd taken twice; areas 1024 and 9216
    g = np.array([[10, 10, 50, 50, 2500, 0, 0, 0], [10, 10, 50, 50, 2500, 0, 1, 0], [100, 0, 10, 20, 200, 1, 2, 0],
                  [0, 100, 100, 100, 10000, 1, 3, 1], [200, 200, 32, 32, 1024, 2, 4, 0], [300, 300, 96, 96, 9216, 2, 5, 0]], dtype=np.float64)
    d = np.array([[10, 10, 50, 50, .9, 0], [10, 10, 50, 50, .9, 0], [100, 0, 10, 10, .8, 1], [10, 110, 20, 20, .7, 1],
                  [50, 150, 30, 30, .7, 1], [200, 200, 32, 32, .6, 2], [300, 300, 96, 96, .6, 2], [300, 300, 96, 96, .6, 7]], dtype=np.float64)
    out.append(("by hand", d, g, 3))
    return out
