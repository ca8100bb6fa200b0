"""The IOU tracker (Bochinski, Eiselein, Sikora, AVSS 2017, Algorithm 1) with the max_age extension, as plain loops over
tracks and rows written from the paper and the issue's rule - nothing vectorised over rows, no code shared with
viddet_amd/track.py.  tests/test_track_cpu.py holds track_host equal to it; the GPU tests hold vd_track equal to track_host."""
import math

import numpy as np

f32 = np.float32


def _mn(x, y):
    return f32(np.nan) if (math.isnan(x) or math.isnan(y)) else (x if x <= y else y)


def _mx(x, y):
    return f32(np.nan) if (math.isnan(x) or math.isnan(y)) else (x if x >= y else y)


def iou(a, b):
    """float32, no +1; 0 unless both extents of the intersection are > 0"""
    with np.errstate(all="ignore"):
        iw = f32(_mn(a[2], b[2]) - _mx(a[0], b[0]))
        ih = f32(_mn(a[3], b[3]) - _mx(a[1], b[1]))
        if not (iw > 0 and ih > 0):
            return f32(0)
        inter = f32(iw * ih)
        aa = f32(f32(a[2] - a[0]) * f32(a[3] - a[1]))
        ab = f32(f32(b[2] - b[0]) * f32(b[3] - b[1]))
        return f32(inter / f32(f32(aa + ab) - inter))


def candidate_class(id_, score, num_class):
    """the row's class, or -1: id >= 0, a finite score, the class (the id truncated) below num_class where given"""
    id_, score = float(id_), float(score)
    if math.isnan(id_) or id_ < 0 or math.isnan(score) or math.isinf(score):
        return -1
    c = 0x7fffffff if id_ >= 2147483648.0 else int(id_)
    if num_class is not None and c >= int(num_class):
        return -1
    return c


def track_loops(ids, scores, bboxes, clip_start=None, num_class=None, sigma_l=0.0, sigma_h=0.5, sigma_iou=0.5, t_min=2, max_age=0):
    ids = np.asarray(ids, dtype=f32)
    bboxes = np.asarray(bboxes, dtype=f32)
    F, N = bboxes.shape[0], bboxes.shape[1]
    ids = ids.reshape(F, N)
    scores = np.asarray(scores, dtype=f32).reshape(F, N)
    sigma_l, sigma_h, sigma_iou = f32(sigma_l), f32(sigma_h), f32(sigma_iou)
    track = np.full((F, N), -1, dtype=np.int32)
    tlen = np.zeros((F, N), dtype=np.int32)
    tscore = np.full((F, N), -1, dtype=f32)
    bounds = [0, F] if clip_start is None else [int(v) for v in clip_start]
    for v in range(len(bounds) - 1):
        tracks = []                                    # every track of the clip, by id: dict(cls, rows [(t, i)], best, box, miss, open)
        for t in range(bounds[v], bounds[v + 1]):
            cand = []
            for i in range(N):
                c = candidate_class(ids[t, i], scores[t, i], num_class)
                if c >= 0 and scores[t, i] >= sigma_l:
                    cand.append([i, c, False])         # row, class, taken
            for tr in tracks:                          # by id = in order of creation
                if not tr["open"]:
                    continue
                best, best_iou = None, None
                for cd in cand:                        # in row order: only a strictly larger IoU replaces the choice
                    if cd[2] or cd[1] != tr["cls"]:
                        continue
                    v_ = iou(tr["box"], bboxes[t, cd[0]])
                    if best is None or (v_ > best_iou) or (math.isnan(v_) and not math.isnan(best_iou)):
                        best, best_iou = cd, v_
                if best is not None and best_iou >= sigma_iou:
                    best[2] = True
                    tr["rows"].append((t, best[0]))
                    tr["box"] = bboxes[t, best[0]]
                    tr["miss"] = 0
                    if scores[t, best[0]] > tr["best"]:
                        tr["best"] = scores[t, best[0]]
                else:
                    tr["miss"] += 1
                    if tr["miss"] > max_age:
                        tr["open"] = False
            for cd in cand:
                if not cd[2]:
                    tracks.append(dict(cls=cd[1], rows=[(t, cd[0])], best=scores[t, cd[0]], box=bboxes[t, cd[0]], miss=0, open=True))
        for n, tr in enumerate(tracks):
            if tr["best"] >= sigma_h and len(tr["rows"]) >= t_min:
                for t, i in tr["rows"]:
                    track[t, i], tlen[t, i], tscore[t, i] = n, len(tr["rows"]), tr["best"]
    return track, tlen, tscore
