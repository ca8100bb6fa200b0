"""SORT as the paper writes it (Bewley et al., ICIP 2016), in loops and float64: the oracle that tests/test_sort_cpu.py holds
viddet_amd.sort.sort_host against.  A track is the full 7-state filter - x = (u, v, s, r, du, dv, ds) with the 7 x 7 matrices F,
H, Q, R, P of the paper's reference implementation - and the association is a brute-force enumeration of every matching of
admissible pairs, scored by (pairs, sum of the quantised IoUs).  Nothing here is shared with the definition but the class rule
of the rows (seq_nms.row_classes); the stated departures (only admissible pairs enter, tracks per class, t_min / sigma_h decide
at the clip's end) are the definition's."""
import numpy as np

from viddet_amd.seq_nms import _clips, row_classes

Q_ONE = 1 << 20

F_MAT = np.eye(7)
F_MAT[0, 4] = F_MAT[1, 5] = F_MAT[2, 6] = 1.0
H_MAT = np.eye(4, 7)
R_MAT = np.diag([1.0, 1.0, 10.0, 10.0])
P0_MAT = np.diag([10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4])
Q_MAT = np.diag([1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 1e-4])


def box_to_z(b):
    w, h = b[2] - b[0], b[3] - b[1]
    return np.array([b[0] + w / 2.0, b[1] + h / 2.0, w * h, w / h])


def x_to_box(x):
    w = np.sqrt(x[2] * x[3])
    h = x[2] / w
    return np.array([x[0] - w / 2.0, x[1] - h / 2.0, x[0] + w / 2.0, x[1] + h / 2.0])


class KalmanBox:
    """the paper's KalmanBoxTracker: a constant-velocity model on (u, v, s), r constant"""

    def __init__(self, box):
        self.x = np.zeros(7)
        self.x[:4] = box_to_z(np.asarray(box, dtype=np.float64))
        self.P = P0_MAT.copy()

    def predict(self):
        if self.x[6] + self.x[2] <= 0:
            self.x[6] = 0.0
        self.x = F_MAT @ self.x
        self.P = F_MAT @ self.P @ F_MAT.T + Q_MAT
        return x_to_box(self.x)

    def update(self, box):
        y = box_to_z(np.asarray(box, dtype=np.float64)) - H_MAT @ self.x
        S = H_MAT @ self.P @ H_MAT.T + R_MAT
        K = self.P @ H_MAT.T @ np.linalg.inv(S)
        self.x = self.x + K @ y
        self.P = (np.eye(7) - K @ H_MAT) @ self.P
        return x_to_box(self.x)


def iou64(a, b):
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if not (iw > 0 and ih > 0):
        return 0.0
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def best_matching(q, adm):
    """q (R,K) quantised IoUs, adm (R,K) bool -> (the track of every row or -1, the margin of the best matching over the
    runner-up).  Every matching of admissible pairs is enumerated; its value is the sum of 2**27 - (2**20 - q) over its pairs,
    so one more pair outweighs any sum of IoUs: (pairs, quantised sum) in one number."""
    R, K = q.shape
    found = []                                                             # (value, the rows' tracks)

    def walk(i, taken, value, cols):
        if i == R:
            found.append((value, tuple(cols)))
            return
        walk(i + 1, taken, value, cols + [-1])
        for k in range(K):
            if adm[i, k] and k not in taken:
                walk(i + 1, taken | {k}, value + (1 << 27) - (Q_ONE - int(q[i, k])), cols + [k])

    walk(0, frozenset(), 0, [])
    found.sort(key=lambda f: -f[0])
    margin = found[0][0] - found[1][0] if len(found) > 1 else 1 << 27
    return list(found[0][1]), margin


def sort_oracle(ids, scores, bboxes, clip_start=None, num_class=None, sigma_l=0.0, sigma_h=0.5, sigma_iou=0.3, t_min=2, max_age=1,
                margins=None):
    """-> (track (F,N), tlen (F,N), the predicted boxes [(frame, track id, box)]).  margins, a dict, receives 'iou': the least
    |iou - sigma_iou| over every (row, track) of equal classes, and 'assign': the least margin of a frame's best matching."""
    ids, scores, bboxes = np.asarray(ids, np.float32), np.asarray(scores, np.float32), np.asarray(bboxes, np.float32)
    F, N = bboxes.shape[0], bboxes.shape[1]
    sc = scores.reshape(F, N)
    cls = row_classes(ids.reshape(F, N), sc, num_class)
    cls = np.where(sc >= np.float32(sigma_l), cls, -1)
    track = np.full((F, N), -1, dtype=np.int64)
    tlen = np.zeros((F, N), dtype=np.int64)
    predicted = []
    least_iou, least_assign = np.inf, np.inf
    for t0, t1 in _clips(clip_start, F):
        active, made = [], []                                              # a track: dict(id, cls, kf, miss, len, max)
        local = np.full((t1 - t0, N), -1, dtype=np.int64)
        for t in range(t0, t1):
            boxes = [tr["kf"].predict() for tr in active]
            predicted += [(t, tr["id"], b) for tr, b in zip(active, boxes)]
            rows = [j for j in range(N) if cls[t, j] >= 0]
            cols = [-1] * len(rows)
            if rows and active:
                q = np.zeros((len(rows), len(active)), dtype=np.int64)
                adm = np.zeros(q.shape, dtype=bool)
                for i, j in enumerate(rows):
                    for k, tr in enumerate(active):
                        if tr["cls"] == cls[t, j]:
                            o = iou64(boxes[k], bboxes[t, j].astype(np.float64))
                            least_iou = min(least_iou, abs(o - sigma_iou))
                            adm[i, k] = o >= sigma_iou
                            q[i, k] = int(o * Q_ONE)
                cols, margin = best_matching(q, adm)
                least_assign = min(least_assign, margin)
            hit = set()
            for j, k in zip(rows, cols):
                if k >= 0:
                    tr = active[k]
                    tr["kf"].update(bboxes[t, j])
                    tr["miss"], tr["len"], tr["max"] = 0, tr["len"] + 1, max(tr["max"], sc[t, j])
                    local[t - t0, j] = tr["id"]
                    hit.add(k)
            for k, tr in enumerate(active):
                if k not in hit:
                    tr["miss"] += 1
            active = [tr for tr in active if tr["miss"] <= max_age]
            for j, k in zip(rows, cols):
                if k < 0:
                    tr = dict(id=len(made), cls=int(cls[t, j]), kf=KalmanBox(bboxes[t, j]), miss=0, len=1, max=sc[t, j])
                    local[t - t0, j] = tr["id"]
                    active.append(tr)
                    made.append(tr)
        for tr in made:
            if tr["max"] >= np.float32(sigma_h) and tr["len"] >= t_min:
                on = local == tr["id"]
                track[t0:t1][on] = tr["id"]
                tlen[t0:t1][on] = tr["len"]
    if margins is not None:
        margins["iou"], margins["assign"] = least_iou, least_assign
    return track, tlen, predicted
