"""The stitching pass of DESIGN.md 38 in loops and float64: the oracle that tests/test_stitch_cpu.py holds
viddet_amd.stitch.stitch_host against.  A track's filter is tests/sort_oracle.py's KalmanBox, the full 7-state filter with its
7 x 7 matrices, run over the track's members and extrapolated over the gap with the matrices too; the links are a brute-force
enumeration of every matching of admissible (tail, head) pairs, scored by (pairs, sum of the quantised IoUs).  Nothing here is
shared with the definition but the class rule of the rows (seq_nms.row_classes)."""
import copy

import numpy as np

from tests.sort_oracle import Q_ONE, KalmanBox, best_matching, iou64
from viddet_amd.seq_nms import _clips, row_classes


def stitch_oracle(ids, scores, bboxes, track, clip_start=None, num_class=None, max_gap=30, sigma_iou=0.3, max_tracks=512,
                  margins=None):
    """-> (strack (F,N), tlen (F,N), the links [(clip, tail id, head id, iou)]).  margins, a dict, receives 'iou': the least
    |iou - sigma_iou| over every (tail, head) of equal classes within max_gap frames, and 'assign': the least margin of a clip's
    best matching over the runner-up."""
    ids, scores, bboxes = np.asarray(ids, np.float32), np.asarray(scores, np.float32), np.asarray(bboxes, np.float32)
    F, N = bboxes.shape[0], bboxes.shape[1]
    cls = row_classes(ids.reshape(F, N), scores.reshape(F, N), num_class)
    strack = np.full((F, N), -1, dtype=np.int64)
    tlen = np.zeros((F, N), dtype=np.int64)
    least_iou, least_assign = np.inf, np.inf
    links = []
    for v, (t0, t1) in enumerate(_clips(clip_start, F)):
        members = {}                                                       # id -> [(frame, row)] in frame order
        for t in range(t0, t1):
            seen = set()
            for i in range(N):
                u = int(track[t, i])
                if cls[t, i] >= 0 and 0 <= u < (t1 - t0) * N and u not in seen:
                    seen.add(u)
                    members.setdefault(u, []).append((t, i))
        part = sorted(members)[:max_tracks]
        tails = []
        for u in part:
            (t, i), rest = members[u][0], members[u][1:]
            kf, last = KalmanBox(bboxes[t, i]), t
            for t, i in rest:
                for _ in range(t - last):
                    kf.predict()
                kf.update(bboxes[t, i])
                last = t
            tails.append(kf)
        P = len(part)
        succ = {}
        if P >= 2:
            q = np.zeros((P, P), dtype=np.int64)
            adm = np.zeros((P, P), dtype=bool)
            for a, ua in enumerate(part):
                ta, ia = members[ua][-1]
                for b, ub in enumerate(part):
                    tb, ib = members[ub][0]
                    if a != b and 1 <= tb - ta <= max_gap and cls[ta, ia] == cls[tb, ib]:
                        kf = copy.deepcopy(tails[a])
                        for _ in range(tb - ta):
                            box = kf.predict()
                        o = iou64(box, bboxes[tb, ib].astype(np.float64))
                        least_iou = min(least_iou, abs(o - sigma_iou))
                        adm[a, b] = o >= sigma_iou
                        q[a, b] = int(o * Q_ONE) if adm[a, b] else 0
            cols, margin = best_matching(q, adm)
            least_assign = min(least_assign, margin)
            for a, b in enumerate(cols):
                if b >= 0:
                    succ[part[a]] = part[b]
                    links.append((v, part[a], part[b], q[a, b] / Q_ONE))
        heads = set(succ.values())
        for u in members:
            if u in heads:
                continue
            chain = [u]
            while chain[-1] in succ:
                chain.append(succ[chain[-1]])
            n = sum(len(members[c]) for c in chain)
            for c in chain:
                for t, i in members[c]:
                    strack[t, i], tlen[t, i] = u, n
    if margins is not None:
        margins["iou"], margins["assign"] = least_iou, least_assign
    return strack, tlen, links
