"""HOTA as the paper writes it (Luiten et al., IJCV 2021, sections 4 to 6 and the form of its evaluation code), in loops and
float64: the oracle that tests/test_hota_metric_cpu.py holds viddet_amd.hota_metric.hota_match_host and hota_summary to.  The
similarity is a float64 IoU, the normalised similarity and the global alignment score are floats, a frame's matching is a
brute-force enumeration of every matching under the score-sum objective, and the alpha tests and the figures come straight from
the formulas.  Nothing here is shared with the definition but the class rule of the rows (seq_nms.row_classes), the clip
offsets (seq_nms._clips) and the stated departures: classes must agree unless agnostic, the first row of an id in its frame
stands, a zero denominator gives 0."""
import math

import numpy as np

from viddet_amd.seq_nms import _clips, row_classes

ALPHAS = [np.float32(0.05 * k) for k in range(1, 20)]


def iou64(a, b):
    a, b = [float(x) for x in a], [float(x) for x in b]
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if not (iw > 0 and ih > 0):                                            # a NaN compares false
        return 0.0
    inter = iw * ih
    o = inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)
    return o if o > 0 else 0.0                                             # inf / inf: a NaN counts as 0


def best_matching(score):
    """score: {(i, k): s > 0} over rows i and columns k -> ({i: k} of the largest score sum, its margin over the runner-up: the
    best sum of a DIFFERENT set of pairs).  Every matching is enumerated; a row may stay single at score 0."""
    rows = sorted({i for i, _ in score})
    found = []

    def walk(n, taken, total, pairs):
        if n == len(rows):
            found.append((total, pairs))
            return
        i = rows[n]
        walk(n + 1, taken, total, pairs)
        for (r, k), s in score.items():
            if r == i and k not in taken:
                walk(n + 1, taken | {k}, total + s, pairs + ((i, k),))

    walk(0, frozenset(), 0.0, ())
    found.sort(key=lambda f: -f[0])
    margin = found[0][0] - found[1][0] if len(found) > 1 else math.inf
    return dict(found[0][1]), margin


def _first_rows(eligible, ids):
    seen, out = set(), []
    for r, (ok, i) in enumerate(zip(eligible, ids)):
        if ok and int(i) not in seen:
            seen.add(int(i))
            out.append(r)
    return out


def hota_oracle(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, clip_start=None, num_class=None, agnostic=False, margins=None):
    """-> (match (F,G) as hota_match_host returns it, [per clip: dict(TP, FN, FP: lists per alpha; mc: per alpha {(a, p): n};
    cg, cp: {id: n}; GT, PRED; the per-alpha lists DetA@ ... and their means DetA ...; sim: {(t, g): the matched pair's IoU})]).
    margins, a dict, receives 'alpha': the least |S - alpha| over every matched pair and alpha, and 'assign': the least margin of a
    frame's best matching over its runner-up."""
    gt_boxes, bboxes = np.asarray(gt_boxes, np.float32), np.asarray(bboxes, np.float32)
    F, G, N = gt_boxes.shape[0], gt_boxes.shape[1], bboxes.shape[1]
    gt_cls, gt_id, track = np.asarray(gt_cls), np.asarray(gt_id), np.asarray(track)
    pcls = row_classes(np.asarray(ids, np.float32).reshape(F, N), np.asarray(scores, np.float32).reshape(F, N), num_class)
    match = np.full((F, G), -2, dtype=np.int32)
    least_alpha, least_assign = math.inf, math.inf
    clips = []
    for t0, t1 in _clips(clip_start, F):
        rows_g, rows_p, sim = {}, {}, {}
        pm, cg, cp = {}, {}, {}
        for t in range(t0, t1):
            rows_g[t] = _first_rows([gt_cls[t, g] >= 0 and 0 <= gt_id[t, g] < 1024 for g in range(G)], gt_id[t])
            rows_p[t] = _first_rows([pcls[t, j] >= 0 and track[t, j] >= 0 for j in range(N)], track[t])
            S = {}
            for g in rows_g[t]:
                for j in rows_p[t]:
                    if agnostic or gt_cls[t, g] == pcls[t, j]:
                        o = iou64(gt_boxes[t, g], bboxes[t, j])
                        if o > 0:
                            S[g, j] = o
            sim[t] = S
            for (g, j), o in S.items():
                rowsum = sum(v for (g2, _), v in S.items() if g2 == g)
                colsum = sum(v for (_, j2), v in S.items() if j2 == j)
                key = int(gt_id[t, g]), int(track[t, j])
                pm[key] = pm.get(key, 0.0) + o / (rowsum + colsum - o)
            for g in rows_g[t]:
                cg[int(gt_id[t, g])] = cg.get(int(gt_id[t, g]), 0) + 1
            for j in rows_p[t]:
                cp[int(track[t, j])] = cp.get(int(track[t, j]), 0) + 1
        align = {(a, p): v / (cg[a] + cp[p] - v) for (a, p), v in pm.items()}
        matched = []                                                       # (t, g, j, S) in frame, row order
        for t in range(t0, t1):
            for g in rows_g[t]:
                match[t, g] = -1
            if rows_g[t] and rows_p[t] and sim[t]:
                score = {(g, j): align[int(gt_id[t, g]), int(track[t, j])] * o for (g, j), o in sim[t].items()}
                pairs, margin = best_matching(score)
                least_assign = min(least_assign, margin)
                for g in sorted(pairs):
                    match[t, g] = pairs[g]
                    matched.append((t, g, pairs[g], sim[t][g, pairs[g]]))
        c = dict(GT=sum(cg.values()), PRED=sum(cp.values()), cg=cg, cp=cp, TP=[], FN=[], FP=[], mc=[],
                 sim={(t, g): o for t, g, _, o in matched})
        per = {k: [] for k in ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")}
        for alpha in ALPHAS:
            al = float(alpha)
            tps = [(t, g, j, o) for t, g, j, o in matched if o >= al]
            least_alpha = min([least_alpha] + [abs(o - al) for _, _, _, o in matched])
            mc = {}
            for t, g, j, _ in tps:
                key = int(gt_id[t, g]), int(track[t, j])
                mc[key] = mc.get(key, 0) + 1
            tp = len(tps)
            fn, fp = c["GT"] - tp, c["PRED"] - tp
            c["TP"].append(tp), c["FN"].append(fn), c["FP"].append(fp), c["mc"].append(mc)
            div = lambda x, y: x / y if y else 0.0
            # the paper's A(c) of a TP c = (a, p): TPA = mc, FNA = cg - mc, FPA = cp - mc; every TP of the pair shares it
            per["AssA"].append(div(sum(n * (n / (cg[a] + cp[p] - n)) for (a, p), n in mc.items()), tp))
            per["AssRe"].append(div(sum(n * (n / cg[a]) for (a, p), n in mc.items()), tp))
            per["AssPr"].append(div(sum(n * (n / cp[p]) for (a, p), n in mc.items()), tp))
            per["DetA"].append(div(tp, tp + fn + fp))
            per["DetRe"].append(div(tp, tp + fn))
            per["DetPr"].append(div(tp, tp + fp))
            per["LocA"].append(div(sum(o for _, _, _, o in tps), tp))
            per["HOTA"].append(math.sqrt(per["DetA"][-1] * per["AssA"][-1]))
        for k, v in per.items():
            c[k + "@"] = v
            c[k] = sum(v) / len(v)
        clips.append(c)
    if margins is not None:
        margins["alpha"], margins["assign"] = least_alpha, least_assign
    return match, clips


def crowd(seed, F, G, N, A, P, num_class=2, spread=200.0):
    """F frames of G label rows and N prediction rows whose boxes crowd one corner of the frame, so that (almost) every column
    is in play: dense ids drawn per frame from [0, A) and [0, P) - a few of them twice in a frame, a few outside the range -,
    a few rows that are no candidates (class -1, a NaN score), the first predictions copies of label boxes (IoU 1: ties)"""
    rng = np.random.default_rng(seed)

    def boxes(n):
        c, wh = rng.uniform(50, 50 + spread, (F, n, 2)), rng.uniform(60, 100, (F, n, 2))
        return np.concatenate([c - wh / 2, c + wh / 2], axis=2).astype(np.float32)

    def draw(n, hi):
        ids = np.stack([rng.permutation(max(n, hi))[:n] % hi for _ in range(F)]).astype(np.int32)
        twice = rng.random(F) < 0.5
        ids[twice, n - 1] = ids[twice, 0]                                   # the id of row 0 again: the lower row stands
        ids[rng.random((F, n)) < 0.04] = hi                                 # outside: takes no part
        ids[rng.random((F, n)) < 0.03] = -1
        return ids

    gt_boxes, bboxes = boxes(G), boxes(N)
    k = min(G, N) // 3
    bboxes[:, :k] = gt_boxes[:, :k]
    gt_cls = rng.integers(0, num_class, (F, G)).astype(np.int32)
    gt_cls[rng.random((F, G)) < 0.05] = -1
    ids = rng.integers(0, num_class, (F, N, 1)).astype(np.float32)
    ids[rng.random((F, N, 1)) < 0.05] = -1
    scores = rng.uniform(0.1, 1.0, (F, N, 1)).astype(np.float32)
    scores[rng.random((F, N, 1)) < 0.03] = np.nan
    return gt_boxes, gt_cls, draw(G, A), ids, scores, bboxes, draw(N, P)


def random_clip(seed, F=10, objects=5, num_class=2, N=None):
    """A seeded clip of `objects` ground-truth tracks (at most 6) answered by a noisy tracker: boxes jittered by a few percent,
    misses, false positives, an identity switch half way and a track that is cut in two -> the seven arrays"""
    from tests.mot_cases import build
    rng = np.random.default_rng(seed)
    gt, pred = [], []
    base = rng.uniform(0, 300, (objects, 2))
    size = rng.uniform(30, 60, (objects, 2))
    vel = rng.uniform(-6, 6, (objects, 2))
    cls = rng.integers(0, num_class, objects)
    born, dies = rng.integers(0, 3, objects), rng.integers(F - 2, F + 1, objects)
    swap = tuple(rng.choice(objects, 2, replace=False)) if objects >= 2 else None
    cut = int(rng.integers(0, objects))
    for t in range(F):
        g_rows, p_rows = [], []
        for o in range(objects):
            if not born[o] <= t < dies[o]:
                continue
            x, y = base[o] + vel[o] * t
            w, h = size[o]
            g_rows.append(((x, y, x + w, y + h), int(cls[o]), int(o) * 7 + 1))
            if rng.random() < 0.15:
                continue                                                   # a miss
            dx, dy, dw, dh = rng.uniform(-0.08, 0.08, 4) * (w, h, w, h)
            tid = o
            if swap and t >= F // 2 and o in swap:
                tid = swap[1] if o == swap[0] else swap[0]                 # the two exchange their prediction ids
            if o == cut and t >= F // 2 + 1:
                tid = objects + 3                                          # the track is cut: a new id
            pc = int(cls[o]) if rng.random() > 0.05 else int((cls[o] + 1) % num_class)
            p_rows.append(((x + dx, y + dy, x + w + dw, y + h + dh), pc, float(rng.uniform(0.3, 1.0)), 10 + 3 * tid))
        if rng.random() < 0.3:
            x, y = rng.uniform(0, 300, 2)
            p_rows.append(((x, y, x + 40, y + 40), int(rng.integers(0, num_class)), 0.5, 90 + t // 3))   # a false positive
        order = rng.permutation(len(p_rows))
        gt.append(g_rows)
        pred.append([p_rows[i] for i in order])
    return build(gt, pred, N=N)
