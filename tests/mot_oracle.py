"""The MOT metric (viddet_amd/mot_metric.py) once more, as plain Python loops over dicts and sets: what the tests hold
mot_match_host and mot_summary to.  It shares seq_nms.iou_matrix and seq_nms.row_classes with the definition and nothing else:
the assignment is its own scalar augmenting-path loop (`assign_loops`), and `brute_best` walks all matchings of small pools for
the values that are unique: the number of pairs and the sum of q."""
import functools
import itertools

import numpy as np

from viddet_amd.seq_nms import iou_matrix, row_classes

NONE = None                                       # a forbidden cell of assign_loops
BIG = 1 << 62


def assign_loops(cost):
    """cost: a list of R rows of C entries, integers or NONE (forbidden) -> the column of every row, least total cost; rows are
    inserted in order, among columns of equal least slack the lowest wins.  ValueError where a row cannot be assigned.  The
    textbook loop, columns 1 .. C with column 0 standing for the row being inserted."""
    R, C = len(cost), len(cost[0]) if cost else 0
    u, v, p, way = [0] * (R + 1), [0] * (C + 1), [0] * (C + 1), [0] * (C + 1)
    for i in range(1, R + 1):
        p[0] = i
        j0 = 0
        minv = [BIG] * (C + 1)
        used = [False] * (C + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], BIG, -1
            for j in range(1, C + 1):
                if used[j]:
                    continue
                c = cost[i0 - 1][j - 1]
                if c is not NONE:
                    cur = c - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                if minv[j] < delta:
                    delta, j1 = minv[j], j
            if j1 < 0:
                raise ValueError("row %d cannot be assigned" % (i - 1))
            for j in range(C + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                elif minv[j] < BIG:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col = [-1] * R
    for j in range(1, C + 1):
        if p[j]:
            col[p[j] - 1] = j - 1
    return col


def brute_assign(cost):
    """the least total cost over all assignments of every row to a column of its own, None where there is none"""
    R, C = len(cost), len(cost[0]) if cost else 0
    best = None
    for perm in itertools.permutations(range(C), R):
        cells = [cost[i][perm[i]] for i in range(R)]
        if any(c is NONE for c in cells):
            continue
        s = sum(cells)
        if best is None or s < best:
            best = s
    return best


def brute_best(rows, cols, q):
    """q: {(g, j): int} over the admissible pairs -> (pairs, sum of q) of the best matching of rows to cols: the most pairs, then
    the largest sum"""
    def rest(i, free):
        if i == len(rows):
            return (0, 0)
        best = rest(i + 1, free)                                      # the row stays single
        for j in sorted(free):
            if (rows[i], j) in q:
                k, s = rest(i + 1, free - {j})
                best = max(best, (k + 1, s + q[(rows[i], j)]))
        return best

    return rest(0, frozenset(cols))


def _clip_list(clip_start, F):
    if clip_start is None:
        return [(0, F)]
    cs = [int(c) for c in clip_start]
    return list(zip(cs[:-1], cs[1:]))


def match_oracle(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, clip_start=None, num_class=None, iou_thresh=0.5,
                 agnostic=False, seen=None, brute_limit=7):
    """-> (match, miou, flags, adm) as mot_match_host returns them.  `seen`, a dict, counts what occurred: carry-overs,
    assignments with both pools >= 2, switches, unmatched rows of either side, and the frames checked by brute force."""
    gt_boxes, bboxes = np.asarray(gt_boxes, np.float32), np.asarray(bboxes, np.float32)
    F, G, N = gt_boxes.shape[0], gt_boxes.shape[1], bboxes.shape[1]
    pcls = row_classes(np.asarray(ids, np.float32).reshape(F, N), np.asarray(scores, np.float32).reshape(F, N), num_class)
    thr = np.float32(iou_thresh)
    match = np.full((F, G), -2, np.int32)
    miou = np.zeros((F, G), np.float32)
    flags = np.zeros((F, G), np.int32)
    adm = np.zeros((F, G, 4), np.uint32)
    seen = {} if seen is None else seen
    for k in ("carry", "assign22", "switch", "gt_unmatched", "pred_unmatched", "brute"):
        seen.setdefault(k, 0)
    for t0, t1 in _clip_list(clip_start, F):
        last = {}
        for t in range(t0, t1):
            gc, have = [], set()
            for g in range(G):
                a = int(gt_id[t][g])
                if int(gt_cls[t][g]) >= 0 and 0 <= a < 1024 and a not in have:
                    have.add(a)
                    gc.append(g)
            pc, have = [], set()
            for j in range(N):
                p = int(track[t][j])
                if pcls[t][j] >= 0 and p >= 0 and p not in have:
                    have.add(p)
                    pc.append(j)
            iou = iou_matrix(gt_boxes[t], bboxes[t])
            ok = set()
            for g in gc:
                for j in pc:
                    if iou[g, j] >= thr and (agnostic or int(gt_cls[t][g]) == int(pcls[t][j])):
                        ok.add((g, j))
                        adm[t, g, j // 32] |= np.uint32(1 << (j % 32))
            row_of_id = {int(track[t][j]): j for j in pc}
            free = set(pc)
            m, carried = {}, set()
            for g in gc:
                p = last.get(int(gt_id[t][g]))
                j = row_of_id.get(p) if p is not None else None
                if j is not None and j in free and (g, j) in ok:
                    m[g] = j
                    carried.add(g)
                    free.discard(j)
            rg, cp = [g for g in gc if g not in m], sorted(free)
            if rg and cp:
                q = {(g, j): int(np.floor(np.float64(iou[g, j]) * 1048576.0)) for g in rg for j in cp if (g, j) in ok}
                cost = [[(1 << 20) - q[(g, j)] if (g, j) in q else NONE for j in cp] + [(1 << 27) if r == s else NONE for s in range(len(rg))]
                        for r, g in enumerate(rg)]
                col = assign_loops(cost)
                got = [(g, cp[c]) for g, c in zip(rg, col) if c < len(cp)]
                if len(rg) <= brute_limit and len(cp) <= brute_limit:
                    assert brute_best(rg, cp, q) == (len(got), sum(q[pr] for pr in got)), (t, rg, cp)
                    seen["brute"] += 1
                if len(rg) >= 2 and len(cp) >= 2:
                    seen["assign22"] += 1
                for g, j in got:
                    m[g] = j
            for g in gc:
                match[t, g] = m.get(g, -1)
                if g in m:
                    a, p = int(gt_id[t][g]), int(track[t][m[g]])
                    miou[t, g] = iou[g, m[g]]
                    if a in last and last[a] != p:
                        flags[t, g] |= 1
                        seen["switch"] += 1
                    if g in carried:
                        flags[t, g] |= 2
                    last[a] = p
            seen["carry"] += len(carried)
            seen["gt_unmatched"] += len(gc) - len(m)
            seen["pred_unmatched"] += len(pc) - len(m)
    return match, miou, flags, adm


def summary_oracle(records, gt_id, track, clip_start=None):
    """mot_summary as loops -> {'clips': [...], 'all': {...}} with the same keys"""
    match, miou, flags, adm = records
    F, G = match.shape
    N = track.shape[1]
    counts = ("frames", "gt_tracks", "GT", "PRED", "TP", "FN", "FP", "IDSW", "Frag", "MT", "PT", "ML", "IDTP", "IDFP", "IDFN")

    def rates(c, s):
        div = lambda a, b: float(a) / float(b) if b else 0.0
        c["FN"], c["FP"] = c["GT"] - c["TP"], c["PRED"] - c["TP"]
        c["IDFN"], c["IDFP"] = c["GT"] - c["IDTP"], c["PRED"] - c["IDTP"]
        c["MOTA"] = 1.0 - float(c["FN"] + c["FP"] + c["IDSW"]) / float(c["GT"]) if c["GT"] else 0.0
        c["MOTP"] = div(s, c["TP"])
        c["precision"], c["recall"] = div(c["TP"], c["PRED"]), div(c["TP"], c["GT"])
        c["IDF1"], c["IDP"], c["IDR"] = div(2 * c["IDTP"], c["GT"] + c["PRED"]), div(c["IDTP"], c["PRED"]), div(c["IDTP"], c["GT"])
        return c

    total, total_sum, clips = dict.fromkeys(counts, 0), 0.0, []
    for t0, t1 in _clip_list(clip_start, F):
        c = dict.fromkeys(counts, 0)
        c["frames"] = t1 - t0
        s = 0.0
        history, n = {}, {}
        for t in range(t0, t1):
            have = set()
            for j in range(N):
                if int(track[t][j]) >= 0 and int(track[t][j]) not in have:
                    have.add(int(track[t][j]))
                    c["PRED"] += 1
            for g in range(G):
                if match[t, g] == -2:
                    continue
                c["GT"] += 1
                history.setdefault(int(gt_id[t][g]), []).append(bool(match[t, g] >= 0))
                if match[t, g] >= 0:
                    c["TP"] += 1
                    s += float(miou[t, g])
                    total_sum += float(miou[t, g])
                c["IDSW"] += int(flags[t, g]) & 1
                for j in range(N):
                    if (int(adm[t, g, j // 32]) >> (j % 32)) & 1:
                        key = (int(gt_id[t][g]), int(track[t][j]))
                        n[key] = n.get(key, 0) + 1
        for a, h in history.items():
            c["gt_tracks"] += 1
            was, ever = True, False
            for k, now in enumerate(h):
                if now and k > 0 and not was and ever:
                    c["Frag"] += 1
                was, ever = now, ever or now
            # 80 % and 20 % in integers: the tests' tracks sit exactly on the borders
            c["MT" if 5 * sum(h) >= 4 * len(h) else "ML" if 5 * sum(h) < len(h) else "PT"] += 1
        # IDTP: the heaviest one-to-one pairing of ground-truth ids with prediction ids, by its own assignment
        ga, gp = sorted({a for a, _ in n}), sorted({p for _, p in n})
        if n:
            top = max(n.values())
            cost = [[top - n.get((a, p), 0) for p in gp] + [top if r == s2 else NONE for s2 in range(len(ga))] for r, a in enumerate(ga)]
            col = assign_loops(cost)
            c["IDTP"] = sum(n.get((a, gp[k]), 0) for a, k in zip(ga, col) if k < len(gp))
            if len(ga) <= 6 and len(gp) <= 6:                      # and by brute force where that is small
                best = 0
                small, large, flip = (ga, gp, False) if len(ga) <= len(gp) else (gp, ga, True)
                for others in itertools.permutations(large + [None] * len(small), len(small)):
                    best = max(best, sum(n.get((o, s1) if flip else (s1, o), 0) for s1, o in zip(small, others) if o is not None))
                assert best == c["IDTP"]
        for k in counts:
            total[k] += c[k]
        clips.append(rates(c, s))
    return dict(clips=clips, all=rates(total, total_sum))


# ---- the random clips: the ground truth jittered and thinned, plus clutter, linked by track_host --------------------------------
def random_tracks(F, G, N, seed, classes=2, clip_start=None, max_age=0, size=256.0):
    """-> (gt_boxes (F,G,4), gt_cls, gt_id (F,G) int32, ids, scores (F,N,1), bboxes (F,N,4) float32, track (F,N) int32): up to G
    objects that drift (born and dying inside the clip), detected with jitter and holes; clutter rows fill up to N; the rows of
    a frame are shuffled; track is track_host's at `max_age`.  Some padded rows and a few ground-truth rows that are no
    candidates (class -1, id 1024, a repeated id) are mixed in."""
    from viddet_amd.track import track_host
    rng = np.random.default_rng([seed, F, G, N])
    gt_boxes = np.zeros((F, G, 4), np.float32)
    gt_cls, gt_id = np.full((F, G), -1, np.int32), np.full((F, G), -1, np.int32)
    ids, scores = np.full((F, N, 1), -1, np.float32), np.full((F, N, 1), -1, np.float32)
    bboxes = np.full((F, N, 4), -1, np.float32)
    for t0, t1 in _clip_list(clip_start, F):
        T = t1 - t0
        n_obj = int(rng.integers(max(1, G // 2), G + 1))
        c = rng.uniform(0.1, 0.9, (n_obj, 2)) * size
        wh = rng.uniform(16, 60, (n_obj, 2))
        vel = rng.normal(0, 3.0, (n_obj, 2))
        cls = rng.integers(0, classes, n_obj)
        birth = rng.integers(0, max(1, T // 3), n_obj)
        death = rng.integers(T - T // 3, T + 1, n_obj)
        for t in range(T):
            alive = [k for k in range(n_obj) if birth[k] <= t < max(death[k], birth[k] + 1)]
            rows = rng.permutation(G)[:len(alive)]
            dets = []
            for g, k in zip(sorted(rows), alive):
                p = c[k] + vel[k] * t
                box = np.r_[p - wh[k] / 2, p + wh[k] / 2]
                gt_boxes[t0 + t, g], gt_cls[t0 + t, g], gt_id[t0 + t, g] = box, cls[k], k
                if rng.random() < 0.06:                               # a row that is no candidate
                    kind = int(rng.integers(0, 3))
                    if kind == 0:
                        gt_cls[t0 + t, g] = -1
                    elif kind == 1:
                        gt_id[t0 + t, g] = 1024
                    else:
                        gt_id[t0 + t, g] = alive[0]                   # a repeated id (or its own)
                if rng.random() >= 0.2:                               # detected
                    dets.append((cls[k] if rng.random() < 0.9 else (cls[k] + 1) % classes, rng.uniform(0.3, 1.0),
                                 box + rng.normal(0, 0.05, 4) * np.r_[wh[k], wh[k]]))
            for _ in range(int(rng.integers(0, max(1, N // 4) + 1))):  # clutter
                p, s = rng.uniform(0, size, 2), rng.uniform(10, 50, 2)
                dets.append((int(rng.integers(0, classes)), rng.uniform(0.05, 0.6), np.r_[p, p + s]))
            dets = dets[:N]
            for j, d in zip(sorted(rng.permutation(N)[:len(dets)]), dets):
                ids[t0 + t, j, 0], scores[t0 + t, j, 0], bboxes[t0 + t, j] = d
    track = track_host(ids, scores, bboxes, clip_start=clip_start, num_class=classes, sigma_h=0.0, t_min=1, max_age=max_age)[0]
    return gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track


SHAPES = [(1, 1, 1), (2, 3, 3), (5, 64, 65), (6, 128, 128), (40, 20, 20)]
THREE_CLIPS = [0, 7, 7, 19, 24]                   # three clips of unequal length and an empty one between them


@functools.lru_cache(maxsize=None)
def random_cases():
    """(name, arrays, kwargs) over SHAPES x max_age (0, 7) x agnostic, and the three clips in one call"""
    out = []
    for F, G, N in SHAPES:
        for age in (0, 7):
            arrays = random_tracks(F, G, N, seed=11 + age, max_age=age)
            for ag in (False, True):
                out.append(("%dx%dx%d_age%d_%s" % (F, G, N, age, "ag" if ag else "cls"), arrays, dict(num_class=2, agnostic=ag)))
    for age in (0, 7):
        arrays = random_tracks(THREE_CLIPS[-1], 6, 8, seed=5 + age, clip_start=THREE_CLIPS, max_age=age)
        for ag in (False, True):
            out.append(("clips_age%d_%s" % (age, "ag" if ag else "cls"), arrays, dict(num_class=2, agnostic=ag, clip_start=THREE_CLIPS)))
    return out


def tie_case(F, G, N, seed, spots=10):
    """rows of both sides drawn from a few fixed boxes, one class, distinct ids: equal costs everywhere, so the assignment's tie
    rules decide; the track ids are shuffled from frame to frame for some rows, which makes carry-overs compete with them"""
    rng = np.random.default_rng([seed, F, G, N])
    grid = np.array([[16.0 * k, 8.0 * (k % 3), 16.0 * k + 24.0, 8.0 * (k % 3) + 24.0] for k in range(spots)], np.float32)
    gt_boxes = grid[rng.integers(0, spots, (F, G))]
    bboxes = grid[rng.integers(0, spots, (F, N))]
    gt_cls, ids, scores = np.zeros((F, G), np.int32), np.zeros((F, N, 1), np.float32), np.full((F, N, 1), 0.9, np.float32)
    gt_id = np.stack([rng.permutation(G) for _ in range(F)]).astype(np.int32)
    track = np.stack([rng.permutation(N + 3)[:N] for _ in range(F)]).astype(np.int32)
    gt_cls[rng.random((F, G)) < 0.05] = -1
    track[rng.random((F, N)) < 0.05] = -1
    return gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track


@functools.lru_cache(maxsize=None)
def tie_cases():
    """(name, arrays, kwargs): small enough for the brute force, and wider than a wavefront's 64 columns"""
    return [("ties_%dx%dx%d" % shape, tie_case(*shape, seed=3, spots=spots), dict(num_class=1))
            for shape, spots in (((4, 6, 7), 3), ((3, 100, 100), 10), ((2, 128, 128), 10))]
