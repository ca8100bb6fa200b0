"""The MOT tracking metric: the CLEAR MOT figures (Bernardin and Stiefelhagen, "Evaluating Multiple Object Tracking Performance:
The CLEAR MOT Metrics", 2008) and the identity figures (Ristani et al., "Performance Measures and a Data Set for Multi-Target,
Multi-Camera Tracking", 2016) of the tracks that --track, the live sessions and --tubelet produce: the definition.

`mot_match_host` is the normative per-frame matching: NumPy, float32 where boxes meet (seq_nms.iou_matrix),
integers everywhere else.  The device entry point vd_mot_match (viddet_amd/csrc/vd_mot_eval.hip, `ops.mot_match`) equals it bit
for bit on all four outputs.  `mot_summary` is the host accumulation that both paths share.

Per clip [t0, t1), frames in order, with last[a] (a in [0, 1024)) the prediction id a ground-truth id was matched to last, all
"none" at t0:
  1. candidates: a prediction row is eligible iff seq_nms.row_classes makes it a candidate and track[t, j] >= 0, and a candidate
     iff no lower eligible row of its frame carries the same track id (the tubelet membership rule); a ground-truth row is
     eligible iff gt_cls >= 0 and 0 <= gt_id < 1024, and a candidate iff no lower eligible row of its frame carries the same id.
     Other rows take no part and are never counted (a prediction with track -1 is not tracker output).
  2. admissible pairs: both rows candidates, iou >= float32(iou_thresh), and (agnostic or equal classes); adm[t, g, j // 32]
     has bit j % 32 set exactly for them.
  3. carry-over: ground-truth candidates in ascending row order; where last[gt_id] is prediction id p, the candidate prediction
     row j carrying p is still free and (g, j) is admissible, g is matched to j and both leave the pool.
  4. the rest: with q = int(floor(iou * 2**20)) (exact in float32), among the remaining candidates the matching over admissible
     pairs with the most pairs, among those the one with the largest sum of q.  That (pairs, sum) is unique, the assignment is
     not, so the algorithm is fixed: `assign_host` on the cost 2**20 - q of an admissible pair, one dummy column per row at
     2**27, everything else forbidden; rows = the remaining ground-truth candidates in row order, columns = the remaining
     prediction candidates in row order, then the dummies.  Entered only when both pools are non-empty.
  5. records: match[t, g] the prediction row, -1 an unmatched candidate, -2 no candidate; miou the pair's IoU, else 0; flags bit
     0: an id switch - a matched g whose last[a] is set and differs from the matched prediction id (a carry-over match never
     switches) -, bit 1: the match is a carry-over; then last[a] becomes the matched id.  An unmatched frame leaves last[a] as it
     is (no switch-time limit).

Stated departures: a zero denominator gives 0.0 (py-motmetrics: NaN); classes must agree unless `agnostic`; no
TRANSFER / ASCEND / MIGRATE events; the distance is the project's float32 IoU, quantised to 2**-20 for the assignment.

This module imports NumPy only.
"""
import numpy as np

from .seq_nms import MAX_ROWS, _clips, iou_matrix, row_classes

_F = np.float32
MAX_GT_ID = 1024                                  # ground-truth track ids lie in [0, MAX_GT_ID): the `last` table of vd_mot_match
Q_ONE = 1 << 20                                   # q of an IoU of 1
DUMMY_COST = 1 << 27                              # a ground-truth row that stays unmatched
FORBIDDEN = np.int64(1) << np.int64(62)           # assign_host: a cell that may not be chosen
MAX_COST = 1 << 40                                # assign_host: |cost| stays below this, so no potential leaves int64
COUNTS = ("frames", "gt_tracks", "GT", "PRED", "TP", "FN", "FP", "IDSW", "Frag", "MT", "PT", "ML", "IDTP", "IDFP", "IDFN")
RATES = ("MOTA", "MOTP", "precision", "recall", "IDF1", "IDP", "IDR")


def assign_host(cost):
    """The assignment of every row of cost (R,C) int64 to a column of its own at the least total cost; a cell equal to FORBIDDEN
    may not be chosen.  -> (R,) int64, the column of every row.  ValueError where no such assignment exists.

    Successive shortest augmenting paths with potentials, rows inserted in ascending order, in int64.  Among the columns of equal
    least slack the lowest wins.  Vectorised over the columns only: every step is a minimum over (slack, column index) and an
    elementwise update, which is the operation a workgroup with a thread per column performs (vd_mot_eval.hip)."""
    cost = np.asarray(cost)
    if cost.ndim != 2 or cost.dtype.kind not in "iu":
        raise ValueError("assign_host: cost must be an (R,C) integer matrix, got %r %s" % (cost.shape, cost.dtype))
    cost = cost.astype(np.int64)
    R, C = cost.shape
    ok = cost != FORBIDDEN
    if (np.abs(np.where(ok, cost, 0)) >= MAX_COST).any():
        raise ValueError("assign_host: |cost| must stay below 2**40")
    u = np.zeros(R, dtype=np.int64)                                  # the rows' potentials
    v = np.zeros(C, dtype=np.int64)                                  # the columns'
    row_of = np.full(C, -1, dtype=np.int64)                          # the row a column is matched to
    for i in range(R):
        minv = np.full(C, FORBIDDEN, dtype=np.int64)                 # the least slack to every column over the rows of the tree
        way = np.full(C, -1, dtype=np.int64)                         # the column ahead of it on that path, -1: the new row
        used = np.zeros(C, dtype=bool)
        i0, j0 = i, -1
        while True:
            cur = cost[i0] - u[i0] - v
            better = ok[i0] & ~used & (cur < minv)
            minv = np.where(better, cur, minv)
            way = np.where(better, j0, way)
            key = np.where(used, FORBIDDEN, minv)
            j1 = int(np.argmin(key)) if C else -1                    # the first minimum: the lowest column of a tie
            delta = key[j1] if C else FORBIDDEN
            if delta == FORBIDDEN:
                raise ValueError("assign_host: row %d cannot be assigned" % i)
            u[i] += delta
            u[row_of[used]] += delta                                 # the used columns are matched, to rows of their own
            v[used] -= delta
            minv = np.where(~used & (minv != FORBIDDEN), minv - delta, minv)
            used[j1] = True
            j0 = j1
            if row_of[j1] < 0:
                break
            i0 = int(row_of[j1])
        while j0 >= 0:                                               # the path back to the new row, every column handed on
            jp = int(way[j0])
            row_of[j0] = row_of[jp] if jp >= 0 else i
            j0 = jp
    col_of = np.full(R, -1, dtype=np.int64)
    col_of[row_of[row_of >= 0]] = np.nonzero(row_of >= 0)[0]
    return col_of


def first_of_id(eligible, ids):
    """(n,) bool, (n,) integers -> (n,) bool: the eligible rows that no lower eligible row shares its id with"""
    out = np.zeros(len(ids), dtype=bool)
    rows = np.nonzero(eligible)[0]
    if len(rows):
        out[rows[np.unique(ids[rows], return_index=True)[1]]] = True
    return out


def masked_track(ids, scores, track, num_class=None):
    """track (F,N) with -1 on every row that seq_nms.row_classes makes no candidate: the table mot_summary reads.  The matching
    gives the same records on either table, since such rows take no part."""
    track = np.asarray(track)
    F, N = track.shape
    ok = row_classes(np.asarray(ids, dtype=_F).reshape(F, N), np.asarray(scores, dtype=_F).reshape(F, N), num_class) >= 0
    return np.where(ok, track, -1).astype(np.int32)


def _check_inputs(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, who):
    gt_boxes, bboxes = np.asarray(gt_boxes, dtype=_F), np.asarray(bboxes, dtype=_F)
    ids, scores = np.asarray(ids, dtype=_F), np.asarray(scores, dtype=_F)
    if gt_boxes.ndim != 3 or gt_boxes.shape[2] != 4 or bboxes.ndim != 3 or bboxes.shape[2] != 4 or bboxes.shape[0] != gt_boxes.shape[0]:
        raise ValueError("%s: expected gt_boxes (F,G,4) and bboxes (F,N,4), got %r %r" % (who, gt_boxes.shape, bboxes.shape))
    F, G, N = gt_boxes.shape[0], gt_boxes.shape[1], bboxes.shape[1]
    if not 1 <= G <= MAX_ROWS or not 1 <= N <= MAX_ROWS:
        raise ValueError("%s: G=%d label rows and N=%d prediction rows per frame, 1 to %d of either are taken" % (who, G, N, MAX_ROWS))
    if ids.size != F * N or scores.size != F * N:
        raise ValueError("%s: expected ids (F,N[,1]) and scores (F,N[,1]), got %r %r" % (who, ids.shape, scores.shape))
    tables = []
    for name, a, shape in (("gt_cls", gt_cls, (F, G)), ("gt_id", gt_id, (F, G)), ("track", track, (F, N))):
        a = np.asarray(a)
        if a.shape != shape or a.dtype.kind not in "iu":
            raise ValueError("%s: expected %s %r of integers, got %r %s" % (who, name, shape, a.shape, a.dtype))
        tables.append(a.astype(np.int64))
    return [gt_boxes] + tables[:2] + [ids.reshape(F, N), scores.reshape(F, N), bboxes, tables[2]]


def check_iou_thresh(iou_thresh, who):
    try:
        f = _F(iou_thresh)
    except (TypeError, ValueError):
        raise ValueError("%s: iou_thresh must be a number, got %r" % (who, iou_thresh))
    if not (f > 0 and f <= 1):
        raise ValueError("%s: iou_thresh must lie in (0, 1], got %r" % (who, iou_thresh))
    return f


def mot_match_host(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, clip_start=None, num_class=None, iou_thresh=0.5,
                   agnostic=False):
    """gt_boxes (F,G,4), gt_cls (F,G), gt_id (F,G), ids (F,N[,1]), scores (F,N[,1]), bboxes (F,N,4), track (F,N) ->
    (match (F,G) int32, miou (F,G) float32, flags (F,G) int32, adm (F,G,4) uint32), as the module's head defines them.  Rows of
    frames that no clip covers get -2 / 0 / 0 / 0."""
    gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track = _check_inputs(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track,
                                                                        "mot_match_host")
    thr = check_iou_thresh(iou_thresh, "mot_match_host")
    F, G, N = gt_boxes.shape[0], gt_boxes.shape[1], bboxes.shape[1]
    pcls = row_classes(ids, scores, num_class)
    match = np.full((F, G), -2, dtype=np.int32)
    miou = np.zeros((F, G), dtype=_F)
    flags = np.zeros((F, G), dtype=np.int32)
    adm = np.zeros((F, G, 4), dtype=np.uint32)
    bit = np.uint32(1) << (np.arange(N, dtype=np.uint32) % np.uint32(32))
    for t0, t1 in _clips(clip_start, F):
        last = np.full(MAX_GT_ID, -1, dtype=np.int64)
        for t in range(t0, t1):
            gc = first_of_id((gt_cls[t] >= 0) & (gt_id[t] >= 0) & (gt_id[t] < MAX_GT_ID), gt_id[t])
            pc = first_of_id((pcls[t] >= 0) & (track[t] >= 0), track[t])
            iou = iou_matrix(gt_boxes[t], bboxes[t])
            with np.errstate(invalid="ignore"):
                ok = gc[:, None] & pc[None, :] & (iou >= thr)
            if not agnostic:
                ok &= gt_cls[t][:, None] == pcls[t][None, :]
            for w in range((N + 31) // 32):
                adm[t, :, w] = np.bitwise_or.reduce(np.where(ok[:, 32 * w:32 * w + 32], bit[32 * w:32 * w + 32], np.uint32(0)), axis=1)
            m = np.where(gc, -1, -2).astype(np.int64)
            carried = np.zeros(G, dtype=bool)
            free = pc.copy()
            # 3. carry-over, in row order
            for g in np.nonzero(gc)[0]:
                p = last[gt_id[t, g]]
                if p >= 0:
                    j = np.nonzero(pc & (track[t] == p))[0]
                    if len(j) and free[j[0]] and ok[g, j[0]]:
                        m[g], carried[g], free[j[0]] = j[0], True, False
            # 4. the rest
            rg, cp = np.nonzero(gc & (m < 0))[0], np.nonzero(free)[0]
            if len(rg) and len(cp):
                q = np.floor(iou[np.ix_(rg, cp)] * _F(Q_ONE)).astype(np.int64)
                cost = np.full((len(rg), len(cp) + len(rg)), FORBIDDEN, dtype=np.int64)
                cost[:, :len(cp)] = np.where(ok[np.ix_(rg, cp)], Q_ONE - q, FORBIDDEN)
                cost[np.arange(len(rg)), len(cp) + np.arange(len(rg))] = DUMMY_COST
                col = assign_host(cost)
                hit = col < len(cp)
                m[rg[hit]] = cp[col[hit]]
            # 5. records
            on = np.nonzero(m >= 0)[0]
            a, p = gt_id[t, on], track[t, m[on]]
            switch = (last[a] >= 0) & (last[a] != p)
            match[t] = m
            miou[t, on] = iou[on, m[on]]
            flags[t, on] = switch.astype(np.int32) | (carried[on].astype(np.int32) << 1)
            last[a] = p
    return match, miou, flags, adm


def _rate(num, den):
    return float(num) / float(den) if den else 0.0


def _figures(c, iou_sum):
    """the rates of one block of counts (a dict of the COUNTS without the three identity counts' complements)"""
    c["FN"], c["FP"] = c["GT"] - c["TP"], c["PRED"] - c["TP"]
    c["IDFN"], c["IDFP"] = c["GT"] - c["IDTP"], c["PRED"] - c["IDTP"]
    c["MOTA"] = 1.0 - float(c["FN"] + c["FP"] + c["IDSW"]) / float(c["GT"]) if c["GT"] else 0.0
    c["MOTP"] = iou_sum / float(c["TP"]) if c["TP"] else 0.0
    c["precision"], c["recall"] = _rate(c["TP"], c["PRED"]), _rate(c["TP"], c["GT"])
    c["IDF1"] = _rate(2 * c["IDTP"], c["GT"] + c["PRED"])
    c["IDP"], c["IDR"] = _rate(c["IDTP"], c["PRED"]), _rate(c["IDTP"], c["GT"])
    return c


def id_true_positives(pairs):
    """pairs (k,2) int64, one row per (frame, admissible pair): ground-truth id, prediction id -> IDTP, the largest number of
    those rows that a one-to-one pairing of ground-truth ids with prediction ids covers (any id may stay single)"""
    if not len(pairs):
        return 0
    ga, a = np.unique(pairs[:, 0], return_inverse=True)
    gp, p = np.unique(pairs[:, 1], return_inverse=True)
    n = np.zeros((len(ga), len(gp)), dtype=np.int64)
    np.add.at(n, (a, p), 1)
    top = int(n.max())
    cost = np.full((len(ga), len(gp) + len(ga)), FORBIDDEN, dtype=np.int64)
    cost[:, :len(gp)] = top - n
    cost[np.arange(len(ga)), len(gp) + np.arange(len(ga))] = top      # single: weight 0
    col = assign_host(cost)
    hit = col < len(gp)
    return int(n[np.nonzero(hit)[0], col[hit]].sum())


def mot_summary(records, gt_id, track, clip_start=None):
    """records = (match, miou, flags, adm) of mot_match_host / ops.mot_match, gt_id (F,G) and track (F,N) the id tables the
    matching read - track with -1 on every row that is no detection (masked_track) - -> {'clips': [per clip], 'all': overall},
    each a dict of COUNTS (integers) and RATES (floats).
      GT / PRED   the candidate rows: match != -2; track >= 0 on the first row of its id in the frame
      Frag        over a ground-truth track's candidate frames in order, the frames where it is matched, was unmatched in its
                  previous candidate frame and was matched at some earlier one
      MT, PT, ML  matched in at least 80 % / in under 20 % of its candidate frames (in integers: 5 * matched >= 4 * frames,
                  5 * matched < frames), PT the others
      MOTP        sum(miou) / TP, the sum in float64 in clip, frame, row order (a clip's own from 0.0 likewise)
      IDTP        per clip id_true_positives of the (gt id, prediction id) of every admissible pair (read off adm); summed
    A zero denominator gives 0.0."""
    match, miou, flags, adm = [np.asarray(a) for a in records]
    gt_id, track = np.asarray(gt_id).astype(np.int64), np.asarray(track).astype(np.int64)
    F, G = match.shape
    N = track.shape[1]
    if miou.shape != (F, G) or flags.shape != (F, G) or adm.shape != (F, G, 4) or gt_id.shape != (F, G) or track.shape[0] != F:
        raise ValueError("mot_summary: the records and the id tables do not fit: %r %r %r %r %r %r"
                         % (match.shape, miou.shape, flags.shape, adm.shape, gt_id.shape, track.shape))
    adm = adm.view(np.uint32) if adm.dtype == np.int32 else adm.astype(np.uint32)
    bits = ((adm[:, :, np.arange(N) // 32] >> (np.arange(N, dtype=np.uint32) % np.uint32(32))) & np.uint32(1)).astype(bool)
    clips, total, total_iou = [], dict.fromkeys(COUNTS, 0), 0.0
    for t0, t1 in _clips(clip_start, F):
        c = dict.fromkeys(COUNTS, 0)
        c["frames"] = t1 - t0
        m = match[t0:t1]
        c["GT"], c["TP"] = int((m != -2).sum()), int((m >= 0).sum())
        c["IDSW"] = int((flags[t0:t1] & 1).sum())
        for t in range(t0, t1):
            c["PRED"] += int(first_of_id(track[t] >= 0, track[t]).sum())
        vals = miou[t0:t1][m >= 0].astype(np.float64)                # frame, row order
        iou_sum = float(np.cumsum(vals)[-1]) if len(vals) else 0.0   # one after the other
        if len(vals):
            total_iou = float(np.cumsum(np.concatenate(([total_iou], vals)))[-1])
        ft, fg = np.nonzero(m != -2)
        a, hit = gt_id[t0:t1][ft, fg], m[ft, fg] >= 0
        for one in np.unique(a):
            h = hit[a == one]                                        # the track's candidate frames in order
            c["gt_tracks"] += 1
            seen = np.concatenate(([False], np.logical_or.accumulate(h)[:-1]))
            c["Frag"] += int((h[1:] & ~h[:-1] & seen[1:]).sum())
            k, n = int(h.sum()), len(h)
            c["MT" if 5 * k >= 4 * n else "ML" if 5 * k < n else "PT"] += 1
        pt, pg, pj = np.nonzero(bits[t0:t1])
        c["IDTP"] = id_true_positives(np.stack([gt_id[t0:t1][pt, pg], track[t0:t1][pt, pj]], axis=1))
        for k in COUNTS:
            total[k] += c[k]
        clips.append(_figures(c, iou_sum))
    return dict(clips=clips, all=_figures(total, total_iou))


def check_dataset(dataset):
    """the sample ids of a set of clips with track labels; NotImplementedError for a set that has none"""
    if not all(hasattr(dataset, a) for a in ("get_sample_ids", "get_label", "frames_per_video", "image_size")):
        raise NotImplementedError("MOTMetric: the dataset has no clips with ground-truth tracks (the combined set of several "
                                  "--dataset names has none)")
    ids = list(dataset.get_sample_ids())
    if ids and isinstance(ids[0], (list, tuple)):
        raise NotImplementedError("MOTMetric: window sample ids (--mult_out) are not built")
    ids = [int(i) for i in ids]
    if len(ids) % int(dataset.frames_per_video):
        raise ValueError("MOTMetric: %d samples are no whole clips of %d frames" % (len(ids), dataset.frames_per_video))
    return ids


def _integral(a, what, sid):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        fine = np.isfinite(a) & (a == np.floor(a)) & (np.abs(a) < 2 ** 31)
    if not fine.all():
        with np.errstate(invalid="ignore"):
            bad = a[~(np.isfinite(a) & (a == np.floor(a)) & (np.abs(a) < 2 ** 31))]
        raise ValueError("MOTMetric: sample id %d holds a %s that is no integer: %r" % (sid, what, bad[0]))
    return a.astype(np.int64)


def pack_clips(dataset, results):
    """-> (arrays, clip_start): arrays = gt_boxes (F,G,4) f32, gt_cls (F,G) i32, gt_id (F,G) i32, ids (F,N) f32, scores (F,N)
    f32, bboxes (F,N,4) f32, track (F,N) i32 over the dataset's images in get_sample_ids() order, padded to the largest G and N
    present (at least 1; a padded row: class -1, id -1, track -1).  results: {sid: [[label, score, x1, y1, x2, y2, track]]} in
    source pixels.  An image without a row is a frame without predictions.  Rows of sample ids the dataset does not hold are
    dropped."""
    sids = check_dataset(dataset)
    T = int(dataset.frames_per_video)
    labels, preds = [], []
    for sid in sids:
        rows = np.asarray(dataset.get_label(sid), dtype=np.float64)
        rows = rows.reshape(len(rows), -1) if rows.size else np.zeros((0, 6))
        if len(rows) > MAX_ROWS:
            raise ValueError("MOTMetric: sample id %d holds %d label rows, at most %d are taken" % (sid, len(rows), MAX_ROWS))
        gid = _integral(rows[:, 5], "ground-truth track id", sid)
        if ((gid < 0) | (gid >= MAX_GT_ID)).any():
            raise ValueError("MOTMetric: sample id %d holds the ground-truth track id %d, ids in [0, %d) are taken"
                             % (sid, gid[(gid < 0) | (gid >= MAX_GT_ID)][0], MAX_GT_ID))
        _integral(rows[:, 4], "ground-truth class", sid)
        labels.append(rows)
        p = np.asarray(results.get(sid, []), dtype=np.float64).reshape(-1, 7)
        if len(p) > MAX_ROWS:
            raise ValueError("MOTMetric: sample id %d holds %d prediction rows, at most %d are taken" % (sid, len(p), MAX_ROWS))
        _integral(p[:, 6], "track id", sid)
        preds.append(p)
    F = len(sids)
    G, N = max([1] + [len(r) for r in labels]), max([1] + [len(p) for p in preds])
    gt_boxes, gt_cls, gt_id = np.zeros((F, G, 4), _F), np.full((F, G), -1, np.int32), np.full((F, G), -1, np.int32)
    ids, scores, bboxes = np.full((F, N), -1, _F), np.full((F, N), -1, _F), np.full((F, N, 4), -1, _F)
    track = np.full((F, N), -1, np.int32)
    for t, (rows, p) in enumerate(zip(labels, preds)):
        g, n = len(rows), len(p)
        gt_boxes[t, :g], gt_cls[t, :g], gt_id[t, :g] = rows[:, :4], rows[:, 4], rows[:, 5]
        ids[t, :n], scores[t, :n], bboxes[t, :n], track[t, :n] = p[:, 0], p[:, 1], p[:, 2:6], p[:, 6]
    return (gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track), list(range(0, F + 1, T))


class MOTMetric:
    """Collects the tracked prediction rows of every image in update(); get() matches them against the dataset's labels
    (`get_sample_ids`, `get_label` with the track id in column 5, `frames_per_video`, `classes`) clip by clip and returns the
    overall figures as (names, values); `summary` keeps mot_summary's result (per clip too) of the last get()."""

    def __init__(self, dataset, iou_thresh=0.5, agnostic=False):
        check_dataset(dataset)
        check_iou_thresh(iou_thresh, "MOTMetric")
        self.name = "MOT"
        self.dataset = dataset
        self._iou_thresh = iou_thresh
        self._agnostic = bool(agnostic)
        self._results = {}
        self.summary = None

    def reset(self):
        self._results = {}

    def update(self, pred_bboxes, pred_labels, pred_scores, gt_bboxes=None, gt_ids=None, gt_difficults=None, sid=None, tracks=None,
               *args, **kwargs):
        """pred_bboxes (B,N,4), pred_labels (B,N), pred_scores (B,N), tracks (B,N) (arrays or lists of per-image arrays) of the
        image(s) with sample id `sid`, boxes in source pixels; every row is kept as [label, score, x1, y1, x2, y2, track].  The
        ground-truth arguments are not read: get() takes it from the dataset."""
        if sid is None or isinstance(sid, (list, tuple)):
            raise NotImplementedError("MOTMetric.update: one integer sample id per call is taken, got %r (window sample ids of "
                                      "--mult_out are not built)" % (sid,))
        if tracks is None:
            raise ValueError("MOTMetric.update: tracks is missing - every prediction row carries its track id")
        as_numpy = lambda a: np.concatenate([np.asarray(x, dtype=np.float64) for x in a], axis=0) if isinstance(a, (list, tuple)) \
            else np.asarray(a, dtype=np.float64)
        for box, label, score, trk in zip(*[as_numpy(x) for x in (pred_bboxes, pred_labels, pred_scores, tracks)]):
            box = box.reshape(-1, 4)
            rows = np.concatenate([label.reshape(-1, 1), score.reshape(-1, 1), box, trk.reshape(-1, 1)], axis=1)
            self._results.setdefault(int(sid), []).extend(rows.tolist())

    def _num_class(self):
        return len(self.dataset.classes)

    def _match(self, arrays, clip_start):
        return mot_match_host(*arrays, clip_start=clip_start, num_class=self._num_class(), iou_thresh=self._iou_thresh,
                              agnostic=self._agnostic)

    def get(self):
        arrays, cs = pack_clips(self.dataset, self._results)
        records = self._match(arrays, cs)
        self.summary = mot_summary(records, arrays[2], masked_track(arrays[3], arrays[4], arrays[6], self._num_class()), cs)
        return format_summary(self.summary["all"])


def format_summary(c):
    """(names, values) of one block of figures: the rates as '{:.4f}', the counts as integers"""
    names = list(RATES) + list(COUNTS)
    return names, ["{:.4f}".format(c[k]) for k in RATES] + [str(int(c[k])) for k in COUNTS]
