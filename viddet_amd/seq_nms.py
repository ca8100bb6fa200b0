"""Sequence NMS for the detections of video clips (Han et al., "Seq-NMS for Video Object Detection", 2016): the definition.

`seq_nms_host` is the normative restatement: NumPy, every operation on a score or a coordinate in float32, in a
fixed order.  The device entry point vd_seq_nms (viddet_amd/csrc/vd_seq_nms.hip, `ops.seq_nms`) equals it bit for bit.

Per clip and class, all candidate rows start alive, then rounds repeat while a row is alive:
  1. link and score: frames from last to first, alive rows in row order: b = 0, p = -1; over the alive rows j of the next
     frame in row order, where iou(i, j) > link_thresh and best[t+1][j] > b take b, p from j; best[t][i] = score + b, next = p
  2. the start is the alive row with the largest best, ties to the lowest frame, then the lowest row; the sequence follows next
  3. rescore: 'avg' - the fp32 sum of the rows' scores in frame order / their number; 'max' - their maximum; the rows are final
  4. suppress: in every frame of the sequence, the alive rows of the class with iou > nms_thresh to its row are dead
A row is a candidate iff id >= 0 and its score is finite (and its class is below `num_class` where that is given: the device
walks classes [0, num_class)); the class is the id truncated like astype(int).  iou = inter / ((a1 + a2) - inter) with
iw = min(x2) - max(x1), ih likewise, 0 unless both > 0; no +1; both comparisons are strict.
"""
import numpy as np

_F = np.float32
RESCORE = {"avg": 0, "max": 1}
MAX_ROWS = 128          # rows per frame vd_seq_nms takes (a 128-bit mask per row)


def parse_option(seq_nms, post_nms, who):
    """The `seq_nms=` option of `who` (detect_video): None / False -> None; True or a dict of link_thresh / nms_thresh / rescore
    and `clip` -> (the dict as given, `clip` or None).  A ValueError names what is not usable."""
    if seq_nms is None or seq_nms is False:
        return None
    kw = {} if seq_nms is True else dict(seq_nms)
    clip = kw.pop("clip", None)
    unknown = sorted(set(kw) - {"link_thresh", "nms_thresh", "rescore"})
    if unknown:
        raise ValueError("%s: seq_nms takes link_thresh, nms_thresh and rescore, got %s" % (who, ", ".join(unknown)))
    if post_nms > MAX_ROWS:
        raise ValueError("%s with seq_nms: post_nms=%d rows per frame, Seq-NMS takes at most %d" % (who, post_nms, MAX_ROWS))
    return kw, clip


def row_classes(ids, scores, num_class=None):
    """(F,N) int64: the class of every candidate row, -1 for a row that is no candidate"""
    ids = np.asarray(ids, dtype=_F).reshape(ids.shape[0], ids.shape[1])
    scores = np.asarray(scores, dtype=_F).reshape(ids.shape)
    with np.errstate(invalid="ignore"):
        ok = (ids >= 0) & np.isfinite(scores)
        big = ids >= _F(2147483648.0)
        cls = np.where(ok & ~big, np.where(ok & ~big, ids, 0).astype(np.int64), np.int64(0x7fffffff))
    if num_class is not None:
        ok &= cls < int(num_class)
    return np.where(ok, cls, -1)


def iou_matrix(a, b):
    """(Na,4) x (Nb,4) float32 corner boxes -> (Na,Nb) float32, operation for operation what vd_seq_nms computes"""
    a, b = np.asarray(a, dtype=_F), np.asarray(b, dtype=_F)
    with np.errstate(all="ignore"):
        iw = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
        ih = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
        inter = iw * ih
        aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        iou = inter / ((aa[:, None] + ab[None, :]) - inter)
        return np.where((iw > 0) & (ih > 0), iou, _F(0)).astype(_F)


def _clips(clip_start, F):
    if clip_start is None:
        return [(0, F)]
    cs = [int(v) for v in np.asarray(clip_start).reshape(-1)]
    if len(cs) < 2 or cs[0] != 0 or cs[-1] != F or any(b < a for a, b in zip(cs, cs[1:])):
        raise ValueError("clip_start must be V+1 ascending offsets from 0 to F=%d, got %r" % (F, cs))
    return list(zip(cs[:-1], cs[1:]))


def seq_nms_host(ids, scores, bboxes, clip_start=None, link_thresh=0.5, nms_thresh=0.3, rescore="avg", num_class=None,
                 stats=None):
    """ids (F,N,1), scores (F,N,1), bboxes (F,N,4) -> (ids, scores, bboxes, perm): per frame the final rows by new score
    descending (stably by old row), then -1 rows; perm (F,N) int32 is the old row of every output row, or -1.  `stats`, a dict,
    receives 'rounds' (the rounds of every (clip, class), summed)."""
    if rescore not in RESCORE:
        raise ValueError("rescore must be 'avg' or 'max', got %r" % (rescore,))
    ids = np.asarray(ids, dtype=_F)
    scores = np.asarray(scores, dtype=_F)
    bboxes = np.asarray(bboxes, dtype=_F)
    F, N = bboxes.shape[0], bboxes.shape[1]
    if bboxes.shape != (F, N, 4) or ids.size != F * N or scores.size != F * N:
        raise ValueError("expected ids (F,N,1), scores (F,N,1), bboxes (F,N,4), got %r %r %r" % (ids.shape, scores.shape, bboxes.shape))
    lt, nt = _F(link_thresh), _F(nms_thresh)
    sc = scores.reshape(F, N)
    cls = row_classes(ids.reshape(F, N), sc, num_class)
    new = np.zeros((F, N), dtype=_F)
    final = np.zeros((F, N), dtype=bool)
    rounds = 0
    for t0, t1 in _clips(clip_start, F):
        if t1 == t0:
            continue
        same = [cls[t][:, None] == cls[t][None, :] for t in range(t0, t1)]
        nms = [(iou_matrix(bboxes[t], bboxes[t]) > nt) & same[t - t0] & ~np.eye(N, dtype=bool) for t in range(t0, t1)]
        link = [(iou_matrix(bboxes[t], bboxes[t + 1]) > lt) & (cls[t][:, None] == cls[t + 1][None, :]) for t in range(t0, t1 - 1)]
        for c in np.unique(cls[t0:t1][cls[t0:t1] >= 0]):
            alive = cls[t0:t1] == c                                      # (T,N)
            T = t1 - t0
            best = np.zeros((T, N), dtype=_F)
            nxt = np.full((T, N), -1, dtype=np.int64)
            while alive.any():
                rounds += 1
                for t in range(T - 1, -1, -1):
                    b = np.zeros(N, dtype=_F)
                    p = np.full(N, -1, dtype=np.int64)
                    if t + 1 < T and alive[t + 1].any():
                        # the first j, in row order, whose best is the largest above 0 among the linked alive rows
                        v = np.where(link[t] & alive[t + 1][None, :] & (best[t + 1] > 0)[None, :], best[t + 1][None, :], _F(0))
                        j = np.argmax(v, axis=1)
                        b = v[np.arange(N), j].astype(_F)
                        p = np.where(b > 0, j, -1)
                    with np.errstate(over="ignore"):
                        best[t] = sc[t0 + t] + b
                    nxt[t] = p
                # the start: largest best, lowest frame, lowest row (argmax of the row-major flattening: the first maximum)
                flat = np.where(alive, best, -np.inf).reshape(-1)
                k = int(np.argmax(flat))
                t, i = divmod(k, N)
                seq = []
                while i >= 0:
                    seq.append((t, i))
                    t, i = t + 1, int(nxt[t, i])
                if rescore == "avg":
                    s = _F(0)
                    with np.errstate(over="ignore"):
                        for t, i in seq:
                            s = _F(s + sc[t0 + t, i])
                        s = _F(s / _F(len(seq)))
                else:
                    s = sc[t0 + seq[0][0], seq[0][1]]
                    for t, i in seq[1:]:
                        if sc[t0 + t, i] > s:
                            s = sc[t0 + t, i]
                for t, i in seq:
                    new[t0 + t, i] = s
                    final[t0 + t, i] = True
                    alive[t, i] = False
                    alive[t] &= ~nms[t][i]
    if stats is not None:
        stats["rounds"] = rounds
    out_ids = np.full((F, N, 1), -1, dtype=_F)
    out_scores = np.full((F, N, 1), -1, dtype=_F)
    out_boxes = np.full((F, N, 4), -1, dtype=_F)
    perm = np.full((F, N), -1, dtype=np.int32)
    for t in range(F):
        rows = np.nonzero(final[t])[0]
        order = rows[np.argsort(-new[t, rows], kind="stable")]
        n = len(order)
        perm[t, :n] = order
        out_ids[t, :n, 0] = ids.reshape(F, N)[t, order]
        out_scores[t, :n, 0] = new[t, order]
        out_boxes[t, :n] = bboxes[t, order]
    return out_ids, out_scores, out_boxes, perm
