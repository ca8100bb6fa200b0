"""Linking the detections of a clip into tracks with SORT (Bewley, Ge, Ott, Ramos and Upcroft, "Simple Online and Realtime
Tracking", ICIP 2016): every active track is predicted by a constant-velocity Kalman filter, the predictions are matched to the
frame's detections by a minimum-cost assignment: the definition.

`sort_host` is the normative restatement: NumPy, every filter operation ONE float32 operation in a fixed order, no
product and sum contracted, `/` and `sqrt` correctly rounded.  The device entry point vd_track_sort
(viddet_amd/csrc/vd_track_sort.hip, `ops.track_sort`) equals it bit for bit.

The filter.  Bewley's state is u, v (centre), s (area), r (aspect w / h, no velocity), du, dv, ds, with R = diag(1, 1, 10, 10),
P0 = diag(10, 10, 10, 10, 1e4, 1e4, 1e4) and Q = diag(1, 1, 1, 1, .01, .01, 1e-4).  With them the 7 x 7 covariance stays block
diagonal for ever, so the definition is the decoupled form: three two-state filters (x, xd, p00, p01, p11) for u, v and s and a
scalar one (r, p), 17 floats a track:
  measurement of a box   w = x2 - x1, h = y2 - y1, z = (x1 + w/2, y1 + h/2, w*h, w/h)
  start                  x = z, xd = 0, (p00, p01, p11) = (10, 0, 1e4); p = 10 for r
  predict                first `if s + ds <= 0: ds = 0` (a NaN compares false); per pair, all on the old values: x = x + xd,
                         p00 = ((p00 + p01) + (p01 + p11)) + q0, p01 = p01 + p11, p11 = p11 + q1; for r: p = p + 1
  box of a state         w = sqrt(s*r), h = s / w, box = (u - w/2, v - h/2, u + w/2, v + h/2)
  update with z          per pair: S = p00 + R, k0 = p00 / S, k1 = p01 / S, y = z - x, x = x + k0*y, xd = xd + k1*y,
                         p11 = p11 - k1*p01, p01 = p01 - k0*p01, p00 = p00 - k0*p00;
                         for r: S = p + 10, k = p / S, r = r + k*(z - r), p = p - k*p
Degenerate boxes (zero height, infinite or NaN coordinates, a negative s*r) get no special case: the NaNs travel, a pair whose
IoU is NaN is never admissible, and such a track ages out.

A row is a candidate as in track.track_host (seq_nms.row_classes and score >= sigma_l).  Per clip, frames in order
(`sort_step`, a function of (state, frame)):
  1. predict: every active track, in order of creation.
  2. associate: rows = the frame's candidates in row order; columns = the active tracks in creation order, then one dummy per
     row.  Cell (row i, track k) is admissible iff the classes are equal and iou(predicted box of k, box of i) >= sigma_iou
     (seq_nms.iou_matrix's arithmetic, track side first; the plain >=, so a NaN is not admissible) and costs
     2**20 - int(iou * 2**20); a row's own dummy costs 2**27; everything else is FORBIDDEN.  The column of every row is
     mot_metric.assign_host(cost): the most pairs, then the largest quantised IoU sum, with assign_host's tie rules.  Entered
     only when the frame has a candidate and a track is active.
  3. update: a matched track is updated with its row, its miss count 0, its length one more, its maximum max(maximum, score);
     the row gets the track's id and `tbox`, the box of the posterior state.  Every other track's miss count grows by one and
     the track is closed once it exceeds max_age; the survivors keep their order.
  4. start: every candidate that took its dummy - every candidate where step 2 was skipped - starts a track, in row order; its
     `tbox` is the box of its start state.  A track's id is its creation number within the clip, one counter for all classes.
  5. decide, at the clip's end: a track is kept iff its maximum score >= sigma_h and it holds at least t_min rows.  Ids are not
     renumbered.
At most N * (max_age + 1) tracks are active at once, as in track_host.

Stated departures from Bewley's code: it solves the assignment over ALL pairs and discards the matches under the threshold
afterwards, here only admissible pairs enter; tracks are per class; there is no min_hits gate on output - t_min and sigma_h
decide at the clip's end, as track_host does.  The defaults sigma_iou 0.3 and max_age 1 are the paper's.

`sort_online_host` is steps 1 to 4 on a stream that never says where it ends, a state carried from call to call (DESIGN.md 39;
vd_track_kf_push, `ops.KalmanTrackState`, equals it bit for bit); track.finalize_tracks is step 5 on its rows, once a clip has
ended.

This module imports NumPy only.
"""
import numpy as np

from .mot_metric import DUMMY_COST, FORBIDDEN, Q_ONE, assign_host
from .seq_nms import _clips, iou_matrix, row_classes
from .track import check_params

_F = np.float32
DEFAULTS = dict(sigma_l=0.0, sigma_h=0.5, sigma_iou=0.3, t_min=2, max_age=1)
R_PAIR = (1.0, 1.0, 10.0)                          # the measurement noise of u, v, s
R_ASPECT = 10.0                                    # and of r
P0 = (10.0, 0.0, 1e4)                              # p00, p01, p11 of a new track; r starts at p = 10
Q0 = (1.0, 1.0, 1.0)                               # the process noise of u, v, s ...
Q1 = (0.01, 0.01, 1e-4)                            # ... of du, dv, ds ...
Q_ASPECT = 1.0                                     # ... and of r
STATE_FLOATS = 17
_KEYS = ("x", "xd", "p00", "p01", "p11", "r", "p")


# ------------------------------------------------------------------ the filter, on K tracks at once; the arrays' dtype is the
# arithmetic's (float32 is the definition; float64 only compares the decoupled form with the 7 x 7 one)
def measure(boxes):
    """(K,4) corner boxes -> z (K,4): u, v, s, r"""
    b = np.asarray(boxes)
    two = b.dtype.type(2)
    with np.errstate(all="ignore"):
        w = b[:, 2] - b[:, 0]
        h = b[:, 3] - b[:, 1]
        return np.stack([b[:, 0] + w / two, b[:, 1] + h / two, w * h, w / h], axis=1)


def kf_start(z):
    """z (K,4) -> the filter of K new tracks: x, xd, p00, p01, p11 (K,3) for u, v, s and r, p (K,)"""
    z = np.asarray(z)
    dt, K = z.dtype.type, z.shape[0]
    return dict(x=z[:, :3].copy(), xd=np.zeros((K, 3), dt), p00=np.full((K, 3), dt(P0[0])), p01=np.full((K, 3), dt(P0[1])),
                p11=np.full((K, 3), dt(P0[2])), r=z[:, 3].copy(), p=np.full(K, dt(P0[0])))


def kf_empty(dtype=_F):
    return kf_start(np.zeros((0, 4), dtype))


def kf_take(kf, idx):
    return {k: kf[k][idx] for k in _KEYS}


def kf_cat(a, b):
    return {k: np.concatenate([a[k], b[k]]) for k in _KEYS}


def kf_predict(kf):
    dt = kf["x"].dtype.type
    q0, q1 = np.array(Q0, dtype=dt), np.array(Q1, dtype=dt)
    with np.errstate(all="ignore"):
        xd = kf["xd"].copy()
        xd[:, 2] = np.where(kf["x"][:, 2] + xd[:, 2] <= 0, dt(0), xd[:, 2])
        p00, p01, p11 = kf["p00"], kf["p01"], kf["p11"]
        return dict(x=kf["x"] + xd, xd=xd, p00=((p00 + p01) + (p01 + p11)) + q0, p01=p01 + p11, p11=p11 + q1, r=kf["r"].copy(),
                    p=kf["p"] + dt(Q_ASPECT))


def kf_box(kf):
    """the corner boxes (K,4) of the states"""
    x, two = kf["x"], kf["x"].dtype.type(2)
    with np.errstate(all="ignore"):
        w = np.sqrt(x[:, 2] * kf["r"])
        h = x[:, 2] / w
        return np.stack([x[:, 0] - w / two, x[:, 1] - h / two, x[:, 0] + w / two, x[:, 1] + h / two], axis=1)


def kf_update(kf, z):
    dt = kf["x"].dtype.type
    z = np.asarray(z, dtype=dt)
    with np.errstate(all="ignore"):
        p00, p01, p11 = kf["p00"], kf["p01"], kf["p11"]
        S = p00 + np.array(R_PAIR, dtype=dt)
        k0, k1 = p00 / S, p01 / S
        y = z[:, :3] - kf["x"]
        Sr = kf["p"] + dt(R_ASPECT)
        k = kf["p"] / Sr
        return dict(x=kf["x"] + k0 * y, xd=kf["xd"] + k1 * y, p11=p11 - k1 * p01, p01=p01 - k0 * p01, p00=p00 - k0 * p00,
                    r=kf["r"] + k * (z[:, 3] - kf["r"]), p=kf["p"] - k * kf["p"])


# ------------------------------------------------------------------ the frame step
def new_state():
    """no active track: 'next_id' and, per active track in order of creation, the filter 'kf' and 'cls', 'id', 'miss', 'len', 'max'"""
    z = np.zeros(0, np.int64)
    return dict(next_id=0, kf=kf_empty(), cls=z, id=z.copy(), miss=z.copy(), len=z.copy(), max=np.zeros(0, _F))


def association_cost(pred_boxes, track_cls, row_boxes, row_cls, sigma_iou):
    """Step 2's cost matrix (R, K + R) int64: the R candidate rows against K predicted tracks, then a dummy per row"""
    R, K = len(row_cls), len(track_cls)
    cost = np.full((R, K + R), FORBIDDEN, dtype=np.int64)
    iou = iou_matrix(pred_boxes, row_boxes).T                                          # (R, K), track side first
    with np.errstate(invalid="ignore"):
        adm = (np.asarray(row_cls)[:, None] == np.asarray(track_cls)[None, :]) & (iou >= _F(sigma_iou))
    q = (np.where(adm, iou, _F(0)) * _F(Q_ONE)).astype(np.int64)                        # exact in float32
    cost[:, :K] = np.where(adm, Q_ONE - q, FORBIDDEN)
    cost[np.arange(R), K + np.arange(R)] = DUMMY_COST
    return cost


def sort_step(state, cls, sc, boxes, sigma_iou=0.3, max_age=1):
    """One frame: state (new_state() or an earlier call's; not changed), cls (N,) the rows' classes with -1 for a row that is no
    candidate, sc (N,) and boxes (N,4) float32 -> (the new state, track (N,) the row's id or -1, tlen (N,) the rows of its track
    so far, tscore (N,) its maximum so far, tbox (N,4) its posterior box, closed: the tracks this frame closed)."""
    si = _F(sigma_iou)
    cls, sc, boxes = np.asarray(cls), np.asarray(sc, dtype=_F), np.asarray(boxes, dtype=_F)
    N = len(cls)
    track = np.full(N, -1, dtype=np.int64)
    tlen = np.zeros(N, dtype=np.int64)
    tscore = np.full(N, -1, dtype=_F)
    tbox = np.full((N, 4), -1, dtype=_F)
    K = len(state["id"])
    kf = kf_predict(state["kf"])                                                       # 1
    rows = np.nonzero(cls >= 0)[0]
    col = np.full(len(rows), -1, dtype=np.int64)
    if len(rows) and K:                                                                # 2
        col = assign_host(association_cost(kf_box(kf), state["cls"], boxes[rows], cls[rows], si))
        col = np.where(col < K, col, -1)
    hit = np.zeros(K, dtype=bool)                                                      # 3
    t_id, t_len, t_max = state["id"].copy(), state["len"].copy(), state["max"].copy()
    m = col >= 0
    if m.any():
        k, j = col[m], rows[m]
        hit[k] = True
        upd = kf_update(kf_take(kf, k), measure(boxes[j]))
        for key in _KEYS:
            kf[key][k] = upd[key]
        t_len[k] += 1
        t_max[k] = np.where(sc[j] > t_max[k], sc[j], t_max[k])
        track[j], tlen[j], tscore[j], tbox[j] = t_id[k], t_len[k], t_max[k], kf_box(upd)
    miss = np.where(hit, 0, state["miss"] + 1)
    live = miss <= max_age
    fresh = rows[~m]                                                                   # 4
    born = kf_start(measure(boxes[fresh]))
    ids = state["next_id"] + np.arange(len(fresh), dtype=np.int64)
    track[fresh], tlen[fresh], tscore[fresh], tbox[fresh] = ids, 1, sc[fresh], kf_box(born)
    out = dict(next_id=state["next_id"] + len(fresh), kf=kf_cat(kf_take(kf, live), born),
               cls=np.concatenate([state["cls"][live], cls[fresh].astype(np.int64)]), id=np.concatenate([t_id[live], ids]),
               miss=np.concatenate([miss[live], np.zeros(len(fresh), np.int64)]),
               len=np.concatenate([t_len[live], np.ones(len(fresh), np.int64)]), max=np.concatenate([t_max[live], sc[fresh]]))
    return out, track, tlen, tscore, tbox, int(K - live.sum())


def sort_host(ids, scores, bboxes, clip_start=None, num_class=None, sigma_l=0.0, sigma_h=0.5, sigma_iou=0.3, t_min=2, max_age=1,
              stats=None):
    """ids (F,N[,1]), scores (F,N[,1]), bboxes (F,N,4) -> (track, tlen, tscore, tbox): the first three are track_host's - the
    row's track id (F,N) int32, -1 for a row that is no candidate or whose track is dropped; the rows of its track, 0 beside -1;
    the track's maximum score, -1 beside -1 - and tbox (F,N,4) float32 is the filtered (posterior) box of the row's track after
    this row's update, -1 where track is -1.  `stats`, a dict, receives per frame 'active' and 'closed' and 'tracks' (the kept
    tracks of every clip), as track_host's."""
    sl, sh, si, t_min, max_age = check_params(sigma_l, sigma_h, sigma_iou, t_min, max_age, "sort_host")
    ids = np.asarray(ids, dtype=_F)
    scores = np.asarray(scores, dtype=_F)
    bboxes = np.asarray(bboxes, dtype=_F)
    if bboxes.ndim != 3 or bboxes.shape[2] != 4 or ids.size != bboxes.shape[0] * bboxes.shape[1] or scores.size != ids.size:
        raise ValueError("expected ids (F,N,1), scores (F,N,1), bboxes (F,N,4), got %r %r %r" % (ids.shape, scores.shape, bboxes.shape))
    F, N = bboxes.shape[0], bboxes.shape[1]
    sc = scores.reshape(F, N)
    cls = row_classes(ids.reshape(F, N), sc, num_class)
    with np.errstate(invalid="ignore"):
        cls = np.where(sc >= sl, cls, -1)
    track = np.full((F, N), -1, dtype=np.int32)
    tlen = np.zeros((F, N), dtype=np.int32)
    tscore = np.full((F, N), -1, dtype=_F)
    tbox = np.full((F, N, 4), -1, dtype=_F)
    n_active = np.zeros(F, dtype=np.int64)
    n_closed = np.zeros(F, dtype=np.int64)
    kept_per_clip = []
    for t0, t1 in _clips(clip_start, F):
        state = new_state()
        local = np.full((t1 - t0, N), -1, dtype=np.int64)         # the row's track, numbered inside the clip
        length = np.zeros((t1 - t0) * N, dtype=np.int32)          # per track of the clip: a clip makes at most one per row
        best = np.full((t1 - t0) * N, -1, dtype=_F)
        for t in range(t0, t1):
            state, tr, ln, mx, tbox[t], n_closed[t] = sort_step(state, cls[t], sc[t], bboxes[t], si, max_age)
            on = tr >= 0
            local[t - t0] = tr
            length[tr[on]], best[tr[on]] = ln[on], mx[on]         # both only grow: the track's last row carries them
            n_active[t] = len(state["id"])
        made = state["next_id"]
        kept = (best[:made] >= sh) & (length[:made] >= t_min)
        kept_per_clip.append(int(kept.sum()))
        if made:
            on = (local >= 0) & kept[np.maximum(local, 0)]
            track[t0:t1] = np.where(on, local, -1)
            tlen[t0:t1] = np.where(on, length[np.maximum(local, 0)], 0)
            tscore[t0:t1] = np.where(on, best[np.maximum(local, 0)], _F(-1))
            tbox[t0:t1] = np.where(on[..., None], tbox[t0:t1], _F(-1))
    if stats is not None:
        stats["active"], stats["closed"], stats["tracks"] = n_active, n_closed, kept_per_clip
    return track, tlen, tscore, tbox


def online_rows(ids, scores, bboxes, num_class, sigma_l):
    """The frames of one push as (sc (F,N), cls (F,N) with -1 for a row that is no candidate, bboxes (F,N,4)), float32: what
    sort_host and byte_host make of a clip"""
    ids = np.asarray(ids, dtype=_F)
    scores = np.asarray(scores, dtype=_F)
    bboxes = np.asarray(bboxes, dtype=_F)
    if bboxes.ndim != 3 or bboxes.shape[2] != 4 or ids.size != bboxes.shape[0] * bboxes.shape[1] or scores.size != ids.size:
        raise ValueError("expected ids (F,N,1), scores (F,N,1), bboxes (F,N,4), got %r %r %r" % (ids.shape, scores.shape, bboxes.shape))
    F, N = bboxes.shape[0], bboxes.shape[1]
    sc = scores.reshape(F, N)
    cls = row_classes(ids.reshape(F, N), sc, num_class)
    with np.errstate(invalid="ignore"):
        cls = np.where(sc >= sigma_l, cls, -1)
    return sc, cls, bboxes


def sort_online_host(state, ids, scores, bboxes, num_class=None, sigma_l=0.0, sigma_iou=0.3, max_age=1, stats=None):
    """SORT on a stream that never says where it ends (vd_track_kf_push, `ops.KalmanTrackState`, equals it bit
    for bit): sort_host's frame loop on sort_step, unchanged, on the given frames, starting from `state` (None: a fresh stream;
    else an earlier call's, which is not changed) -> (the new state, track, tlen, tscore, tbox).  Per row, (F,N) and (F,N,4):
    `track` int32, the id of the row's track - a creation number counted over the whole stream - or -1 for a row that is no
    candidate; `tlen` int32, the rows of its track so far, this one included (0 beside -1); `tscore` float32, the track's
    maximum score so far (-1 beside -1); `tbox` float32, the track's posterior box after this row's update (-1 beside -1).
    Nothing is decided here, so sigma_h and t_min are no arguments: track.finalize_tracks(..., tbox=) makes sort_host's arrays
    of a finished clip's rows.  Pushing a clip in pieces gives what one call on all of it gives.  `stats`, a dict, receives per
    frame 'active' and 'closed'."""
    sl, _, si, _, max_age = check_params(sigma_l, 0.5, sigma_iou, 1, max_age, "sort_online_host")
    sc, cls, bboxes = online_rows(ids, scores, bboxes, num_class, sl)
    F, N = sc.shape
    track = np.full((F, N), -1, dtype=np.int32)
    tlen = np.zeros((F, N), dtype=np.int32)
    tscore = np.full((F, N), -1, dtype=_F)
    tbox = np.full((F, N, 4), -1, dtype=_F)
    n_active = np.zeros(F, dtype=np.int64)
    n_closed = np.zeros(F, dtype=np.int64)
    state = new_state() if state is None else state
    for t in range(F):
        state, track[t], tlen[t], tscore[t], tbox[t], n_closed[t] = sort_step(state, cls[t], sc[t], bboxes[t], si, max_age)
        n_active[t] = len(state["id"])
    if stats is not None:
        stats["active"], stats["closed"] = n_active, n_closed
    return state, track, tlen, tscore, tbox
