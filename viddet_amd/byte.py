"""Linking the detections of a clip into tracks with BYTE (Zhang, Sun, Jiang, Yu, Weng, Yuan, Luo, Liu and Wang, "ByteTrack:
Multi-Object Tracking by Associating Every Detection Box", ECCV 2022): two associations a frame - the high-score rows are matched
to the predicted tracks first, what is left of the tracks then looks for its object among the low-score rows, and a low-score row
never starts a track: the definition.

`byte_host` is the normative restatement: NumPy, on viddet_amd/sort.py's filter unchanged (measure, kf_start,
kf_predict, kf_box, kf_update: float32, one operation at a time), mot_metric.assign_host and seq_nms.iou_matrix / row_classes.
The device entry point vd_track_byte (viddet_amd/csrc/vd_track_byte.hip, `ops.track_byte`) equals it bit for bit.

Parameters (DEFAULTS): sigma_l 0.1, rows below it take no part; sigma_d 0.5, the split - a candidate with score >= sigma_d is a
HIGH row, every other candidate a LOW row; sigma_new 0.6, an unmatched high row starts a track iff score >= sigma_new; sigma_iou
0.2, the first association (the paper's match_thresh 0.8 on 1 - IoU); sigma_iou2 0.5, the second; sigma_h 0.5 and t_min 2 as in
track_host; max_age 7, the table's limit (the paper's buffer of 30 does not fit TRACK_MAX_ACTIVE).  All float comparisons are in
float32 and the plain >=; a NaN parameter is refused; no ordering between the thresholds is demanded (sigma_l > sigma_d simply
leaves no low rows).

A row is a candidate as in sort_host (seq_nms.row_classes, a finite score, score >= sigma_l).  Per clip, frames in order
(`byte_step`, a function of (state, frame); the state is sort.new_state()'s):
  1. predict: every active track in creation order, exactly as sort_step does.
  2. first association: rows = the high rows in row order; columns = ALL active tracks in creation order, then one dummy per
     row; a cell is admissible iff the classes are equal and iou(predicted box, row box) >= sigma_iou (track side first,
     iou_matrix's arithmetic); costs 2**20 - int(iou * 2**20), DUMMY_COST and FORBIDDEN; the matching is assign_host.  Skipped
     when there is no high row or no active track.
  3. second association: rows = the low rows in row order; columns = the same K track columns in the same positions, where a
     track is eligible iff step 2 did not match it AND its miss count on entry to this frame is 0; every other track's column is
     FORBIDDEN throughout (kept in place, so assign_host's lowest-column tie rule sees the order a kernel sees that masks
     columns); admissible iff eligible, equal classes and iou >= sigma_iou2; assign_host again.  Skipped when there is no low row
     or no active track.
  4. update: a track matched in either pass is updated with its row - miss 0, length + 1, maximum = max(maximum, score) - and
     the row gets its id and `tbox`; every other track's miss count grows by one and it is closed above max_age; the survivors
     keep their order.
  5. start: the high rows left unmatched whose score >= sigma_new, in row order, behind the survivors; one id counter per clip,
     advanced only by started tracks.  An unmatched low row, and an unmatched high row below sigma_new, gets track = -1.
  6. decide at the clip's end as sort_host does (sigma_h, t_min).  Ids are not renumbered.
At most N * (max_age + 1) tracks are active, since a frame starts at most N.

Stated departures from the ByteTrack code: the filter is Bewley's (SORT's), not the xyah filter with size-proportional noise;
there is no score fusion into the cost; there is no "unconfirmed" stage, because t_min decides at the clip's end; only admissible
pairs enter the assignment; tracks are per class; a lost track's velocity is not zeroed beyond kf_predict's own `s + ds <= 0` rule.

`byte_online_host` is steps 1 to 5 on a stream that never says where it ends, a state carried from call to call (DESIGN.md 39;
vd_track_kf_push, `ops.KalmanTrackState`, equals it bit for bit); track.finalize_tracks is step 6 on its rows, once a clip has
ended.

This module imports NumPy only.
"""
import numpy as np

from .mot_metric import FORBIDDEN, assign_host
from .seq_nms import _clips, row_classes
from .sort import _KEYS, association_cost, kf_box, kf_cat, kf_predict, kf_start, kf_take, kf_update, measure, new_state, online_rows
from .track import check_params

_F = np.float32
DEFAULTS = dict(sigma_l=0.1, sigma_d=0.5, sigma_new=0.6, sigma_iou=0.2, sigma_iou2=0.5, sigma_h=0.5, t_min=2, max_age=7)
EXTRA = ("sigma_d", "sigma_new", "sigma_iou2")    # what BYTE takes beyond track.check_params' five


def check_byte_params(sigma_l=0.1, sigma_d=0.5, sigma_new=0.6, sigma_iou=0.2, sigma_iou2=0.5, sigma_h=0.5, t_min=2, max_age=7,
                      who="byte"):
    """The eight parameters as (sigma_l, sigma_d, sigma_new, sigma_iou, sigma_iou2, sigma_h: float32; t_min, max_age: int); a
    ValueError names the argument that is not usable"""
    sl, sh, si, t_min, max_age = check_params(sigma_l, sigma_h, sigma_iou, t_min, max_age, who)
    extra = []
    for name, v in zip(EXTRA, (sigma_d, sigma_new, sigma_iou2)):
        try:
            f = _F(v)
        except (TypeError, ValueError):
            raise ValueError("%s: %s must be a number, got %r" % (who, name, v))
        if f != f:
            raise ValueError("%s: %s must not be NaN" % (who, name))
        extra.append(f)
    return sl, extra[0], extra[1], si, extra[2], sh, t_min, max_age


def byte_step(state, cls, sc, boxes, sigma_d=0.5, sigma_new=0.6, sigma_iou=0.2, sigma_iou2=0.5, max_age=7):
    """One frame: state (sort.new_state() or an earlier call's; not changed), cls (N,) the rows' classes with -1 for a row that
    is no candidate, sc (N,) and boxes (N,4) float32 -> (the new state, track (N,) the row's id or -1, tlen (N,) the rows of its
    track so far, tscore (N,) its maximum so far, tbox (N,4) its posterior box, closed: the tracks this frame closed, first and
    second: the pairs the two associations made)."""
    sd, sn, si, si2 = _F(sigma_d), _F(sigma_new), _F(sigma_iou), _F(sigma_iou2)
    cls, sc, boxes = np.asarray(cls), np.asarray(sc, dtype=_F), np.asarray(boxes, dtype=_F)
    N = len(cls)
    track = np.full(N, -1, dtype=np.int64)
    tlen = np.zeros(N, dtype=np.int64)
    tscore = np.full(N, -1, dtype=_F)
    tbox = np.full((N, 4), -1, dtype=_F)
    K = len(state["id"])
    kf = kf_predict(state["kf"])                                                       # 1
    with np.errstate(invalid="ignore"):
        is_high = sc >= sd
    high = np.nonzero((cls >= 0) & is_high)[0]
    low = np.nonzero((cls >= 0) & ~is_high)[0]
    pbox = kf_box(kf)
    row_of = np.full(K, -1, dtype=np.int64)                                            # the row a track is matched to
    col1 = np.full(len(high), -1, dtype=np.int64)
    if len(high) and K:                                                                # 2
        col1 = assign_host(association_cost(pbox, state["cls"], boxes[high], cls[high], si))
        col1 = np.where(col1 < K, col1, -1)
        row_of[col1[col1 >= 0]] = high[col1 >= 0]
    first = int((col1 >= 0).sum())
    second = 0
    if len(low) and K:                                                                 # 3
        eligible = (row_of < 0) & (state["miss"] == 0)
        cost = association_cost(pbox, state["cls"], boxes[low], cls[low], si2)
        cost[:, :K] = np.where(eligible[None, :], cost[:, :K], FORBIDDEN)
        col2 = assign_host(cost)
        col2 = np.where(col2 < K, col2, -1)
        row_of[col2[col2 >= 0]] = low[col2 >= 0]
        second = int((col2 >= 0).sum())
    hit = row_of >= 0                                                                  # 4
    t_id, t_len, t_max = state["id"].copy(), state["len"].copy(), state["max"].copy()
    if hit.any():
        k = np.nonzero(hit)[0]
        j = row_of[k]
        upd = kf_update(kf_take(kf, k), measure(boxes[j]))
        for key in _KEYS:
            kf[key][k] = upd[key]
        t_len[k] += 1
        t_max[k] = np.where(sc[j] > t_max[k], sc[j], t_max[k])
        track[j], tlen[j], tscore[j], tbox[j] = t_id[k], t_len[k], t_max[k], kf_box(upd)
    miss = np.where(hit, 0, state["miss"] + 1)
    live = miss <= max_age
    left = high[col1 < 0]                                                              # 5
    with np.errstate(invalid="ignore"):
        fresh = left[sc[left] >= sn]
    born = kf_start(measure(boxes[fresh]))
    ids = state["next_id"] + np.arange(len(fresh), dtype=np.int64)
    track[fresh], tlen[fresh], tscore[fresh], tbox[fresh] = ids, 1, sc[fresh], kf_box(born)
    out = dict(next_id=state["next_id"] + len(fresh), kf=kf_cat(kf_take(kf, live), born),
               cls=np.concatenate([state["cls"][live], cls[fresh].astype(np.int64)]), id=np.concatenate([t_id[live], ids]),
               miss=np.concatenate([miss[live], np.zeros(len(fresh), np.int64)]),
               len=np.concatenate([t_len[live], np.ones(len(fresh), np.int64)]), max=np.concatenate([t_max[live], sc[fresh]]))
    return out, track, tlen, tscore, tbox, int(K - live.sum()), first, second


def byte_host(ids, scores, bboxes, clip_start=None, num_class=None, sigma_l=0.1, sigma_d=0.5, sigma_new=0.6, sigma_iou=0.2,
              sigma_iou2=0.5, sigma_h=0.5, t_min=2, max_age=7, stats=None):
    """ids (F,N[,1]), scores (F,N[,1]), bboxes (F,N,4) -> sort_host's four: (track, tlen, tscore, tbox).  `stats`, a dict,
    receives per frame 'active' and 'closed', 'first' and 'second' (the pairs of each association), and 'tracks' (the kept
    tracks of every clip)."""
    sl, sd, sn, si, si2, sh, t_min, max_age = check_byte_params(sigma_l, sigma_d, sigma_new, sigma_iou, sigma_iou2, sigma_h, t_min,
                                                                max_age, "byte_host")
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
    n_first = np.zeros(F, dtype=np.int64)
    n_second = np.zeros(F, dtype=np.int64)
    kept_per_clip = []
    for t0, t1 in _clips(clip_start, F):
        state = new_state()
        local = np.full((t1 - t0, N), -1, dtype=np.int64)         # the row's track, numbered inside the clip
        length = np.zeros((t1 - t0) * N, dtype=np.int32)          # per track of the clip: a clip makes at most one per row
        best = np.full((t1 - t0) * N, -1, dtype=_F)
        for t in range(t0, t1):
            state, tr, ln, mx, tbox[t], n_closed[t], n_first[t], n_second[t] = byte_step(state, cls[t], sc[t], bboxes[t], sd, sn,
                                                                                         si, si2, max_age)
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
        stats["first"], stats["second"] = n_first, n_second
    return track, tlen, tscore, tbox


def byte_online_host(state, ids, scores, bboxes, num_class=None, sigma_l=0.1, sigma_d=0.5, sigma_new=0.6, sigma_iou=0.2,
                     sigma_iou2=0.5, max_age=7, stats=None):
    """BYTE on a stream that never says where it ends (vd_track_kf_push, `ops.KalmanTrackState`, equals it bit
    for bit): byte_host's frame loop on byte_step, unchanged, on the given frames, starting from `state` (None: a fresh stream;
    else an earlier call's, which is not changed) -> (the new state, track, tlen, tscore, tbox), per row as
    sort.sort_online_host gives them: the id counted over the whole stream, the length and the maximum so far, the posterior
    box.  Nothing is decided here, so sigma_h and t_min are no arguments: track.finalize_tracks(..., tbox=) makes byte_host's
    arrays of a finished clip's rows.  Pushing a clip in pieces gives what one call on all of it gives; where sigma_d =
    sigma_new = sigma_l it is sort_online_host.  `stats`, a dict, receives per frame 'active', 'closed', 'first' and 'second'."""
    sl, sd, sn, si, si2, _, _, max_age = check_byte_params(sigma_l, sigma_d, sigma_new, sigma_iou, sigma_iou2, 0.5, 1, max_age,
                                                           "byte_online_host")
    sc, cls, bboxes = online_rows(ids, scores, bboxes, num_class, sl)
    F, N = sc.shape
    track = np.full((F, N), -1, dtype=np.int32)
    tlen = np.zeros((F, N), dtype=np.int32)
    tscore = np.full((F, N), -1, dtype=_F)
    tbox = np.full((F, N, 4), -1, dtype=_F)
    counts = np.zeros((4, F), dtype=np.int64)                     # active, closed, first, second
    state = new_state() if state is None else state
    for t in range(F):
        state, track[t], tlen[t], tscore[t], tbox[t], counts[1, t], counts[2, t], counts[3, t] = byte_step(
            state, cls[t], sc[t], bboxes[t], sd, sn, si, si2, max_age)
        counts[0, t] = len(state["id"])
    if stats is not None:
        stats["active"], stats["closed"], stats["first"], stats["second"] = counts
    return state, track, tlen, tscore, tbox
