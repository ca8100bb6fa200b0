"""Linking the detections of a clip into tracks: the IOU tracker of Bochinski, Eiselein and Sikora, "High-Speed
Tracking-by-Detection Without Using Image Information" (AVSS 2017), with a `max_age` extension (0 is the paper): the definition.

`track_host` is the normative restatement: NumPy, every comparison on a score or an IoU in float32, in a fixed
order.  The device entry point vd_track (viddet_amd/csrc/vd_track.hip, `ops.track`) equals it bit for bit.

A row is a candidate iff seq_nms.row_classes makes it one (id >= 0, a finite score, a class below `num_class` where that is
given) and score >= sigma_l.  Per clip, frames in order:
  1. extend: the active tracks in order of creation; a track of class c takes, among the candidates of class c of this frame
     that no track has taken, the one with the largest IoU to the track's last matched box (seq_nms.iou_matrix's arithmetic),
     ties to the lowest row; where that IoU >= sigma_iou the row joins the track, the track's last box is that row's box, its
     miss count 0 and its maximum score max(maximum, score); otherwise, or with no candidate left, the miss count grows by one
     and the track is closed once it exceeds max_age.  (A NaN IoU - infinite coordinates only - ranks above every number, as
     in np.argmax, and matches nothing.)
  2. start: every candidate not taken starts an active track, in row order.  A track's id is its creation number within the
     clip, from 0, one counter for all classes.
  3. decide, at the clip's end: a track is kept iff its maximum score >= sigma_h and it holds at least t_min rows.  Ids are not
     renumbered.
At most N * (max_age + 1) tracks are active at once: an active track has taken a row of one of the last max_age + 1 frames, and
a row belongs to one track.

`track_online_host` is steps 1 and 2 on a stream that never says where it ends, a state carried from call to call (DESIGN.md 31;
vd_track_push, `ops.TrackState`, equals it bit for bit); `finalize_tracks` is step 3 on its rows, once a clip has ended.
"""
import numpy as np

from .lib import TRACK_MAX_ROWS
from .seq_nms import MAX_ROWS, _clips, iou_matrix, row_classes

_F = np.float32
MAX_AGE = 7                                       # max_age lies in [0, MAX_AGE]
MAX_ACTIVE = MAX_ROWS * (MAX_AGE + 1)             # the active-track table of vd_track
DEFAULTS = dict(sigma_l=0.0, sigma_h=0.5, sigma_iou=0.5, t_min=2, max_age=0)
METHODS = ("iou", "sort", "byte")                 # the linking methods of `track=`: this module's, viddet_amd/sort.py's, byte.py's


def check_params(sigma_l=0.0, sigma_h=0.5, sigma_iou=0.5, t_min=2, max_age=0, who="track"):
    """The five parameters as (float32, float32, float32, int, int); a ValueError names the argument that is not usable"""
    out = []
    for name, v in (("sigma_l", sigma_l), ("sigma_h", sigma_h), ("sigma_iou", sigma_iou)):
        try:
            f = _F(v)
        except (TypeError, ValueError):
            raise ValueError("%s: %s must be a number, got %r" % (who, name, v))
        if f != f:
            raise ValueError("%s: %s must not be NaN" % (who, name))
        out.append(f)
    for name, v, lo, hi in (("t_min", t_min, 1, 2 ** 31 - 1), ("max_age", max_age, 0, MAX_AGE)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (who, name, lo, hi, v))
        out.append(int(v))
    return tuple(out)


def parse_option(track, post_nms, who):
    """The `track=` option of `who` (detect_video, open_video): None / False -> None; True or a dict of the method's parameters,
    `clip` and `method` -> (the parameters, the method's defaults filled in, `clip` or None, the method: 'iou', this module's
    tracker and the default, 'sort', viddet_amd/sort.py's, or 'byte', viddet_amd/byte.py's, which takes sigma_d, sigma_new and
    sigma_iou2 beside the five).  A ValueError names what is not usable."""
    if track is None or track is False:
        return None
    kw = {} if track is True else dict(track)
    clip = kw.pop("clip", None)
    method = kw.pop("method", "iou")
    if method not in METHODS:
        raise ValueError("%s: track method must be 'iou' or 'sort', got %r (or 'byte')" % (who, method))
    defaults = DEFAULTS
    if method == "sort":
        from .sort import DEFAULTS as defaults
    elif method == "byte":
        from .byte import DEFAULTS as defaults
    unknown = sorted(set(kw) - set(defaults))
    if unknown:
        extra = ", sigma_d, sigma_new, sigma_iou2" if method == "byte" else ""
        raise ValueError("%s: track takes sigma_l, sigma_h, sigma_iou, t_min and max_age%s (and clip, method), got %s"
                         % (who, extra, ", ".join(unknown)))
    kw = dict(defaults, **kw)
    if method == "byte":
        from .byte import check_byte_params
        check_byte_params(who=who + " with track", **kw)
    else:
        check_params(who=who + " with track", **kw)
    if post_nms > TRACK_MAX_ROWS:
        raise ValueError("%s with track: post_nms=%d rows per frame, the tracker takes at most %d" % (who, post_nms, TRACK_MAX_ROWS))
    return kw, clip, method


def split_online(track, who):
    """The `online` word of open_video's `track=` option, which parse_option does not know (detect_video refuses it as an unknown
    key): track -> (track without the key, online: bool, False where it is not given).  `online: True` asks a session to carry
    the method's tracker from push to push; a ValueError names a value that is no bool."""
    if not isinstance(track, dict) or "online" not in track:
        return track, False
    rest = dict(track)
    online = rest.pop("online")
    if type(online).__name__ not in ("bool", "bool_"):
        raise ValueError("%s: track's online must be a bool, got %r" % (who, online))
    return rest, bool(online)


def track_host(ids, scores, bboxes, clip_start=None, num_class=None, sigma_l=0.0, sigma_h=0.5, sigma_iou=0.5, t_min=2, max_age=0,
               stats=None):
    """ids (F,N[,1]), scores (F,N[,1]), bboxes (F,N,4) -> (track (F,N) int32: the row's track id, -1 for a row that is no
    candidate or whose track is dropped; tlen (F,N) int32: the rows of its track, 0 where track is -1; tscore (F,N) float32: the
    track's maximum score, -1 where track is -1).  `stats`, a dict, receives per frame 'active' (the active tracks after the
    frame's start step) and 'closed' (the tracks its extend step closed), and 'tracks' (the kept tracks of every clip)."""
    sl, sh, si, t_min, max_age = check_params(sigma_l, sigma_h, sigma_iou, t_min, max_age, "track_host")
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
    n_active = np.zeros(F, dtype=np.int64)
    n_closed = np.zeros(F, dtype=np.int64)
    kept_per_clip = []
    for t0, t1 in _clips(clip_start, F):
        local = np.full((t1 - t0, N), -1, dtype=np.int64)         # the row's track, numbered inside the clip
        length, best = [], []                                     # per track of the clip
        active = []                                               # [id, class, last box, misses], in order of creation
        for t in range(t0, t1):
            free = cls[t] >= 0
            if active and free.any():
                iou = iou_matrix(np.stack([a[2] for a in active]), bboxes[t])          # (active, N), once per frame
            survivors = []
            for k, a in enumerate(active):
                rows = np.nonzero(free & (cls[t] == a[1]))[0]
                hit = False
                if len(rows):
                    j = int(rows[np.argmax(iou[k, rows])])         # the first maximum: the lowest row of a tie
                    hit = bool(iou[k, j] >= si)
                if hit:
                    free[j] = False
                    local[t - t0, j] = a[0]
                    a[2], a[3] = bboxes[t, j], 0
                    length[a[0]] += 1
                    if sc[t, j] > best[a[0]]:
                        best[a[0]] = sc[t, j]
                else:
                    a[3] += 1
                if a[3] <= max_age:
                    survivors.append(a)
            n_closed[t] = len(active) - len(survivors)
            active = survivors
            for j in np.nonzero(free)[0]:
                local[t - t0, j] = len(length)
                active.append([len(length), int(cls[t, j]), bboxes[t, j], 0])
                length.append(1)
                best.append(sc[t, j])
            n_active[t] = len(active)
        length = np.asarray(length, dtype=np.int32)
        best = np.asarray(best, dtype=_F)
        kept = (best >= sh) & (length >= t_min)
        kept_per_clip.append(int(kept.sum()))
        if len(length):
            on = (local >= 0) & kept[np.maximum(local, 0)]
            track[t0:t1] = np.where(on, local, -1)
            tlen[t0:t1] = np.where(on, length[np.maximum(local, 0)], 0)
            tscore[t0:t1] = np.where(on, best[np.maximum(local, 0)], _F(-1))
    if stats is not None:
        stats["active"], stats["closed"], stats["tracks"] = n_active, n_closed, kept_per_clip
    return track, tlen, tscore


def track_online_host(state, ids, scores, bboxes, num_class=None, sigma_l=0.0, sigma_iou=0.5, max_age=0):
    """The tracker on a stream that never says where it ends (vd_track_push, `ops.TrackState`, equals it bit for
    bit): track_host's extend and start steps on the given frames, starting from `state` (None: a fresh stream) ->
    (the new state, track, tlen, tscore).  Per row, (F,N): `track` int32, the id of the row's track - a creation number counted
    over the whole stream - or -1 for a row that is no candidate; `tlen` int32, the rows of its track so far, this one included
    (0 beside -1); `tscore` float32, the track's maximum score so far (-1 beside -1).  Nothing is decided here, so sigma_h and
    t_min are no arguments: finalize_tracks makes track_host's arrays of a finished clip's rows.  A state is a dict of 'next_id'
    and 'active', the active tracks [id, class, last box, misses, length, maximum] in order of creation; the one given is not
    changed.  Pushing a clip in pieces gives what one call on all of it gives."""
    sl, _, si, _, max_age = check_params(sigma_l, 0.5, sigma_iou, 1, max_age, "track_online_host")
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
    next_id = 0 if state is None else int(state["next_id"])
    active = [] if state is None else [[a[0], a[1], np.array(a[2], dtype=_F), a[3], a[4], _F(a[5])] for a in state["active"]]
    for t in range(F):
        free = cls[t] >= 0
        if active and free.any():
            iou = iou_matrix(np.stack([a[2] for a in active]), bboxes[t])              # (active, N), once per frame
        survivors = []
        for k, a in enumerate(active):
            rows = np.nonzero(free & (cls[t] == a[1]))[0]
            hit = False
            if len(rows):
                j = int(rows[np.argmax(iou[k, rows])])             # the first maximum: the lowest row of a tie
                hit = bool(iou[k, j] >= si)
            if hit:
                free[j] = False
                a[2], a[3] = bboxes[t, j].copy(), 0
                a[4] += 1
                if sc[t, j] > a[5]:
                    a[5] = sc[t, j]
                track[t, j], tlen[t, j], tscore[t, j] = a[0], a[4], a[5]
            else:
                a[3] += 1
            if a[3] <= max_age:
                survivors.append(a)
        active = survivors
        for j in np.nonzero(free)[0]:
            active.append([next_id, int(cls[t, j]), bboxes[t, j].copy(), 0, 1, sc[t, j]])
            track[t, j], tlen[t, j], tscore[t, j] = next_id, 1, sc[t, j]
            next_id += 1
    return dict(next_id=next_id, active=active), track, tlen, tscore


def finalize_tracks(track, tlen, tscore, sigma_h=0.5, t_min=2, tbox=None):
    """track_online_host's three outputs over ALL frames of one finished clip, (F,N) each -> track_host's three arrays: a
    track's length and maximum are the largest `tlen` and `tscore` among its rows (both only grow, and its last row carries
    them); it is kept iff its maximum >= sigma_h and it holds at least t_min rows; the rows of a dropped track become
    -1 / 0 / -1.  Ids are not renumbered.  tbox (F,N,4): the fourth output of sort.sort_online_host / byte.byte_online_host;
    given it, a fourth array comes back, sort_host's / byte_host's `tbox`: the row's box where its track is kept, -1 where it
    is dropped."""
    _, sh, _, t_min, _ = check_params(0.0, sigma_h, 0.5, t_min, 0, "finalize_tracks")
    track = np.asarray(track, dtype=np.int32)
    tlen = np.asarray(tlen, dtype=np.int32)
    tscore = np.asarray(tscore, dtype=_F)
    if track.ndim != 2 or tlen.shape != track.shape or tscore.shape != track.shape:
        raise ValueError("expected track, tlen and tscore (F,N), got %r %r %r" % (track.shape, tlen.shape, tscore.shape))
    if tbox is not None:
        tbox = np.asarray(tbox, dtype=_F)
        if tbox.shape != track.shape + (4,):
            raise ValueError("expected tbox %r beside track %r, got %r" % (track.shape + (4,), track.shape, tbox.shape))
        first = finalize_tracks(track, tlen, tscore, sigma_h, t_min)
        return first + (np.where((first[0] >= 0)[..., None], tbox, _F(-1)).astype(_F),)
    on = track >= 0
    if not on.any():
        return np.full(track.shape, -1, np.int32), np.zeros(track.shape, np.int32), np.full(track.shape, -1, _F)
    # (ids are creation numbers: a clip of a session starts at 0; a clip cut out of a longer stream starts higher)
    lo = int(track[on].min())
    idx = np.where(on, track - lo, 0)
    n = int(idx.max()) + 1
    length = np.zeros(n, dtype=np.int32)
    best = np.full(n, -np.inf, dtype=_F)
    np.maximum.at(length, idx[on], tlen[on])
    np.maximum.at(best, idx[on], tscore[on])
    kept = on & ((best >= sh) & (length >= t_min))[idx]
    return (np.where(kept, track, -1).astype(np.int32), np.where(kept, length[idx], 0).astype(np.int32),
            np.where(kept, best[idx], _F(-1)).astype(_F))


def clip_summary(track, tlen, clip_start=None):
    """Per clip (tracks, rows, mean_len): the kept tracks, the rows they hold and rows / tracks (0.0 without a track)"""
    track, tlen = np.asarray(track), np.asarray(tlen)
    out = []
    for t0, t1 in _clips(clip_start, track.shape[0]):
        tr = track[t0:t1]
        n = len(np.unique(tr[tr >= 0]))
        rows = int((tr >= 0).sum())
        out.append((n, rows, rows / n if n else 0.0))
    return out
