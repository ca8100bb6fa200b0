"""Tubelet rescoring and gap filling over the tracks of a clip (the "tubelet rescoring" of Kang et al., "T-CNN: Tubelets with
Convolutional Neural Networks for Object Detection from Videos", 2016, on the tracks of viddet_amd/track.py): the definition.

`tubelet_host` is the normative restatement: NumPy, every operation on a score or a coordinate in float32, in a
fixed order.  The device entry point vd_tubelet (viddet_amd/csrc/vd_tubelet.hip, `ops.tubelet`) equals it bit for bit.

Per clip [t0, t1), with `track` the per-row ids of track_host / vd_track / finalize_tracks:
  1. present rows and membership: a row is present iff seq_nms.row_classes makes it a candidate.  A present row is a member of
     track u = track[t, i] iff 0 <= u < (t1 - t0) * N and no lower row of its frame is a member of u already (the lowest row of
     a frame carries an id, further rows with it are untracked: any table is safe).  A track's members are ordered by frame.
  2. rescore: 'avg' - s_u is the float32 sum of the members' scores in frame order, from float32(0), one rounding per add, then
     divided by float32(len), correctly rounded (seq_nms_host's step 3); 'max' - s_u is the first member's score, replaced by
     a later member's where that is greater (track_host's maximum: of -0.0 and 0.0 the earlier one); every member's new score
     is s_u.  None - the scores stay.  A row that is no member keeps its score.
  3. fill: consecutive members of a track at frames f0 < f1 with g = f1 - f0, 1 < g <= max_gap + 1, give every frame f0 + j,
     0 < j < g, one candidate fill row: the id of the member at f0, the track u, w = float32(j) / float32(g), every coordinate
     a + (b - a) * w (a the member at f0, b the one at f1, every operation rounded to float32, no FMA), the score s_u, under
     None the same formula on the two members' scores.
  4. assemble, per frame: the kept rows - the present rows in old row order, with drop_untracked only the members - then the
     fills in ascending track id, admitted while kept + admitted < N (dropped[t] counts the others); kept and admitted rows
     sorted by new score descending, stably, by float comparison (-0.0 and 0.0 tie); rows of -1 follow.
The members' scores are finite, so no sum, quotient, maximum or interpolated score is a NaN (an overflow gives an infinity,
never inf - inf: b - a of finite numbers is no NaN, and w > 0): the sort compares numbers only.
"""
import numpy as np

from .seq_nms import MAX_ROWS, _clips, row_classes
from .track import MAX_AGE

_F = np.float32
RESCORE = {None: 0, "avg": 1, "max": 2}           # vd_tubelet's `rescore` argument
DEFAULTS = dict(rescore="avg", max_gap=MAX_AGE, drop_untracked=False)


def check_params(rescore="avg", max_gap=MAX_AGE, drop_untracked=False, who="tubelet"):
    """The three parameters as (rescore, int, bool); a ValueError names the argument that is not usable"""
    if not (rescore is None or (isinstance(rescore, str) and rescore in RESCORE)):
        raise ValueError("%s: rescore must be 'avg', 'max' or None, got %r" % (who, rescore))
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= int(max_gap) <= MAX_AGE:
        raise ValueError("%s: max_gap must be an integer in [0, %d], got %r" % (who, MAX_AGE, max_gap))
    if not isinstance(drop_untracked, (bool, np.bool_)):
        raise ValueError("%s: drop_untracked must be a bool, got %r" % (who, drop_untracked))
    return rescore, int(max_gap), bool(drop_untracked)


def parse_option(tubelet, tracked, who):
    """The `tubelet=` option of `who` (detect_video): None / False -> None; True or a dict of the three parameters -> the dict
    as given.  tracked: the call has `track` on - the pass runs over its tracks.  A ValueError names what is not usable."""
    if tubelet is None or tubelet is False:
        return None
    kw = {} if tubelet is True else dict(tubelet)
    unknown = sorted(set(kw) - set(DEFAULTS))
    if unknown:
        raise ValueError("%s: tubelet takes rescore, max_gap and drop_untracked, got %s" % (who, ", ".join(unknown)))
    check_params(who=who + " with tubelet", **kw)
    if not tracked:
        raise ValueError("%s: tubelet needs track: the pass runs over the tracks of the clip" % who)
    return kw


def tubelet_host(ids, scores, bboxes, track, clip_start=None, num_class=None, rescore="avg", max_gap=MAX_AGE, drop_untracked=False,
                 stats=None):
    """ids (F,N[,1]), scores (F,N[,1]), bboxes (F,N,4), track (F,N) int32 -> (ids, scores, bboxes of the inputs' shapes; perm
    (F,N) int32: the old row of an output row, -2 for a filled row, -1 for an empty one; track_out (F,N) int32: the output row's
    track, -1 where it has none or the row is empty; dropped (F,) int32: the fills of the frame that found no room).  `stats`, a
    dict, receives per clip 'tracks' (the tracks with a member), 'filled' (the admitted fills) and 'dropped'."""
    rescore, max_gap, drop_untracked = check_params(rescore, max_gap, drop_untracked, "tubelet_host")
    ids = np.asarray(ids, dtype=_F)
    scores = np.asarray(scores, dtype=_F)
    bboxes = np.asarray(bboxes, dtype=_F)
    if bboxes.ndim != 3 or bboxes.shape[2] != 4 or ids.size != bboxes.shape[0] * bboxes.shape[1] or scores.size != ids.size:
        raise ValueError("expected ids (F,N,1), scores (F,N,1), bboxes (F,N,4), got %r %r %r" % (ids.shape, scores.shape, bboxes.shape))
    F, N = bboxes.shape[0], bboxes.shape[1]
    if N > MAX_ROWS:
        raise ValueError("N=%d rows per frame, at most %d are taken" % (N, MAX_ROWS))
    track = np.asarray(track)
    if track.shape != (F, N) or track.dtype.kind not in "iu":
        raise ValueError("expected track (F,N) = (%d,%d) of integers, got %r %s" % (F, N, track.shape, track.dtype))
    track = track.astype(np.int64)
    idf, sc = ids.reshape(F, N), scores.reshape(F, N)
    present = row_classes(idf, sc, num_class) >= 0
    out_ids = np.full((F, N), -1, dtype=_F)
    out_scores = np.full((F, N), -1, dtype=_F)
    out_boxes = np.full((F, N, 4), -1, dtype=_F)
    perm = np.full((F, N), -1, dtype=np.int32)
    track_out = np.full((F, N), -1, dtype=np.int32)
    dropped = np.zeros(F, dtype=np.int32)
    per_clip = dict(tracks=[], filled=[], dropped=[])
    for t0, t1 in _clips(clip_start, F):
        T = t1 - t0
        filled = 0
        # 1. members: per frame the first row of every usable id
        ok = present[t0:t1] & (track[t0:t1] >= 0) & (track[t0:t1] < T * N)
        member = np.zeros((T, N), dtype=bool)
        for t in range(T):
            r = np.nonzero(ok[t])[0]
            member[t, r[np.unique(track[t0 + t, r], return_index=True)[1]]] = True
        mt, mi = np.nonzero(member)                                # by frame, then row
        mu = track[t0 + mt, mi]
        by = np.lexsort((mt, mu))                                  # by track, its members by frame
        mu, mt, mi = mu[by], mt[by], mi[by]
        ms = sc[t0 + mt, mi]
        first = np.nonzero(np.r_[True, mu[1:] != mu[:-1]])[0] if len(mu) else np.zeros(0, np.int64)
        length = np.diff(np.r_[first, len(mu)])
        group = np.repeat(np.arange(len(first)), length)           # the member's track, numbered by ascending id
        # 2. rescore: the k-th member of every track side by side, k ascending: frame order inside every track
        new = sc[t0:t1].copy()
        s_u = np.zeros(len(first), dtype=_F)
        with np.errstate(over="ignore"):
            if rescore == "avg":
                for k in range(int(length.max()) if len(length) else 0):
                    on = length > k
                    s_u[on] = s_u[on] + ms[first[on] + k]
                s_u = (s_u / length.astype(_F)).astype(_F)
            elif rescore == "max":
                s_u = ms[first].copy()
                for k in range(1, int(length.max()) if len(length) else 0):
                    on = np.nonzero(length > k)[0]
                    v = ms[first[on] + k]
                    s_u[on] = np.where(v > s_u[on], v, s_u[on])
        if rescore is not None:
            new[mt, mi] = s_u[group]
        # 3. fills: the pairs of consecutive members with a hole of at most max_gap frames between them
        pair = np.nonzero((mu[1:] == mu[:-1]) & (mt[1:] - mt[:-1] > 1) & (mt[1:] - mt[:-1] <= max_gap + 1))[0] if len(mu) else []
        holes = (mt[pair + 1] - mt[pair] - 1) if len(pair) else np.zeros(0, np.int64)
        pa = np.repeat(pair, holes)                                # one entry per fill row: its pair,
        pj = np.arange(len(pa)) - np.repeat(np.cumsum(holes) - holes, holes) + 1 if len(pa) else np.zeros(0, np.int64)   # its j
        if len(pa):
            pg = (mt[pa + 1] - mt[pa])
            w = (pj.astype(_F) / pg.astype(_F)).astype(_F)
            a, b = bboxes[t0 + mt[pa], mi[pa]], bboxes[t0 + mt[pa + 1], mi[pa + 1]]
            with np.errstate(all="ignore"):
                fbox = (a + (b - a) * w[:, None]).astype(_F)
                if rescore is None:
                    fs = (ms[pa] + (ms[pa + 1] - ms[pa]) * w).astype(_F)
                else:
                    fs = s_u[group[pa]]
            fid = idf[t0 + mt[pa], mi[pa]]
            ft = mt[pa] + pj
            fu = mu[pa]
        # 4. assemble: kept rows in row order, then the fills by ascending id (the pairs are in that order already)
        for t in range(T):
            rows = np.nonzero(member[t] if drop_untracked else present[t0 + t])[0]
            e_id, e_s, e_box = idf[t0 + t, rows], new[t, rows], bboxes[t0 + t, rows]
            e_perm = rows.astype(np.int32)
            e_trk = np.where(member[t, rows], track[t0 + t, rows], -1).astype(np.int32)
            if len(pa):
                cand = np.nonzero(ft == t)[0]
                room = N - len(rows)
                dropped[t0 + t] = max(0, len(cand) - room)
                cand = cand[:room]
                filled += len(cand)
                e_id, e_s, e_box = np.r_[e_id, fid[cand]], np.r_[e_s, fs[cand]], np.concatenate([e_box, fbox[cand]])
                e_perm = np.r_[e_perm, np.full(len(cand), -2, np.int32)]
                e_trk = np.r_[e_trk, fu[cand].astype(np.int32)]
            order = np.argsort(-e_s, kind="stable")                # no NaN among the scores (see above)
            n = len(order)
            out_ids[t0 + t, :n], out_scores[t0 + t, :n], out_boxes[t0 + t, :n] = e_id[order], e_s[order], e_box[order]
            perm[t0 + t, :n], track_out[t0 + t, :n] = e_perm[order], e_trk[order]
        per_clip["tracks"].append(len(first))
        per_clip["filled"].append(int(filled))
        per_clip["dropped"].append(int(dropped[t0:t1].sum()))
    if stats is not None:
        stats.update(per_clip)
    return out_ids.reshape(ids.shape), out_scores.reshape(scores.shape), out_boxes, perm, track_out, dropped
