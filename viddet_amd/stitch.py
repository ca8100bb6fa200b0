"""Re-linking the track fragments of a clip across long gaps: the definition.

A tracker closes a track that misses more than max_age frames (at most track.MAX_AGE = 7: the active table is LDS), and the
object comes back under a new id.  Once the clip has ended the fragments can be matched end to start, in the manner of the
appearance-free link of StrongSORT (Du et al., "StrongSORT: Make DeepSORT Great Again", IEEE TMM 2023), without its learned
model: every track's filter state at its last row is extrapolated over the gap, the fragments are matched with the assignment
the trackers use, and every chain takes its first fragment's id.

`stitch_host` is the normative restatement: NumPy, every operation ONE float32 operation in a fixed order, no
product and sum contracted, `/` and `sqrt` correctly rounded.  The device entry point vd_track_stitch
(viddet_amd/csrc/vd_track_stitch.hip, `ops.stitch`) equals it bit for bit on all five outputs.

The filter is sort.py's, imported: measure, kf_start, kf_predict, kf_update, kf_box.

Per clip [t0, t1), with `track` the per-row ids of track_host / sort_host / byte_host / vd_track* / finalize_tracks:
  1. members: smooth_host's step 1 word for word.  A row is present iff seq_nms.row_classes makes it a candidate.  A present row
     is a member of track u = track[t, i] iff 0 <= u < (t1 - t0) * N and no lower row of its frame is a member of u already: any
     table is safe.  A track is an id with at least one member; its members in frame order lie at frames f_0 < .. < f_{n-1}.
  2. participants: the tracks in ascending id, the first STITCH_MAX_TRACKS = 512 of them.  The others enter no link and are
     counted in overflow[clip]; they keep their id, their length and their maximum.
  3. tails and heads of a participant: its tail state is smooth.py's step 3 over the whole track, never cut:
         post_0 = kf_start(measure(box_0)),  post_i = kf_update(kf_predict^(f_i - f_{i-1})(post_{i-1}), measure(box_i));
     its tail is (f_{n-1}, the class of member n-1, post_{n-1}), its head (f_0, the class of member 0, the input box of member 0).
  4. tail a and head b are admissible iff a != b, 1 <= g = f_0(b) - f_{n-1}(a) <= max_gap, the classes are equal and
         q = iou(kf_box(kf_predict^g(post_a)), head box of b) >= sigma_iou
     (seq_nms.iou_matrix's arithmetic, the track side first; the plain >=, so a NaN is not admissible).  Such a pair costs
     Q_ONE - int(q * 2**20), a row's own dummy DUMMY_COST, everything else is FORBIDDEN; rows are the participants as tails,
     columns the participants as heads, both in ascending id, then a dummy per row.  The links are mot_metric.assign_host(cost):
     the most links, then the largest quantised IoU sum, with assign_host's tie rules.  Entered only when the clip has two or
     more participants.
  5. chains: a link runs strictly forward in time, so the links form chains without a cycle.  Every track takes the id of its
     chain's first track, tlen is the members of the whole chain, tscore the chain's maximum: within a track m = the first
     member's score, then `if s > m: m = s` in frame order; then the tracks of the chain folded in chain order by the same rule.
     Rows that are no member get -1 / 0 / -1.  stitches[clip] counts the links.
On a table of track_host / sort_host / byte_host with nothing linked the three arrays are the tracker's own.

Stated departures from StrongSORT's AFLink and GSI: no appearance model - AFLink's is learned; no gate on the tail's length - a
tail of one row has velocity 0; no Gaussian-smoothed interpolation - the tubelet fill stays linear and fills holes of at most 7
frames, so a wider stitched hole is bridged in id only; tracks are per class.

This module imports NumPy only.
"""
import numpy as np

from .mot_metric import DUMMY_COST, FORBIDDEN, Q_ONE, assign_host
from .seq_nms import MAX_ROWS, _clips, row_classes
from .smooth import _predict_n, _put
from .sort import kf_box, kf_predict, kf_start, kf_take, kf_update, measure

_F = np.float32
STITCH_MAX_TRACKS = 512                             # the participants of a clip: the assignment's rows, and its head columns
STITCH_MAX_GAP = 32                                 # the frames a tail is extrapolated over at most
DEFAULTS = dict(max_gap=30, sigma_iou=0.3)


def check_params(max_gap=30, sigma_iou=0.3, who="stitch"):
    """(max_gap as an int, sigma_iou as a float32); a ValueError names the argument that is not usable"""
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 1 <= int(max_gap) <= STITCH_MAX_GAP:
        raise ValueError("%s: max_gap must be an integer in [1, %d], got %r" % (who, STITCH_MAX_GAP, max_gap))
    try:
        si = _F(sigma_iou)
    except (TypeError, ValueError):
        raise ValueError("%s: sigma_iou must be a number, got %r" % (who, sigma_iou))
    if isinstance(sigma_iou, bool) or si != si:
        raise ValueError("%s: sigma_iou must be a number and not NaN, got %r" % (who, sigma_iou))
    return int(max_gap), si


def parse_option(stitch, tracked, who):
    """The `stitch=` option of `who` (detect_video): None / False -> None; True or {'max_gap': g, 'sigma_iou': s} -> the dict as
    given.  tracked: the call has `track` on - the pass runs over its tracks.  A ValueError names what is not usable."""
    if stitch is None or stitch is False:
        return None
    kw = {} if stitch is True else dict(stitch)
    unknown = sorted(set(kw) - set(DEFAULTS))
    if unknown:
        raise ValueError("%s: stitch takes max_gap and sigma_iou, got %s" % (who, ", ".join(unknown)))
    check_params(who=who + " with stitch", **kw)
    if not tracked:
        raise ValueError("%s: stitch needs track: the pass runs over the tracks of the clip" % who)
    return kw


def pair_iou(a, b):
    """(K,4) x (K,4) float32 corner boxes -> (K,) float32: seq_nms.iou_matrix's arithmetic on K pairs, `a` the track side"""
    a, b = np.asarray(a, dtype=_F), np.asarray(b, dtype=_F)
    with np.errstate(all="ignore"):
        iw = np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0])
        ih = np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1])
        inter = iw * ih
        aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        iou = inter / ((aa + ab) - inter)
        return np.where((iw > 0) & (ih > 0), iou, _F(0)).astype(_F)


def link_cost(tail, tail_frame, tail_cls, head_box, head_frame, head_cls, max_gap, sigma_iou):
    """Step 4's cost matrix (P, 2 P) int64 of P participants - `tail` their filter states - and the number of admissible cells"""
    P = len(tail_frame)
    cost = np.full((P, 2 * P), FORBIDDEN, dtype=np.int64)
    cost[np.arange(P), P + np.arange(P)] = DUMMY_COST
    gap = np.asarray(head_frame)[None, :] - np.asarray(tail_frame)[:, None]
    near = (gap >= 1) & (gap <= max_gap) & (np.asarray(tail_cls)[:, None] == np.asarray(head_cls)[None, :])
    near[np.arange(P), np.arange(P)] = False
    a, b = np.nonzero(near)
    if len(a) == 0:
        return cost, 0
    pred = np.empty((P, max_gap + 1, 4), dtype=_F)                   # the tail's box after g predictions
    state = tail
    for g in range(1, int(gap[a, b].max()) + 1):
        state = kf_predict(state)
        pred[:, g] = kf_box(state)
    q = pair_iou(pred[a, gap[a, b]], np.asarray(head_box)[b])
    with np.errstate(invalid="ignore"):
        adm = q >= _F(sigma_iou)
    a, b, q = a[adm], b[adm], q[adm]
    cost[a, b] = Q_ONE - (q * _F(Q_ONE)).astype(np.int64)            # exact in float32
    return cost, int(len(a))


def stitch_host(ids, scores, bboxes, track, clip_start=None, num_class=None, max_gap=30, sigma_iou=0.3, stats=None):
    """ids (F,N[,1]), scores (F,N[,1]), bboxes (F,N,4), track (F,N) int32 -> (strack (F,N) int32: the id of the first track of
    the row's chain, -1 for a row that is no member; tlen (F,N) int32: the members of its chain, 0 beside -1; tscore (F,N)
    float32: the chain's maximum score, -1 beside -1; stitches (V,) int32: the links of every clip; overflow (V,) int32: its
    tracks beyond the first STITCH_MAX_TRACKS).  `stats`, a dict, receives per clip 'tracks', 'pairs' (the admissible cells) and
    'links'."""
    max_gap, si = check_params(max_gap, sigma_iou, "stitch_host")
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
    sc = scores.reshape(F, N)
    cls = row_classes(ids.reshape(F, N), sc, num_class)
    present = cls >= 0
    clips = _clips(clip_start, F)
    strack = np.full((F, N), -1, dtype=np.int32)
    tlen = np.zeros((F, N), dtype=np.int32)
    tscore = np.full((F, N), -1, dtype=_F)
    stitches = np.zeros(len(clips), dtype=np.int32)
    overflow = np.zeros(len(clips), dtype=np.int32)
    per_clip = dict(tracks=[], pairs=[], links=[])
    for v, (t0, t1) in enumerate(clips):
        T = t1 - t0
        # 1. members: per frame the first row of every usable id
        ok = present[t0:t1] & (track[t0:t1] >= 0) & (track[t0:t1] < T * N)
        member = np.zeros((T, N), dtype=bool)
        for t in range(T):
            r = np.nonzero(ok[t])[0]
            member[t, r[np.unique(track[t0 + t, r], return_index=True)[1]]] = True
        mt, mi = np.nonzero(member)
        mu = track[t0 + mt, mi]
        by = np.lexsort((mt, mu))                                  # by track, its members by frame
        mu, mt, mi = mu[by], mt[by], mi[by]
        M = len(mu)
        if M == 0:
            for k in per_clip:
                per_clip[k].append(0)
            continue
        first = np.nonzero(np.r_[True, mu[1:] != mu[:-1]])[0]      # the tracks, in ascending id
        n = np.diff(np.r_[first, M])
        K = len(first)
        msc = sc[t0 + mt, mi]
        best = msc[first].copy()                                   # a track's maximum, its members in frame order
        for k in range(1, int(n.max())):
            on = n > k
            s = msc[first[on] + k]
            best[on] = np.where(s > best[on], s, best[on])
        # 2. participants
        P = min(K, STITCH_MAX_TRACKS)
        overflow[v] = K - P
        root = np.arange(K)
        clen = n.astype(np.int64)
        cmax = best.copy()
        pairs = links = 0
        if P >= 2:
            fp, cnt = first[:P], n[:P]
            # 3. tails: the k-th member of every participant side by side
            box = bboxes[t0 + mt, mi]
            post = kf_start(measure(box))                          # rows of members that are no first one are overwritten
            for k in range(1, int(cnt.max())):
                idx = fp[cnt > k] + k
                _put(post, idx, kf_update(_predict_n(kf_take(post, idx - 1), mt[idx] - mt[idx - 1]), measure(box[idx])))
            last = fp + cnt - 1
            # 4. the assignment
            cost, pairs = link_cost(kf_take(post, last), mt[last], cls[t0 + mt[last], mi[last]], box[fp], mt[fp],
                                    cls[t0 + mt[fp], mi[fp]], max_gap, si)
            col = assign_host(cost)
            a = np.nonzero(col < P)[0]
            b = col[a]
            links = len(a)
            # 5. chains
            if links:
                prev = np.full(K, -1, dtype=np.int64)
                succ = np.full(K, -1, dtype=np.int64)
                prev[b], succ[a] = a, b
                for r in np.nonzero((prev < 0) & (succ >= 0))[0]:
                    chain = [int(r)]
                    while succ[chain[-1]] >= 0:
                        chain.append(int(succ[chain[-1]]))
                    m = best[r]
                    for c in chain[1:]:
                        if best[c] > m:
                            m = best[c]
                    root[chain], clen[chain], cmax[chain] = r, n[chain].sum(), m
        stitches[v] = links
        per_clip["tracks"].append(int(K))
        per_clip["pairs"].append(int(pairs))
        per_clip["links"].append(int(links))
        k = np.repeat(np.arange(K), n)                             # the track of every member
        strack[t0 + mt, mi] = mu[first][root[k]]
        tlen[t0 + mt, mi] = clen[k]
        tscore[t0 + mt, mi] = cmax[k]
    if stats is not None:
        stats.update(per_clip)
    return strack, tlen, tscore, stitches, overflow
