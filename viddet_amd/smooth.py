"""Smoothing the boxes of a clip along its tracks with the fixed-interval (Rauch, Tung and Striebel, "Maximum likelihood estimates
of linear dynamic systems", AIAA Journal 1965) smoother of sort.py's Kalman filter: the definition.

A track is known once the clip has ended, so every box of it can be estimated from the frames before AND after it: the forward
pass is the filter of sort.py, unchanged, the backward pass carries the later frames' evidence back.

`smooth_host` is the normative restatement: NumPy, every operation ONE float32 operation in a fixed order, no
product and sum contracted, `/` and `sqrt` correctly rounded.  The device entry point vd_track_smooth
(viddet_amd/csrc/vd_track_smooth.hip, `ops.smooth`) equals it bit for bit on both outputs.

The filter is sort.py's decoupled form of Bewley's 7-state filter, imported: measure, kf_start, kf_predict, kf_update, kf_box;
three pairs (x, xd, p00, p01, p11) for u, v, s and a scalar (r, p) for the aspect, 17 floats a state.  The 7 x 7 covariance is
block diagonal in the forward pass, and the smoother gain C = P F^T P_pred^-1 of a block-diagonal P and P_pred is block diagonal
too: the backward pass is decoupled as well, a 2 x 2 gain per pair and a scalar one for r.

Per clip [t0, t1), with `track` the per-row ids of track_host / sort_host / byte_host / vd_track* / finalize_tracks:
  1. members: tubelet_host's step 1 word for word.  A row is present iff seq_nms.row_classes makes it a candidate.  A present row
     is a member of track u = track[t, i] iff 0 <= u < (t1 - t0) * N and no lower row of its frame is a member of u already: any
     table is safe.
  2. segments: a track's members in frame order; where two consecutive members lie more than max_gap + 1 frames apart the track
     is cut.  A segment is a maximal run without a cut: members m_0 .. m_{n-1} at frames f_0 < .. < f_{n-1}.
  3. forward, for n >= 2:  post_0 = kf_start(measure(box_0)),
                           post_i = kf_update(kf_predict^(f_i - f_{i-1})(post_{i-1}), measure(box_i)).
     For a track of sort_host or byte_host and max_gap >= the tracker's max_age, kf_box(post_i) is that tracker's tbox.
  4. backward: S = (x, xd, r) of post_{n-1}.  For i = n-2 .. 0 with g = f_{i+1} - f_i: the chain a_0 = post_i,
     a_j = kf_predict(a_{j-1}), j = 1..g (kf_predict's `s + ds <= 0` rule included).  For j = g-1 .. 0, f = a_j, p = a_{j+1},
     per pair u, v, s (F = [[1, 1], [0, 1]], so P F^T = [[p00 + p01, p01], [p01 + p11, p11]]):
         A = f.p00 + f.p01, B = f.p01, C = f.p01 + f.p11, D = f.p11
         det = p.p00 * p.p11 - p.p01 * p.p01
         c00 = (A * p.p11 - B * p.p01) / det,  c01 = (B * p.p00 - A * p.p01) / det
         c10 = (C * p.p11 - D * p.p01) / det,  c11 = (D * p.p00 - C * p.p01) / det
         dx = S.x - p.x,  dxd = S.xd - p.xd
         S.x = f.x + (c00 * dx + c01 * dxd),  S.xd = f.xd + (c10 * dx + c11 * dxd)
     and for the aspect  S.r = f.r + (f.p / p.p) * (S.r - p.r).
     Every product, sum, difference and quotient above is one float32 operation, in the order written (dx and dxd from the old
     S).  After j = 0, S is member i's smoothed state.
  5. output: a member's sbox is kf_box of (S.x, S.r) - for the last member kf_box(post_{n-1}).  A member whose four smoothed
     coordinates are not all finite keeps its input box; degenerate boxes get no other special case.  Members of a segment with
     n == 1, rows that are no members and rows of frames that no clip covers keep the bits of their input box.  slen is the
     number of members of the row's segment, 0 for a row that is no member.

The smoothed covariance is not needed for the smoothed mean and is not computed.  This module imports NumPy only.
"""
import numpy as np

from .seq_nms import MAX_ROWS, _clips, row_classes
from .sort import _KEYS, kf_box, kf_predict, kf_start, kf_take, kf_update, measure
from .track import MAX_AGE

_F = np.float32
DEFAULTS = dict(max_gap=MAX_AGE)


def check_params(max_gap=MAX_AGE, who="smooth"):
    """max_gap as an int; a ValueError names the argument that is not usable"""
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= int(max_gap) <= MAX_AGE:
        raise ValueError("%s: max_gap must be an integer in [0, %d], got %r" % (who, MAX_AGE, max_gap))
    return int(max_gap)


def parse_option(smooth, tracked, who):
    """The `smooth=` option of `who` (detect_video): None / False -> None; True or {'max_gap': g} -> the dict as given.
    tracked: the call has `track` on - the pass runs over its tracks.  A ValueError names what is not usable."""
    if smooth is None or smooth is False:
        return None
    kw = {} if smooth is True else dict(smooth)
    unknown = sorted(set(kw) - set(DEFAULTS))
    if unknown:
        raise ValueError("%s: smooth takes max_gap, got %s" % (who, ", ".join(unknown)))
    check_params(who=who + " with smooth", **kw)
    if not tracked:
        raise ValueError("%s: smooth needs track: the pass runs over the tracks of the clip" % who)
    return kw


def _put(kf, sel, new):
    for k in _KEYS:
        kf[k][sel] = new[k]


def _predict_n(kf, g):
    """kf_predict applied g[k] times to state k"""
    kf = {k: kf[k].copy() for k in _KEYS}
    for j in range(1, int(g.max()) + 1 if len(g) else 0):
        sel = np.nonzero(g >= j)[0]
        _put(kf, sel, kf_predict(kf_take(kf, sel)))
    return kf


def rts_step(S, f, p):
    """One backward step of step 4: S = dict(x (K,3), xd (K,3), r (K,)) the smoothed state at the later frame, f the filtered state
    a_j and p = kf_predict(f) -> the smoothed state at f's frame.  The arrays' dtype is the arithmetic's."""
    with np.errstate(all="ignore"):
        A = f["p00"] + f["p01"]
        B = f["p01"]
        C = f["p01"] + f["p11"]
        D = f["p11"]
        det = p["p00"] * p["p11"] - p["p01"] * p["p01"]
        c00 = (A * p["p11"] - B * p["p01"]) / det
        c01 = (B * p["p00"] - A * p["p01"]) / det
        c10 = (C * p["p11"] - D * p["p01"]) / det
        c11 = (D * p["p00"] - C * p["p01"]) / det
        dx = S["x"] - p["x"]
        dxd = S["xd"] - p["xd"]
        return dict(x=f["x"] + (c00 * dx + c01 * dxd), xd=f["xd"] + (c10 * dx + c11 * dxd),
                    r=f["r"] + (f["p"] / p["p"]) * (S["r"] - p["r"]))


def smooth_host(ids, scores, bboxes, track, clip_start=None, num_class=None, max_gap=MAX_AGE, stats=None):
    """ids (F,N[,1]), scores (F,N[,1]), bboxes (F,N,4), track (F,N) int32 -> (sbox (F,N,4) float32: the smoothed box of every
    member of a segment of two or more members, the input box elsewhere; slen (F,N) int32: the members of the row's segment, 0
    for a row that is no member).  `stats`, a dict, receives per clip 'segments' and 'members' and 'filtered' (F,N,4): the forward
    posterior box of every member of a segment with n >= 2, the input box elsewhere."""
    max_gap = check_params(max_gap, "smooth_host")
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
    present = row_classes(ids.reshape(F, N), scores.reshape(F, N), num_class) >= 0
    sbox = bboxes.copy()
    filtered = bboxes.copy()
    slen = np.zeros((F, N), dtype=np.int32)
    per_clip = dict(segments=[], members=[])
    for t0, t1 in _clips(clip_start, F):
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
        per_clip["members"].append(int(M))
        if M == 0:
            per_clip["segments"].append(0)
            continue
        # 2. segments
        first = np.nonzero(np.r_[True, (mu[1:] != mu[:-1]) | (mt[1:] - mt[:-1] > max_gap + 1)])[0]
        n = np.diff(np.r_[first, M])
        per_clip["segments"].append(len(first))
        slen[t0 + mt, mi] = np.repeat(n, n)
        first, n = first[n >= 2], n[n >= 2]
        if len(first) == 0:
            continue
        box = bboxes[t0 + mt, mi]                                  # (M,4), the members' input boxes
        # 3. forward: the k-th member of every segment side by side; the posterior of every member is kept
        post = kf_start(measure(box))                              # rows of members that are no first one are overwritten
        for k in range(1, int(n.max())):
            idx = first[n > k] + k
            _put(post, idx, kf_update(_predict_n(kf_take(post, idx - 1), mt[idx] - mt[idx - 1]), measure(box[idx])))
        seg_rows = np.concatenate([np.arange(a, a + c) for a, c in zip(first, n)])
        filtered[t0 + mt[seg_rows], mi[seg_rows]] = kf_box(kf_take(post, seg_rows))
        # 4. backward: the k-th member from the end of every segment side by side
        last = first + n - 1
        S = dict(x=post["x"][last].copy(), xd=post["xd"][last].copy(), r=post["r"][last].copy())     # per segment
        out = np.empty((M, 4), dtype=_F)
        out[last] = kf_box(dict(x=S["x"], r=S["r"]))
        for k in range(1, int(n.max())):
            on = np.nonzero(n > k)[0]
            idx = last[on] - k
            g = mt[idx + 1] - mt[idx]
            a0 = kf_take(post, idx)
            for j in range(int(g.max()) - 1, -1, -1):
                sel = np.nonzero(g > j)[0]
                f = _predict_n(kf_take(a0, sel), np.full(len(sel), j))
                new = rts_step({k_: S[k_][on[sel]] for k_ in S}, f, kf_predict(f))
                for k_ in S:
                    S[k_][on[sel]] = new[k_]
            out[idx] = kf_box(dict(x=S["x"][on], r=S["r"][on]))
        # 5. output: a smoothed box that is not finite gives way to the input box
        good = np.isfinite(out[seg_rows]).all(axis=1)
        sbox[t0 + mt[seg_rows], mi[seg_rows]] = np.where(good[:, None], out[seg_rows], box[seg_rows])
    if stats is not None:
        stats.update(per_clip)
        stats["filtered"] = filtered
    return sbox, slen
