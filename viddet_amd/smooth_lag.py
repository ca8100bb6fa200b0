"""Fixed-lag smoothing of the boxes of a stream of frames along its tracks: smooth.py's Rauch-Tung-Striebel pass for a camera
feed, where nobody says how many frames follow: the definition.

A frame's box is given out `lag` frames late, estimated from everything before it and the `lag` frames after it: the forward
pass of smooth.py is causal and is kept, the backward pass starts at a horizon `lag` frames ahead instead of the clip's end.

`smooth_lag_host` is the normative restatement: NumPy, every operation ONE float32 operation in the order smooth.py writes, no
product and sum contracted.  The device entry point vd_track_smooth_push (viddet_amd/csrc/vd_track_smooth_live.hip,
`ops.SmoothLagState`) equals it bit for bit on both outputs.

The frames of ONE stream arrive in calls of F >= 0 frames; `track` is the per-row id of an online tracker (track_online_host,
sort_online_host, byte_online_host), counted over the stream.  Frame u is final once frame u + lag has been taken, or at a
flush.  For every emitted frame u, with the horizon h = min(u + lag, the last frame taken):
  members   a present row (seq_nms.row_classes >= 0) of stream frame t is a member of track k = track[t, i] iff
            0 <= k < (t + 1) * N and no lower row of its frame is a member of k already: smooth.py's step 1 in causal form.
            An online tracker creates at most N ids a frame, so its table satisfies the bound; rows outside it are no members:
            any table is safe.
  segments  smooth.py's step 2: a member's predecessor is the member of its id in the nearest of the max_gap + 1 frames
            before it.  The segment of a member at u is truncated behind h.
  forward   step 3 unchanged: a member without predecessor starts a filter, every other one predicts its predecessor's
            posterior over the gap and updates.  The posterior of a member never depends on a later frame.
  backward  step 4 unchanged (smooth.rts_step), from the last member of the truncated segment - the last one at a frame <= h -
            back to the member at u.
  output    step 5: the input bits are kept for a row that is no member, for a member whose truncated segment has one member
            and for a smoothed box that is not finite.  slen is the member count of the truncated segment, 0 for no member.
So on a table within the id bound, frame u comes out as row u of smooth_host on the frames [0, h] (the truncation property),
and with lag >= T - 1 one push and a flush are smooth_host on the clip.

The loop is resumable: the state keeps, for the last 16 frames (lag <= 15, max_gap + 1 <= 8) in a ring of slots t % 16, every
row's member id, input box, posterior state, predecessor and successor as (frame, row) and position in its segment - what the
device keeps in its state block.  This module imports NumPy only.
"""
import numpy as np

from .seq_nms import MAX_ROWS, row_classes
from .smooth import _predict_n, check_params as _check_gap, rts_step
from .sort import _KEYS, kf_box, kf_predict, kf_start, kf_take, kf_update, measure
from .track import MAX_AGE

_F = np.float32
RING = 16                                          # frame slots of the state
MAX_LAG = RING - 1
DEFAULTS = dict(max_gap=MAX_AGE)                   # `lag` has no default: a latency must be chosen
_SHAPES = dict(x=(3,), xd=(3,), p00=(3,), p01=(3,), p11=(3,), r=(), p=())


def check_params(lag, max_gap=MAX_AGE, who="smooth_lag"):
    """(lag, max_gap) as ints; a ValueError names the argument that is not usable"""
    if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 0 <= int(lag) <= MAX_LAG:
        raise ValueError("%s: lag must be an integer in [0, %d], got %r" % (who, MAX_LAG, lag))
    return int(lag), _check_gap(max_gap, who)


def parse_option(smooth, tracked, who):
    """The `smooth=` option of `who` (open_video): None / False -> None; {'lag': L} or {'lag': L, 'max_gap': g} -> the dict as
    given.  True is refused: a latency must be chosen.  tracked: the session has `track` on.  A ValueError names what is not
    usable."""
    if smooth is None or smooth is False:
        return None
    if smooth is True:
        raise ValueError("%s: smooth needs lag: a session gives a frame out `lag` frames late, say {'lag': L} with L in [0, %d]"
                         % (who, MAX_LAG))
    kw = dict(smooth)
    unknown = sorted(set(kw) - {"lag"} - set(DEFAULTS))
    if unknown:
        raise ValueError("%s: smooth takes lag, max_gap, got %s" % (who, ", ".join(unknown)))
    if "lag" not in kw:
        raise ValueError("%s: smooth needs lag: a session gives a frame out `lag` frames late, say {'lag': L} with L in [0, %d]"
                         % (who, MAX_LAG))
    check_params(who=who + " with smooth", **kw)
    if not tracked:
        raise ValueError("%s: smooth needs track: the pass runs over the tracks of the stream" % who)
    return kw


def new_state(N):
    """a fresh stream of N rows a frame: no frame taken, none emitted, every slot empty"""
    post = {k: np.zeros((RING, N) + _SHAPES[k], _F) for k in _KEYS}
    neg = lambda: np.full((RING, N), -1, np.int64)
    return dict(N=int(N), frames=0, emitted=0, slot_frame=np.full(RING, -1, np.int64), mem=neg(), box=np.zeros((RING, N, 4), _F),
                post=post, prev_f=neg(), prev_i=neg(), next_f=neg(), next_i=neg(), pos=np.zeros((RING, N), np.int64))


def _copy(state):
    return {k: ({f: a.copy() for f, a in v.items()} if isinstance(v, dict) else v.copy() if isinstance(v, np.ndarray) else v)
            for k, v in state.items()}


def _take_frame(st, t, present, track, box, max_gap):
    """stream frame t into slot t % 16: members, links, the forward step"""
    N, s = st["N"], t % RING
    # members: per frame the first row of every usable id
    ok = present & (track >= 0) & (track < (t + 1) * N)
    mem = np.full(N, -1, np.int64)
    r = np.nonzero(ok)[0]
    first = r[np.unique(track[r], return_index=True)[1]]
    mem[first] = track[first]
    st["slot_frame"][s] = t
    st["mem"][s], st["box"][s] = mem, box
    st["prev_f"][s] = st["prev_i"][s] = st["next_f"][s] = st["next_i"][s] = -1
    st["pos"][s] = 0
    rows = np.nonzero(mem >= 0)[0]
    if len(rows) == 0:
        return
    # links: the member of the id in the nearest of the max_gap + 1 frames before
    pf = np.full(len(rows), -1, np.int64)
    pi = np.full(len(rows), -1, np.int64)
    for d in range(1, max_gap + 2):
        f = t - d
        if f < 0:
            break
        hit = mem[rows][:, None] == st["mem"][f % RING][None, :]          # a frame's member ids differ: one hit a row at most
        got = hit.any(axis=1) & (pf < 0)
        pf[got], pi[got] = f, hit.argmax(axis=1)[got]
    st["prev_f"][s, rows], st["prev_i"][s, rows] = pf, pi
    has = pf >= 0
    st["next_f"][pf[has] % RING, pi[has]], st["next_i"][pf[has] % RING, pi[has]] = t, rows[has]
    # forward: start, or predict over the gap and update from the predecessor's posterior
    z = measure(box[rows])
    post = kf_start(z)
    if has.any():
        a0 = {k: st["post"][k][pf[has] % RING, pi[has]] for k in _KEYS}
        upd = kf_update(_predict_n(a0, t - pf[has]), z[has])
        for k in _KEYS:
            post[k][has] = upd[k]
        st["pos"][s, rows[has]] = st["pos"][pf[has] % RING, pi[has]] + 1
    for k in _KEYS:
        st["post"][k][s, rows] = post[k]


def _emit(st, u, h):
    """frame u against the horizon h (u <= h < u + 16, both in the ring) -> (sbox (N,4), slen (N,))"""
    s = u % RING
    sbox = st["box"][s].copy()
    slen = np.zeros(st["N"], np.int32)
    rows = np.nonzero(st["mem"][s] >= 0)[0]
    if len(rows) == 0:
        return sbox, slen
    # the last member of the truncated segment: follow the successors while they lie at a frame <= h
    cf, ci = np.full(len(rows), u, np.int64), rows.copy()
    for _ in range(RING):
        nf, ni = st["next_f"][cf % RING, ci], st["next_i"][cf % RING, ci]
        go = (nf >= 0) & (nf <= h)
        if not go.any():
            break
        cf, ci = np.where(go, nf, cf), np.where(go, ni, ci)
    n = st["pos"][cf % RING, ci] + 1
    slen[rows] = n
    # backward, from that member's posterior to the member at u
    last = {k: st["post"][k][cf % RING, ci] for k in _KEYS}
    S = dict(x=last["x"].copy(), xd=last["xd"].copy(), r=last["r"].copy())
    for _ in range(RING):
        on = np.nonzero(cf > u)[0]
        if len(on) == 0:
            break
        pf, pi = st["prev_f"][cf[on] % RING, ci[on]], st["prev_i"][cf[on] % RING, ci[on]]
        g = cf[on] - pf
        a0 = {k: st["post"][k][pf % RING, pi] for k in _KEYS}
        for j in range(int(g.max()) - 1, -1, -1):
            sel = np.nonzero(g > j)[0]
            f = _predict_n(kf_take(a0, sel), np.full(len(sel), j))
            new = rts_step({k: S[k][on[sel]] for k in S}, f, kf_predict(f))
            for k in S:
                S[k][on[sel]] = new[k]
        cf[on], ci[on] = pf, pi
    out = kf_box(dict(x=S["x"], r=S["r"]))
    good = (n >= 2) & np.isfinite(out).all(axis=1)
    sbox[rows[good]] = out[good]
    return sbox, slen


def smooth_lag_host(state, ids, scores, bboxes, track, num_class, lag, max_gap=MAX_AGE, flush=False):
    """The next F >= 0 frames of ONE stream - ids (F,N[,1]), scores (F,N[,1]), bboxes (F,N,4), track (F,N) integers, the per-row
    id of an online tracker counted over the stream - on `state` (None: a fresh stream; else an earlier call's, which is not
    changed) -> (the new state, t0, sbox (m,N,4) float32, slen (m,N) int32) for the m >= 0 frames [t0, t0 + m) that became
    final: frame u is final once frame u + lag has been taken, or at flush=True, which emits every frame taken and returns a
    fresh state (None).  Cutting a stream into calls in any way, with one flush at the end, gives the bits of one call."""
    lag, max_gap = check_params(lag, max_gap, "smooth_lag_host")
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
    if state is not None and state["N"] != N:
        raise ValueError("the state is a stream of N=%d rows per frame, got N=%d" % (state["N"], N))
    track = track.astype(np.int64)
    present = row_classes(ids.reshape(F, N), scores.reshape(F, N), num_class) >= 0
    st = new_state(N) if state is None else _copy(state)
    t0 = st["emitted"]
    sboxes, slens = [], []
    for k in range(F):
        t = st["frames"]
        _take_frame(st, t, present[k], track[k], bboxes[k], max_gap)
        st["frames"] = t + 1
        if t >= lag:
            box, n = _emit(st, t - lag, t)
            sboxes.append(box), slens.append(n)
            st["emitted"] = t - lag + 1
    if flush:
        for u in range(st["emitted"], st["frames"]):
            box, n = _emit(st, u, st["frames"] - 1)
            sboxes.append(box), slens.append(n)
        st = None
    sbox = np.stack(sboxes) if sboxes else np.zeros((0, N, 4), _F)
    slen = np.stack(slens) if slens else np.zeros((0, N), np.int32)
    return st, t0, sbox, slen
