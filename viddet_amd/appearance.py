"""Appearance association for SORT from the backbone's own features: a descriptor of every detected row pooled
from a route tensor under its box, and sort.py's tracker with one thing replaced, the cost of a cell.  This is the joint
detection and embedding idea (Wang et al., "Towards Real-Time Multi-Object Tracking", ECCV 2020) without a second head, fused
with the IoU as BoT-SORT does (Aharon, Orfaig and Bobrovsky, 2022): min(d_iou, d_app) behind a proximity gate.

`embed_host` is the normative restatement of the descriptor (vd_roi_embed, viddet_amd/csrc/vd_appearance.hip, `ops.roi_embed`
equals it bit for bit).  Every step is ONE float32 operation in the stated order, no product and sum contracted, `/` correctly
rounded.  With bw = x2 - x1, bh = y2 - y1 and k = (0.125, 0.375, 0.625, 0.875):
  no descriptor   a row whose id is not >= 0 (a NaN is not), or with a coordinate that is not finite: all zeros
  sample grid     cx_i = (x1 + bw * k_i) * (1 / stride) - 0.5; then cx = cx if cx >= 0 else 0 (a NaN becomes 0) and
                  cx = cx if cx <= Wf - 1 else Wf - 1; x0 = min(floor(cx), max(Wf - 2, 0)), x1i = min(x0 + 1, Wf - 1),
                  ax = cx - x0; y alike.  Degenerate and inverted boxes get no special case.
  sample          per channel t = f[y0,x0] + ax * (f[y0,x1i] - f[y0,x0]), u the same on row y1i, v = t + ay * (u - t)
  pool            the 16 samples summed one after the other, y outer and x inner, from the first; then * 0.0625
  centre          m = hsum(p) / C, hsum the halving sum p[:n/2] + p[n/2:n] until one element is left; d = p - m
  quantise        a = max |d| (a NaN travels); a == 0 or not finite: no descriptor; else q = int8(rint((d / a) * 127)), ties to
                  even
Image b reads map map_index[b] (b itself without one), cut to [0, S).

`app_sort_host` is sort.sort_host with the cost of a cell replaced (the filter, the IoU, the frame step's order and
mot_metric.assign_host are imported, not restated).  For candidate row i with descriptor e_i and active track k with descriptor
g_k - that of the track's most recent matched row that had one, the row that started it counts - with dot, na, nb the exact
integer dot product and squared norms:
  has    = na > 0 and nb > 0                       a zero vector is no descriptor
  cos_q  = 0 when dot <= 0 or not has, else int(floor(float64(dot) * 2**20 / sqrt(float64(na) * float64(nb)))): float64
           operations, each correctly rounded; the three integers are exact in float64
  adm    = same class and iou >= sigma_iou         sort.py's rule and arithmetic
  near   = same class and iou >= sigma_prox
  app    = near and has and cos_q >= int(float32(sigma_app) * float32(2**20))
  the cell is admissible iff adm or app and costs 2**20 - max(iou_q if adm else 0, cos_q if app else 0)
So appearance can admit a pair that geometry alone would refuse, but only in the prediction's neighbourhood, and among the
admissible pairs the larger of the two similarities decides.  With `emb` all zero the result is sort_host's bit for bit.

Stated departures: no gallery and no moving average (DeepSORT and JDE keep one), no Mahalanobis gate; sigma_app = 0.8 and
sigma_prox = 0.1 are provisional defaults, not tuned.

This module imports NumPy only.
"""
import numpy as np

from .mot_metric import DUMMY_COST, FORBIDDEN, Q_ONE, assign_host
from .seq_nms import _clips, iou_matrix
from .sort import _KEYS, kf_box, kf_cat, kf_predict, kf_start, kf_take, kf_update, measure, new_state, online_rows
from .track import check_params

_F = np.float32
GRID = (0.125, 0.375, 0.625, 0.875)
LEVELS = {8: 0, 16: 1, 32: 2}                      # the stride of a route tensor -> its place in ROUTE_TENSORS
MIN_C, MAX_C, MAX_ROWS = 8, 1024, 128
APP_DEFAULTS = dict(sigma_app=0.8, sigma_prox=0.1)
OPTION_DEFAULTS = dict(level=8, keep_maps=False, **APP_DEFAULTS)


# ------------------------------------------------------------------ the descriptor
def hsum(p):
    """the halving sum along the last axis (a power of two long): p[:n/2] + p[n/2:n] until one element is left"""
    p = np.asarray(p)
    with np.errstate(all="ignore"):
        while p.shape[-1] > 1:
            h = p.shape[-1] // 2
            p = p[..., :h] + p[..., h:]
    return p[..., 0]


def check_embed_shape(C, stride, who):
    if isinstance(C, bool) or int(C) != C or not MIN_C <= int(C) <= MAX_C or int(C) & (int(C) - 1):
        raise ValueError("%s: C must be a power of two in [%d, %d], got %r" % (who, MIN_C, MAX_C, C))
    if isinstance(stride, bool) or stride not in LEVELS:
        raise ValueError("%s: stride must be 8, 16 or 32, got %r" % (who, stride))
    return int(C), int(stride)


def _axis(lo, side, inv, n):
    """the 4 sample positions along one axis of K rows: (i0, i1 (K,4) int64, a (K,4) float32)"""
    k = np.array(GRID, dtype=_F)
    with np.errstate(all="ignore"):
        c = (lo[:, None] + side[:, None] * k[None, :]) * inv - _F(0.5)
        c = np.where(c >= _F(0), c, _F(0))
        c = np.where(c <= _F(n - 1), c, _F(n - 1))
    i0 = np.minimum(np.floor(c).astype(np.int64), max(n - 2, 0))
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, c - i0.astype(_F)


def embed_host(fmap, ids, bboxes, stride, map_index=None):
    """fmap (S,Hf,Wf,C) float32 (a bf16 map is upcast first, exactly), ids (B,N[,1]), bboxes (B,N,4) in network-input pixels ->
    emb (B,N,C) int8: the module's definition.  Image b reads map map_index[b], or map b, cut to [0, S)."""
    fmap = np.asarray(fmap, dtype=_F)
    bboxes = np.asarray(bboxes, dtype=_F)
    if fmap.ndim != 4 or bboxes.ndim != 3 or bboxes.shape[2] != 4:
        raise ValueError("embed_host: expected fmap (S,Hf,Wf,C) and bboxes (B,N,4), got %r %r" % (fmap.shape, bboxes.shape))
    S, Hf, Wf, C = fmap.shape
    C, stride = check_embed_shape(C, stride, "embed_host")
    B, N = bboxes.shape[0], bboxes.shape[1]
    ids = np.asarray(ids, dtype=_F)
    if ids.size != B * N or S < 1 or Hf < 1 or Wf < 1:
        raise ValueError("embed_host: expected ids (B,N[,1]) and a map of at least one cell, got %r %r" % (ids.shape, fmap.shape))
    ids = ids.reshape(B, N)
    mi = np.arange(B) if map_index is None else np.asarray(map_index).reshape(-1).astype(np.int64)
    if mi.size != B:
        raise ValueError("embed_host: map_index must hold B=%d entries, got %d" % (B, mi.size))
    mi = np.clip(mi, 0, S - 1)
    emb = np.zeros((B, N, C), dtype=np.int8)
    inv = _F(1.0) / _F(stride)
    with np.errstate(all="ignore"):
        ok = (ids >= 0) & np.isfinite(bboxes).all(axis=2)
        for b in range(B):
            rows = np.nonzero(ok[b])[0]
            if not len(rows):
                continue
            f = fmap[mi[b]]
            bx = bboxes[b, rows]
            x0, x1, ax = _axis(bx[:, 0], bx[:, 2] - bx[:, 0], inv, Wf)
            y0, y1, ay = _axis(bx[:, 1], bx[:, 3] - bx[:, 1], inv, Hf)
            acc = None
            for iy in range(4):
                for ix in range(4):
                    a, c = ax[:, ix, None], ay[:, iy, None]
                    f00, f01 = f[y0[:, iy], x0[:, ix]], f[y0[:, iy], x1[:, ix]]
                    f10, f11 = f[y1[:, iy], x0[:, ix]], f[y1[:, iy], x1[:, ix]]
                    t = f00 + a * (f01 - f00)
                    u = f10 + a * (f11 - f10)
                    v = t + c * (u - t)
                    acc = v if acc is None else acc + v
            p = acc * _F(0.0625)
            d = p - (hsum(p) / _F(C))[:, None]
            a = np.max(np.abs(d), axis=1)                                              # a NaN travels
            good = np.isfinite(a) & (a != 0)
            q = np.rint((d / a[:, None]) * _F(127))
            emb[b, rows[good]] = q[good].astype(np.int8)
    return emb


# ------------------------------------------------------------------ the cosine of a cell
def cos_q_matrix(e, g):
    """e (R,C), g (K,C) int8 -> (cos_q (R,K) int64, has (R,K) bool): the module's definition"""
    e, g = np.asarray(e).astype(np.float64), np.asarray(g).astype(np.float64)           # integers below 2**53: every sum is exact
    dot = (e @ g.T).astype(np.int64)
    na, nb = (e * e).sum(axis=1).astype(np.int64)[:, None], (g * g).sum(axis=1).astype(np.int64)[None, :]
    has = (na > 0) & (nb > 0)
    on = has & (dot > 0)
    den = np.sqrt(np.where(on, na, 1).astype(np.float64) * np.where(on, nb, 1).astype(np.float64))
    c = np.floor(np.where(on, dot, 0).astype(np.float64) * np.float64(Q_ONE) / den).astype(np.int64)
    return np.where(on, c, 0), has


def cos_q(e, g):
    """two int8 vectors -> cos_q, an int"""
    return int(cos_q_matrix(np.asarray(e).reshape(1, -1), np.asarray(g).reshape(1, -1))[0][0, 0])


def check_app_params(sigma_app=0.8, sigma_prox=0.1, who="app_sort_host"):
    """(sigma_app, sigma_prox) as float32, both in [0, 1]; a ValueError names the argument that is not usable"""
    out = []
    for name, v in (("sigma_app", sigma_app), ("sigma_prox", sigma_prox)):
        try:
            f = _F(v)
        except (TypeError, ValueError):
            raise ValueError("%s: %s must be a number, got %r" % (who, name, v))
        if isinstance(v, bool) or not _F(0) <= f <= _F(1):
            raise ValueError("%s: %s must be a number in [0, 1], got %r" % (who, name, v))
        out.append(f)
    return tuple(out)


def app_threshold(sigma_app):
    return int(_F(sigma_app) * _F(Q_ONE))


def association_cost_app(pred_boxes, track_cls, track_emb, row_boxes, row_cls, row_emb, sigma_iou, sigma_prox, sigma_app):
    """sort.association_cost with the fused cell: (R, K + R) int64"""
    R, K = len(row_cls), len(track_cls)
    cost = np.full((R, K + R), FORBIDDEN, dtype=np.int64)
    iou = iou_matrix(pred_boxes, row_boxes).T                                          # (R, K), track side first
    with np.errstate(invalid="ignore"):
        same = np.asarray(row_cls)[:, None] == np.asarray(track_cls)[None, :]
        adm = same & (iou >= _F(sigma_iou))
        near = same & (iou >= _F(sigma_prox))
    iou_q = (np.where(adm, iou, _F(0)) * _F(Q_ONE)).astype(np.int64)                    # exact in float32
    cq, has = cos_q_matrix(row_emb, track_emb)
    app = near & has & (cq >= app_threshold(sigma_app))
    sim = np.maximum(np.where(adm, iou_q, 0), np.where(app, cq, 0))
    cost[:, :K] = np.where(adm | app, Q_ONE - sim, FORBIDDEN)
    cost[np.arange(R), K + np.arange(R)] = DUMMY_COST
    return cost


def new_app_state():
    """sort.new_state() and 'desc': per active track the flat row (frame * N + row) of its descriptor, -1 without one"""
    return dict(new_state(), desc=np.zeros(0, np.int64))


def app_sort_step(state, cls, sc, boxes, emb_flat, first, sigma_iou=0.3, max_age=1, sigma_app=0.8, sigma_prox=0.1):
    """sort.sort_step with the fused cost.  emb_flat (F*N, C) int8: every row's descriptor; first: the flat index of this
    frame's row 0.  -> sort_step's six results."""
    si = _F(sigma_iou)
    cls, sc, boxes = np.asarray(cls), np.asarray(sc, dtype=_F), np.asarray(boxes, dtype=_F)
    N = len(cls)
    Cn = emb_flat.shape[1]
    track = np.full(N, -1, dtype=np.int64)
    tlen = np.zeros(N, dtype=np.int64)
    tscore = np.full(N, -1, dtype=_F)
    tbox = np.full((N, 4), -1, dtype=_F)
    K = len(state["id"])
    kf = kf_predict(state["kf"])                                                       # 1
    rows = np.nonzero(cls >= 0)[0]
    row_emb = emb_flat[first + rows]
    row_has = (row_emb.astype(np.int64) ** 2).sum(axis=1) > 0
    col = np.full(len(rows), -1, dtype=np.int64)
    if len(rows) and K:                                                                # 2
        t_emb = np.where((state["desc"] >= 0)[:, None], emb_flat[np.maximum(state["desc"], 0)], np.zeros((1, Cn), np.int8))
        col = assign_host(association_cost_app(kf_box(kf), state["cls"], t_emb, boxes[rows], cls[rows], row_emb, si, sigma_prox,
                                               sigma_app))
        col = np.where(col < K, col, -1)
    hit = np.zeros(K, dtype=bool)                                                      # 3
    t_id, t_len, t_max, t_desc = state["id"].copy(), state["len"].copy(), state["max"].copy(), state["desc"].copy()
    m = col >= 0
    if m.any():
        k, j = col[m], rows[m]
        hit[k] = True
        upd = kf_update(kf_take(kf, k), measure(boxes[j]))
        for key in _KEYS:
            kf[key][k] = upd[key]
        t_len[k] += 1
        t_max[k] = np.where(sc[j] > t_max[k], sc[j], t_max[k])
        t_desc[k] = np.where(row_has[m], first + j, t_desc[k])
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
               len=np.concatenate([t_len[live], np.ones(len(fresh), np.int64)]), max=np.concatenate([t_max[live], sc[fresh]]),
               desc=np.concatenate([t_desc[live], np.where(row_has[~m], first + fresh, -1).astype(np.int64)]))
    return out, track, tlen, tscore, tbox, int(K - live.sum())


def app_sort_host(ids, scores, bboxes, emb, clip_start=None, num_class=None, sigma_l=0.0, sigma_h=0.5, sigma_iou=0.3, t_min=2,
                  max_age=1, sigma_app=0.8, sigma_prox=0.1, stats=None):
    """ids (F,N[,1]), scores (F,N[,1]), bboxes (F,N,4), emb (F,N,C) int8 -> sort_host's (track, tlen, tscore, tbox), linked
    with the fused cost of the module's head.  `stats` as sort_host's."""
    sl, sh, si, t_min, max_age = check_params(sigma_l, sigma_h, sigma_iou, t_min, max_age, "app_sort_host")
    sa, sp = check_app_params(sigma_app, sigma_prox, "app_sort_host")
    sc, cls, bboxes = online_rows(ids, scores, bboxes, num_class, sl)
    F, N = sc.shape
    emb = np.asarray(emb)
    if emb.dtype != np.int8 or emb.ndim != 3 or emb.shape[:2] != (F, N):
        raise ValueError("app_sort_host: emb must be (F,N,C) = (%d,%d,C) int8, got %s %r" % (F, N, emb.dtype, emb.shape))
    emb_flat = emb.reshape(F * N, emb.shape[2])
    track = np.full((F, N), -1, dtype=np.int32)
    tlen = np.zeros((F, N), dtype=np.int32)
    tscore = np.full((F, N), -1, dtype=_F)
    tbox = np.full((F, N, 4), -1, dtype=_F)
    n_active = np.zeros(F, dtype=np.int64)
    n_closed = np.zeros(F, dtype=np.int64)
    kept_per_clip = []
    for t0, t1 in _clips(clip_start, F):
        state = new_app_state()
        local = np.full((t1 - t0, N), -1, dtype=np.int64)
        length = np.zeros((t1 - t0) * N, dtype=np.int32)
        best = np.full((t1 - t0) * N, -1, dtype=_F)
        for t in range(t0, t1):
            state, tr, ln, mx, tbox[t], n_closed[t] = app_sort_step(state, cls[t], sc[t], bboxes[t], emb_flat, t * N, si, max_age,
                                                                    sa, sp)
            on = tr >= 0
            local[t - t0] = tr
            length[tr[on]], best[tr[on]] = ln[on], mx[on]
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


# ------------------------------------------------------------------ the option of detect_video
def split_appearance(track):
    """The `appearance` key of a `track=` option, which track.parse_option does not know: track -> (track without the key, its
    value or None)"""
    if not isinstance(track, dict) or "appearance" not in track:
        return track, None
    rest = dict(track)
    return rest, rest.pop("appearance")


def parse_option(appearance, method, seq_nms, who):
    """The `appearance` key of `who`'s track option (detect_video): None / False -> None; True or {'level': 8|16|32,
    'sigma_app':, 'sigma_prox':, 'keep_maps':} -> the dict with the defaults filled in.  method: the track method; seq_nms: the
    call has Seq-NMS on.  A ValueError names what is not usable."""
    if appearance is None or appearance is False:
        return None
    kw = {} if appearance is True else dict(appearance)
    unknown = sorted(set(kw) - set(OPTION_DEFAULTS))
    if unknown:
        raise ValueError("%s: appearance takes level, sigma_app, sigma_prox and keep_maps, got %s" % (who, ", ".join(unknown)))
    kw = dict(OPTION_DEFAULTS, **kw)
    if isinstance(kw["level"], bool) or kw["level"] not in LEVELS:
        raise ValueError("%s: appearance level must be 8, 16 or 32, got %r" % (who, kw["level"]))
    check_app_params(kw["sigma_app"], kw["sigma_prox"], who + " with appearance")
    if method != "sort":
        raise ValueError("%s: appearance needs track method 'sort', got %r: the fused cost is defined for SORT's association alone"
                         % (who, method))
    if seq_nms:
        raise ValueError("%s: appearance beside seq_nms is not taken: Seq-NMS permutes the rows ahead of the tracker" % who)
    return kw
