"""The HOTA tracking metric (Luiten et al., "HOTA: A Higher Order Metric for Evaluating Multi-Object Tracking", IJCV 2021) of the
tracks that --track, the live sessions and --tubelet produce, in the form the paper's evaluation code takes: ONE assignment per
frame on `global alignment score x similarity`, thresholded afterwards at every alpha.  The definition.  That evaluation code
was not available to generate a fixture: its rules are restated here with unpinned parity, as DESIGN.md 26 does for pycocotools.

`hota_match_host` is the normative per-frame matching: NumPy, float32 where boxes meet (seq_nms.iou_matrix),
integers everywhere after it - so a device may add in any order and still be equal bit for bit.  The device entry point
vd_hota_match (viddet_amd/csrc/vd_hota_eval.hip, `ops.hota_match`) equals it on all three outputs.  `hota_summary` is the host
accumulation that both paths share, in float64.

Per clip [t0, t1):
  1. candidates: mot_metric's rule 1 on both sides - the first eligible row of an id in its frame stands; ground-truth ids lie
     in [0, 1024); a prediction with track -1 is not tracker output.
  2. similarity: S[g, j] the float32 IoU, taken as 0 unless both rows are candidates and (agnostic or equal classes), a NaN as
     0; q = int(floor(S * 2**20)) (exact in float32); a pair is admissible iff q > 0.
  3. pass one, over all frames: with rq, cq the row and column sums of q in the frame, n = (q << 20) // (rq[g] + cq[j] - q) per
     admissible pair - the paper's normalised similarity in units of 2**-20 - is added into pm[a, p] of the pair's ground-truth
     id a and prediction id p; cg[a], cp[p] count the candidate rows of an id.
  4. alignment: A[a, p] = (pm << 20) // (((cg[a] + cp[p]) << 20) - pm), 0 where pm is 0.
  5. pass two, every frame on its own: the score of an admissible pair is s = (A[a, p] * q) >> 20, in [0, 2**20].  rows = the
     ground-truth candidates in row order, columns = the prediction candidates in row order, then one dummy per row; an
     admissible pair costs 2**20 - s, a row's own dummy 2**20 (a match of score zero), everything else is forbidden;
     `mot_metric.assign_host` gives the matching of the largest score sum, with its tie rules.  Entered only when both pools are
     non-empty.
  6. records: match[t, g] the prediction row, -1 an unmatched candidate, -2 no candidate; msim the pair's float32 IoU, else 0;
     mscore the pair's s, else 0.  Frames that no clip covers get -2 / 0 / 0.

Stated departures from the evaluation code: a zero denominator gives 0.0 (it gives LocA 1.0 there); classes must
agree unless `agnostic` and the counts are pooled over classes (it scores each class apart and averages); the similarity and
the scores are quantised to 2**-20; the alpha test is the plain float32 `>=`, with no epsilon.

This module imports NumPy only.
"""
import numpy as np

from .mot_metric import (FORBIDDEN, MAX_GT_ID, Q_ONE, MOTMetric, _check_inputs, assign_host, check_dataset, first_of_id, masked_track,
                         pack_clips)
from .seq_nms import _clips, iou_matrix, row_classes

_F = np.float32
MAX_FRAMES = 1 << 22                              # pm << 20 stays inside int64
ALPHAS = np.array([_F(0.05 * k) for k in range(1, 20)], dtype=_F)
PER_ALPHA = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")    # reported as the mean over ALPHAS
AT_ZERO = ("HOTA(0)", "LocA(0)", "HOTALocA(0)")                                      # at the first alpha, 0.05
RATES = PER_ALPHA + AT_ZERO
COUNTS = ("frames", "gt_tracks", "pred_tracks", "GT", "PRED")


def hota_match_host(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, clip_start=None, num_class=None, agnostic=False):
    """gt_boxes (F,G,4), gt_cls (F,G), gt_id (F,G), ids (F,N[,1]), scores (F,N[,1]), bboxes (F,N,4), track (F,N) ->
    (match (F,G) int32, msim (F,G) float32, mscore (F,G) int32), as the module's head defines them."""
    gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track = _check_inputs(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track,
                                                                        "hota_match_host")
    F, G, N = gt_boxes.shape[0], gt_boxes.shape[1], bboxes.shape[1]
    if F > MAX_FRAMES:
        raise ValueError("hota_match_host: F=%d frames, at most %d are taken" % (F, MAX_FRAMES))
    pcls = row_classes(ids, scores, num_class)
    match = np.full((F, G), -2, dtype=np.int32)
    msim = np.zeros((F, G), dtype=_F)
    mscore = np.zeros((F, G), dtype=np.int32)
    for t0, t1 in _clips(clip_start, F):
        if t1 == t0:
            continue
        gc = np.stack([first_of_id((gt_cls[t] >= 0) & (gt_id[t] >= 0) & (gt_id[t] < MAX_GT_ID), gt_id[t]) for t in range(t0, t1)])
        pc = np.stack([first_of_id((pcls[t] >= 0) & (track[t] >= 0), track[t]) for t in range(t0, t1)])
        ga, gp = np.unique(gt_id[t0:t1][gc]), np.unique(track[t0:t1][pc])          # the clip's ids, dense by their rank
        ai, pi = np.searchsorted(ga, gt_id[t0:t1]), np.searchsorted(gp, track[t0:t1])   # read on candidate rows only
        pm = np.zeros((len(ga), len(gp)), dtype=np.int64)
        cg, cp = np.zeros(len(ga), dtype=np.int64), np.zeros(len(gp), dtype=np.int64)
        sims, qs = [], []
        # 3. pass one
        for k, t in enumerate(range(t0, t1)):
            S = iou_matrix(gt_boxes[t], bboxes[t])
            ok = gc[k][:, None] & pc[k][None, :]
            if not agnostic:
                ok &= gt_cls[t][:, None] == pcls[t][None, :]
            with np.errstate(invalid="ignore"):
                S = np.where(ok & (S > 0), S, _F(0))
            q = np.floor(S * _F(Q_ONE)).astype(np.int64)
            rq, cq = q.sum(axis=1), q.sum(axis=0)
            g, j = np.nonzero(q > 0)
            np.add.at(pm, (ai[k][g], pi[k][j]), (q[g, j] << 20) // (rq[g] + cq[j] - q[g, j]))
            np.add.at(cg, ai[k][gc[k]], 1)
            np.add.at(cp, pi[k][pc[k]], 1)
            sims.append(S)
            qs.append(q)
        # 4. alignment
        den = ((cg[:, None] + cp[None, :]) << 20) - pm
        A = np.where(pm > 0, (pm << 20) // np.where(pm > 0, den, 1), 0)
        # 5. pass two, 6. records
        for k, t in enumerate(range(t0, t1)):
            m = np.where(gc[k], -1, -2).astype(np.int64)
            rg, cpx = np.nonzero(gc[k])[0], np.nonzero(pc[k])[0]
            if len(rg) and len(cpx):
                q = qs[k][np.ix_(rg, cpx)]
                s = (A[np.ix_(ai[k][rg], pi[k][cpx])] * q) >> 20
                cost = np.full((len(rg), len(cpx) + len(rg)), FORBIDDEN, dtype=np.int64)
                cost[:, :len(cpx)] = np.where(q > 0, Q_ONE - s, FORBIDDEN)
                cost[np.arange(len(rg)), len(cpx) + np.arange(len(rg))] = Q_ONE
                col = assign_host(cost)
                hit = col < len(cpx)
                m[rg[hit]] = cpx[col[hit]]
                msim[t, rg[hit]] = sims[k][rg[hit], cpx[col[hit]]]
                mscore[t, rg[hit]] = s[np.nonzero(hit)[0], col[hit]]
            match[t] = m
    return match, msim, mscore


def clip_tables(records, gt_id, track, t0, t1):
    """The id tables of the clip [t0, t1) that hota_summary counts on: (ga, gp, cg, cp, a, p, sim) - the clip's ground-truth ids
    and prediction ids (ascending), the candidate rows of each, and per matched pair in frame, row order the index of its
    ground-truth id in ga, of its prediction id in gp and its msim.  track carries -1 on every row that is no detection."""
    match, msim = np.asarray(records[0]), np.asarray(records[1])
    m = match[t0:t1]
    pcand = np.stack([first_of_id(track[t] >= 0, track[t]) for t in range(t0, t1)]) if t1 > t0 else np.zeros((0, track.shape[1]), bool)
    ga, cg = np.unique(gt_id[t0:t1][m != -2], return_counts=True)
    gp, cp = np.unique(track[t0:t1][pcand], return_counts=True)
    ft, fg = np.nonzero(m >= 0)                                       # frame, row order
    fj = m[ft, fg]
    if len(ft) and (fj.max() >= track.shape[1] or not pcand[ft, fj].all()):
        raise ValueError("hota_summary: the records match a row that is no candidate of the track table")
    a, p = np.searchsorted(ga, gt_id[t0:t1][ft, fg]), np.searchsorted(gp, track[t0:t1][ft, fj])
    return ga, gp, cg.astype(np.int64), cp.astype(np.int64), a, p, msim[t0:t1][ft, fg]


def _rate(num, den):
    return float(num) / float(den) if den else 0.0


def _finish(c):
    """the rates of one block: the per-alpha lists from the counts and sums it holds, their means, the figures at alpha 0.05"""
    K = len(ALPHAS)
    c["FN"], c["FP"] = [c["GT"] - tp for tp in c["TP"]], [c["PRED"] - tp for tp in c["TP"]]
    per = {}
    per["DetA"] = [_rate(c["TP"][k], c["TP"][k] + c["FN"][k] + c["FP"][k]) for k in range(K)]
    per["DetRe"] = [_rate(c["TP"][k], c["TP"][k] + c["FN"][k]) for k in range(K)]
    per["DetPr"] = [_rate(c["TP"][k], c["TP"][k] + c["FP"][k]) for k in range(K)]
    for name in ("AssA", "AssRe", "AssPr", "LocA"):
        per[name] = [_rate(c["_" + name][k], c["TP"][k]) for k in range(K)]
    per["HOTA"] = [float(np.sqrt(per["DetA"][k] * per["AssA"][k])) for k in range(K)]
    for name in PER_ALPHA:
        c[name + "@"] = per[name]
        c[name] = float(np.sum(np.asarray(per[name], dtype=np.float64)) / K)
    c["HOTA(0)"], c["LocA(0)"] = per["HOTA"][0], per["LocA"][0]
    c["HOTALocA(0)"] = c["HOTA(0)"] * c["LocA(0)"]
    for name in ("AssA", "AssRe", "AssPr", "LocA"):
        del c["_" + name]
    return c


def hota_summary(records, gt_id, track, clip_start=None):
    """records = (match, msim, mscore) of hota_match_host / ops.hota_match, gt_id (F,G) and track (F,N) the id tables the
    matching read - track with -1 on every row that is no detection (mot_metric.masked_track) - -> {'clips': [per clip],
    'all': overall}, each a dict of
      frames, gt_tracks, pred_tracks, GT, PRED   integers: the candidate rows (match != -2; the first row of a track id >= 0 in
                                                 its frame) and the ids they carry
      TP, FN, FP                                 lists, one integer per alpha of ALPHAS: a matched pair is a TP at alpha iff
                                                 msim >= alpha (float32); FN = GT - TP, FP = PRED - TP
      <name>@ for name in PER_ALPHA              lists, one float per alpha: DetA = TP / (TP + FN + FP), DetRe, DetPr; with mc[a, p]
                                                 the TPs of an id pair, AssA = sum(mc * mc / max(1, cg + cp - mc)) / TP, AssRe
                                                 over cg, AssPr over cp; LocA = sum(msim of the TPs) / TP, the sum in frame, row
                                                 order; HOTA = sqrt(DetA * AssA)
      <name> for name in PER_ALPHA               their means over the 19 alphas
      HOTA(0), LocA(0), HOTALocA(0)              at alpha 0.05, the last their product
    'all' combines the clips as the evaluation code does: the counts summed, AssA / AssRe / AssPr / LocA the clips' weighted by
    each clip's TP at that alpha.  A zero denominator gives 0.0."""
    match, msim, mscore = [np.asarray(a) for a in records]
    gt_id, track = np.asarray(gt_id).astype(np.int64), np.asarray(track).astype(np.int64)
    F, G = match.shape
    if msim.shape != (F, G) or mscore.shape != (F, G) or gt_id.shape != (F, G) or track.ndim != 2 or track.shape[0] != F:
        raise ValueError("hota_summary: the records and the id tables do not fit: %r %r %r %r %r"
                         % (match.shape, msim.shape, mscore.shape, gt_id.shape, track.shape))
    K = len(ALPHAS)
    sums = ("_AssA", "_AssRe", "_AssPr", "_LocA")
    total = dict.fromkeys(COUNTS, 0)
    total["TP"] = [0] * K
    for k in sums:
        total[k] = [0.0] * K
    clips = []
    for t0, t1 in _clips(clip_start, F):
        ga, gp, cg, cp, a, p, sim = clip_tables((match, msim), gt_id, track, t0, t1)
        c = dict(frames=t1 - t0, gt_tracks=len(ga), pred_tracks=len(gp), GT=int(cg.sum()), PRED=int(cp.sum()), TP=[])
        for k in sums:
            c[k] = []
        for alpha in ALPHAS:
            sel = sim >= alpha
            tp = int(sel.sum())
            mc = np.zeros((len(ga), len(gp)), dtype=np.int64)
            np.add.at(mc, (a[sel], p[sel]), 1)
            ia, ip = np.nonzero(mc)
            n = mc[ia, ip]
            sq = (n * n).astype(np.float64)
            c["TP"].append(tp)
            c["_AssA"].append(float(np.sum(sq / np.maximum(1, cg[ia] + cp[ip] - n))))
            c["_AssRe"].append(float(np.sum(sq / np.maximum(1, cg[ia]))))
            c["_AssPr"].append(float(np.sum(sq / np.maximum(1, cp[ip]))))
            vals = sim[sel].astype(np.float64)
            c["_LocA"].append(float(np.cumsum(vals)[-1]) if len(vals) else 0.0)      # one after the other
        for k in COUNTS:
            total[k] += c[k]
        for k in range(K):
            total["TP"][k] += c["TP"][k]
            # AssA_c * TP_c, the clip's weight; LocA likewise, which is the sum over its TPs
            for name in sums:
                total[name][k] += _rate(c[name][k], c["TP"][k]) * c["TP"][k]
        clips.append(_finish(c))
    return dict(clips=clips, all=_finish(total))


def format_summary(c):
    """(names, values) of one block of figures, a `name value` line each: the rates as '{:.4f}', the counts as integers"""
    names = list(RATES) + list(COUNTS)
    return names, ["{:.4f}".format(c[k]) for k in RATES] + [str(int(c[k])) for k in COUNTS]


class HOTAMetric(MOTMetric):
    """Collects the tracked prediction rows of every image in update() (MOTMetric's); get() matches them against the dataset's
    labels clip by clip and returns the overall figures as (names, values); `summary` keeps hota_summary's result (per clip
    too) of the last get()."""

    def __init__(self, dataset, agnostic=False):
        check_dataset(dataset)
        self.name = "HOTA"
        self.dataset = dataset
        self._agnostic = bool(agnostic)
        self._results = {}
        self.summary = None

    def _match(self, arrays, clip_start):
        return hota_match_host(*arrays, clip_start=clip_start, num_class=self._num_class(), agnostic=self._agnostic)

    def get(self):
        arrays, cs = pack_clips(self.dataset, self._results)
        records = self._match(arrays, cs)
        self.summary = hota_summary(records, arrays[2], masked_track(arrays[3], arrays[4], arrays[6], self._num_class()), cs)
        return format_summary(self.summary["all"])
