"""The closed forms of the HOTA metric's tests (CPU and GPU): small clips whose outputs are written out by hand."""
import math

import numpy as np

from tests.mot_cases import A, A5, A8, B, C, build

ONE = 1 << 20                                                  # a score of 1 in mscore's units
THIRD = ONE // 3                                               # floor(2**20 / 3) = 349525
NAN_BOX = (float("nan"), 0, 10, 10)
INF_BOX = (0, 0, float("inf"), float("inf"))
FLAT_BOX = (5, 5, 5, 5)                                         # zero area
K = 19                                                         # alphas
TOL = 1e-12                                                    # on a rate: the float64 roundings of a mean over 19 terms


def closed_forms():
    """[(name, arrays, kwargs, expect)]: expect holds match / msim / mscore as nested lists, and `all` (and `clips`), the figures
    of hota_summary that the case is about; a list stands for a per-alpha list"""
    out = []
    ones = dict(HOTA=1.0, DetA=1.0, AssA=1.0, DetRe=1.0, DetPr=1.0, AssRe=1.0, AssPr=1.0, LocA=1.0)
    ones.update({"HOTA(0)": 1.0, "LocA(0)": 1.0, "HOTALocA(0)": 1.0})
    # a perfect tracker: q = 2^20, n = 2^40 / 2^20, pm = 4 * 2^20, A = 4 * 2^40 / ((8 - 4) * 2^20) = 2^20: every figure 1
    gt = [[(A, 0, 0), (B, 1, 1)]] * 4
    pred = [[(B, 1, 0.9, 9), (A, 0, 0.9, 5)]] * 4
    out.append(("perfect", build(gt, pred), dict(num_class=2), dict(
        match=[[1, 0]] * 4, msim=[[1.0, 1.0]] * 4, mscore=[[ONE, ONE]] * 4,
        all=dict(ones, frames=4, gt_tracks=2, pred_tracks=2, GT=8, PRED=8, TP=[8] * K, FN=[0] * K, FP=[0] * K))))
    # one ground-truth track of 6 frames answered by two prediction tracks of 3: pm = 3 * 2^20, cg = 6, cp = 3,
    # A = 3 / (9 - 3) = 1/2 exactly; mc = 3 for either pair: AssA = 2 * (9 / (6 + 3 - 3)) / 6 = 1/2, AssRe = 2 * (9 / 6) / 6 = 1/2,
    # AssPr = 2 * (9 / 3) / 6 = 1; DetA = 6 / 6
    gt = [[(A, 0, 0)]] * 6
    pred = [[(A, 0, 0.9, 1)]] * 3 + [[(A, 0, 0.9, 2)]] * 3
    out.append(("one_track_answered_by_two", build(gt, pred), {}, dict(
        match=[[0]] * 6, msim=[[1.0]] * 6, mscore=[[ONE // 2]] * 6,
        all=dict(DetA=1.0, AssA=0.5, HOTA=math.sqrt(0.5), AssRe=0.5, AssPr=1.0, LocA=1.0, DetRe=1.0, DetPr=1.0, GT=6, PRED=6,
                 gt_tracks=1, pred_tracks=2, TP=[6] * K, **{"HOTA@": [math.sqrt(0.5)] * K, "HOTA(0)": math.sqrt(0.5)}))))
    # one prediction track on every second frame: TP = 3, FN = 3, FP = 0: DetA = 3 / 6; mc = 3, cg = 6, cp = 3:
    # AssA = (9 / 6) / 3 = 1/2; HOTA = sqrt(1/4); the alignment is 3 / (9 - 3) again
    pred = [[(A, 0, 0.9, 1)], []] * 3
    out.append(("every_second_frame", build(gt, pred), {}, dict(
        match=[[0], [-1]] * 3, msim=[[1.0], [0.0]] * 3, mscore=[[ONE // 2], [0]] * 3,
        all=dict(DetA=0.5, AssA=0.5, HOTA=0.5, DetRe=0.5, DetPr=1.0, AssRe=0.5, AssPr=1.0, LocA=1.0, GT=6, PRED=3, TP=[3] * K,
                 FN=[3] * K, FP=[0] * K))))
    # a pair at IoU exactly 0.5: float32(0.05 * 10) is 0.5 (0.05 * 10 rounds to 0.5 in float64 already), so the pair is a TP
    # at the alphas 0.05 .. 0.50 - ten of them - and at none above; alone in its clip its alignment is 1 and its score q
    tp = [1] * 10 + [0] * 9
    out.append(("iou_exactly_one_half", build([[(A, 0, 0)]], [[(A5, 0, 0.9, 0)]]), {}, dict(
        match=[[0]], msim=[[0.5]], mscore=[[ONE // 2]],
        all=dict(TP=tp, FN=[1 - x for x in tp], FP=[1 - x for x in tp], DetA=10 / 19, AssA=10 / 19, HOTA=10 / 19, LocA=5 / 19,
                 **{"DetA@": [float(x) for x in tp], "LocA@": [0.5 * x for x in tp], "HOTA(0)": 1.0, "LocA(0)": 0.5,
                    "HOTALocA(0)": 0.5}))))
    # two ground-truth tracks whose prediction ids swap half way: no carry-over holds a pair together, every frame is matched
    # by position and the swap stays one.  pm = 3 * 2^20 for all four id pairs, cg = cp = 6: A = 3 / (12 - 3) = 1/3, floored.
    # mc = 3 for all four pairs: AssA = 4 * (9 / (6 + 6 - 3)) / 12 = 1/3, AssRe = AssPr = 4 * (9 / 6) / 12 = 1/2; DetA = 1
    gt = [[(A, 0, 0), (B, 0, 1)]] * 6
    pred = [[(A, 0, 0.9, 7), (B, 0, 0.9, 8)]] * 3 + [[(A, 0, 0.9, 8), (B, 0, 0.9, 7)]] * 3
    out.append(("swap_half_way", build(gt, pred), {}, dict(
        match=[[0, 1]] * 6, msim=[[1.0, 1.0]] * 6, mscore=[[THIRD, THIRD]] * 6,
        all=dict(DetA=1.0, AssA=1 / 3, AssRe=0.5, AssPr=0.5, HOTA=math.sqrt(1 / 3), LocA=1.0, TP=[12] * K, gt_tracks=2,
                 pred_tracks=2))))
    # a prediction of another class: no match; agnostic matches it
    arrays = build([[(A, 1, 0)]], [[(A, 0, 0.9, 0)]])
    out.append(("class_mismatch", arrays, dict(num_class=2), dict(
        match=[[-1]], msim=[[0.0]], mscore=[[0]],
        all=dict(GT=1, PRED=1, TP=[0] * K, FN=[1] * K, FP=[1] * K, HOTA=0.0, DetA=0.0, AssA=0.0, LocA=0.0, **{"LocA(0)": 0.0}))))
    out.append(("class_mismatch_agnostic", arrays, dict(num_class=2, agnostic=True), dict(
        match=[[0]], msim=[[1.0]], mscore=[[ONE]], all=dict(ones, GT=1, PRED=1, TP=[1] * K))))
    # a duplicate track id and a duplicate ground-truth id in a frame: the lower row of either stands, the other takes no part
    out.append(("duplicate_ids", build([[(A, 0, 0), (B, 0, 0)]], [[(A, 0, 0.9, 4), (B, 0, 0.9, 4)]]), {}, dict(
        match=[[0, -2]], msim=[[1.0, 0.0]], mscore=[[ONE, 0]], all=dict(ones, GT=1, PRED=1, gt_tracks=1, pred_tracks=1, TP=[1] * K))))
    # rows outside the ids that are taken: ground-truth ids -1 and 1024, a track of -1
    out.append(("id_range", build([[(A, 0, -1), (B, 0, 1023), (C, 0, 1024)]], [[(A, 0, 0.9, 0), (B, 0, 0.9, 1), (C, 0, 0.9, -1)]]), {},
                dict(match=[[-2, 1, -2]], msim=[[0.0, 1.0, 0.0]], mscore=[[0, ONE, 0]],
                     all=dict(GT=1, PRED=2, TP=[1] * K, FP=[1] * K, DetA=0.5, AssA=1.0, HOTA=math.sqrt(0.5), gt_tracks=1, pred_tracks=2))))
    # degenerate boxes on both sides - a NaN box, an infinite box (inf / inf: a NaN, which counts as 0), a zero-area box - are
    # candidates that meet nothing: TP = 1 of GT = PRED = 4: DetA = 1 / (1 + 3 + 3)
    gt = [[(A, 0, 0), (NAN_BOX, 0, 1), (INF_BOX, 0, 2), (FLAT_BOX, 0, 3)]]
    pred = [[(NAN_BOX, 0, 0.9, 1), (INF_BOX, 0, 0.9, 2), (FLAT_BOX, 0, 0.9, 3), (A, 0, 0.9, 0)]]
    out.append(("degenerate_boxes", build(gt, pred), {}, dict(
        match=[[3, -1, -1, -1]], msim=[[1.0, 0.0, 0.0, 0.0]], mscore=[[ONE, 0, 0, 0]],
        all=dict(GT=4, PRED=4, TP=[1] * K, FN=[3] * K, FP=[3] * K, DetA=1 / 7, AssA=1.0, HOTA=math.sqrt(1 / 7), LocA=1.0))))
    # an empty clip between two clips: every figure of it is 0.0, and it weighs nothing in 'all'
    gt = [[(A, 0, 0)]] * 4
    pred = [[(A, 0, 0.9, 5)]] * 4
    empty = dict(dict.fromkeys(ones, 0.0), frames=0, GT=0, PRED=0, gt_tracks=0, pred_tracks=0, TP=[0] * K, FN=[0] * K, FP=[0] * K)
    out.append(("empty_clip_between", build(gt, pred), dict(clip_start=[0, 2, 2, 4]), dict(
        match=[[0]] * 4, mscore=[[ONE]] * 4, all=dict(ones, frames=4, GT=4, PRED=4, gt_tracks=2, pred_tracks=2, TP=[4] * K),
        clips=[dict(ones, frames=2, GT=2), empty, dict(ones, frames=2, GT=2)])))
    # two clips: ids do not leak.  As ONE clip this is one_track_answered_by_two (AssA 1/2, scores 2^19); as two clips either
    # is perfect
    pred = [[(A, 0, 0.9, 5)]] * 2 + [[(A, 0, 0.9, 6)]] * 2
    out.append(("two_clips", build(gt, pred), dict(clip_start=[0, 2, 4]), dict(
        match=[[0]] * 4, mscore=[[ONE]] * 4, all=dict(ones, frames=4, GT=4, PRED=4, gt_tracks=2, pred_tracks=2),
        clips=[dict(ones, frames=2), dict(ones, frames=2)])))
    out.append(("two_clips_as_one", build(gt, pred), {}, dict(
        match=[[0]] * 4, mscore=[[ONE // 2]] * 4, all=dict(AssA=0.5, DetA=1.0, gt_tracks=1, pred_tracks=2))))
    # a tie: two prediction rows on the ground-truth box.  q = 2^20 both, rq = 2 * 2^20, cq = 2^20: n = 2^40 / (2 * 2^20) = 2^19
    # for either; cg = cp = 1: A = 2^39 / (2 * 2^20 - 2^19) = 2^20 / 3, floored; s = A for either.  assign_host, row 0: the
    # slacks are (2^20 - s, 2^20 - s, 2^20) over the two rows and the dummy; the first minimum is column 0, which is free: the
    # lower row.  TP = 1, FP = 1: DetA = 1/2; mc = 1, cg = cp = 1: AssA = 1
    out.append(("tie_to_the_lower_row", build([[(A, 0, 0)]], [[(A, 0, 0.5, 1), (A, 0, 0.9, 2)]]), {}, dict(
        match=[[0]], msim=[[1.0]], mscore=[[THIRD]],
        all=dict(GT=1, PRED=2, TP=[1] * K, FP=[1] * K, FN=[0] * K, DetA=0.5, AssA=1.0, HOTA=math.sqrt(0.5), DetPr=0.5, DetRe=1.0))))
    # a worse box that carries the right id wins over a better box of a new id: frame 2's scores are A[0, 3] * 0.8 against
    # A[0, 9] * 1.  Frame 2: q = (2^20, int(0.8f * 2^20)) - see below -; the alignment of the long pair outweighs the IoU
    gt = [[(A, 0, 0)]] * 3
    pred = [[(A, 0, 0.9, 3)], [(A, 0, 0.9, 3)], [(A, 0, 0.9, 9), (A8, 0, 0.9, 3)]]
    out.append(("alignment_outweighs_iou", build(gt, pred), {}, dict(
        match=[[0], [0], [1]], msim=[[1.0], [1.0], [float(np.float32(0.8))]],
        all=dict(GT=3, PRED=4, TP=[3] * 16 + [2] * 3, gt_tracks=1, pred_tracks=2))))
    return out


def check_expected(records, summary, expect):
    match, msim, mscore = records
    if "match" in expect:
        assert np.asarray(match).tolist() == expect["match"]
    if "msim" in expect:
        assert np.array_equal(np.asarray(msim), np.asarray(expect["msim"], np.float32))
    if "mscore" in expect:
        assert np.asarray(mscore).tolist() == expect["mscore"]
    blocks = [(summary["all"], expect.get("all", {}))] + list(zip(summary["clips"], expect.get("clips", [])))
    for got, want in blocks:
        for k, v in want.items():
            if isinstance(v, list) and v and isinstance(v[0], float):
                assert len(got[k]) == len(v) and all(abs(a - b) <= TOL for a, b in zip(got[k], v)), (k, got[k], v)
            elif isinstance(v, float):
                assert abs(got[k] - v) <= TOL, (k, got[k], v)
            else:
                assert got[k] == v, (k, got[k], v)
