"""The closed forms of the MOT metric's tests (CPU and GPU): small clips whose every output is written out by hand."""
import numpy as np

A, B, C = (0, 0, 10, 10), (20, 0, 30, 10), (40, 0, 50, 10)     # three boxes that do not meet
A8 = (0, 0, 10, 8)                                             # IoU with A: 80 / ((100 + 80) - 80) = 0.8
A5 = (0, 0, 10, 5)                                             # IoU with A: 50 / ((100 + 50) - 50) = 0.5, exactly
CARRY, SWITCH = 2, 1                                           # the bits of `flags`


def build(gt, pred, G=None, N=None):
    """gt: per frame [(box, cls, id)], pred: per frame [(box, cls, score, track)] -> the seven arrays of mot_match_host, padded
    with rows that are no candidates"""
    F = len(gt)
    G = G or max(1, max(len(f) for f in gt))
    N = N or max(1, max(len(f) for f in pred))
    gt_boxes, gt_cls, gt_id = np.zeros((F, G, 4), np.float32), np.full((F, G), -1, np.int32), np.full((F, G), -1, np.int32)
    ids, scores = np.full((F, N, 1), -1, np.float32), np.full((F, N, 1), -1, np.float32)
    bboxes, track = np.full((F, N, 4), -1, np.float32), np.full((F, N), -1, np.int32)
    for t in range(F):
        for g, (box, cls, a) in enumerate(gt[t]):
            gt_boxes[t, g], gt_cls[t, g], gt_id[t, g] = box, cls, a
        for j, (box, cls, score, trk) in enumerate(pred[t]):
            bboxes[t, j], ids[t, j, 0], scores[t, j, 0], track[t, j] = box, cls, score, trk
    return gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track


def closed_forms():
    """[(name, arrays, kwargs, expect)]: expect holds match / miou / flags / adm0 (word 0 of adm) as nested lists, and `all`, the
    overall figures of mot_summary that the case is about"""
    out = []
    f8 = float(np.float32(0.8))
    # a perfect track: matched in frame 0 by the assignment, carried over ever after
    gt = [[(A, 0, 0)]] * 4
    pred = [[(A, 0, 0.9, 5)]] * 4
    out.append(("perfect", build(gt, pred), {}, dict(
        match=[[0]] * 4, miou=[[1.0]] * 4, flags=[[0]] + [[CARRY]] * 3, adm0=[[1]] * 4,
        all=dict(frames=4, gt_tracks=1, GT=4, PRED=4, TP=4, FN=0, FP=0, IDSW=0, Frag=0, MT=1, PT=0, ML=0, IDTP=4, IDFP=0, IDFN=0,
                 MOTA=1.0, MOTP=1.0, precision=1.0, recall=1.0, IDF1=1.0, IDP=1.0, IDR=1.0))))
    # two tracks that swap identities at frame 3: the carry-over finds its row at the other object, which is not admissible
    gt = [[(A, 0, 0), (B, 0, 1)]] * 6
    pred = [[(A, 0, 0.9, 7), (B, 0, 0.9, 8)]] * 3 + [[(A, 0, 0.9, 8), (B, 0, 0.9, 7)]] * 3
    out.append(("swap", build(gt, pred), {}, dict(
        match=[[0, 1]] * 6, miou=[[1.0, 1.0]] * 6, flags=[[0, 0]] + [[CARRY] * 2] * 2 + [[SWITCH] * 2] + [[CARRY] * 2] * 2,
        adm0=[[1, 2]] * 6,
        # n[a, p] = 3 for all four pairs: the best pairing of ids covers 3 + 3 of the 12 rows
        all=dict(GT=12, PRED=12, TP=12, FN=0, FP=0, IDSW=2, Frag=0, MT=2, IDTP=6, IDFP=6, IDFN=6, MOTA=1.0 - 2.0 / 12.0, MOTP=1.0,
                 IDF1=0.5, IDP=0.5, IDR=0.5))))
    # a carried-over match that the IoU-best assignment would break: track 3 moves to the worse box, track 9 sits on the object
    gt = [[(A, 0, 0)]] * 2
    pred = [[(A, 0, 0.9, 3)], [(A, 0, 0.9, 9), (A8, 0, 0.9, 3)]]
    out.append(("carry_over_wins", build(gt, pred), {}, dict(
        match=[[0], [1]], miou=[[1.0], [f8]], flags=[[0], [CARRY]], adm0=[[1], [3]],
        all=dict(GT=2, PRED=3, TP=2, FN=0, FP=1, IDSW=0, MOTA=0.5, MOTP=(1.0 + f8) / 2.0, IDTP=2, IDF1=4.0 / 5.0))))
    # two identical prediction boxes: equal cost, the lower row
    out.append(("tie_to_the_lower_row", build([[(A, 0, 0)]], [[(A, 0, 0.5, 1), (A, 0, 0.9, 2)]]), {}, dict(
        match=[[0]], miou=[[1.0]], flags=[[0]], adm0=[[3]], all=dict(GT=1, PRED=2, TP=1, FP=1, MOTA=0.0, IDTP=1, IDF1=2.0 / 3.0))))
    # a duplicate track id and a duplicate ground-truth id in a frame: the lower row of either stands, the other takes no part
    out.append(("duplicate_ids", build([[(A, 0, 0), (B, 0, 0)]], [[(A, 0, 0.9, 4), (B, 0, 0.9, 4)]]), {}, dict(
        match=[[0, -2]], miou=[[1.0, 0.0]], flags=[[0, 0]], adm0=[[1, 0]], all=dict(GT=1, PRED=1, TP=1, FN=0, FP=0, MOTA=1.0, gt_tracks=1))))
    # ground-truth ids -1, 1023 and 1024: only 1023 indexes the table
    out.append(("gt_id_range", build([[(A, 0, -1), (B, 0, 1023), (C, 0, 1024)]], [[(A, 0, 0.9, 0), (B, 0, 0.9, 1), (C, 0, 0.9, 2)]]), {},
                dict(match=[[-2, 1, -2]], miou=[[0.0, 1.0, 0.0]], flags=[[0, 0, 0]], adm0=[[0, 2, 0]],
                     all=dict(GT=1, PRED=3, TP=1, FN=0, FP=2, MOTA=-1.0, gt_tracks=1, IDTP=1, IDF1=0.5))))
    # a row with track -1 is not tracker output: it neither matches nor counts
    out.append(("track_minus_one", build([[(A, 0, 0)]], [[(A, 0, 0.9, -1), (A8, 0, 0.9, 2)]]), {}, dict(
        match=[[1]], miou=[[f8]], flags=[[0]], adm0=[[2]], all=dict(GT=1, PRED=1, TP=1, FP=0, MOTA=1.0, MOTP=f8))))
    # a class mismatch, with agnostic off and on
    arrays = build([[(A, 1, 0)]], [[(A, 0, 0.9, 0)]])
    out.append(("class_mismatch", arrays, dict(num_class=2), dict(
        match=[[-1]], miou=[[0.0]], flags=[[0]], adm0=[[0]], all=dict(GT=1, PRED=1, TP=0, FN=1, FP=1, MOTA=-1.0, MOTP=0.0, IDTP=0, IDF1=0.0, ML=1))))
    out.append(("class_mismatch_agnostic", arrays, dict(num_class=2, agnostic=True), dict(
        match=[[0]], miou=[[1.0]], flags=[[0]], adm0=[[1]], all=dict(GT=1, PRED=1, TP=1, FN=0, FP=0, MOTA=1.0, MT=1))))
    # IoU exactly at the threshold is admissible; the next float32 above it is not
    arrays = build([[(A, 0, 0)]], [[(A5, 0, 0.9, 0)]])
    out.append(("iou_at_the_threshold", arrays, dict(iou_thresh=0.5), dict(
        match=[[0]], miou=[[0.5]], flags=[[0]], adm0=[[1]], all=dict(TP=1, MOTP=0.5))))
    out.append(("iou_below_the_threshold", arrays, dict(iou_thresh=float(np.nextafter(np.float32(0.5), np.float32(1)))), dict(
        match=[[-1]], miou=[[0.0]], flags=[[0]], adm0=[[0]], all=dict(TP=0, FN=1, FP=1))))
    # a hole of 3 frames: one fragmentation, no switch (the track comes back with its id: a carry-over)
    gt = [[(A, 0, 0)]] * 7
    pred = [[(A, 0, 0.9, 3)]] * 2 + [[]] * 3 + [[(A, 0, 0.9, 3)]] * 2
    out.append(("hole_of_three", build(gt, pred), {}, dict(
        match=[[0], [0], [-1], [-1], [-1], [0], [0]], miou=[[1.0]] * 2 + [[0.0]] * 3 + [[1.0]] * 2,
        flags=[[0], [CARRY], [0], [0], [0], [CARRY], [CARRY]], adm0=[[1]] * 2 + [[0]] * 3 + [[1]] * 2,
        all=dict(GT=7, PRED=4, TP=4, FN=3, FP=0, IDSW=0, Frag=1, MT=0, PT=1, ML=0, MOTA=1.0 - 3.0 / 7.0, IDTP=4, IDF1=8.0 / 11.0))))
    # tracks at 80 % (mostly tracked), at 20 % (partly) and at 1 of 6, just under 20 % (mostly lost)
    gt = [[(A, 0, 0)] + ([(B, 0, 1)] if t < 5 else []) + ([(C, 0, 2)] if t < 6 else []) for t in range(10)]
    pred = [([(A, 0, 0.9, 0)] if t < 8 else []) + ([(B, 0, 0.9, 1), (C, 0, 0.9, 2)] if t == 0 else []) for t in range(10)]
    out.append(("coverage_borders", build(gt, pred), {}, dict(
        all=dict(gt_tracks=3, GT=21, PRED=10, TP=10, FN=11, FP=0, MT=1, PT=1, ML=1, Frag=0, IDSW=0, MOTA=1.0 - 11.0 / 21.0))))
    # an empty clip between two clips: last[] starts afresh, so frame 2 is an assignment again
    gt = [[(A, 0, 0)]] * 4
    pred = [[(A, 0, 0.9, 5)]] * 4
    out.append(("empty_clip_between", build(gt, pred), dict(clip_start=[0, 2, 2, 4]), dict(
        match=[[0]] * 4, flags=[[0], [CARRY], [0], [CARRY]], adm0=[[1]] * 4,
        all=dict(frames=4, gt_tracks=2, GT=4, TP=4, MOTA=1.0, IDTP=4, IDF1=1.0),
        clips=[dict(frames=2, GT=2, TP=2, MOTA=1.0), dict(frames=0, GT=0, PRED=0, TP=0, MOTA=0.0, MOTP=0.0, IDF1=0.0, recall=0.0),
               dict(frames=2, GT=2, TP=2, IDF1=1.0)])))
    # no predictions at all
    out.append(("no_predictions", build([[(A, 0, 0), (B, 0, 1)]] * 3, [[]] * 3), {}, dict(
        match=[[-1, -1]] * 3, miou=[[0.0, 0.0]] * 3, flags=[[0, 0]] * 3, adm0=[[0, 0]] * 3,
        all=dict(GT=6, PRED=0, TP=0, FN=6, FP=0, MOTA=0.0, MOTP=0.0, precision=0.0, recall=0.0, IDF1=0.0, IDP=0.0, IDR=0.0, ML=2))))
    # no ground truth at all: every rate is 0.0, the predictions are false positives
    out.append(("no_ground_truth", build([[]] * 2, [[(A, 0, 0.9, 0)]] * 2), {}, dict(
        match=[[-2]] * 2, miou=[[0.0]] * 2, flags=[[0]] * 2, adm0=[[0]] * 2,
        all=dict(gt_tracks=0, GT=0, PRED=2, TP=0, FN=0, FP=2, MOTA=0.0, MOTP=0.0, precision=0.0, recall=0.0, IDF1=0.0, IDP=0.0,
                 IDR=0.0, IDTP=0, IDFP=2, IDFN=0))))
    return out


def check_expected(records, summary, expect):
    match, miou, flags, adm = records
    adm = np.asarray(adm).view(np.uint32) if np.asarray(adm).dtype == np.int32 else np.asarray(adm)
    if "match" in expect:
        assert match.tolist() == expect["match"]
    if "miou" in expect:
        assert np.array_equal(miou, np.asarray(expect["miou"], np.float32))
    if "flags" in expect:
        assert flags.tolist() == expect["flags"]
    if "adm0" in expect:
        assert adm[..., 0].tolist() == expect["adm0"] and not adm[..., 1:].any()
    for k, v in expect.get("all", {}).items():
        assert summary["all"][k] == v, (k, summary["all"][k], v)
    for got, want in zip(summary["clips"], expect.get("clips", [])):
        for k, v in want.items():
            assert got[k] == v, (k, got[k], v)
