"""The contract of vd_voc_match (include/viddet_hip.h) restated in NumPy, and the cases both device-metric test
files use.

`match_reference` is written in the PARALLEL form the kernel has - every detection finds its best ground truth on its own, and
a detection is a true positive iff no detection with the same best row precedes it in (score descending, row) order - not as a
copy of VOCMApMetric.update's sequential `taken` loop.  tests/test_device_metric_cpu.py proves the two equal; the GPU tests then
compare the kernel with the host metric itself.
"""
import numpy as np

from viddet_amd.bbox import bbox_iou
from viddet_amd.metrics import VOCMApMetric

NAMES = ["c0", "c1", "c2", "c3"]


def _np_less(a, b):
    """numpy's sort order of floats: NaN behind everything"""
    return (a < b) | (np.isnan(b) & ~np.isnan(a))


def match_reference(ids, scores, boxes, gt, clip, thresh, num_labels=len(NAMES)):
    """ids (B,N), scores (B,N), boxes (B,N,4), gt (B,M,5|6), all float32; clip None or < 0: the detections are not clipped.
    -> rec_cls (B,N) int32, rec_score (B,N) float32, rec_hit (B,N) int8, npos (num_labels,), ndiff (num_labels,) int64 (ndiff:
    the difficult rows per class, which the metric needs to know that a class with only such rows was present)."""
    ids, scores = np.asarray(ids, np.float32), np.asarray(scores, np.float32)
    boxes, gt = np.asarray(boxes, np.float32), np.asarray(gt, np.float32)
    B, N = ids.shape
    M, w = gt.shape[1], gt.shape[2]
    rec_cls, rec_hit = np.full((B, N), -1, np.int32), np.full((B, N), -2, np.int8)
    npos, ndiff = np.zeros(num_labels, np.int64), np.zeros(num_labels, np.int64)
    rows = np.arange(N)
    for b in range(B):
        det = ids[b] >= 0
        cls = np.where(det, ids[b], -1).astype(np.int32)
        box = np.clip(boxes[b], 0, clip) if clip is not None and clip >= 0 else boxes[b]
        g_on = gt[b, :, 4] >= 0
        g_cls = np.where(g_on, gt[b, :, 4], -1).astype(np.int32)
        g_diff = (gt[b, :, 5] != 0) if w == 6 else np.zeros(M, bool)
        counted = g_on & (g_cls < num_labels)
        np.add.at(npos, g_cls[counted & ~g_diff], 1)
        np.add.at(ndiff, g_cls[counted & g_diff], 1)
        rec_cls[b] = cls
        best = np.full(N, -1)
        if M and N:
            same = det[:, None] & g_on[None, :] & (cls[:, None] == g_cls[None, :])
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = np.where(same, bbox_iou(box, gt[b, :, :4]), -np.inf)      # an IoU is >= 0, -0 or NaN: -inf never wins
            arg = iou.argmax(axis=1)                                             # first maximum; the first NaN beats everything
            top = iou[rows, arg]
            best = np.where(same.any(axis=1) & ~(top < thresh), arg, -1)
        # first claimant: j precedes d iff -score[j] sorts before -score[d], ties by row (the stable argsort of the host)
        k = -scores[b]
        before = _np_less(k[:, None], k[None, :]) | (~_np_less(k[None, :], k[:, None]) & (rows[:, None] < rows[None, :]))
        rival = (best[:, None] == best[None, :]) & (best[:, None] >= 0) & before             # [j, d]
        later = rival.any(axis=0)
        hit = np.where(later, 0, 1)
        hit = np.where(g_diff[np.maximum(best, 0)] if M else False, -1, hit)
        hit = np.where(best < 0, 0, hit)
        rec_hit[b] = np.where(det, hit, -2)
    return rec_cls, scores.copy(), rec_hit, npos, ndiff


def host_update(metric, ids, scores, boxes, gt, clip, order=None):
    """VOCMApMetric.update image by image on the arrays validate() would hand it (detections clipped as it clips them)"""
    boxes = np.clip(boxes, 0, clip) if clip is not None and clip >= 0 else boxes
    for b in (range(len(ids)) if order is None else order):
        metric.update([boxes[b]], [ids[b]], [scores[b]], [gt[b, :, :4]], [gt[b, :, 4:5]],
                      [gt[b, :, 5:6]] if gt.shape[2] > 5 else None)


def host_metric(cases, thresh=0.5, names=NAMES):
    m = VOCMApMetric(thresh, names)
    for c in cases:
        host_update(m, c["ids"], c["scores"], c["boxes"], c["gt"], c["clip"])
    return m


def assert_same_metric(dev, host):
    """equal get() (NaN positions included) and EQUAL dictionaries"""
    (na, va), (nb, vb) = dev.get(), host.get()
    assert na == nb
    assert np.array_equal(np.asarray(va, np.float64), np.asarray(vb, np.float64), equal_nan=True), (va, vb)
    for what in ("_npos", "_scores", "_hits"):
        a = {int(k): v for k, v in getattr(dev, what).items()}
        b = {int(k): v for k, v in getattr(host, what).items()}
        assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
        for k in a:
            if what == "_scores":
                assert np.array_equal(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64), equal_nan=True), (what, k)
            else:
                assert a[k] == b[k], (what, k, a[k], b[k])


def _case(ids, scores, boxes, gt, clip=None):
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    c = dict(ids=f(ids), scores=f(scores), boxes=f(boxes), gt=f(gt), clip=clip)
    assert c["ids"].shape == c["scores"].shape == c["boxes"].shape[:2] and c["gt"].shape[0] == c["ids"].shape[0]
    return c


def fixed_cases():
    """name -> case: the hand-made situations of the issue, each as a small batch"""
    A, Bx, Cx, Dx = [10, 10, 50, 50], [60, 60, 90, 90], [12, 11, 49, 52], [100, 100, 120, 130]
    pad_d, pad_g5, pad_g6 = [-1, -1, -1, -1], [-1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1]
    below = float(np.nextafter(np.float32(2), np.float32(3)))
    out = {}
    # two detections on one ground truth: the higher score claims it in either row order; equal scores: the lower row
    out["two_on_one"] = _case(ids=[[0, 0]] * 3, scores=[[0.9, 0.5], [0.5, 0.9], [0.7, 0.7]], boxes=[[A, Cx]] * 3,
                              gt=[[A + [0]]] * 3)
    # a difficult row hit twice (-1, -1) beside a non-difficult row of the same class (1)
    out["difficult_twice"] = _case(ids=[[1, 1, 1]], scores=[[0.9, 0.8, 0.7]], boxes=[[A, Cx, Bx]],
                                   gt=[[A + [1, 1], Bx + [1, 0]]])
    out["absent_classes"] = _case(ids=[[2, 3, 0]], scores=[[0.9, 0.8, 0.7]], boxes=[[A, A, A]], gt=[[A + [0], Bx + [1]]])
    out["gt_all_padded"] = _case(ids=[[0, 1]], scores=[[0.9, 0.8]], boxes=[[A, Bx]], gt=[[pad_g5, pad_g5, pad_g5]])
    out["no_gt_rows"] = _case(ids=[[0, 1], [2, -1]], scores=[[0.9, 0.8], [0.3, -1]], boxes=[[A, Bx], [A, pad_d]],
                              gt=np.zeros((2, 0, 5)))
    out["dets_all_padded"] = _case(ids=[[-1, -1, -1]], scores=[[-1, -1, -1]], boxes=[[pad_d] * 3], gt=[[A + [0], Bx + [1]]])
    out["padded_in_the_middle"] = _case(ids=[[0, -1, 1, -1, 0]], scores=[[0.9, -1, 0.8, -1, 0.95]],
                                        boxes=[[A, pad_d, Bx, pad_d, Cx]],
                                        gt=[[pad_g6, A + [0, 0], pad_g6, Bx + [1, 0], pad_g6]])
    # [0,0,2,1] on [0,0,1,1] is 0.5 in fp32 and matches (the drop is `max < thresh`); one ulp wider does not
    out["iou_at_threshold"] = _case(ids=[[0], [0]], scores=[[0.9], [0.9]], boxes=[[[0, 0, 2, 1]], [[0, 0, below, 1]]],
                                    gt=[[[0, 0, 1, 1, 0]]] * 2)
    # two rows of the class at equal IoU: the first one wins (1 in the first image, -1 in the second where it is difficult)
    out["equal_iou_first_row"] = _case(ids=[[2], [2]], scores=[[0.9], [0.9]], boxes=[[Cx]] * 2,
                                       gt=[[A + [2, 0], A + [2, 1]], [A + [2, 1], A + [2, 0]]])
    # detections reaching outside [0, 64]; the second clips to zero area and meets a zero-area ground truth: 0 / 0 = NaN keeps
    # its match; the ground truth is not clipped (the last row reaches outside and matches nothing once its detection is cut)
    out["clip"] = _case(ids=[[1, 1, 0, 3]], scores=[[0.9, 0.8, 0.7, 0.6]],
                        boxes=[[[50, 50, 100, 100], [-10, -5, -1, -2], [-20, -20, 30, 30], Dx]],
                        gt=[[[50, 50, 64, 64, 1], [0, 0, 0, 0, 1], [0, 0, 30, 30, 0], Dx + [3]]], clip=64)
    out["no_clip"] = _case(ids=[[1, 0, 3]], scores=[[0.9, 0.7, 0.6]], boxes=[[[50, 50, 100, 100], [-20, -20, 30, 30], Dx]],
                           gt=[[[50, 50, 100, 100, 1], [-20, -20, 30, 30, 0], Dx + [3]]], clip=None)
    return out


# (N, M) -> seed under which random_case() exercises everything `coverage` lists (searched on the CPU; the tests assert it)
RANDOM_N, RANDOM_M = (1, 7, 100, 257), (1, 5, 65, 512)
SEEDS = {(1, 1): 15, (1, 5): 3, (1, 65): 3, (1, 512): 30, (7, 5): 2}          # every other pair: seed 0


def random_case(N, M, seed, B=3, C=len(NAMES)):
    """Detections made by jittering ground-truth boxes, rows in random order; padded rows anywhere in both lists; difficult
    rows; scores from a few values (ties); some detections of another class than the row they came from"""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0, 80, (B, M, 2))
    gt = np.concatenate([lo, lo + rng.uniform(5, 40, (B, M, 2)), rng.integers(0, C, (B, M, 1)),
                         rng.random((B, M, 1)) < 0.3], axis=2).astype(np.float32)
    if M > 1:
        gt[rng.random((B, M)) < 0.2] = -1
        gt[:, 0, 4] = np.abs(gt[:, 0, 4]) % C                         # at least one real row per image
        gt[:, 0, :4] = np.abs(gt[:, 0, :4])
    src = rng.integers(0, M, (B, N))
    if N > 1:
        src[:, 1] = src[:, 0]                                          # two detections from one row
    take = np.take_along_axis
    boxes = take(gt[..., :4], src[..., None].repeat(4, axis=2), axis=1)
    wide = rng.random((B, N, 1)) < 0.2
    boxes = boxes + np.where(wide, rng.uniform(-15, 15, (B, N, 4)), rng.uniform(-2, 2, (B, N, 4)))
    ids = take(gt[..., 4], src, axis=1)
    other = rng.random((B, N)) < 0.15
    ids = np.where(other & (ids >= 0), rng.integers(0, C, (B, N)), ids)
    scores = rng.choice(np.linspace(0.1, 0.9, 9), (B, N))
    if N > 1:
        gone = rng.random((B, N)) < 0.15
        gone[:, :2] = False
        ids, scores = np.where(gone, -1, ids), np.where(gone, -1, scores)
    return _case(ids, scores, boxes.astype(np.float32), gt, clip=100)


def coverage(case, thresh=0.5):
    """what the HOST metric meets in a case: the set of hit codes, whether a ground-truth row is claimed twice, whether a
    detection row has no class"""
    m = host_metric([case], thresh)
    codes = set(h for v in m._hits.values() for h in v)
    # a row claimed twice, worked out here from the host's own expressions: two detections of a class whose arg-max rows (kept
    # ones) coincide
    boxes = np.clip(case["boxes"], 0, case["clip"]) if case["clip"] is not None else case["boxes"]
    twice = False
    for b in range(len(boxes)):
        on = case["gt"][b, :, 4] >= 0
        for c in np.unique(case["ids"][b][case["ids"][b] >= 0]):
            d, g = case["ids"][b] == c, on & (case["gt"][b, :, 4] == c)
            if d.sum() > 1 and g.any():
                with np.errstate(divide="ignore", invalid="ignore"):
                    iou = bbox_iou(boxes[b][d], case["gt"][b, g, :4])
                arg = iou.argmax(axis=1)[~(iou.max(axis=1) < thresh)]
                twice = twice or len(np.unique(arg)) < len(arg)
    return dict(codes=codes, twice=bool(twice), unclassed=bool((case["ids"] < 0).any()))


def assert_covers(case, N):
    cov = coverage(case)
    if N == 1:
        # three images of one detection each cannot hold more than the three codes: no row can be claimed twice and no
        # detection row can be spared for padding
        assert cov["codes"] == {1, 0, -1}, cov
    else:
        assert cov["codes"] == {1, 0, -1} and cov["twice"] and cov["unclassed"], cov
