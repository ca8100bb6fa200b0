"""Inputs of the tracker tests (tests/test_track_cpu.py, tests/test_track_gpu.py): random clips (tests/seqnms_cases.py's, whose
tracks drift, jitter, drop rows and change rows from frame to frame), the closed-form cases with the expected ids written out
by hand, and the two clips that fill vd_track's table of active tracks."""
import numpy as np

from tests.seqnms_cases import random_clip  # noqa: F401  (re-exported)

SIZES = [(1, 1), (2, 3), (5, 64), (5, 65), (9, 100), (6, 128), (40, 20)]
OFF_DEFAULT = dict(sigma_l=0.3, sigma_h=0.7, sigma_iou=0.35, t_min=3, max_age=2)       # every parameter off its default


def rows(frames, N=None, cls=None):
    """frames: per frame a list of (box, score) or (box, score, class), None for an invalid row -> (ids, scores, bboxes)"""
    N = N or max(1, max(len(f) for f in frames))
    ids = -np.ones((len(frames), N, 1), np.float32)
    scores = -np.ones((len(frames), N, 1), np.float32)
    bboxes = -np.ones((len(frames), N, 4), np.float32)
    for t, f in enumerate(frames):
        for i, r in enumerate(f):
            if r is not None:
                ids[t, i, 0], scores[t, i, 0], bboxes[t, i] = (r[2] if len(r) > 2 else 0), r[1], r[0]
    return ids, scores, bboxes


def _b(x, y=0.0, w=10.0, h=10.0):
    return [x, y, x + w, y + h]


def closed_form():
    """[(name, (ids, scores, bboxes), keyword arguments, the expected `track` (F,N), the expected `tlen` or None)]"""
    out = []
    # two boxes that cross, A moving right from row 0 and B moving left from row 1, 5 px per frame; in frame 2 they have passed
    # each other and A sits in row 1.  IoUs at sigma_iou 0.3: frame 1 A->row 0 5/15, B->row 1 5/15; frame 2 track 0 (last box
    # [5,15]) sees row 0 = B [2,12] at 7/13 and row 1 = A [10,20] at 5/15 and takes B: the greedy rule swaps the identities
    cross = rows([[(_b(0), .9), (_b(12), .8)], [(_b(5), .9), (_b(7), .8)], [(_b(2), .8), (_b(10), .9)]])
    out.append(("cross", cross, dict(sigma_iou=0.3), [[0, 1], [0, 1], [0, 1]], [[3, 3], [3, 3], [3, 3]]))
    # the first track takes what the second one needed: A [0,10] and B [6,16]; X [3,13] has 7/13 to both, Y [-3,7] 7/13 to A
    # and 1/19 to B.  Track 0 ties between X (row 0) and Y (row 1) and takes X; B is left with Y, misses and closes; Y starts 2
    steal = rows([[(_b(0), .9), (_b(6), .9)], [(_b(3), .9), (_b(-3), .9)]])
    out.append(("steal", steal, dict(t_min=1), [[0, 1], [0, 2]], [[2, 1], [2, 1]]))
    out.append(("steal_t_min", steal, dict(), [[0, -1], [0, -1]], [[2, 0], [2, 0]]))
    # a one-frame gap
    gap = rows([[(_b(0), .9)], [(_b(1), .9)], [None], [(_b(3), .9)], [(_b(4), .9)]])
    out.append(("gap_age0", gap, dict(max_age=0), [[0], [0], [-1], [1], [1]], [[2], [2], [0], [2], [2]]))
    out.append(("gap_age1", gap, dict(max_age=1), [[0], [0], [-1], [0], [0]], [[4], [4], [0], [4], [4]]))
    # an IoU of exactly 0.5: [0,0,10,10] and [0,0,10,20], 100 / 200
    half = rows([[(_b(0), .9)], [(_b(0, h=20.0), .9)]])
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    out.append(("half_matched", half, dict(sigma_iou=0.5, t_min=1), [[0], [0]], [[2], [2]]))
    out.append(("half_not", half, dict(sigma_iou=above, t_min=1), [[0], [1]], [[1], [1]]))
    # two equal IoUs (8/12 both): the lowest row joins, the other starts track 1
    tie = rows([[(_b(0), .9), None], [(_b(2), .9), (_b(-2), .9)]])
    out.append(("tie", tie, dict(t_min=1), [[0, -1], [0, 1]], [[2, 0], [2, 1]]))
    # A (0.9, two frames) id 0, B (0.3 < sigma_h) id 1, C (one frame < t_min) id 2, D (two frames) id 3: 1 and 2 leave a gap
    far = rows([[(_b(0), .9), (_b(100), .3)], [(_b(0), .9), (_b(100), .3), (_b(200), .9), (_b(300), .6)], [None, None, None, (_b(300), .9)]])
    out.append(("dropped", far, dict(), [[0, -1, -1, -1], [0, -1, -1, 3], [-1, -1, -1, 3]], [[2, 0, 0, 0], [2, 0, 0, 2], [0, 0, 0, 2]]))
    # the same box twice, of two classes, which change rows in frame 1: per class the tracks follow their class, with one
    # class (ids all 0 would be the same as num_class=1 on class-0 rows: see below) the lowest row is taken first
    pair = rows([[(_b(0), .9, 0), (_b(0), .9, 1)], [(_b(0), .9, 1), (_b(0), .9, 0)]])
    out.append(("two_classes", pair, dict(num_class=2), [[0, 1], [1, 0]], None))
    out.append(("two_classes_cut", pair, dict(num_class=1), [[0, -1], [-1, 0]], None))          # class 1 is no candidate
    same = (np.zeros_like(pair[0]), pair[1], pair[2])
    out.append(("one_class", same, dict(num_class=1), [[0, 1], [0, 1]], None))
    # NaN / inf scores and a NaN id are no candidates
    bad = rows([[(_b(0), .9), (_b(50), .9), (_b(100), .9), (_b(150), .9)], [(_b(0), .9), (_b(50), .9), (_b(100), .9), (_b(150), .9)]])
    bad[1][0, 1, 0], bad[1][1, 2, 0], bad[0][0, 3, 0], bad[1][1, 3, 0] = np.nan, np.inf, np.nan, -np.inf
    out.append(("non_finite", bad, dict(t_min=1), [[0, -1, 1, -1], [0, 2, -1, -1]], [[2, 0, 1, 0], [2, 1, 0, 0]]))
    # nothing at all
    none = (-np.ones((3, 5, 1), np.float32), -np.ones((3, 5, 1), np.float32), -np.ones((3, 5, 4), np.float32))
    out.append(("all_invalid", none, dict(num_class=2), -np.ones((3, 5), int), np.zeros((3, 5), int)))
    return out


def capacity(extend):
    """F = 10 frames of N = 128 rows of one class on a 16 x 8 grid of 10 px boxes 20 px apart.  extend False: every frame's
    grid is shifted by 10 px against the last 9, so that no box overlaps a box of the 9 frames before it (max_age = 7: the
    table grows by 128 per frame to 1024).  extend True: the boxes stand still, so that all 128 tracks extend in every frame."""
    F, N = 10, 128
    ids = np.zeros((F, N, 1), np.float32)
    scores = np.full((F, N, 1), 0.9, np.float32)
    bboxes = np.zeros((F, N, 4), np.float32)
    gx, gy = np.meshgrid(np.arange(16) * 20.0, np.arange(8) * 20.0)
    for t in range(F):
        dx = 0.0 if extend else 10.0 * (t % 2) + 1000.0 * (t // 2)
        dy = 0.0 if extend else 0.0
        x, y = gx.reshape(-1) + dx, gy.reshape(-1) + dy
        bboxes[t] = np.stack([x, y, x + 10.0, y + 10.0], axis=1)
    return ids, scores, bboxes
