"""Inputs of the BYTE tests (tests/test_byte_cpu.py, tests/test_byte_gpu.py): the closed-form cases with the expected ids written
out by hand, the seeded walkers with score dips that the paper-form oracle (tests/byte_oracle.py) decides with a margin, and the
clips that fill vd_track_byte's table and run both of its assignments wide."""
import numpy as np

from tests import sort_cases as SC
from tests.sort_cases import GPU_SIZES, capacity, crowded, random_clip, rows, same_tbox, walkers  # noqa: F401  (re-exported)


def A(x, s, c=0):
    """the 40 x 80 box at x, y = 0, with score s (and class c)"""
    return ([x, 0.0, x + 40.0, 80.0], s, c)


def dip_case():
    return rows([[A(0, .9)], [A(2, .9)], [A(4, .3)], [A(6, .3)], [A(8, .9)]])


def clutter_case():
    return rows([[A(0, .9)], [A(0, .9)], [A(1, .3), A(12, .9)]])


def closed_form():
    """[(name, (ids, scores, bboxes), keyword arguments, the expected `track` (F,N), the expected `tlen` or None)]"""
    out = []
    # the score dips below sigma_d for two frames: the second association carries the track through
    out.append(("dip", dip_case(), dict(), [[0], [0], [0], [0], [0]], [[5]] * 5))
    # a low clutter row nearer to the prediction than the object's own high row: the high row is matched first
    out.append(("clutter", clutter_case(), dict(), [[0, -1], [0, -1], [-1, 0]], [[3, 0], [3, 0], [0, 3]]))
    # a low row (0.3) and a high row below sigma_new (0.55) never start a track
    three = [A(0, .9), A(200, .3), A(400, .55)]
    out.append(("no_start", rows([three, three]), dict(), [[0, -1, -1], [0, -1, -1]], [[2, 0, 0], [2, 0, 0]]))
    # the second association takes only tracks seen in the last frame: after a gap the low row is left alone
    out.append(("second_needs_last_frame", rows([[A(0, .9)], [A(0, .9)], [None], [A(0, .3)], [A(0, .9)]]), dict(),
                [[0], [0], [-1], [-1], [0]], [[3], [3], [0], [0], [3]]))
    out.append(("second_without_gap", rows([[A(0, .9)], [A(0, .9)], [A(0, .3)], [A(0, .9)]]), dict(), [[0], [0], [0], [0]], [[4]] * 4))
    # 40 x 80 boxes 20 px apart: IoU 20 / 60 = 1/3, admissible at sigma_iou 0.2 but not at sigma_iou2 0.5
    out.append(("sigma_iou2", rows([[A(0, .9)], [A(0, .9)], [A(20, .3)], [A(0, .9)]]), dict(), [[0], [0], [-1], [0]],
                [[3], [3], [0], [3]]))
    out.append(("sigma_iou2_low", rows([[A(0, .9)], [A(0, .9)], [A(20, .3)]]), dict(sigma_iou2=0.3), [[0], [0], [0]], [[3]] * 3))
    # the same box twice, of two classes, which change rows in frame 1, high and then low: the tracks follow their class
    pair = rows([[A(0, .9, 0), A(0, .9, 1)], [A(0, .9, 1), A(0, .9, 0)], [A(0, .3, 0), A(0, .3, 1)]])
    out.append(("two_classes", pair, dict(num_class=2), [[0, 1], [1, 0], [0, 1]], [[3, 3]] * 3))
    out.append(("two_classes_cut", pair, dict(num_class=1), [[0, -1], [-1, 0], [0, -1]], None))
    # two tracks with the same state, both eligible, and one low row: both cells cost the same, the lowest column wins
    twin = rows([[A(0, .9), A(0, .9)], [A(1, .3), None]])
    out.append(("tie_columns_second", twin, dict(t_min=1), [[0, 1], [0, -1]], [[2, 1], [2, 0]]))
    # ... and where the first of the twins was matched by the high row, the low row takes the second
    twin2 = rows([[A(0, .9), A(0, .9)], [A(1, .3), A(1, .9)]])
    out.append(("second_takes_what_first_left", twin2, dict(t_min=1), [[0, 1], [1, 0]], [[2, 2], [2, 2]]))
    # sigma_l above sigma_d: no low rows at all (sort_host at that sigma_l; every candidate here is above sigma_new too)
    far = rows([[A(0, .9), A(100, .3)], [A(0, .9), A(100, .3), A(200, .9), A(300, .7)], [None, None, None, A(300, .9)]])
    out.append(("no_low_rows", far, dict(sigma_l=0.65, sigma_d=0.5, sigma_new=0.5), [[0, -1, -1, -1], [0, -1, -1, 2], [-1, -1, -1, 2]],
                None))
    # a one-frame clip: the high rows at or above sigma_new start, nothing else does
    one = rows([[([0.1, 0.2, 33.43, 71.7], .9), ([5.5, 7.25, 6.75, 300.3], .55), ([1e3, 2e3, 1e3 + 1e-3, 2e3 + 7.7], .7),
                 ([50.0, 50.0, 60.0, 70.0], .3)]])
    out.append(("one_frame", one, dict(t_min=1), [[0, -1, 1, -1]], [[1, 0, 1, 0]]))
    # a zero-height box, an infinite and a NaN coordinate beside a sound box (tests/sort_cases.py's): each starts a track
    # whose state holds a NaN, no IoU with it is admissible in either pass, so it ages out and the next frame starts another
    bad = [c for c in SC.closed_form() if c[0] == "degenerate"][0]
    out.append(("degenerate", bad[1], dict(t_min=1, max_age=1), bad[3], bad[4]))
    low_bad = rows([[(SC._b(0), .9), ([20, 0, 30, 0], .9), ([60, np.nan, 70, 10], .9)],
                    [(SC._b(0), .3), ([20, 0, 30, 0], .3), ([60, np.nan, 70, 10], .3)]])
    out.append(("degenerate_low", low_bad, dict(t_min=1), [[0, 1, 2], [0, -1, -1]], [[2, 1, 1], [2, 0, 0]]))
    none = (-np.ones((3, 5, 1), np.float32), -np.ones((3, 5, 1), np.float32), -np.ones((3, 5, 4), np.float32))
    out.append(("all_invalid", none, dict(num_class=2), -np.ones((3, 5), int), np.zeros((3, 5), int)))
    return out


def dipped(seed, dip=0.3, low=(0.15, 0.45), **gen):
    """sort_cases.walkers(seed) with score dips: a seeded share `dip` of the rows, in runs of 1 to 3 frames per object, has its
    score drawn from `low` (below sigma_d 0.5).  An object is known by its class and its score, which walkers keeps constant."""
    ids, scores, bboxes = walkers(seed, **gen)
    rng = np.random.RandomState(1000 + seed)
    T, N = scores.shape[:2]
    keys = sorted({(float(ids[t, i, 0]), float(scores[t, i, 0])) for t in range(T) for i in range(N) if ids[t, i, 0] >= 0})
    out = scores.copy()
    for key in keys:
        t = 1 + rng.randint(0, 3)
        while t < T:
            if rng.uniform() < dip:
                run = 1 + rng.randint(0, 3)
                s = rng.uniform(*low)
                for tt in range(t, min(T, t + run)):
                    for i in range(N):
                        if (float(ids[tt, i, 0]), float(scores[tt, i, 0])) == key:
                            out[tt, i, 0] = s
                t += run + 1
            else:
                t += 1
    return ids, out, bboxes


def capacity_low(extend):
    """track_cases.capacity(extend), F = 10 and N = 128, with every second frame's scores low (0.3).  extend False: the boxes of
    a frame overlap no earlier frame's, only the even frames start tracks, the table grows by 128 every other frame (512 at the
    most: a track is closed after 8 misses) and the second association finds nothing admissible.  extend True: the boxes
    stand still, the odd frames' 128 low rows are all matched by the second association."""
    ids, scores, bboxes = capacity(extend)
    scores = scores.copy()
    scores[1::2] = 0.3
    return ids, scores, bboxes


def capacity_full():
    """track_cases.capacity(False) with frame 8 = frame 7's boxes scored 0.3: frames 0 to 7 fill the table to 1024 tracks, then
    128 low rows meet it in the second association - 1024 columns, the last 128 eligible - and all find their track."""
    ids, scores, bboxes = capacity(False)
    scores, bboxes = scores.copy(), bboxes.copy()
    bboxes[8] = bboxes[7]
    scores[8] = 0.3
    return ids, scores, bboxes


def crowded_pair():
    """sort_cases.crowded(5, 128): frame 0 scored 0.8; frame 1's odd rows 0.3 (low), its even rows 0.8 (high)"""
    ids, scores, bboxes = crowded(5, 128)
    scores = np.full_like(scores, 0.8)
    scores[1, 1::2] = 0.3
    return ids, scores, bboxes


CROWDED_KW = dict(sigma_iou=0.3, sigma_iou2=0.5, t_min=1, max_age=1)
