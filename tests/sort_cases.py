"""Inputs of the SORT tests (tests/test_sort_cpu.py, tests/test_sort_gpu.py): the closed-form cases with the expected ids written
out by hand, the seeded clips of a few objects that the paper-form oracle (tests/sort_oracle.py) decides with a margin, the
clips that fill vd_track_sort's table of active tracks and its assignment, and the degenerate boxes."""
import numpy as np

from tests.seqnms_cases import random_clip  # noqa: F401  (re-exported)
from tests.track_cases import capacity, rows  # noqa: F401  (re-exported)

GPU_SIZES = [(1, 1), (3, 2), (6, 63), (6, 64), (6, 65), (12, 128)]         # a lane of vd_track holds rows `lane` and `lane + 64`


def _b(x, y=0.0, w=10.0, h=10.0):
    return [x, y, x + w, y + h]


def gap_case():
    """A 40 x 80 box moving 12 px a frame, seen for 3 frames, missed for 2, seen again.  The constant-velocity prediction is at
    x = 59.99 when the box returns at 60 (IoU 0.999); the track's last box, at 24, overlaps it with 4/76 = 0.053."""
    return rows([[(_b(0, w=40.0, h=80.0), .9)], [(_b(12, w=40.0, h=80.0), .9)], [(_b(24, w=40.0, h=80.0), .9)], [None], [None],
                 [(_b(60, w=40.0, h=80.0), .9)]])


def closed_form():
    """[(name, (ids, scores, bboxes), keyword arguments, the expected `track` (F,N), the expected `tlen` or None)]"""
    out = []
    out.append(("gap", gap_case(), dict(max_age=2, sigma_iou=0.5), [[0], [0], [0], [-1], [-1], [0]], [[4], [4], [4], [0], [0], [4]]))
    # max_age = 1 closes the track after its second miss: the returning box starts track 1, both are kept at t_min = 1
    out.append(("gap_expired", gap_case(), dict(max_age=1, sigma_iou=0.5, t_min=1), [[0], [0], [0], [-1], [-1], [1]],
                [[3], [3], [3], [0], [0], [1]]))
    # tests/track_cases.py's crossing: A moves right from row 0 and B left from row 1, 5 px a frame; in frame 2 they have passed
    # each other and A sits in row 1.  Frame 1 (no velocity yet): 5/15 each to its own, 3/17 to the other.  Frame 2: the velocity
    # gain after one update is 1e4 / 10012, so A is predicted at [9.99, 19.99] and B at [2.01, 12.01]: each meets its own box with
    # an IoU of 0.998, the other's with 2/18.  track_host, from the last boxes, hands B to track 0 (7/13 against 5/15).
    cross = rows([[(_b(0), .9), (_b(12), .8)], [(_b(5), .9), (_b(7), .8)], [(_b(2), .8), (_b(10), .9)]])
    out.append(("cross", cross, dict(sigma_iou=0.3), [[0, 1], [0, 1], [1, 0]], [[3, 3], [3, 3], [3, 3]]))
    # the same box twice, of two classes, which change rows in frame 1: the tracks follow their class
    pair = rows([[(_b(0), .9, 0), (_b(0), .9, 1)], [(_b(0), .9, 1), (_b(0), .9, 0)]])
    out.append(("two_classes", pair, dict(num_class=2), [[0, 1], [1, 0]], None))
    out.append(("two_classes_cut", pair, dict(num_class=1), [[0, -1], [-1, 0]], None))          # class 1 is no candidate
    # two tracks with the same state and one row: both cells cost the same, the lowest column - the first track - wins
    twin = rows([[(_b(0), .9), (_b(0), .9)], [(_b(1), .9), None]])
    out.append(("tie_columns", twin, dict(t_min=1, max_age=0), [[0, 1], [0, -1]], [[2, 1], [2, 0]]))
    # one track and two rows with equal IoUs (8/12 both, cost c): row 0 is inserted first and takes the track (u0 = c).  Row 1's
    # least slack is the track's column (c against 2**27 for its dummy); from row 0, at the tree's tip, row 0's dummy then has
    # the slack 2**27 - c, and so has row 1's own: the lowest column of the tie is row 0's dummy, so the path hands the track
    # to row 1 and row 0 starts track 1.  Either matching has the same (pairs, sum); assign_host's rule picks this one.
    tie = rows([[(_b(0), .9), None], [(_b(2), .9), (_b(-2), .9)]])
    out.append(("tie_rows", tie, dict(t_min=1), [[0, -1], [1, 0]], [[2, 0], [1, 2]]))
    # a box that stands still, missed for max_age = 2 frames and back: the same track; missed for 3: closed at exactly
    # max_age + 1 misses, the box starts track 1
    still = [(_b(0), .9)]
    out.append(("age_kept", rows([still, still, [None], [None], still]), dict(max_age=2, t_min=1), [[0], [0], [-1], [-1], [0]],
                [[3], [3], [0], [0], [3]]))
    out.append(("age_expired", rows([still, still, [None], [None], [None], still]), dict(max_age=2, t_min=1),
                [[0], [0], [-1], [-1], [-1], [1]], [[2], [2], [0], [0], [0], [1]]))
    # A (0.9, two frames) id 0, B (0.3 < sigma_h) id 1, C (one frame < t_min) id 2, D (two frames) id 3: 1 and 2 leave a gap
    far = rows([[(_b(0), .9), (_b(100), .3)], [(_b(0), .9), (_b(100), .3), (_b(200), .9), (_b(300), .6)], [None, None, None, (_b(300), .9)]])
    out.append(("dropped", far, dict(), [[0, -1, -1, -1], [0, -1, -1, 3], [-1, -1, -1, 3]], [[2, 0, 0, 0], [2, 0, 0, 2], [0, 0, 0, 2]]))
    # sigma_l: the 0.3 row takes no part at all, so D is track 2
    out.append(("sigma_l", far, dict(sigma_l=0.5), [[0, -1, -1, -1], [0, -1, -1, 2], [-1, -1, -1, 2]], None))
    # a one-frame clip: tbox is the box of z alone - w = sqrt((w*h) * (w/h)), h = (w*h) / w - on sides that are no round numbers
    one = rows([[([0.1, 0.2, 33.43, 71.7], .9), ([5.5, 7.25, 6.75, 300.3], .8), ([1e3, 2e3, 1e3 + 1e-3, 2e3 + 7.7], .7)]])
    out.append(("one_frame", one, dict(t_min=1), [[0, 1, 2]], [[1, 1, 1]]))
    # a zero-height box, an infinite and a NaN coordinate beside a sound box: candidates all (their scores are finite), each
    # starts a track whose state holds a NaN, no IoU with it is admissible, so it ages out and the next frame's starts another
    bad = rows([[(_b(0), .9), ([20, 0, 30, 0], .9), ([40, 0, np.inf, 10], .9), ([60, np.nan, 70, 10], .9)]] * 3)
    out.append(("degenerate", bad, dict(t_min=1, max_age=1), [[0, 1, 2, 3], [0, 4, 5, 6], [0, 7, 8, 9]],
                [[3, 1, 1, 1], [3, 1, 1, 1], [3, 1, 1, 1]]))
    # nothing at all
    none = (-np.ones((3, 5, 1), np.float32), -np.ones((3, 5, 1), np.float32), -np.ones((3, 5, 4), np.float32))
    out.append(("all_invalid", none, dict(num_class=2), -np.ones((3, 5), int), np.zeros((3, 5), int)))
    return out


def walkers(seed, T=10, objects=6, classes=2, miss=0.15, size=(16.0, 60.0), speed=6.0, jitter=0.5, extent=400.0):
    """A seeded clip of at most `objects` boxes that move at a constant velocity with a little jitter on every side, each at
    least 16 px a side, each missing from a frame with probability `miss`; the rows of every frame are shuffled.  The generator
    is fixed: tests/test_sort_cpu.py chooses seeds for which the oracle decides every frame with a margin.
    -> (ids, scores, bboxes), N = objects."""
    rng = np.random.RandomState(seed)
    pos = rng.uniform(0.0, extent, (objects, 2))
    vel = rng.uniform(-speed, speed, (objects, 2))
    wh = rng.uniform(size[0], size[1], (objects, 2))
    cls = rng.randint(0, classes, objects)
    score = rng.uniform(0.55, 0.95, objects)
    ids = -np.ones((T, objects, 1), np.float32)
    scores = -np.ones((T, objects, 1), np.float32)
    bboxes = -np.ones((T, objects, 4), np.float32)
    for t in range(T):
        order = rng.permutation(objects)
        seen = rng.uniform(size=objects) >= miss
        jit = rng.uniform(-jitter, jitter, (objects, 4))
        n = 0
        for o in order:
            if seen[o]:
                c = pos[o] + vel[o] * t
                box = np.array([c[0] - wh[o, 0] / 2, c[1] - wh[o, 1] / 2, c[0] + wh[o, 0] / 2, c[1] + wh[o, 1] / 2]) + jit[o]
                ids[t, n, 0], scores[t, n, 0], bboxes[t, n] = cls[o], score[o], box
                n += 1
    return ids, scores, bboxes


def crowded(seed=5, N=128):
    """Two frames of N boxes of one class in a row, 40 x 40 and 4 px apart, so that a box overlaps its six neighbours on either
    side with an IoU above 0.3 (36/44, 32/48, ... 16/64 is the first below); the second frame is the first one shifted by a
    seeded jitter of up to 6 px, its rows in a seeded order: N admissible rows against N tracks, most rows with 13 admissible
    cells, and augmenting paths that displace earlier rows."""
    rng = np.random.RandomState(seed)
    x = 4.0 * np.arange(N)
    ids = np.zeros((2, N, 1), np.float32)
    scores = rng.uniform(0.6, 0.9, (2, N, 1)).astype(np.float32)
    bboxes = np.zeros((2, N, 4), np.float32)
    bboxes[0] = np.stack([x, np.zeros(N), x + 40.0, np.full(N, 40.0)], axis=1)
    order = rng.permutation(N)
    x1 = (x + rng.uniform(-6.0, 6.0, N))[order]
    bboxes[1] = np.stack([x1, np.zeros(N), x1 + 40.0, np.full(N, 40.0)], axis=1)
    return ids, scores, bboxes


def same_tbox(got, want):
    """the pass condition on tbox: equal on the uint32 view wherever the definition's value is not a NaN, a NaN wherever it is"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.isnan(got[nan]).all()) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
