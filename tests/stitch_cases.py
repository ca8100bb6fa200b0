"""Inputs of the stitching tests (tests/test_stitch_cpu.py, tests/test_stitch_gpu.py): the closed forms of DESIGN.md 38, tables
of sort_host with occlusion holes cut into every object, the cap case, the two widest cases and several clips behind one
another.  A case is (ids, scores, bboxes, track)."""
import functools

import numpy as np

from tests.sort_cases import walkers
from viddet_amd.sort import sort_host

f32 = np.float32
KEEP_ALL = dict(t_min=1, sigma_h=0.0)                # every track of the tracker is kept


def build(F, entries, N=None):
    """entries: (frame, box, score, class, track id), packed into the rows of their frame in the order given"""
    per = [[e for e in entries if e[0] == t] for t in range(F)]
    N = N or max(1, max(len(p) for p in per))
    ids, scores = -np.ones((F, N, 1), f32), -np.ones((F, N, 1), f32)
    bboxes, track = -np.ones((F, N, 4), f32), -np.ones((F, N), np.int32)
    for t, p in enumerate(per):
        for i, (_, box, s, c, u) in enumerate(p):
            ids[t, i, 0], scores[t, i, 0], bboxes[t, i], track[t, i] = c, s, box, u
    return ids, scores, bboxes, track


def mover(frames, x0=100.0, vx=12.0, y0=50.0, seed=0, jitter=1.0, score=0.9, cls=0, track=0):
    """the entries of a 40 x 80 box that moves vx px a frame with a seeded jitter on every side, at `frames`"""
    rng = np.random.RandomState(seed)
    jit = rng.uniform(-jitter, jitter, (max(frames) + 1, 4))
    return [(t, np.array([x0 + vx * t, y0, x0 + vx * t + 40.0, y0 + 80.0]) + jit[t], score, cls, track) for t in frames]


def tracked(data, **kw):
    """(ids, scores, bboxes) and sort_host's ids on them"""
    kw = dict(dict(max_age=1), **kw)
    return tuple(data) + (sort_host(*data, **kw)[0],)


@functools.lru_cache(maxsize=None)
def hidden_one():
    """one object, visible in frames 0..9 and 22..31, SORT at max_age 1: tracks 0 and 1, 13 frames between tail and head"""
    return tracked(build(32, mover(list(range(10)) + list(range(22, 32))))[:3])


@functools.lru_cache(maxsize=None)
def crossing():
    """two objects that cross behind an occluder, +12 and -12 px a frame, hidden in frames 10..19: tracks 0, 1 and 2, 3"""
    seen = list(range(10)) + list(range(20, 30))
    return tracked(build(30, mover(seen, 100.0, 12.0, seed=1) + mover(seen, 460.0, -12.0, seed=2))[:3])


@functools.lru_cache(maxsize=None)
def other_class():
    """hidden_one whose second fragment is of class 1"""
    return tracked(build(32, mover(list(range(10))) + mover(list(range(22, 32)), cls=1))[:3], num_class=2)


@functools.lru_cache(maxsize=None)
def three_fragments():
    """one object visible in frames 0..7, 14..21 and 28..35: tracks 0, 1, 2; the scores 0.7, 0.9, 0.8"""
    e = mover(list(range(8)), score=0.7) + [(t, b, 0.9, c, u) for t, b, _, c, u in mover(list(range(14, 22)))] + \
        [(t, b, 0.8, c, u) for t, b, _, c, u in mover(list(range(28, 36)))]
    return tracked(build(36, e)[:3])


def compete():
    """tracks 0 (at x = 0) and 1 (at x = 10) stand still in frames 0..2; track 2 appears at x = 2 in frames 5 and 6: both tails
    reach its head, track 0 at an IoU of 38/42, track 1 at 32/48"""
    b = lambda x: [x, 0.0, x + 40.0, 80.0]
    e = []
    for t in range(3):
        e += [(t, b(0.0), .9, 0, 0), (t, b(10.0), .8, 0, 1)]
    e += [(5, b(2.0), .7, 0, 2), (6, b(2.0), .7, 0, 2)]
    return build(7, e)


def nan_head():
    """hidden_one with a NaN in the second fragment's first box"""
    ids, scores, bboxes, track = hidden_one()
    bboxes = bboxes.copy()
    bboxes[22, 0, 1] = np.nan
    return ids, scores, bboxes, track


def nan_tail():
    """hidden_one with a NaN in the first fragment's last box"""
    ids, scores, bboxes, track = hidden_one()
    bboxes = bboxes.copy()
    bboxes[9, 0, 2] = np.nan
    return ids, scores, bboxes, track


def _grid(shift):
    """128 boxes of 10 px on a 16 x 8 grid 20 px apart"""
    i = np.arange(128)
    x, y = 20.0 * (i % 16) + shift, 20.0 * (i // 16) + shift
    return np.stack([x, y, x + 10.0, y + 10.0], axis=1).astype(f32)


@functools.lru_cache(maxsize=None)
def cap():
    """F = 5, N = 128: the odd frames' grid is shifted by a box, so no box overlaps one of the frame before, and SORT at max_age 0
    makes 640 tracks of one row; the boxes of frame t + 2 sit on frame t's"""
    ids = np.zeros((5, 128, 1), f32)
    scores = np.random.RandomState(7).uniform(0.5, 0.9, (5, 128, 1)).astype(f32)
    bboxes = np.stack([_grid(10.0 * (t % 2)) for t in range(5)])
    case = tracked((ids, scores, bboxes), max_age=0, **KEEP_ALL)
    assert case[3].max() == 639
    return case


@functools.lru_cache(maxsize=None)
def sparse_wide():
    """F = 6, N = 128: 128 objects on the grid drift 1 px a frame, seen in frames 0, 1 and 4, 5: 256 tracks, 128 links"""
    ids = np.zeros((6, 128, 1), f32)
    scores = np.random.RandomState(8).uniform(0.5, 0.9, (6, 128, 1)).astype(f32)
    bboxes = np.stack([_grid(1.0 * t) for t in range(6)])
    ids[2:4], scores[2:4], bboxes[2:4] = -1, -1, -1
    case = tracked((ids, scores, bboxes), **KEEP_ALL)
    assert case[3].max() == 255
    return case


@functools.lru_cache(maxsize=None)
def crowded_wide(seed=5):
    """32 boxes of 40 px, 1 px apart, seen in frames 0, 1 and - shifted by a seeded jitter of up to 3 px, in a seeded row order -
    in frames 4, 5: at sigma_iou 0.05 every one of the 32 tails reaches every one of the 32 heads"""
    rng = np.random.RandomState(seed)
    x = 1.0 * np.arange(32)
    ids = np.zeros((6, 32, 1), f32)
    scores = rng.uniform(0.5, 0.9, (6, 32, 1)).astype(f32)
    bboxes = -np.ones((6, 32, 4), f32)
    for t in (0, 1):
        bboxes[t] = np.stack([x, np.zeros(32), x + 40.0, np.full(32, 40.0)], axis=1)
    for t in (4, 5):
        x1 = (x + rng.uniform(-3.0, 3.0, 32))[rng.permutation(32)]
        bboxes[t] = np.stack([x1, np.zeros(32), x1 + 40.0, np.full(32, 40.0)], axis=1)
    ids[2:4], scores[2:4] = -1, -1
    return tracked((ids, scores, bboxes), **KEEP_ALL)


def cut_holes(data, seed, lo=2, hi=None):
    """sort_cases.walkers rows with an occlusion cut out of every object: walkers keeps an object's score constant, so the rows
    of one score are one object; a seeded run of lo .. hi frames of it is removed"""
    ids, scores, bboxes = (a.copy() for a in data)
    F = ids.shape[0]
    if F < 3:                                        # nothing to cut a hole into
        return ids, scores, bboxes
    hi = max(lo, F // 2) if hi is None else hi
    rng = np.random.RandomState(seed)
    for s in np.unique(scores[scores >= 0]):
        n = rng.randint(lo, hi + 1)
        a = rng.randint(0, max(1, F - n))
        gone = (scores[a:a + n, :, 0] == s)
        ids[a:a + n][gone], scores[a:a + n][gone], bboxes[a:a + n][gone] = -1, -1, -1
    return ids, scores, bboxes


HOLED_SIZES = [(1, 1), (6, 63), (12, 64), (40, 65), (16, 128), (40, 20)]


@functools.lru_cache(maxsize=None)
def holed(F, N, max_age=1, seed=None):
    """sort_host's table (every track kept) on walkers at (F, N) with a hole cut into every object"""
    seed = 5 * F + N if seed is None else seed
    data = cut_holes(walkers(seed, T=F, objects=N, miss=0.1, jitter=1.0, extent=400.0 + 8.0 * N), seed)
    return tracked(data, num_class=2, max_age=max_age, **KEEP_ALL)


def pad_cat(parts, N=128):
    """cases of unequal shape behind one another, padded to N rows -> (ids, scores, bboxes, track, clip_start)"""
    outs = []
    for k in range(4):
        padded = []
        for p in parts:
            a = p[k]
            padded.append(np.concatenate([a, np.full((a.shape[0], N - a.shape[1]) + a.shape[2:], -1, a.dtype)], axis=1))
        outs.append(np.concatenate(padded))
    return tuple(outs) + ([0] + [int(c) for c in np.cumsum([p[0].shape[0] for p in parts])],)


def three_clips():
    return pad_cat([holed(12, 64), crossing(), cap()])


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    return got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def same_five(got, want):
    """all five outputs equal, the float one on its int32 view"""
    return (len(got) == len(want) == 5 and all(np.array_equal(np.asarray(got[k]), np.asarray(want[k])) for k in (0, 1, 3, 4))
            and all(np.asarray(got[k]).dtype == np.int32 for k in (0, 1, 3, 4)) and same_bits(got[2], want[2]))
