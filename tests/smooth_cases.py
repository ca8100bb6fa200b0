"""Inputs of the smoothing tests (tests/test_smooth_cpu.py, tests/test_smooth_gpu.py): the closed forms, seeded tables from
sort_host on sort_cases.walkers, seeded hostile tables, jittered constant-velocity tracks with missing frames, one long thin
clip and three clips of unequal length."""
import functools

import numpy as np

from tests.sort_cases import GPU_SIZES, walkers
from tests.track_cases import rows
from viddet_amd.sort import sort_host

f32 = np.float32
GAPS = [0, 2, 7]
STILL = [32.0, 64.0, 48.0, 80.0]                     # power-of-two sides: u, v, s, r and every filter step on them are exact


def one_track(frames, boxes, F=None):
    """a clip of one row a frame: `boxes[k]` at frame `frames[k]`, nothing elsewhere -> (ids, scores, bboxes, track)"""
    F = (max(frames) + 1) if F is None else F
    at = dict(zip(frames, boxes))
    data = rows([[(list(at[t]), .9)] if t in at else [None] for t in range(F)])
    track = np.array([[0 if t in at else -1] for t in range(F)], np.int32)
    return data + (track,)


def still(frames=range(6)):
    return one_track(list(frames), [STILL] * len(list(frames)))


def outlier():
    """a stationary track of 6 frames whose frame 3 lies 6 px to the right"""
    boxes = [list(STILL) for _ in range(6)]
    boxes[3] = [STILL[0] + 6.0, STILL[1], STILL[2] + 6.0, STILL[3]]
    return one_track(list(range(6)), boxes)


def moving(frames, seed=0):
    """a 40 x 80 box that moves (5, -3) px a frame with a seeded jitter of 1 px on every side, at `frames`"""
    rng = np.random.RandomState(seed)
    boxes = [np.array([100.0 + 5 * t, 300.0 - 3 * t, 140.0 + 5 * t, 380.0 - 3 * t]) + rng.uniform(-1, 1, 4) for t in frames]
    return one_track(list(frames), boxes)


def holed():
    """frames 0..4 and 9..13: a hole of 4 frames"""
    return moving(list(range(5)) + list(range(9, 14)))


def long_thin():
    """(40, 2): one moving object with holes of 1, 2, 3 and 7 frames, alternating between the two rows; the deepest serial chain"""
    frames = [t for t in range(40) if t not in (3, 8, 9, 15, 16, 17, 24, 25, 26, 27, 28, 29, 30)]
    ids, scores, bboxes, track = moving(frames, seed=4)
    pad = lambda a, v: np.concatenate([a, np.full_like(a, v)], axis=1)
    ids, scores, bboxes, track = pad(ids, -1), pad(scores, -1), pad(bboxes, -1), pad(track, -1)
    for a in (ids, scores, bboxes, track):
        a[1::2] = a[1::2, ::-1].copy()                # the odd frames' object sits in row 1
    return ids, scores, bboxes, track


def keep_cases():
    """(ids, scores, bboxes, track, clip_start, expected slen (F,N)): every row keeps its input bits -
    frame 0: a one-member segment (id 0), a non-member (id -1), an id outside [0, T * N), a row of score -1 with a usable id;
    frames 1 and 2 (a clip of their own): id 1 in rows 0 and 1 of both frames - the higher row repeats it and is no member; the
    lower rows are a segment of two, the only rows that move; frame 3 (a clip): id 2 twice, a one-member segment and its repeat."""
    b = lambda x: [x, 10.0, x + 20.0, 50.0]
    data = rows([[(b(0), .9), (b(30), .9), (b(60), .9), None],
                 [(b(0), .9), (b(3), .8), None, None],
                 [(b(2), .9), (b(5), .8), None, None],
                 [(b(0), .9), (b(1), .9), None, None]])
    track = np.array([[0, -1, 4, 1], [1, 1, -1, -1], [1, 1, -1, -1], [2, 2, -1, -1]], np.int32)
    slen = np.array([[1, 0, 0, 0], [2, 0, 0, 0], [2, 0, 0, 0], [1, 0, 0, 0]], np.int32)
    return data + (track, [0, 1, 3, 4], slen)


def nan_case():
    """two tracks of 6 frames side by side: row 0's box of frame 2 holds a NaN, row 1 is sound"""
    a = moving(list(range(6)), seed=1)
    b = moving(list(range(6)), seed=2)
    ids, scores = np.concatenate([a[0], b[0]], axis=1), np.concatenate([a[1], b[1]], axis=1)
    bboxes = np.concatenate([a[2], b[2] + f32(200)], axis=1)
    bboxes[2, 0, 1] = np.nan
    track = np.concatenate([a[3], b[3] + 1], axis=1).astype(np.int32)
    return ids, scores, bboxes, track


@functools.lru_cache(maxsize=None)
def sort_table(F, N, max_age, seed=None):
    """(ids, scores, bboxes, track): sort_cases.walkers at (F, N) and sort_host's ids on it (t_min 1, sigma_h 0: every track kept)"""
    seed = 3 * F + N if seed is None else seed
    case = walkers(seed, T=F, objects=N, miss=0.25, jitter=1.0, extent=400.0 + 8.0 * N)
    track = sort_host(*case, num_class=2, max_age=max_age, t_min=1, sigma_h=0.0)[0]
    return case + (track,)


SORT_TABLES = [(F, N, a) for (F, N) in GPU_SIZES for a in (1, 7)]


@functools.lru_cache(maxsize=None)
def hostile(F, N, seed=0):
    """(ids, scores, bboxes, track): ids drawn from [-2, F*N + 3) - most of them from a few values, so that tracks have several
    members and ids repeat within a frame; a share of rows with score -1; boxes with zero height, an infinity and a NaN"""
    rng = np.random.RandomState(seed + 31 * F + N)
    ids = np.zeros((F, N, 1), f32)
    scores = rng.uniform(0.1, 0.9, (F, N, 1)).astype(f32)
    xy = rng.uniform(0, 500, (F, N, 2))
    wh = rng.uniform(8, 80, (F, N, 2))
    bboxes = np.concatenate([xy, xy + wh], axis=2).astype(f32)
    few = rng.randint(0, max(2, N // 2), (F, N))
    wide = rng.randint(-2, F * N + 3, (F, N))
    track = np.where(rng.uniform(size=(F, N)) < 0.8, few, wide).astype(np.int32)
    track[:, : min(N, 3)] = np.array([-2, F * N + 2, F * N - 1], np.int32)[: min(N, 3)]
    gone = rng.uniform(size=(F, N)) < 0.15
    ids[gone], scores[gone] = -1, -1
    kind = rng.randint(0, 40, (F, N))
    bboxes[..., 3] = np.where(kind == 0, bboxes[..., 1], bboxes[..., 3])            # zero height
    bboxes[..., 2] = np.where(kind == 1, np.inf, bboxes[..., 2])
    bboxes[..., 0] = np.where(kind == 2, np.nan, bboxes[..., 0])
    return ids, scores, bboxes, track


@functools.lru_cache(maxsize=None)
def cv_tracks(count=200, seed=0, jitter=0.5, miss=0.15):
    """`count` seeded constant-velocity tracks of 2 to 40 frames, each a clip of its own with one row a frame: `jitter` px on
    every side, a share `miss` of the frames missing, coordinates up to about 650 -> (ids, scores, bboxes, track, clip_start)"""
    rng = np.random.RandomState(seed)
    parts, cs = [], [0]
    for _ in range(count):
        T = rng.randint(2, 41)
        wh = rng.uniform(16, 120, 2)
        vel = rng.uniform(-6, 6, 2)
        lo = np.maximum(0, -vel * T) + wh / 2
        hi = np.minimum(650, 650 - vel * T) - wh / 2
        pos = rng.uniform(lo, np.maximum(lo + 1, hi))
        frames = [t for t in range(T) if rng.uniform() >= miss]
        boxes = [np.concatenate([pos + vel * t - wh / 2, pos + vel * t + wh / 2]) + rng.uniform(-jitter, jitter, 4) for t in frames]
        parts.append(one_track(frames, boxes, F=T) if frames else one_track([], [], F=T))
        cs.append(cs[-1] + T)
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4)) + (cs,)


def three_clips():
    """three clips of unequal length behind one another, padded to 128 rows -> (ids, scores, bboxes, track, clip_start)"""
    parts = [sort_table(6, 65, 1), long_thin(), sort_table(12, 128, 7)]
    N = 128
    outs = []
    for k in range(4):
        padded = []
        for p in parts:
            a = p[k]
            padded.append(np.concatenate([a, np.full((a.shape[0], N - a.shape[1]) + a.shape[2:], -1, a.dtype)], axis=1))
        outs.append(np.concatenate(padded))
    return tuple(outs) + ([0, 6, 46, 58],)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def second_difference(boxes):
    """the mean absolute second difference of (n,4) boxes at consecutive frames"""
    b = np.asarray(boxes, np.float64)
    return np.abs(b[2:] - 2 * b[1:-1] + b[:-2])
