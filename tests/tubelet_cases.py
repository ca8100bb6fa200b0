"""Inputs of the tubelet tests (tests/test_tubelet_cpu.py, tests/test_tubelet_gpu.py): closed forms whose expected outputs are
written out by hand, and random clips (tests/seqnms_cases.py's) linked by track_host, whose holes the pass fills."""
import functools
import itertools

import numpy as np

from tests.seqnms_cases import random_clip
from tests.track_cases import _b, closed_form as track_closed_form, rows
from viddet_amd.track import track_host

f32 = np.float32
SIZES = [(1, 1), (2, 3), (5, 64), (5, 65), (6, 128), (40, 20)]
MAX_AGES = [0, 2, 7]
# every parameter combination: rescore x max_gap x drop_untracked
PARAMS = [dict(rescore=r, max_gap=g, drop_untracked=d) for r, g, d in itertools.product(("avg", "max", None), (0, 2, 7), (False, True))]
BIG = 2 ** 31 - 1


def _lerp(a, b, j, g):
    """the formula of the definition on float32 scalars, one rounding per operation"""
    w = f32(f32(j) / f32(g))
    return f32(f32(a) + f32(f32(f32(b) - f32(a)) * w))


def _avg(*s):
    acc = f32(0)
    for v in s:
        acc = f32(acc + f32(v))
    return f32(acc / f32(len(s)))


def closed_form():
    """[(name, (ids, scores, bboxes), track (F,N), keyword arguments, expected)], `expected` a dict of any of scores (F,N), perm,
    track_out, dropped, ids (F,N) and boxes {(frame, row): box}"""
    out = []

    def add(name, data, track, kw, **expect):
        out.append((name, data, np.asarray(track, np.int32).reshape(data[2].shape[:2]), kw, expect))

    # track_cases' gap clip - a box moving 1 px per frame, frame 2 missing - linked at max_age 1: the hole's box is the midpoint
    gap = dict((c[0], c) for c in track_closed_form())["gap_age1"]
    gap, gap_track = gap[1], gap[3]
    nine, mid = f32(0.9), {(2, 0): [2, 0, 12, 10]}
    whole = dict(perm=[[0], [0], [-2], [0], [0]], track_out=[[0]] * 5, dropped=[0] * 5, ids=[[0]] * 5, boxes=mid)
    add("gap_avg", gap, gap_track, dict(rescore="avg"), scores=[[_avg(nine, nine, nine, nine)]] * 5, **whole)
    add("gap_max", gap, gap_track, dict(rescore="max"), scores=[[nine]] * 5, **whole)
    add("gap_none", gap, gap_track, dict(rescore=None), scores=[[nine]] * 5, **whole)
    # the same boxes with scores that are exact in binary: 2.5 / 4, the maximum, .25 + (.75 - .25) / 2
    exact = (gap[0], np.array([.5, .25, -1, .75, 1.0], f32).reshape(5, 1, 1), gap[2])
    add("gap_exact_avg", exact, gap_track, dict(rescore="avg"), scores=[[.625]] * 5, **whole)
    add("gap_exact_max", exact, gap_track, dict(rescore="max"), scores=[[1.0]] * 5, **whole)
    add("gap_exact_none", exact, gap_track, dict(rescore=None), scores=[[.5], [.25], [.5], [.75], [1.0]], **whole)
    # max_gap 0: nothing is filled, the scores are still the track's
    add("max_gap_0", exact, gap_track, dict(rescore="avg", max_gap=0), scores=[[.625], [.625], [-1], [.625], [.625]],
        perm=[[0], [0], [-1], [0], [0]], track_out=[[0], [0], [-1], [0], [0]], dropped=[0] * 5)
    # a hole of 7 frames, g = 8: the weights j / 8 are exact, [0,0,10,10] -> [8,16,26,42] moves (1,2,2,4) per frame
    far = rows([[(_b(0), .25)]] + [[None]] * 7 + [[([8, 16, 26, 42], .75)]])
    add("hole_7", far, [[0]] * 9, dict(rescore=None, max_gap=7),
        scores=[[.25 + j / 16.0] for j in range(9)], perm=[[0]] + [[-2]] * 7 + [[0]], track_out=[[0]] * 9, dropped=[0] * 9,
        boxes=dict(((j, 0), [j, 2 * j, 10 + 2 * j, 10 + 4 * j]) for j in range(1, 8)))
    add("hole_7_at_max_gap_6", far, [[0]] * 9, dict(rescore=None, max_gap=6),
        perm=[[0]] + [[-1]] * 7 + [[0]], track_out=[[0]] + [[-1]] * 7 + [[0]], dropped=[0] * 9)
    # a hole of 6 frames, g = 7: the weights j / 7 are rounded, every coordinate follows the formula operation by operation
    a7, b7 = [0, 0, 10, 10], [1, 3, 20, 31]
    sev = rows([[(a7, .3)]] + [[None]] * 6 + [[(b7, .8)]])
    add("hole_6_sevenths", sev, [[0]] * 8, dict(rescore=None, max_gap=6),
        scores=[[f32(.3)]] + [[_lerp(f32(.3), f32(.8), j, 7)] for j in range(1, 7)] + [[f32(.8)]],
        perm=[[0]] + [[-2]] * 6 + [[0]], track_out=[[0]] * 8, dropped=[0] * 8,
        boxes=dict(((j, 0), [_lerp(a7[c], b7[c], j, 7) for c in range(4)]) for j in range(1, 7)))
    # a hole of 8 frames at max_gap 7: left empty
    wide = rows([[(_b(0), .5)]] + [[None]] * 8 + [[(_b(9), .5)]])
    add("hole_8", wide, [[0]] * 10, dict(max_gap=7), scores=[[.5]] + [[-1]] * 8 + [[.5]],
        perm=[[0]] + [[-1]] * 8 + [[0]], track_out=[[0]] + [[-1]] * 8 + [[0]], dropped=[0] * 10)
    # a full frame: track 0 skips frame 1, whose two rows are taken: its fill is dropped and counted
    full = rows([[(_b(0), .9), (_b(100), .8)], [(_b(100), .8), (_b(200), .7)], [(_b(2), .9), None]])
    add("full_frame", full, [[0, 1], [1, 2], [0, -1]], dict(rescore=None), dropped=[0, 1, 0],
        perm=[[0, 1], [0, 1], [0, -1]], track_out=[[0, 1], [1, 2], [0, -1]])
    # two fills and one free row: track 0 (row 1 of frame 0) wins over track 1 (row 0), and sorts ahead of the kept row
    two = rows([[(_b(100), .6), (_b(0), .9)], [(_b(200), .7), None], [(_b(4), .9), (_b(104), .6)]])
    add("two_fills_one_row", two, [[1, 0], [2, -1], [0, 1]], dict(rescore=None), dropped=[0, 1, 0], scores=[[.9, .6], [.9, .7], [.9, .6]],
        perm=[[1, 0], [-2, 0], [0, 1]], track_out=[[0, 1], [0, 2], [0, 1]], boxes={(1, 0): [2, 0, 12, 10], (1, 1): _b(200)})
    # an id twice in a frame: the lower row carries it, the other is untracked and keeps its score
    dup = rows([[(_b(0), .5), (_b(50), .875), (_b(100), .75)], [(_b(0), .75), None, (_b(100), .25)]])
    add("duplicate_id", dup, [[0, 0, 1], [0, -1, 1]], dict(rescore="avg"), scores=[[.875, .625, .5], [.625, .5, -1]],
        perm=[[1, 0, 2], [0, 2, -1]], track_out=[[-1, 0, 1], [0, 1, -1]], dropped=[0, 0])
    add("duplicate_id_dropped", dup, [[0, 0, 1], [0, -1, 1]], dict(rescore="avg", drop_untracked=True),
        scores=[[.625, .5, -1], [.625, .5, -1]], perm=[[0, 2, -1], [0, 2, -1]], track_out=[[0, 1, -1], [0, 1, -1]], dropped=[0, 0])
    # ids that are no ids: -1, F * N = 8 and 2**31 - 1; F * N - 1 is the largest that is one
    odd = rows([[(_b(0), .5), (_b(50), .25), (_b(100), .125), (_b(150), .0625)]] * 2)
    add("bad_ids", odd, [[-1, 8, BIG, 7]] * 2, dict(rescore="max"), scores=[[.5, .25, .125, .0625]] * 2,
        perm=[[0, 1, 2, 3]] * 2, track_out=[[-1, -1, -1, 7]] * 2, dropped=[0, 0])
    add("bad_ids_dropped", odd, [[-1, 8, BIG, 7]] * 2, dict(rescore="max", drop_untracked=True), scores=[[.0625, -1, -1, -1]] * 2,
        perm=[[3, -1, -1, -1]] * 2, track_out=[[7, -1, -1, -1]] * 2, dropped=[0, 0])
    # a float32 sum that depends on the order: (1e8 + 1) - 1e8 is 0 in frame order, any other order gives 1 / 3
    big = rows([[(_b(0), 1e8)], [(_b(1), 1.0)], [(_b(2), -1e8)]])
    add("avg_in_frame_order", big, [[0]] * 3, dict(rescore="avg"), scores=[[0.0]] * 3, perm=[[0]] * 3, track_out=[[0]] * 3)
    # -0.0 and 0.0 tie, equal scores keep their order; the bits of a score are carried
    zeros = rows([[(_b(0), 0.0), (_b(20), -0.0), (_b(40), 0.0), (_b(60), .5)]])
    add("zeros_tie", zeros, [[-1] * 4], dict(rescore=None), scores=[[.5, 0.0, -0.0, 0.0]], perm=[[3, 0, 1, 2]], track_out=[[-1] * 4])
    # a fill that ties with the kept rows of its frame comes after them
    tie = rows([[(_b(0), .5), None, None], [(_b(50), .5), (_b(100), .5), None], [(_b(2), .5), None, None]])
    add("fill_ties_last", tie, [[0, -1, -1], [-1, -1, -1], [0, -1, -1]], dict(rescore="max"),
        perm=[[0, -1, -1], [0, 1, -2], [0, -1, -1]], track_out=[[0, -1, -1], [-1, -1, 0], [0, -1, -1]], scores=[[.5, -1, -1], [.5, .5, .5], [.5, -1, -1]])
    add("drop_untracked", tie, [[0, -1, -1], [-1, -1, -1], [0, -1, -1]], dict(rescore="max", drop_untracked=True),
        perm=[[0, -1, -1], [-2, -1, -1], [0, -1, -1]], track_out=[[0, -1, -1]] * 3, scores=[[.5, -1, -1]] * 3, dropped=[0] * 3)
    # NaN and infinite scores and a NaN id are no rows, whatever id the table gives them: they are no members and are not kept
    bad = rows([[(_b(0), .5), (_b(50), .9), (_b(100), .9), (_b(150), .9)], [None] * 4, [(_b(2), .5), (_b(52), .9), (_b(102), .9), (_b(152), .9)]])
    for t in (0, 2):
        bad[1][t, 1, 0], bad[1][t, 2, 0], bad[0][t, 3, 0] = np.nan, np.inf, np.nan
    bad[1][2, 2, 0] = -np.inf
    add("non_finite", bad, [[0, 1, 2, 3], [-1] * 4, [0, 1, 2, 3]], dict(rescore="avg"), scores=[[.5, -1, -1, -1]] * 3,
        perm=[[0, -1, -1, -1], [-2, -1, -1, -1], [0, -1, -1, -1]], track_out=[[0, -1, -1, -1]] * 3, dropped=[0] * 3,
        boxes={(1, 0): [1, 0, 11, 10]})
    # an empty clip between two clips whose ids both start at 0: nothing is filled across a boundary, each hole inside is
    clips = rows([[(_b(0), .5)], [None], [(_b(2), .5)], [(_b(50), .25)], [None], [(_b(54), .25)]])
    add("three_clips", clips, [[0], [-1], [0], [0], [-1], [0]], dict(clip_start=[0, 3, 3, 6]), scores=[[.5]] * 3 + [[.25]] * 3,
        perm=[[0], [-2], [0]] * 2, track_out=[[0]] * 6, boxes={(1, 0): [1, 0, 11, 10], (4, 0): [52, 0, 62, 10]})
    # ids are per clip: 3 would be an id in one clip of 6 frames of one row, in a clip of 3 frames it is none
    add("clip_bounds_the_ids", clips, [[3], [-1], [3], [3], [-1], [3]], dict(clip_start=[0, 3, 3, 6]), perm=[[0], [-1], [0]] * 2,
        track_out=[[-1]] * 6, scores=[[.5], [-1], [.5], [.25], [-1], [.25]])
    none = (-np.ones((3, 5, 1), f32), -np.ones((3, 5, 1), f32), -np.ones((3, 5, 4), f32))
    add("all_invalid", none, np.zeros((3, 5), int), dict(num_class=2), scores=-np.ones((3, 5)), perm=-np.ones((3, 5), int),
        track_out=-np.ones((3, 5), int), dropped=[0, 0, 0], ids=-np.ones((3, 5)))
    return out


def check_expected(got, expect):
    """the hand-written values of a closed form against the six outputs (scores by value AND sign)"""
    ids, scores, bboxes, perm, track_out, dropped = got
    F, N = perm.shape
    if "scores" in expect:
        want = np.asarray(expect["scores"], f32).reshape(F, N)
        assert np.array_equal(scores.reshape(F, N), want) and np.array_equal(np.signbit(scores.reshape(F, N)), np.signbit(want)), scores.reshape(F, N)
    if "ids" in expect:
        assert np.array_equal(ids.reshape(F, N), np.asarray(expect["ids"], f32).reshape(F, N))
    for key, value in (("perm", perm), ("track_out", track_out), ("dropped", dropped)):
        if key in expect:
            assert value.tolist() == np.asarray(expect[key]).tolist(), (key, value.tolist())
    for (t, i), box in expect.get("boxes", {}).items():
        assert np.array_equal(bboxes[t, i], np.asarray(box, f32)), (t, i, bboxes[t, i])


@functools.lru_cache(maxsize=None)
def random_case(T, N, max_age):
    """(ids, scores, bboxes, track): a random clip and track_host's ids on it at `max_age` (t_min 1, sigma_h 0: every track kept)"""
    case = random_clip(T, N, seed=7 * T + N, spread=40.0 + N, fill=1.0 if N < 4 else 0.8)
    track = track_host(*case, max_age=max_age, t_min=1, sigma_h=0.0)[0]
    return case + (track,)


RANDOM = [(T, N, a) for (T, N) in SIZES for a in MAX_AGES]


def three_clips():
    """three random clips of unequal length behind one another -> (ids, scores, bboxes, track, clip_start)"""
    parts = [random_case(5, 64, 2), random_case(40, 20, 7), random_case(6, 128, 7)]
    N = 128
    outs = []
    for k in range(4):
        padded = []
        for p in parts:
            a = p[k]
            pad = np.full((a.shape[0], N - a.shape[1]) + a.shape[2:], -1, a.dtype)
            padded.append(np.concatenate([a, pad], axis=1))
        outs.append(np.concatenate(padded))
    return tuple(outs) + ([0, 5, 45, 51],)
