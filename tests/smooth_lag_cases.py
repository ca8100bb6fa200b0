"""Inputs of the fixed-lag smoothing tests (tests/test_smooth_lag_cpu.py, tests/test_smooth_lag_gpu.py): the closed forms of
tests/smooth_cases.py as streams, seeded clips under the ids of the three online trackers, and the helpers that cut a stream
into calls."""
import functools

import numpy as np

from tests import byte_cases as BC
from tests import smooth_cases as MC
from tests import sort_cases as SC
from viddet_amd.byte import byte_online_host
from viddet_amd.smooth import smooth_host
from viddet_amd.smooth_lag import smooth_lag_host
from viddet_amd.sort import sort_online_host
from viddet_amd.track import track_online_host

LAGS = [0, 1, 3, 7, 15]
GAPS = [0, 1, 7]


def closed_forms():
    """name -> (ids, scores, bboxes, track): every closed form of smooth_cases whose table keeps the causal id bound"""
    return dict(still=MC.still(), still_holes=MC.still([0, 1, 4, 5, 6, 9]), outlier=MC.outlier(), holed=MC.holed(),
                long_thin=MC.long_thin(), nan=MC.nan_case(), moving=MC.moving(list(range(0, 24, 2)) + [24, 25, 33, 34, 35]))


@functools.lru_cache(maxsize=None)
def tracked(tracker, seed, T=40, objects=6):
    """(ids, scores, bboxes, track): a seeded clip under the ids of an ONLINE tracker at max_age 3 - 'sort' and 'iou' on
    sort_cases.walkers, 'byte' on byte_cases.dipped"""
    gen = dict(T=T, objects=objects, miss=0.25, jitter=1.0)
    if tracker == "byte":
        case = BC.dipped(seed, **gen)
        track = byte_online_host(None, *case, num_class=2, max_age=3)[1]
    elif tracker == "sort":
        case = SC.walkers(seed, **gen)
        track = sort_online_host(None, *case, num_class=2, max_age=3)[1]
    else:
        case = SC.walkers(seed, **gen)
        track = track_online_host(None, *case, num_class=2, sigma_iou=0.3, max_age=3)[1]
    return tuple(case) + (np.asarray(track, np.int32),)


def within_bound(track):
    """the causal id bound of the definition: track[t, i] < (t + 1) * N"""
    T, N = track.shape
    return bool((track < (np.arange(T)[:, None] + 1) * N).all())


_PREFIX = {}


def prefix(key, case, h, num_class, max_gap):
    """smooth_host on the frames [0, h] of `case`, kept per (key, h, num_class, max_gap): it does not depend on the lag"""
    k = (key, h, num_class, max_gap)
    if k not in _PREFIX:
        ids, scores, bboxes, track = case
        _PREFIX[k] = smooth_host(ids[:h + 1], scores[:h + 1], bboxes[:h + 1], track[:h + 1], None, num_class, max_gap)
    return _PREFIX[k]


def parts_of(F):
    """all at once, one frame per call, (1, 3, rest)"""
    out = [(F,), (1,) * F]
    if F > 4:
        out.append((1, 3, F - 4))
    return out


def run_host(case, num_class, lag, max_gap, parts=None):
    """the stream through smooth_lag_host in calls of `parts` frames and a flush of no frames -> (sbox (T,N,4), slen (T,N))"""
    ids, scores, bboxes, track = case
    T = bboxes.shape[0]
    state, t, boxes, lens, expect = None, 0, [], [], 0
    for n in list(parts or (T,)) + [0]:
        last = t == T and n == 0
        state, t0, b, s = smooth_lag_host(state, ids[t:t + n], scores[t:t + n], bboxes[t:t + n], track[t:t + n], num_class, lag,
                                          max_gap, flush=last)
        assert t0 == expect and b.shape[0] == s.shape[0]
        t += n
        expect += b.shape[0]
        if not last:
            assert expect == max(0, t - lag) and state["frames"] == t and state["emitted"] == expect
        boxes.append(b), lens.append(s)
    assert state is None and expect == T
    return np.concatenate(boxes), np.concatenate(lens)
