"""CPU: the definition of fixed-lag smoothing (viddet_amd.smooth_lag.smooth_lag_host), none of which touches a GPU.

Truncation: every emitted frame u equals row u of smooth_host on the frames [0, min(u + lag, T - 1)], bit for bit, on tables of
the three online trackers and on the closed forms of tests/smooth_cases.py - the resumable loop never calls smooth_host, so
this is a real test of it.  Then partitions, the full lag, lag 0 against the trackers' filtered boxes, gaps and cuts, the rows
that keep their bits, streams behind one another and empty pushes; then the plumbing: the ABI of vd_track_smooth_push, the
`smooth` option of open_video and the script's --track_smooth_lag.  Every comparison is exact."""
import copy
import os
import re

import numpy as np
import pytest

from tests import smooth_cases as MC
from tests import smooth_lag_cases as LC
from tests import sort_cases as SC
from tests.track_cases import rows
from viddet_amd.byte import byte_online_host
from viddet_amd.smooth import smooth_host
from viddet_amd.smooth_lag import DEFAULTS, MAX_LAG, RING, check_params, parse_option, smooth_lag_host
from viddet_amd.sort import sort_online_host


def _truncation(key, case, num_class, lag, max_gap, parts=None):
    """the stream against smooth_host on every prefix -> the rows that moved"""
    assert LC.within_bound(case[3]), "the case is outside the property's premise"
    sbox, slen = LC.run_host(case, num_class, lag, max_gap, parts)
    T = case[2].shape[0]
    assert sbox.dtype == np.float32 and slen.dtype == np.int32 and sbox.shape == case[2].shape
    for u in range(T):
        want, wlen = LC.prefix(key, case, min(u + lag, T - 1), num_class, max_gap)
        assert MC.same_bits(sbox[u], want[u]) and np.array_equal(slen[u], wlen[u]), (key, u, lag, max_gap)
    return int((sbox.view(np.uint32) != case[2].view(np.uint32)).any(axis=2).sum())


# ------------------------------------------------------------------------------------------------ truncation
@pytest.mark.parametrize("max_gap", LC.GAPS)
@pytest.mark.parametrize("tracker", ["sort", "byte", "iou"])
def test_every_emitted_frame_is_smooth_host_on_the_frames_up_to_its_horizon(tracker, max_gap):
    case = LC.tracked(tracker, 1)                                          # T = 40: the 16-slot ring wraps more than twice
    assert case[2].shape[0] == 40 > 2 * RING and (case[3] >= 0).sum() > 100
    moved = [_truncation((tracker, 1), case, 2, lag, max_gap) for lag in LC.LAGS]
    assert min(moved) > 50, moved
    if max_gap == 7:                                                       # another clip, shorter than the ring
        short = LC.tracked(tracker, 2, T=11, objects=9)
        for lag in (3, 15):
            assert _truncation((tracker, 2), short, 2, lag, max_gap) > 20


@pytest.mark.parametrize("name", sorted(LC.closed_forms()))
def test_truncation_holds_on_the_closed_forms(name):
    case = LC.closed_forms()[name]
    for max_gap in (2, 7):
        for lag in LC.LAGS:
            _truncation(name, case, None, lag, max_gap)


# ------------------------------------------------------------------------------------------------ partitions
@pytest.mark.parametrize("tracker", ["sort", "byte", "iou"])
def test_any_cutting_of_a_stream_gives_the_bits_of_one_call(tracker):
    case = LC.tracked(tracker, 3, T=21, objects=7)
    for lag, max_gap in ((0, 7), (3, 1), (7, 7), (15, 0)):
        whole = LC.run_host(case, 2, lag, max_gap)
        for parts in LC.parts_of(21)[1:]:
            got = LC.run_host(case, 2, lag, max_gap, parts)
            assert MC.same_bits(got[0], whole[0]) and np.array_equal(got[1], whole[1]), (lag, max_gap, parts)


def test_the_state_given_is_not_changed():
    ids, scores, bboxes, track = LC.tracked("sort", 3, T=21, objects=7)
    state, *_ = smooth_lag_host(None, ids[:9], scores[:9], bboxes[:9], track[:9], 2, 3)
    keep = copy.deepcopy(state)
    a = smooth_lag_host(state, ids[9:14], scores[9:14], bboxes[9:14], track[9:14], 2, 3)
    b = smooth_lag_host(state, ids[9:14], scores[9:14], bboxes[9:14], track[9:14], 2, 3, flush=True)
    assert a[1] == b[1] == 6 and a[2].shape[0] == 5 and b[2].shape[0] == 8 and b[0] is None and a[0]["frames"] == 14

    def same(x, y):
        if isinstance(x, dict):
            return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
        return np.array_equal(x, y, equal_nan=True) if isinstance(x, np.ndarray) else x == y
    assert same(state, keep) and not same(state, a[0])
    assert MC.same_bits(a[2], b[2][:5])


# ------------------------------------------------------------------------------------------------ the full lag, lag 0
def test_a_lag_of_the_clip_length_is_smooth_host_on_the_clip():
    for tracker in ("sort", "byte", "iou"):
        case = LC.tracked(tracker, 4, T=16, objects=8)                     # lag 15 >= T - 1
        for max_gap in LC.GAPS:
            want = smooth_host(*case, None, 2, max_gap)
            for parts in LC.parts_of(16):
                got = LC.run_host(case, 2, 15, max_gap, parts)
                assert MC.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    for name, case in LC.closed_forms().items():
        T = case[2].shape[0]
        if T - 1 <= MAX_LAG:
            want = smooth_host(*case)
            got = LC.run_host(case, None, T - 1, 7)
            assert MC.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), name


@pytest.mark.parametrize("tracker", ["sort", "byte"])
def test_lag_0_gives_the_trackers_filtered_boxes(tracker):
    online = dict(sort=sort_online_host, byte=byte_online_host)[tracker]
    total = 0
    for seed in range(4):
        case = LC.tracked(tracker, seed, T=24, objects=8)[:3]
        _, track, tlen, _, tbox = online(None, *case, num_class=2, max_age=3)
        for max_gap in (3, 7):                                             # max_gap >= the tracker's max_age: a track is one segment
            sbox, slen = LC.run_host(case + (track,), 2, 0, max_gap, (1,) * 24)
            on = track >= 0
            assert np.array_equal(slen[on], tlen[on]) and not slen[~on].any()
            later = on & (tlen >= 2)                                       # a member that is not its segment's first
            assert SC.same_tbox(sbox[later], tbox[later])
            assert MC.same_bits(sbox[~later], case[2][~later])             # a first member is a segment of one at its own horizon
        total += int(later.sum())
    assert total > 300


# ------------------------------------------------------------------------------------------------ gaps and cuts
@pytest.mark.parametrize("max_gap", [0, 2, 7])
def test_a_gap_of_max_gap_plus_1_frames_links_and_one_more_cuts(max_gap):
    for extra, linked in ((1, True), (2, False)):
        frames = [0, 1, 2, 2 + max_gap + extra, 3 + max_gap + extra]
        case = MC.moving(frames, seed=7)
        T = frames[-1] + 1
        sbox, slen = LC.run_host(case, None, 15, max_gap)                  # T <= 13: the whole clip is every frame's horizon
        assert slen[frames, 0].tolist() == ([5] * 5 if linked else [3, 3, 3, 2, 2])
        want = smooth_host(*case, max_gap=max_gap)
        assert MC.same_bits(sbox, want[0]) and np.array_equal(slen, want[1]) and T <= 13
        head = LC.run_host(tuple(a[:3] for a in case), None, 15, max_gap)
        assert MC.same_bits(sbox[:3], head[0]) != linked                   # the later members reach the first three iff linked


def test_a_successor_beyond_the_horizon_does_not_count_yet():
    frames = [0, 1, 2, 6, 7]                                               # the gap from 2 to 6: 4 frames
    case = MC.moving(frames, seed=9)
    for lag in range(0, 8):
        sbox, slen = LC.run_host(case, None, lag, 7, (1,) * 8)
        # at u + lag < 6 the member at frame 2 is its truncated segment's last: the box of its forward posterior, slen 3
        want = [min(5, sum(f <= min(u + lag, 7) for f in frames)) for u in frames]
        assert slen[frames, 0].tolist() == want, lag
        alone = smooth_host(*[a[:3] for a in case])
        assert MC.same_bits(sbox[2], alone[0][2]) == (lag < 4)
    assert not slen[[3, 4, 5]].any() and MC.same_bits(sbox[[3, 4, 5]], case[2][[3, 4, 5]])


# ------------------------------------------------------------------------------------------------ rows that keep their bits
def test_rows_that_keep_their_input_bits():
    b = lambda x: [x, 10.0, x + 20.0, 50.0]
    N = 4
    ids, scores, bboxes = rows([[(b(0), .9), (b(30), .9), (b(60), .9), (b(90), .9)],       # frame 0: ids below 4 are usable
                                [(b(2), .9), (b(5), .8), (b(62), .9), (b(92), .9)],         # frame 1: below 8
                                [(b(4), .9), None, (b(64), .9), (b(94), .9)]])              # frame 2: below 12
    track = np.array([[0, -1, 4, 3],        # a member; a non-member; an id AT (t + 1) * N; a member
                      [0, 0, 9, 8],         # a member; its repeat in a higher row; an id above the bound; an id AT the bound
                      [0, 5, 9, 8]], np.int32)      # row 1 is not present; 9 and 8 are usable now - each a segment of one
    for lag in (0, 1, 15):
        sbox, slen = LC.run_host((ids, scores, bboxes, track), None, lag, 7)
        h = [min(u + lag, 2) for u in range(3)]
        assert slen.tolist() == [[h[0] + 1, 0, 0, 1], [h[1] + 1, 0, 0, 0], [3, 0, 1, 1]], lag
        moved = (sbox.view(np.uint32) != bboxes.view(np.uint32)).any(axis=2)
        assert moved.tolist() == (slen >= 2).tolist(), lag                 # only the members of a segment of two or more move
    # a NaN box keeps the input wherever it reaches, and no other row sees it
    ids, scores, bboxes, track = MC.nan_case()
    for lag in (0, 2, 5):
        sbox, slen = LC.run_host((ids, scores, bboxes, track), None, lag, 7)
        assert slen[:, 0].tolist() == [min(u + lag, 5) + 1 for u in range(6)]
        reach = [u for u in range(6) if min(u + lag, 5) >= 2 and (u >= 2 or lag > 0)]      # the NaN is in the row's segment ...
        reach = sorted(set(reach) | ({0} if lag == 0 else set()))                          # ... or the segment has one member
        for u in range(6):
            assert MC.same_bits(sbox[u, 0], bboxes[u, 0]) == (u in reach), (lag, u)
        assert np.isnan(sbox).sum() == 1 and np.isnan(sbox[2, 0, 1])
        alone = LC.run_host((ids[:, 1:], scores[:, 1:], bboxes[:, 1:], track[:, 1:] - 1), None, lag, 7)
        assert MC.same_bits(sbox[:, 1], alone[0][:, 0])


# ------------------------------------------------------------------------------------------------ streams and empty pushes
def test_a_flush_starts_a_fresh_stream_and_empty_pushes_emit_nothing():
    a, b = LC.tracked("sort", 5, T=9, objects=5), LC.tracked("byte", 6, T=12, objects=5)
    state = None
    for case in (a, b, a):                                                 # ids from 0 again in every clip
        state, t0, box1, len1 = smooth_lag_host(state, *case, 2, 4)
        assert t0 == 0 and box1.shape[0] == case[2].shape[0] - 4
        state, t0, box2, len2 = smooth_lag_host(state, case[0][:0], case[1][:0], case[2][:0], case[3][:0], 2, 4, flush=True)
        assert t0 == case[2].shape[0] - 4 and box2.shape[0] == 4 and state is None
        want = LC.run_host(case, 2, 4, 7)
        assert MC.same_bits(np.concatenate([box1, box2]), want[0]) and np.array_equal(np.concatenate([len1, len2]), want[1])
    ids, scores, bboxes, track = a
    empty = (ids[:0], scores[:0], bboxes[:0], track[:0])
    state, t0, box, ln = smooth_lag_host(None, *empty, 2, 3)               # F = 0 on a fresh stream
    assert t0 == 0 and box.shape == (0, 5, 4) and ln.shape == (0, 5) and state["frames"] == state["emitted"] == 0
    state, t0, box, ln = smooth_lag_host(state, *empty, 2, 3, flush=True)  # the flush of an empty stream
    assert t0 == 0 and box.shape == (0, 5, 4) and ln.dtype == np.int32 and state is None
    state, *_ = smooth_lag_host(None, ids[:5], scores[:5], bboxes[:5], track[:5], 2, 3)
    again, t0, box, _ = smooth_lag_host(state, *empty, 2, 3)               # F = 0 in the middle of one
    assert t0 == 2 and box.shape[0] == 0 and again["frames"] == 5 and again["emitted"] == 2


def test_parameters_and_the_option():
    assert DEFAULTS == dict(max_gap=7) and MAX_LAG == 15 and RING == 16
    assert check_params(0) == (0, 7) and check_params(np.int64(15), 0) == (15, 0)
    for bad in (-1, 16, 1.0, True, None, "3"):
        with pytest.raises(ValueError, match="smooth_lag_host: lag must be an integer in \\[0, 15\\]"):
            check_params(bad, 7, who="smooth_lag_host")
    with pytest.raises(ValueError, match="smooth_lag_host: max_gap must be an integer in \\[0, 7\\]"):
        check_params(1, 8, who="smooth_lag_host")
    case = MC.still()
    with pytest.raises(ValueError, match="lag"):
        smooth_lag_host(None, *case, None, 16)
    with pytest.raises(ValueError, match="max_gap"):
        smooth_lag_host(None, *case, None, 1, max_gap=-1)
    with pytest.raises(ValueError, match="expected track"):
        smooth_lag_host(None, case[0], case[1], case[2], case[3].astype(np.float32), None, 1)
    with pytest.raises(ValueError, match="expected ids"):
        smooth_lag_host(None, case[0], case[1], case[2][:, :, :3], case[3], None, 1)
    with pytest.raises(ValueError, match="at most 128"):
        smooth_lag_host(None, np.zeros((1, 129, 1)), np.zeros((1, 129, 1)), np.zeros((1, 129, 4)), np.zeros((1, 129), np.int32), None, 1)
    state, *_ = smooth_lag_host(None, *case, None, 1)
    with pytest.raises(ValueError, match="N=1 rows per frame, got N=2"):
        smooth_lag_host(state, np.zeros((1, 2, 1)), np.zeros((1, 2, 1)), np.zeros((1, 2, 4)), np.zeros((1, 2), np.int32), None, 1)
    assert parse_option(None, False, "open_video") is None and parse_option(False, True, "open_video") is None
    assert parse_option(dict(lag=3), True, "open_video") == dict(lag=3)
    assert parse_option(dict(lag=0, max_gap=2), True, "open_video") == dict(lag=0, max_gap=2)


# ------------------------------------------------------------------------------------------------ the entry point
def test_library_exports_track_smooth_push_and_checks_its_arguments_before_any_launch():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # an entry point was added, nothing changed
    assert len(L.SIGNATURES["vd_track_smooth_push"][1]) == 17
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "viddet_hip.h")).read()
    want = 16 + 4 * 16 + 16 * 128 * (6 * 4 + 16 + 17 * 4)                  # header, slot frames, six words + box + state an entry
    assert int(re.search(r"#define VD_TRACK_SMOOTH_LIVE_STATE_BYTES\s+(\d+)", hdr).group(1)) == L.TRACK_SMOOTH_LIVE_STATE_BYTES == want
    assert want % 16 == 0
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    SB = L.TRACK_SMOOTH_LIVE_STATE_BYTES
    good = dict(ids=P, scores=P, bboxes=P, track=P, V=2, F=6, N=20, num_class=3, lag=4, max_gap=7, flush=0, state=P,
                state_bytes=2 * SB, m=2, out_sbox=P, out_slen=P)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_track_smooth_push(a["ids"], a["scores"], a["bboxes"], a["track"], a["V"], a["F"], a["N"], a["num_class"],
                                      a["lag"], a["max_gap"], a["flush"], a["state"], a["state_bytes"], a["m"], a["out_sbox"],
                                      a["out_slen"], None)
        return rc, lib.vd_last_error()

    bad = [dict(ids=None), dict(scores=None), dict(bboxes=None), dict(track=None), dict(out_sbox=None), dict(out_slen=None),
           dict(state=None), dict(N=0), dict(N=129), dict(N=-1), dict(F=-1), dict(V=0), dict(num_class=0), dict(lag=-1),
           dict(lag=16), dict(max_gap=8), dict(max_gap=-1), dict(state_bytes=2 * SB - 1), dict(state_bytes=0),
           dict(m=1), dict(m=7), dict(m=-1), dict(flush=1, m=5), dict(flush=1, m=11), dict(flush=1, F=0, m=5),
           dict(F=3, m=4), dict(bboxes=P + 4), dict(out_sbox=P + 8), dict(state=P + 4), dict(ids=P + 2), dict(scores=P + 1),
           dict(track=P + 2), dict(out_slen=P + 3)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_track_smooth_push:"), (kw, err)
    # no frame and no flush: nothing to take, nothing becomes final, nothing is launched - the inputs and outputs may be NULL
    assert call(F=0, m=0, ids=None, scores=None, bboxes=None, track=None, out_sbox=None, out_slen=None)[0] == 0


# ------------------------------------------------------------------------------------------------ the session option
def test_open_video_takes_the_smooth_option_on_a_cpu_net():
    import torch
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["a", "b"], device="cpu")
    with pytest.raises(ValueError, match="open_video: smooth needs lag"):
        net.open_video(track=True, smooth=True)
    with pytest.raises(ValueError, match="open_video: smooth needs lag"):
        net.open_video(track=True, smooth={"max_gap": 3})
    for bad in (-1, 16, 1.5, True, None):
        with pytest.raises(ValueError, match="open_video with smooth: lag must be an integer in \\[0, 15\\]"):
            net.open_video(track=True, smooth={"lag": bad})
    with pytest.raises(ValueError, match="open_video with smooth: max_gap must be an integer in \\[0, 7\\]"):
        net.open_video(track=True, smooth={"lag": 2, "max_gap": 8})
    with pytest.raises(ValueError, match="open_video: smooth takes lag, max_gap, got bogus, rescore"):
        net.open_video(track=True, smooth={"lag": 2, "rescore": "avg", "bogus": 1})
    with pytest.raises(ValueError, match="open_video: smooth needs track"):
        net.open_video(smooth={"lag": 2})
    # sort and byte need their own word as ever
    with pytest.raises(NotImplementedError, match="open_video with track method 'sort'"):
        net.open_video(track={"method": "sort"}, smooth={"lag": 2})
    for trk in (True, {"method": "sort", "online": True}, {"method": "byte", "online": True, "max_age": 3}):
        s = net.open_video(track=trk, smooth={"lag": 2, "max_gap": 3})
        assert s._smo_kw == dict(lag=2, max_gap=3) and s._smo is None and s._held is None      # the state is built lazily
        assert s.last_pre_smooth is None and s.last_smooth is None
    for s in (net.open_video(), net.open_video(track=True), net.open_video(track=True, smooth=None), net.open_video(track=True, smooth=False)):
        assert s._smo_kw is None and s.last_pre_smooth is None and s.last_smooth is None       # the session as ever
    # detect_video's smooth is the fixed-interval one: it does not take lag
    with pytest.raises(ValueError, match="detect_video: smooth takes max_gap, got lag"):
        net.detect_video(torch.zeros(4, 3, 64, 64), track=True, smooth={"lag": 1})


# ------------------------------------------------------------------------------------------------ the script
LIVE = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--stream", "--track"]


def test_detect_script_refuses_track_smooth_lag_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    assert D.parse_flags([]).track_smooth_lag is None and D.parse_flags(["--track_smooth_lag", "4"]).track_smooth_lag == 4
    with pytest.raises(NotImplementedError, match="--track_smooth_lag needs --live"):
        D.main(LIVE + ["--track_smooth", "--track_smooth_lag", "2"])
    with pytest.raises(NotImplementedError, match="--track_smooth_lag needs --track_smooth"):
        D.main(LIVE + ["--live", "--track_smooth_lag", "2"])
    for lag in ("16", "-1"):
        with pytest.raises(NotImplementedError, match="--track_smooth_lag must be an integer in \\[0, 15\\]"):
            D.main(LIVE + ["--live", "--track_smooth", "--track_smooth_lag", lag])
    # without the flag the refusal stands word for word
    with pytest.raises(NotImplementedError, match="--track_smooth does not combine with --live: a frame's smoothed box needs the "
                                                  "frames after it - the pass has no online form"):
        D.main(LIVE + ["--live", "--track_smooth"])
    with pytest.raises(NotImplementedError, match="--track_smooth needs --track"):
        D.main([a for a in LIVE if a != "--track"] + ["--live", "--track_smooth", "--track_smooth_lag", "2"])
    # the other passes stay refused beside --live, and sort needs --track_online as ever
    on = LIVE + ["--live", "--track_smooth", "--track_smooth_lag", "2"]
    with pytest.raises(NotImplementedError, match="--tubelet does not combine with --live"):
        D.main(on + ["--tubelet"])
    with pytest.raises(NotImplementedError, match="--live does not combine with --seq_nms"):
        D.main(on + ["--seq_nms"])
    with pytest.raises(NotImplementedError, match="--track_stitch does not combine with --live"):
        D.main(on + ["--track_stitch"])
    with pytest.raises(NotImplementedError, match="--track_method sort does not combine with --live"):
        D.main(on + ["--track_method", "sort"])
    with pytest.raises(NotImplementedError, match="--track_smooth_gap must be an integer in \\[0, 7\\]"):
        D.main(on + ["--track_smooth_gap", "8"])
    for more in ([], ["--track_smooth_lag", "0"], ["--track_smooth_lag", "15", "--track_method", "byte", "--track_online"]):
        with pytest.raises(SystemExit, match="needs an MI355X"):           # and what is not refused gets as far as the GPU check
            D.main(on + more)
