"""CPU: the host half of SORT and BYTE in live sessions, none of which touches a GPU.

Definitions: sort.sort_online_host and byte.byte_online_host over any partition of a clip equal one call on all of it, on all
four outputs, and leave the state they are given unchanged; track.finalize_tracks(..., tbox=) of a finished clip's online rows is
sort_host / byte_host, on all four outputs; byte_online_host at sigma_d = sigma_new = sigma_l is sort_online_host; ids go on
across clips that share a state.  Then the ABI of vd_track_kf_push, the `online` word of open_video's track option and the
script's --track_online.  Every comparison is exact."""
import copy
import os
import re

import numpy as np
import pytest

from tests import byte_cases as BC
from tests import sort_cases as SC
from viddet_amd import byte as B
from viddet_amd import sort as S
from viddet_amd.byte import byte_host, byte_online_host
from viddet_amd.sort import sort_host, sort_online_host
from viddet_amd.track import finalize_tracks

NAMES = ("track", "tlen", "tscore", "tbox")
ONLINE = dict(sort=sort_online_host, byte=byte_online_host)
OFFLINE = dict(sort=sort_host, byte=byte_host)
DEFAULTS = dict(sort=S.DEFAULTS, byte=B.DEFAULTS)
DECIDE = ("sigma_h", "t_min")


def _split(method, kw):
    """a case's keyword arguments -> (those the online definition takes, sigma_h / t_min)"""
    kw = {k: v for k, v in kw.items() if k in DEFAULTS[method] or k == "num_class"}
    return {k: v for k, v in kw.items() if k not in DECIDE}, {k: v for k, v in kw.items() if k in DECIDE}


def _same4(got, want, what=""):
    assert len(got) == len(want) == 4, what
    for name, g, w in zip(NAMES[:3], got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)
    assert got[3].dtype == np.float32 and SC.same_tbox(got[3], want[3]), (what, "tbox")


def _same_state(a, b):
    assert a["next_id"] == b["next_id"]
    for k in ("cls", "id", "miss", "len", "max"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k
    for k in S._KEYS:
        assert np.array_equal(a["kf"][k], b["kf"][k], equal_nan=True), k


def _parts(F):
    """all at once, one frame per call, (1, 3, rest)"""
    out = [(F,), (1,) * F]
    if F > 4:
        out.append((1, 3, F - 4))
    return out


def _online(method, case, okw, parts, state=None, stats=None):
    """the online definition over the partition `parts` of the clip's frames -> (the last state, the four arrays concatenated)"""
    outs, t, per_call = [], 0, []
    for n in parts:
        keep = copy.deepcopy(state)
        st = {}
        new, *o = ONLINE[method](state, *[a[t:t + n] for a in case], stats=st, **okw)
        if state is not None:                                      # the state handed in is not changed
            _same_state(state, keep)
        state = new
        outs.append(o)
        per_call.append(st)
        t += n
    assert t == case[2].shape[0]
    if stats is not None:
        for k in per_call[0]:
            stats[k] = np.concatenate([s[k] for s in per_call])
    return state, [np.concatenate(x) for x in zip(*outs)]


def _cases():
    out = []
    for tag, mod in (("sc", SC), ("bc", BC)):
        for name, case, kw, _, _ in mod.closed_form():
            out.append(("%s_%s" % (tag, name), case, kw))
    for seed in (1, 4, 9):
        out.append(("walkers%d" % seed, SC.walkers(seed), dict(num_class=2)))
        out.append(("dipped%d" % seed, BC.dipped(seed), dict(num_class=2)))
    return out


CASES = _cases()


# ------------------------------------------------------------------------------------------------ the definitions
@pytest.mark.parametrize("method", ["sort", "byte"])
@pytest.mark.parametrize("name,case,kw", CASES, ids=[c[0] for c in CASES])
def test_partitions_equal_one_call_and_finalize_equals_the_clip_tracker(name, case, kw, method):
    okw, dkw = _split(method, kw)
    F = case[2].shape[0]
    stats = {}
    _, whole = _online(method, case, okw, (F,), stats=stats)
    assert [a.dtype for a in whole] == [np.int32, np.int32, np.float32, np.float32]
    assert whole[0].shape == whole[1].shape == whole[2].shape == case[2].shape[:2] and whole[3].shape == case[2].shape
    assert np.array_equal(whole[0] >= 0, whole[1] > 0) and np.array_equal(whole[0] < 0, whole[2] == -1)
    assert (whole[3][whole[0] < 0] == -1).all()
    for parts in _parts(F)[1:]:
        pstats = {}
        _same4(_online(method, case, okw, parts, stats=pstats)[1], whole, parts)
        assert all(np.array_equal(pstats[k], stats[k]) for k in stats)
    # what is decided at the clip's end is decided from the online rows alone
    ostats = {}
    want = OFFLINE[method](*case, stats=ostats, **okw, **dkw)
    _same4(finalize_tracks(*whole[:3], tbox=whole[3], **dkw), want, "finalize")
    assert all(np.array_equal(stats[k], ostats[k]) for k in stats)
    three = finalize_tracks(*whole[:3], **dkw)                     # without tbox=: the three arrays as before
    assert isinstance(three, tuple) and len(three) == 3 and all(np.array_equal(a, b) for a, b in zip(three, want))
    if name.startswith("dipped") and method == "byte":
        assert stats["first"].sum() > 0 and stats["second"].sum() > 0


@pytest.mark.parametrize("method", ["sort", "byte"])
@pytest.mark.parametrize("max_age", [0, 1, 7])
def test_finalize_equals_the_clip_tracker_over_max_age(method, max_age):
    for case in (SC.walkers(2, T=12, miss=0.3), BC.dipped(6, T=12, miss=0.3)):
        for dkw in (dict(), dict(sigma_h=0.8, t_min=3)):
            _, rows = _online(method, case, dict(num_class=2, max_age=max_age), (1, 3, 8))
            want = OFFLINE[method](*case, num_class=2, max_age=max_age, **dkw)
            _same4(finalize_tracks(*rows[:3], tbox=rows[3], **dkw), want, (max_age, dkw))
            assert (rows[0] >= 0).any()


def test_finalize_drops_the_boxes_of_dropped_tracks_and_keeps_the_others():
    """sort_cases' `dropped`: track 1 (best score 0.3 < sigma_h) and track 2 (one row < t_min) are dropped, 0 and 3 kept"""
    name, case, kw, track, tlen = [c for c in SC.closed_form() if c[0] == "dropped"][0]
    _, rows = _online("sort", case, {}, (1, 2))
    assert sorted(set(rows[0][rows[0] >= 0].tolist())) == [0, 1, 2, 3]
    got = finalize_tracks(*rows[:3], tbox=rows[3])
    assert got[0].tolist() == track and got[1].tolist() == tlen
    dropped = (rows[0] >= 0) & (got[0] < 0)
    assert dropped.sum() == 3 and (rows[3][dropped] != -1).any()
    assert (got[3][dropped] == -1).all() and (got[3][got[0] < 0] == -1).all()
    assert np.array_equal(got[3][got[0] >= 0], rows[3][got[0] >= 0]) and (got[0] >= 0).sum() == 4
    _same4(got, sort_host(*case))
    # the same through BYTE, whose low row (0.3) never starts a track: sigma_h drops nothing there, t_min does
    _, rows = _online("byte", case, {}, (3,))
    got = finalize_tracks(*rows[:3], tbox=rows[3])
    _same4(got, byte_host(*case))
    dropped = (rows[0] >= 0) & (got[0] < 0)
    assert dropped.sum() == 1 and (got[3][dropped] == -1).all() and (got[0] >= 0).sum() == 4
    with pytest.raises(ValueError, match="tbox"):
        finalize_tracks(*rows[:3], tbox=rows[3][:, :, :3])


@pytest.mark.parametrize("name,case,kw", CASES, ids=[c[0] for c in CASES])
def test_byte_without_low_rows_is_sort(name, case, kw):
    okw, _ = _split("sort", kw)
    for sl in (okw.pop("sigma_l", 0.0), 0.6):
        ss, *want = sort_online_host(None, *case, sigma_l=sl, **okw)
        bkw = dict(dict(sigma_iou=S.DEFAULTS["sigma_iou"], max_age=S.DEFAULTS["max_age"]), **okw)
        bs, *got = byte_online_host(None, *case, sigma_l=sl, sigma_d=sl, sigma_new=sl, sigma_iou2=0.9, **bkw)
        _same4(got, want, sl)
        _same_state(bs, ss)


@pytest.mark.parametrize("method", ["sort", "byte"])
def test_ids_go_on_across_clips_that_share_a_state(method):
    first, second = BC.dipped(3), BC.dipped(5)
    okw = dict(num_class=2)
    state, rows1 = _online(method, first, okw, (4, 6))
    made = state["next_id"]
    assert made == rows1[0].max() + 1 > 0
    state2, rows2 = _online(method, second, okw, (1, 3, 6), state=state)
    on = rows2[0] >= 0
    # tracks that were active at the boundary may go on (their ids lie below `made`); every track started later lies above
    started = on & (rows2[1] == 1)
    assert started.any() and rows2[0][started].min() == made and state2["next_id"] == rows2[0].max() + 1
    # a state that is flushed between the clips: the second clip alone, its ids from 0 ...
    _, alone = _online(method, second, okw, (10,))
    # ... and through a state whose tracks have all been closed, its ids from `made` on: finalize_tracks' `lo` offset path
    gap = [np.full((8,) + a.shape[1:], -1, np.float32) for a in second]
    aged, _ = _online(method, gap, okw, (8,), state=state)
    assert len(aged["id"]) == 0 and aged["next_id"] == made
    _, shifted = _online(method, second, okw, (2, 8), state=aged)
    assert shifted[0][shifted[0] >= 0].min() == made
    assert np.array_equal(np.where(alone[0] >= 0, alone[0] + made, -1), shifted[0])
    assert np.array_equal(shifted[1], alone[1]) and np.array_equal(shifted[2], alone[2]) and SC.same_tbox(shifted[3], alone[3])
    want = OFFLINE[method](*second, num_class=2)
    got = finalize_tracks(*shifted[:3], tbox=shifted[3])
    assert (want[0] >= 0).any()
    assert np.array_equal(got[0], np.where(want[0] >= 0, want[0] + made, -1))
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and SC.same_tbox(got[3], want[3])


def test_the_online_definitions_check_their_arguments():
    case = SC.walkers(1)
    with pytest.raises(ValueError, match="sort_online_host: max_age"):
        sort_online_host(None, *case, max_age=8)
    with pytest.raises(ValueError, match="byte_online_host: sigma_d must not be NaN"):
        byte_online_host(None, *case, sigma_d=float("nan"))
    with pytest.raises(ValueError, match="expected ids"):
        byte_online_host(None, case[0], case[1], case[2][:, :, :3])
    with pytest.raises(TypeError):
        sort_online_host(None, *case, sigma_h=0.5)                 # nothing is decided online
    with pytest.raises(TypeError):
        byte_online_host(None, *case, t_min=2)
    e = sort_online_host(None, *[a[:0] for a in case])
    assert [a.shape for a in e[1:]] == [(0, 6)] * 3 + [(0, 6, 4)] and e[0]["next_id"] == 0


# ------------------------------------------------------------------------------------------------ ABI
def test_library_exports_track_kf_push_and_checks_its_arguments_before_any_launch():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # an entry point was added, nothing changed
    assert "vd_track_kf_push" in L.SIGNATURES and len(L.SIGNATURES["vd_track_kf_push"][1]) == 20
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "viddet_hip.h")).read()
    assert "int vd_track_kf_push(" in hdr
    assert int(re.search(r"#define VD_TRACK_KF_STATE_BYTES\s+(\d+)", hdr).group(1)) == L.TRACK_KF_STATE_BYTES
    assert L.TRACK_KF_STATE_BYTES == 16 + 5 * 4 * L.TRACK_MAX_ACTIVE + L.TRACK_SORT_WS_PER_CLIP == 159760
    assert L.TRACK_KF_STATE_BYTES % 16 == 0
    src = open(os.path.join(root, "viddet_amd", "csrc", "vd_track_kf_live.hip")).read()
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "vd_track_math.h"')
    assert "vd_track_kf_live.hip" in open(os.path.join(root, "viddet_amd", "csrc", "Makefile")).read()
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    good = dict(ids=P, scores=P, bboxes=P, V=2, F=6, N=20, num_class=3, sl=0.1, sd=0.5, sn=0.6, si=0.2, si2=0.5, max_age=7, state=P,
                state_bytes=2 * L.TRACK_KF_STATE_BYTES, out_track=P, out_len=P, out_score=P, out_tbox=P)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_track_kf_push(a["ids"], a["scores"], a["bboxes"], a["V"], a["F"], a["N"], a["num_class"], a["sl"], a["sd"],
                                  a["sn"], a["si"], a["si2"], a["max_age"], a["state"], a["state_bytes"], a["out_track"],
                                  a["out_len"], a["out_score"], a["out_tbox"], None)
        return rc, lib.vd_last_error()

    nan = float("nan")
    bad = [dict(ids=None), dict(scores=None), dict(bboxes=None), dict(out_track=None), dict(out_len=None), dict(out_score=None),
           dict(out_tbox=None), dict(state=None), dict(N=0), dict(N=129), dict(N=-1), dict(F=0), dict(V=0), dict(num_class=0),
           dict(sl=nan), dict(sd=nan), dict(sn=nan), dict(si=nan), dict(si2=nan), dict(max_age=8), dict(max_age=-1),
           dict(state_bytes=2 * L.TRACK_KF_STATE_BYTES - 1), dict(state_bytes=0), dict(bboxes=P + 4), dict(out_tbox=P + 8),
           dict(state=P + 8), dict(ids=P + 2), dict(scores=P + 1), dict(out_track=P + 2), dict(out_len=P + 1), dict(out_score=P + 3)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_track_kf_push:"), (kw, err)


# ------------------------------------------------------------------------------------------------ the interface
def test_open_video_takes_the_online_word_on_a_cpu_net():
    import torch
    from viddet_amd.model import yolo3_darknet53
    from viddet_amd.track import DEFAULTS as IOU_DEFAULTS
    from viddet_amd.track import parse_option, split_online
    net = yolo3_darknet53(["a", "b"], device="cpu")
    for m in ("sort", "byte"):
        # without the word, or with False: the refusal as ever
        for trk in ({"method": m}, {"method": m, "online": False}):
            with pytest.raises(NotImplementedError, match="open_video with track method '%s': it has no resumable form yet" % m):
                net.open_video(track=trk)
        s = net.open_video(track={"method": m, "online": True, "sigma_h": 0.25, "max_age": 3, "clip": 64})
        want = {k: v for k, v in dict(DEFAULTS[m], max_age=3).items() if k not in DECIDE}
        assert s._trk_method == m and s._trk_kw == want and s._trk_clip == 64 and s._trk is None   # the state is built lazily
        assert s.track_decide == dict(sigma_h=0.25, t_min=2)
        assert s.last_tracks is None and s.last_track_boxes is None
        with pytest.raises(ValueError, match="max_age"):
            net.open_video(track={"method": m, "online": True, "max_age": 8})
        with pytest.raises(ValueError, match="track takes sigma_l.*bogus"):
            net.open_video(track={"method": m, "online": True, "bogus": 1})
    with pytest.raises(ValueError, match="sigma_d"):
        net.open_video(track={"method": "sort", "online": True, "sigma_d": 0.5})
    # the IOU tracker is always online: the word changes nothing
    s = net.open_video(track={"method": "iou", "online": True, "max_age": 2})
    plain = net.open_video(track={"max_age": 2})
    assert s._trk_method == plain._trk_method == "iou" and s._trk_kw == plain._trk_kw and s.track_decide == plain.track_decide
    assert net.open_video(track=True).last_track_boxes is None and net.open_video().last_track_boxes is None
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="open_video: track's online must be a bool"):
            net.open_video(track={"method": "sort", "online": bad})
    # detect_video does not take it, and parse_option's result keeps its three elements
    with pytest.raises(ValueError, match="detect_video: track takes .* got online"):
        net.detect_video(torch.zeros(4, 3, 64, 64), track={"method": "sort", "online": True})
    assert parse_option(dict(method="sort"), 100, "w") == (S.DEFAULTS, None, "sort")
    assert split_online(None, "w") == (None, False) and split_online(True, "w") == (True, False)
    assert split_online(dict(online=True, max_age=1), "w") == (dict(max_age=1), True)
    assert parse_option(split_online(dict(online=True), "w")[0], 100, "w") == (IOU_DEFAULTS, None, "iou")


def test_kalman_track_state_checks_its_parameters_on_the_host():
    from viddet_amd import lib as L
    from viddet_amd import ops
    with pytest.raises(ValueError, match="ops.TrackState"):
        ops.KalmanTrackState(method="iou", device="cpu")
    with pytest.raises(ValueError, match="method must be 'sort' or 'byte'"):
        ops.KalmanTrackState(method="deep", device="cpu")
    for bad in (dict(method="sort", sigma_d=0.5), dict(method="sort", sigma_h=0.5), dict(method="byte", t_min=2),
                dict(method="sort", max_age=8), dict(method="byte", sigma_new=float("nan")), dict(method="byte", N=129),
                dict(method="sort", N=0), dict(method="sort", V=0), dict(method="byte", num_class=0)):
        with pytest.raises(ValueError, match="KalmanTrackState"):
            ops.KalmanTrackState(device="cpu", **bad)
    st = ops.KalmanTrackState(2, 20, 3, method="sort", device="cpu", sigma_l=0.25)
    assert tuple(st.state.shape) == (2, L.TRACK_KF_STATE_BYTES) and int(st.state.max()) == 0 and st.frames == 0
    # SORT on BYTE's frame body: every candidate is a high row that may start a track
    assert (st.sigma_l, st.sigma_d, st.sigma_new, st.sigma_iou, st.sigma_iou2, st.max_age) == (0.25, 0.25, 0.25, st.sigma_iou, st.sigma_iou, 1)
    st = ops.KalmanTrackState(method="byte", device="cpu")
    assert (st.sigma_d, st.sigma_new, st.sigma_iou2, st.max_age) == (0.5, float(np.float32(0.6)), 0.5, 7)


TRK = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--track"]


def test_the_script_refuses_track_online_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    F = D.parse_flags(["--track_online"])
    assert F.track_online is True and D.parse_flags([]).track_online is False
    for m in ("sort", "byte"):
        with pytest.raises(NotImplementedError, match="--track_online needs --live"):
            D.main(TRK + ["--stream", "--track_method", m, "--track_online"])
        # without the flag the refusal is unchanged
        with pytest.raises(NotImplementedError, match="--track_method %s does not combine with --live: it has no resumable form yet" % m):
            D.main(TRK + ["--stream", "--live", "--track_method", m])
        # with it the run gets as far as asking for the GPU
        with pytest.raises(SystemExit):
            D.main(TRK + ["--stream", "--live", "--live_push", "2", "--track_method", m, "--track_online"])
    for extra in ([], ["--track_method", "iou"]):
        with pytest.raises(NotImplementedError, match="--track_online does not combine with --track_method iou"):
            D.main(TRK + ["--stream", "--live", "--track_online"] + extra)
    with pytest.raises(NotImplementedError, match="--track_online needs --live"):
        D.main(TRK + ["--stream", "--track_online"])
    with pytest.raises(NotImplementedError, match="--track_online needs --track"):
        D.main(TRK[:-1] + ["--stream", "--live", "--track_online"])
    # the passes that need later frames stay refused beside --live
    for flag in ("--tubelet", "--track_smooth", "--track_stitch"):
        with pytest.raises(NotImplementedError, match="%s does not combine with --live" % flag):
            D.main(TRK + ["--stream", "--live", "--track_method", "byte", "--track_online", flag])
    with pytest.raises(NotImplementedError, match="--live does not combine with --seq_nms"):
        D.main(TRK + ["--stream", "--live", "--track_method", "sort", "--track_online", "--seq_nms"])
