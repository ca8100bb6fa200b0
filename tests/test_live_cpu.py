"""CPU: the host half of live video sessions, none of which touches a GPU.

Planner: stream.StreamPlanner, fed a clip in any partition and then flushed, returns the launch groups of detect_video on the
whole clip - the two loops detect_video ran before it was put on the planner are written out below as `detect_video_actions` - and
the slot table of every suffix chunk is chunk_slots of stream_window_slots(T, ...).
Tracker: track.track_online_host over any partition equals one call on all frames; its ids are track_host's with nothing
dropped; finalize_tracks of it is track_host at the real sigma_h and t_min, on all three arrays.
Then the ABI of vd_track_push, and the refusals of detect_yolo3.py --live."""
import numpy as np
import pytest

from tests import track_cases as TC
from viddet_amd.stream import StreamPlanner, chunk_slots, ring_size, stream_window_slots, window_rows
from viddet_amd.track import finalize_tracks, track_host, track_online_host


# ------------------------------------------------------------------------------------------------ planner
def detect_video_actions(T, K, step, chunk):
    """The launches of detect_video(frames (T,...), step, chunk) in order - the loops detect_video ran before it was put on the
    planner: ('prefix', a, b) for _stage_frames(.., done, done + m) + pre.run(), ('suffix', t0, n) for suf.run() (K = 1: _forward_infer on the chunk) - and
    with each suffix the frames [first, last) its chunk_slots call is checked against."""
    acts, rings = [], []
    if K == 1:
        for t0 in range(0, T, chunk):
            acts.append(('suffix', t0, min(chunk, T - t0)))
            rings.append(None)
        return acts, rings
    S = ring_size(K, step, chunk)
    reach = (K // 2) * step
    done = 0
    for t0 in range(0, T, chunk):
        n = min(chunk, T - t0)
        need = min(T, t0 + n + reach)
        while done < need:
            m = min(chunk, need - done)
            acts.append(('prefix', done, done + m))
            done += m
        acts.append(('suffix', t0, n))
        rings.append((max(0, done - S), done))
    return acts, rings


def _partitions(T, seed):
    yield (T,)
    yield (1,) * T
    rng = np.random.default_rng(seed)
    for _ in range(20):
        cuts = np.nonzero(rng.random(T - 1) < rng.uniform(0.1, 0.9))[0] + 1 if T > 1 else np.zeros(0, int)
        edges = [0] + cuts.tolist() + [T]
        yield tuple(b - a for a, b in zip(edges, edges[1:]))


@pytest.mark.parametrize("chunk", [1, 2, 3])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("K", [1, 3, 4, 5])
def test_planner_forms_the_groups_of_detect_video(K, step, chunk):
    reach = (K // 2) * step
    S = ring_size(K, step, chunk)
    plan = StreamPlanner(K, step, chunk)                            # one planner through every clip: flush() starts afresh
    seen_short_prefix = seen_open_suffix = False
    for T in range(1, 3 * chunk + 2 * reach + 2 + 1):
        want, rings = detect_video_actions(T, K, step, chunk)
        windows = stream_window_slots(T, K, step)
        tables = [chunk_slots(windows, a, b, chunk, S, *(r if r else (0, T))) if K > 1 else None
                  for (kind, a, b), r in zip([w for w in want if w[0] == 'suffix'], rings)]
        for part in _partitions(T, 1000 * K + 100 * step + 10 * chunk + T):
            assert sum(part) == T
            got, got_tables = [], []
            for n in part:
                acts = plan.push(n)
                # the frames that wait for their group: never a whole group's worth (a full one would have been formed)
                assert 0 <= plan.buffered < chunk, (T, part, plan.buffered)
                assert plan.buffered == plan.frames_in - (plan.out if K == 1 else plan.done)
                got_tables += [plan.slots(a, b) for kind, a, b in acts if kind == 'suffix' and K > 1]
                seen_open_suffix |= any(kind == 'suffix' for kind, _, _ in acts)
                got += acts
            assert plan.frames_in == T
            acts = plan.flush()
            got_tables += [plan.slots(a, b, T) for kind, a, b in acts if kind == 'suffix' and K > 1]
            got += acts
            assert got == want, (T, part)
            assert (plan.frames_in, plan.done, plan.out) == (0, 0, 0)
            if K > 1:
                assert len(got_tables) == len(tables)
                for g, w in zip(got_tables, tables):
                    assert g.dtype == np.int32 and g.shape == (chunk, K) and np.array_equal(g, w)
            seen_short_prefix |= any(kind == 'prefix' and b - a < chunk for kind, a, b in got)
    assert seen_open_suffix and (K == 1 or chunk == 1 or seen_short_prefix)


def test_window_rows_are_rows_of_stream_window_slots():
    for K in (1, 2, 3, 4, 5):
        for step in (1, 2, 3):
            for T in (1, 2, 5, 11):
                full = stream_window_slots(T, K, step)
                for t0 in range(T):
                    for n in range(1, T - t0 + 1):
                        assert np.array_equal(window_rows(t0, n, T, K, step), full[t0:t0 + n])
    with pytest.raises(ValueError):
        window_rows(3, 2, 4, 3, 1)


def test_planner_checks_its_arguments():
    for kw in (dict(K=0), dict(step=0), dict(chunk=0)):
        with pytest.raises(ValueError, match="StreamPlanner needs"):
            StreamPlanner(**dict(dict(K=3, step=1, chunk=2), **kw))
    with pytest.raises(ValueError, match="n >= 1"):
        StreamPlanner(3).push(0)
    assert StreamPlanner(3).flush() == []                           # an empty clip


# ------------------------------------------------------------------------------------------------ tracker
def _tracker_cases():
    out = []
    for name, case, kw, _, _ in TC.closed_form():
        out.append((name, case, kw.get("num_class")))
    for T, N in TC.SIZES:
        out.append(("random%dx%d" % (T, N), TC.random_clip(T, N, seed=7 * T + N, spread=40.0 + N, fill=1.0 if N < 4 else 0.8), 1))
    return out


CASES = _tracker_cases()
PARAMS = [("defaults", {}), ("off_default", TC.OFF_DEFAULT)]


def _online(case, num_class, kw, parts):
    """track_online_host over the partition `parts` of the clip's frames -> the concatenated triple"""
    okw = {k: v for k, v in kw.items() if k in ("sigma_l", "sigma_iou", "max_age")}
    state, outs, t = None, [], 0
    for n in parts:
        keep = None if state is None else (state["next_id"], [list(a[:2]) + [a[2].copy()] + list(a[3:]) for a in state["active"]])
        new, *o = track_online_host(state, *[a[t:t + n] for a in case], num_class=num_class, **okw)
        if keep is not None:                                        # the state handed in is not changed
            assert state["next_id"] == keep[0] and len(state["active"]) == len(keep[1])
            for a, b in zip(state["active"], keep[1]):
                assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3:] == b[3:]
        state = new
        outs.append(o)
        t += n
    assert t == case[2].shape[0]
    return [np.concatenate(x) for x in zip(*outs)]


def _check_online(case, num_class, kw):
    F = case[2].shape[0]
    okw = {k: v for k, v in kw.items() if k in ("sigma_l", "sigma_iou", "max_age")}
    whole = _online(case, num_class, kw, (F,))
    assert whole[0].dtype == np.int32 and whole[1].dtype == np.int32 and whole[2].dtype == np.float32
    assert np.array_equal(whole[0] >= 0, whole[1] > 0) and np.array_equal(whole[0] < 0, whole[2] == -1)
    rng = np.random.default_rng(F)
    parts = [(1,) * F, (1, min(3, F - 1), F - 1 - min(3, F - 1)) if F > 2 else (1,) * F]
    cuts = sorted(set(rng.integers(1, F, 3).tolist())) if F > 1 else []
    parts.append(tuple(b - a for a, b in zip([0] + cuts, cuts + [F])))
    for p in parts:
        p = tuple(n for n in p if n)
        for name, g, w in zip(("track", "tlen", "tscore"), _online(case, num_class, kw, p), whole):
            assert np.array_equal(g, w), (name, p)
    # the ids are track_host's where nothing is dropped
    everything = track_host(*case, num_class=num_class, sigma_h=-np.inf, t_min=1, **okw)
    assert np.array_equal(whole[0], everything[0])
    # and what is decided at the clip's end is decided from the online rows alone
    dkw = {k: v for k, v in kw.items() if k in ("sigma_h", "t_min")}
    want = track_host(*case, num_class=num_class, **kw)
    got = finalize_tracks(*whole, **dkw)
    for name, g, w in zip(("track", "tlen", "tscore"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name
    return whole, want


@pytest.mark.parametrize("pname,kw", PARAMS, ids=[p[0] for p in PARAMS])
@pytest.mark.parametrize("name,case,num_class", CASES, ids=[c[0] for c in CASES])
def test_online_tracker_equals_the_clip_tracker(name, case, num_class, pname, kw):
    _check_online(case, num_class, kw)


@pytest.mark.parametrize("pname,kw", PARAMS, ids=[p[0] for p in PARAMS])
@pytest.mark.parametrize("extend", [False, True], ids=["grow", "extend"])
def test_online_tracker_at_the_capacity_of_the_table(extend, pname, kw):
    whole, want = _check_online(TC.capacity(extend), 1, dict(kw, max_age=7))
    if extend:
        assert (whole[0] == np.arange(128)[None, :]).all() and (whole[1] == np.arange(1, 11)[:, None]).all()
    else:
        assert (whole[0] == np.arange(1280).reshape(10, 128)).all() and (whole[1] == 1).all()


def test_closed_form_cases_keep_their_hand_written_ids():
    for name, case, kw, track, tlen in TC.closed_form():
        kw = dict(kw)
        okw = {k: v for k, v in kw.items() if k in ("sigma_l", "sigma_iou", "max_age", "num_class")}
        _, *o = track_online_host(None, *case, **okw)
        got = finalize_tracks(*o, **{k: v for k, v in kw.items() if k in ("sigma_h", "t_min")})
        assert got[0].tolist() == np.asarray(track).tolist(), name
        if tlen is not None:
            assert got[1].tolist() == np.asarray(tlen).tolist(), name


def test_finalize_on_an_empty_and_on_an_all_invalid_clip():
    e = finalize_tracks(np.zeros((0, 5), np.int32), np.zeros((0, 5), np.int32), np.zeros((0, 5), np.float32))
    assert [a.shape for a in e] == [(0, 5)] * 3 and [a.dtype for a in e] == [np.int32, np.int32, np.float32]
    none = dict((c[0], c) for c in TC.closed_form())["all_invalid"][1]
    state, *o = track_online_host(None, *none, num_class=2)
    assert state["next_id"] == 0 and state["active"] == []
    got = finalize_tracks(*o)
    assert (got[0] == -1).all() and (got[1] == 0).all() and (got[2] == -1).all()
    assert all(np.array_equal(g, w) for g, w in zip(got, track_host(*none, num_class=2)))
    # a clip cut out of a longer stream: its ids do not start at 0
    case = TC.random_clip(6, 20, seed=3)
    _, *o = track_online_host(None, *case)
    shifted = (np.where(o[0] >= 0, o[0] + 1000, -1), o[1], o[2])
    a, b = finalize_tracks(*o), finalize_tracks(*shifted)
    assert np.array_equal(np.where(a[0] >= 0, a[0] + 1000, -1), b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    with pytest.raises(ValueError, match="t_min"):
        finalize_tracks(*o, t_min=0)
    with pytest.raises(ValueError, match=r"\(F,N\)"):
        finalize_tracks(o[0], o[1][:, :3], o[2])
    with pytest.raises(ValueError, match="max_age"):
        track_online_host(None, *case, max_age=8)


# ------------------------------------------------------------------------------------------------ ABI, script
def test_library_exports_track_push_and_checks_its_arguments_before_any_launch():
    import re
    import os
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # an entry point was added, nothing changed
    assert "vd_track_push" in L.SIGNATURES and len(L.SIGNATURES["vd_track_push"][1]) == 16
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "viddet_hip.h")).read()
    assert int(re.search(r"#define VD_TRACK_STATE_BYTES\s+(\d+)", hdr).group(1)) == L.TRACK_STATE_BYTES == 16 + 1024 * 36
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    good = dict(ids=P, scores=P, bboxes=P, V=2, F=6, N=20, num_class=3, sl=0.0, si=0.5, max_age=0, state=P,
                state_bytes=2 * L.TRACK_STATE_BYTES, out_track=P, out_len=P, out_score=P)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_track_push(a["ids"], a["scores"], a["bboxes"], a["V"], a["F"], a["N"], a["num_class"], a["sl"], a["si"],
                               a["max_age"], a["state"], a["state_bytes"], a["out_track"], a["out_len"], a["out_score"], None)
        return rc, lib.vd_last_error()

    nan = float("nan")
    bad = [dict(ids=None), dict(scores=None), dict(bboxes=None), dict(out_track=None), dict(out_len=None), dict(out_score=None),
           dict(state=None), dict(N=0), dict(N=129), dict(N=-1), dict(F=0), dict(V=0), dict(num_class=0), dict(sl=nan), dict(si=nan),
           dict(max_age=8), dict(max_age=-1), dict(state_bytes=2 * L.TRACK_STATE_BYTES - 1), dict(state_bytes=0),
           dict(bboxes=P + 4), dict(state=P + 8), dict(ids=P + 2), dict(scores=P + 1), dict(out_track=P + 2), dict(out_len=P + 1),
           dict(out_score=P + 3)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_track_push:"), (kw, err)


LIVE = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--live"]


def test_detect_script_refuses_live_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    with pytest.raises(NotImplementedError, match="--live needs --stream"):
        D.main(LIVE)
    with pytest.raises(NotImplementedError, match="--live does not combine with --seq_nms"):
        D.main(LIVE + ["--stream", "--seq_nms"])
    for n in ("0", "-2"):
        with pytest.raises(NotImplementedError, match="--live_push must"):
            D.main(LIVE + ["--stream", "--live_push", n])
    # with a clip path it gets as far as asking for the GPU
    for extra in (["--stream"], ["--stream", "--live_push", "3", "--track"]):
        with pytest.raises(SystemExit):
            D.main(LIVE + extra)
    F = D.parse_flags(["--stream", "--live"])
    assert F.live is True and F.live_push == 1 and D.parse_flags([]).live is False


def test_open_video_refusals_are_detect_videos_word_for_word():
    import torch
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["a", "b"], device="cpu", k=3, k_join_type="max", k_join_pos="late", rnn_pos="late")
    with pytest.raises(NotImplementedError) as e1:
        net.detect_video(torch.zeros(4, 3, 64, 64))
    with pytest.raises(NotImplementedError) as e2:
        net.open_video()
    assert str(e1.value).replace("detect_video with ", "", 1) == str(e2.value).replace("open_video with ", "", 1) == net._stream_refusal()
    net = yolo3_darknet53(["a", "b"], device="cpu")
    with pytest.raises(ValueError, match="step >= 1 and chunk >= 1"):
        net.open_video(chunk=0)
    with pytest.raises(ValueError, match="track takes sigma_l.*bogus"):
        net.open_video(track={"bogus": 1})
    with pytest.raises(ValueError, match="max_age"):
        net.open_video(track=dict(max_age=8))
    with pytest.raises(TypeError):
        net.open_video(seq_nms=True)                                        # Seq-NMS has no online form: no such option
    net.set_nms(post_nms=129)
    with pytest.raises(ValueError, match="post_nms=129"):
        net.open_video(track=True)
