"""CPU: the tubelet pass's definition (viddet_amd.tubelet.tubelet_host) equals a plain-loop form written from the
rules (tests/tubelet_oracle.py) on all six outputs, on every case and every parameter combination; the closed forms give the
values written out by hand; the argument checks of vd_tubelet and the refusals of net.detect_video(tubelet=...) and
detect_yolo3.py --tubelet, none of which touches a GPU."""
import numpy as np
import pytest

from tests import tubelet_cases as UC
from tests.tubelet_oracle import tubelet_loops
from viddet_amd.track import track_host
from viddet_amd.tubelet import DEFAULTS, check_params, tubelet_host

NAMES = ("ids", "scores", "bboxes", "perm", "track_out", "dropped")


def _same(data, track, **kw):
    keep = [a.copy() for a in data] + [track.copy()]
    hs, ls = {}, {}
    got = tubelet_host(*data, track, stats=hs, **kw)
    want = tubelet_loops(*data, track, stats=ls, **kw)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w, equal_nan=True), (name, kw)
        if g.dtype == np.float32:
            assert np.array_equal(np.signbit(g), np.signbit(w)), (name, kw)
    assert hs == ls
    assert got[0].shape == data[0].shape and got[1].shape == data[1].shape and got[2].shape == data[2].shape
    assert [g.dtype for g in got] == [np.float32] * 3 + [np.int32] * 3
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(list(data) + [track], keep)), "an input was written"
    ids, scores, bboxes, perm, track_out, dropped = got
    F, N = perm.shape
    empty = perm == -1
    assert (ids.reshape(F, N)[empty] == -1).all() and (scores.reshape(F, N)[empty] == -1).all() and (bboxes[empty] == -1).all()
    assert (track_out[empty] == -1).all() and (track_out[perm == -2] >= 0).all()
    assert not np.isnan(scores).any()
    sc = scores.reshape(F, N)
    for t in range(F):                                                     # every frame: descending, the empty rows last
        n = int((~empty[t]).sum())
        assert not empty[t, :n].any() and (np.diff(sc[t, :n]) <= 0).all()
    assert int((perm == -2).sum()) == sum(hs["filled"]) and int(dropped.sum()) == sum(hs["dropped"])
    return got, hs


@pytest.mark.parametrize("T,N,max_age", UC.RANDOM, ids=["%dx%d_age%d" % c for c in UC.RANDOM])
def test_host_equals_the_loop_form_on_random_clips(T, N, max_age):
    ids, scores, bboxes, track = UC.random_case(T, N, max_age)
    assert (track >= 0).any()
    for kw in UC.PARAMS:
        got, stats = _same((ids, scores, bboxes), track, **kw)
        filled = stats["filled"][0]
        print("%dx%d max_age %d %r: tracks %d filled %d dropped %d" % (T, N, max_age, kw, stats["tracks"][0], filled, stats["dropped"][0]))
        if T >= 5 and max_age >= 2 and kw["max_gap"] >= 2:
            assert filled > 0, "no hole was filled: the equalities would be vacuous"
        if kw["max_gap"] == 0 or max_age == 0:
            assert filled == 0 and stats["dropped"][0] == 0
        if kw["rescore"] is None and not kw["drop_untracked"]:             # the kept rows are the present rows, scores unchanged
            old = got[3] >= 0
            assert np.array_equal(got[1].reshape(T, N)[old], scores.reshape(T, N)[np.nonzero(old)[0], got[3][old]])


def test_some_random_case_drops_a_fill():
    ids, scores, bboxes, track = UC.random_case(40, 20, 7)
    _, stats = _same((ids, scores, bboxes), track, rescore="avg", max_gap=7)
    assert stats["dropped"][0] > 0 and stats["filled"][0] > 0


def test_max_gives_the_tracker_s_own_maximum_on_the_members():
    ids, scores, bboxes, _ = UC.random_case(40, 20, 2)
    track, tlen, tscore = track_host(ids, scores, bboxes, max_age=2)       # the defaults: some tracks are dropped
    out = tubelet_host(ids, scores, bboxes, track, rescore="max", max_gap=0)
    old = out[3]
    on = out[4] >= 0
    assert on.any() and (track < 0).any()
    t = np.nonzero(on)[0]
    assert np.array_equal(out[1].reshape(old.shape)[on], tscore[t, old[on]])
    assert np.array_equal(out[4][on], track[t, old[on]])


def test_several_clips_and_classes():
    data = UC.three_clips()
    got, stats = _same(data[:3], data[3], clip_start=data[4], num_class=1)
    assert all(f > 0 for f in stats["filled"]) and len(stats["tracks"]) == 3
    alone = tubelet_host(*[a[5:45] for a in data[:4]], num_class=1)
    assert all(np.array_equal(g[5:45], a) for g, a in zip(got, alone))
    case = UC.random_clip(9, 40, classes=3, seed=3)
    track = track_host(*case, num_class=3, max_age=3, t_min=1, sigma_h=0.0)[0]
    _same(case, track, num_class=3)
    cut, _ = _same(case, track, num_class=2)                               # class 2 is no candidate: its rows are not present
    assert not (cut[0] == 2).any() and (cut[0] == 1).any()
    flat = (case[0].reshape(9, 40), case[1].reshape(9, 40), case[2])       # (F,N) in, (F,N) out
    assert tubelet_host(*flat, track)[0].shape == (9, 40)
    with pytest.raises(ValueError, match="clip_start"):
        tubelet_host(*case, track, clip_start=[0, 4, 10])


@pytest.mark.parametrize("name,data,track,kw,expect", UC.closed_form(), ids=[c[0] for c in UC.closed_form()])
def test_closed_forms(name, data, track, kw, expect):
    got, _ = _same(data, track, **kw)
    UC.check_expected(got, expect)
    for more in UC.PARAMS:                                                 # and the loop form under every combination
        _same(data, track, **dict(kw, **more))


def test_parameters_are_checked_by_name():
    assert check_params() == ("avg", 7, False) == tuple(DEFAULTS[k] for k in ("rescore", "max_gap", "drop_untracked"))
    ids, scores, bboxes, track = UC.random_case(2, 3, 0)
    for kw, name in ((dict(rescore="mean"), "rescore"), (dict(rescore=0), "rescore"), (dict(rescore=["avg"]), "rescore"),
                     (dict(max_gap=8), "max_gap"), (dict(max_gap=-1), "max_gap"), (dict(max_gap=1.0), "max_gap"), (dict(max_gap=True), "max_gap"),
                     (dict(drop_untracked=1), "drop_untracked"), (dict(drop_untracked=None), "drop_untracked")):
        with pytest.raises(ValueError, match=name):
            tubelet_host(ids, scores, bboxes, track, **kw)
    with pytest.raises(ValueError, match="expected ids"):
        tubelet_host(ids, scores, bboxes[:, :, :3], track)
    with pytest.raises(ValueError, match="expected track"):
        tubelet_host(ids, scores, bboxes, track[:1])
    with pytest.raises(ValueError, match="expected track"):
        tubelet_host(ids, scores, bboxes, track.astype(np.float32))
    with pytest.raises(ValueError, match="at most 128"):
        tubelet_host(np.zeros((1, 129, 1)), np.zeros((1, 129, 1)), np.zeros((1, 129, 4)), np.zeros((1, 129), np.int32))


def test_library_exports_tubelet_and_checks_its_arguments_before_any_launch():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # entry points were added, nothing changed
    assert len(L.SIGNATURES["vd_tubelet"][1]) == 21 and len(L.SIGNATURES["vd_tubelet_ws_bytes"][1]) == 2
    assert len(L.SIGNATURES["vd_tubelet_stages"][1]) == 22
    assert L.TUBELET_MAX_ROWS == 128
    assert lib.vd_tubelet_ws_bytes(6, 20) == L.TUBELET_WS_PER_ROW * 6 * 20 and lib.vd_tubelet_ws_bytes(0, 20) == -1
    assert lib.vd_tubelet_ws_bytes(6, 129) == -1
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    need = lib.vd_tubelet_ws_bytes(6, 20)
    good = dict(ids=P, scores=P, bboxes=P, track=P, clip_start=P, V=2, F=6, N=20, num_class=3, rescore=1, max_gap=7, drop=0,
                out_ids=P, out_scores=P, out_bboxes=P, perm=P, track_out=P, dropped=P, ws=P, ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_tubelet(a["ids"], a["scores"], a["bboxes"], a["track"], a["clip_start"], a["V"], a["F"], a["N"], a["num_class"],
                            a["rescore"], a["max_gap"], a["drop"], a["out_ids"], a["out_scores"], a["out_bboxes"], a["perm"],
                            a["track_out"], a["dropped"], a["ws"], a["ws_bytes"], None)
        return rc, lib.vd_last_error()

    bad = [dict(ids=None), dict(scores=None), dict(bboxes=None), dict(track=None), dict(out_ids=None), dict(out_scores=None),
           dict(out_bboxes=None), dict(perm=None), dict(track_out=None), dict(dropped=None), dict(ws=None), dict(N=0), dict(N=129),
           dict(F=0), dict(V=0), dict(clip_start=None), dict(num_class=0), dict(rescore=3), dict(rescore=-1), dict(max_gap=8),
           dict(max_gap=-1), dict(drop=2), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(bboxes=P + 4), dict(out_bboxes=P + 8),
           dict(ws=P + 2), dict(ids=P + 2), dict(scores=P + 1), dict(track=P + 2), dict(clip_start=P + 2), dict(out_ids=P + 2),
           dict(out_scores=P + 1), dict(perm=P + 3), dict(track_out=P + 1), dict(dropped=P + 2)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_tubelet:"), (kw, err)
    for stages in (0, 16, -1):                                             # `good`'s keys are in the order of the arguments
        assert lib.vd_tubelet_stages(*good.values(), stages, None) == -1 and b"stages" in lib.vd_last_error()


TUB = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--tubelet"]


def test_detect_script_refuses_tubelet_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    with pytest.raises(NotImplementedError, match="--tubelet needs --track"):
        D.main(TUB + ["--stream"])
    with pytest.raises(NotImplementedError, match="--tubelet does not combine with --live"):
        D.main(TUB + ["--track", "--stream", "--live"])
    with pytest.raises(NotImplementedError, match="--tubelet does not combine with --seq_nms"):
        D.main(TUB + ["--track", "--stream", "--seq_nms"])
    with pytest.raises(NotImplementedError, match="--track needs clips"):
        D.main(TUB + ["--track"])
    for extra, name in ((["--tubelet_max_gap", "8"], "--tubelet_max_gap"), (["--tubelet_max_gap", "-1"], "--tubelet_max_gap")):
        with pytest.raises(NotImplementedError, match=name + " must"):
            D.main(TUB + ["--track", "--stream"] + extra)
    with pytest.raises(SystemExit):                                        # argparse's own refusal of a choice
        D.parse_flags(["--tubelet_rescore", "mean"])
    # with --track and clips it gets as far as asking for the GPU
    for extra in (["--stream"], ["--synthetic_videos", "2"], ["--stream", "--tubelet_rescore", "none", "--tubelet_drop_untracked"]):
        with pytest.raises(SystemExit):
            D.main(TUB + ["--track"] + extra)


def test_tubelet_flags_and_the_names_of_the_files():
    import os
    import detect_yolo3 as D
    F = D.parse_flags(["--tubelet"])
    assert F.tubelet is True and (F.tubelet_rescore, F.tubelet_max_gap, F.tubelet_drop_untracked) == ("avg", 7, False)
    assert D.parse_flags([]).tubelet is False and D.tubelet_args(D.parse_flags([])) is None
    assert D.tubelet_args(F) == DEFAULTS
    assert D.tubelet_args(D.parse_flags(["--tubelet", "--tubelet_rescore", "none", "--tubelet_max_gap", "3", "--tubelet_drop_untracked"])) == \
        dict(rescore=None, max_gap=3, drop_untracked=True)
    assert D.pred_dir("r", "p", tub=True) == os.path.join("r", "p", "pred_tub")
    assert D.pred_dir("r", "p", tub=True, trk=True) == os.path.join("r", "p", "pred_tub_trk")
    assert D.pred_dir("r", "p", True, tub=True) == os.path.join("r", "p", "pred_ag_tub")
    assert D.result_name("tracks", tub=True) == "tracks_tub" and D.result_name("vid", tub=True) == "vid_tub"
    assert D.result_name("voc", True, tub=True) == "voc_ag_tub"
    assert D.pred_dir("r", "p") == os.path.join("r", "p", "pred") and D.result_name("tracks", seq=True) == "tracks_seq"


def test_detect_video_refuses_a_bad_tubelet_argument_on_a_cpu_net():
    import torch
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["a", "b"], device="cpu")
    x = torch.zeros(4, 3, 64, 64)
    with pytest.raises(ValueError, match="tubelet needs track"):
        net.detect_video(x, tubelet=True)
    with pytest.raises(ValueError, match="tubelet takes rescore.*bogus"):
        net.detect_video(x, track=True, tubelet={"bogus": 1})
    with pytest.raises(ValueError, match="max_gap"):
        net.detect_video(x, track=True, tubelet=dict(max_gap=8))
    with pytest.raises(ValueError, match="rescore"):
        net.detect_video(x, track=True, tubelet=dict(rescore="mean"))
    with pytest.raises(TypeError):
        net.open_video(tubelet=True)                                       # a live session has no such argument
