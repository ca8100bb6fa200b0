"""CPU: the tracker's definition (viddet_amd.track.track_host) equals a plain-loop form written from the paper
(tests/track_oracle.py) on all three outputs, its closed forms with the ids written out by hand, the dataset's own track
partition on SyntheticTracks, the argument checks of vd_track and the refusals of detect_yolo3.py --track and
net.detect_video(track=...), none of which touches a GPU."""
import os

import numpy as np
import pytest

from tests import track_cases as TC
from tests.track_oracle import track_loops
from viddet_amd.seq_nms import iou_matrix
from viddet_amd.track import check_params, clip_summary, track_host


def _same(case, **kw):
    got = track_host(*case, **kw)
    want = track_loops(*case, **kw)
    for name, g, w in zip(("track", "tlen", "tscore"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, kw)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert np.array_equal(got[0] >= 0, got[1] > 0) and np.array_equal(got[0] < 0, got[2] == -1)
    return got


@pytest.mark.parametrize("T,N", TC.SIZES, ids=["%dx%d" % s for s in TC.SIZES])
@pytest.mark.parametrize("max_age", [0, 1, 7])
def test_host_equals_the_loop_form_on_random_clips(T, N, max_age):
    case = TC.random_clip(T, N, seed=7 * T + N, spread=40.0 + N, fill=1.0 if N < 4 else 0.8)
    keep = [a.copy() for a in case]
    got = _same(case, max_age=max_age, t_min=1 if T == 1 else 2, sigma_h=0.05 if N < 4 else 0.5)
    assert (got[0] >= 0).any()
    assert all(np.array_equal(a, b) for a, b in zip(case, keep)), "an input was written"


@pytest.mark.parametrize("classes,absent", [(1, ()), (3, (1,)), (20, (0, 7, 19))])
def test_host_equals_the_loop_form_with_several_classes(classes, absent):
    case = TC.random_clip(7, 40, classes=classes, seed=classes, absent=absent)
    got = _same(case, num_class=classes)
    assert (got[0] >= 0).any()
    assert np.array_equal(track_host(*case)[0], got[0])                     # no bound is the bound that holds every id
    if classes == 20:                                                      # fewer classes than ids: the rows above are no candidates
        cut = _same(case, num_class=5)
        assert (cut[0][case[0][:, :, 0] >= 5] == -1).all() and (cut[0] >= 0).any()
    # ids all 0 (an agnostic model): one class
    _same((np.where(case[0] >= 0, np.float32(0), case[0]), case[1], case[2]), num_class=1)


def test_host_equals_the_loop_form_with_every_parameter_off_its_default():
    case = TC.random_clip(12, 30, classes=2, seed=11, fill=0.7)
    base = _same(case)
    got = _same(case, **TC.OFF_DEFAULT)
    assert not np.array_equal(base[0], got[0])
    for k, v in TC.OFF_DEFAULT.items():                                    # and each alone
        _same(case, **{k: v})
    _same(case, sigma_l=-np.inf, sigma_h=-np.inf, sigma_iou=0.0, t_min=1)
    assert (track_host(*case, sigma_h=np.inf)[0] == -1).all()


def test_clips_with_an_empty_one_do_not_link_across_their_boundaries():
    one = TC.random_clip(6, 24, classes=2, seed=13, fill=1.0)
    case = [np.concatenate([a, a[:4]]) for a in one]                       # the same boxes on both sides of the boundary
    got = _same(case, clip_start=[0, 6, 6, 10], num_class=2, max_age=1)
    alone = track_host(*one, num_class=2, max_age=1)
    assert all(np.array_equal(g[:6], a) for g, a in zip(got, alone))
    assert got[0][6:].min() == -1 and got[0][6][got[0][6] >= 0].min() == 0   # ids start again at 0
    with pytest.raises(ValueError, match="clip_start"):
        track_host(*case, clip_start=[0, 6, 11])


@pytest.mark.parametrize("name,case,kw,track,tlen", TC.closed_form(), ids=[c[0] for c in TC.closed_form()])
def test_closed_forms(name, case, kw, track, tlen):
    got = _same(case, **kw)
    assert got[0].tolist() == np.asarray(track).tolist()
    if tlen is not None:
        assert got[1].tolist() == np.asarray(tlen).tolist()


def test_the_exact_half_is_an_iou_of_one_half():
    case = dict((c[0], c) for c in TC.closed_form())["half_matched"][1]
    assert iou_matrix(case[2][0], case[2][1])[0, 0] == np.float32(0.5)


def test_parameters_are_checked_by_name():
    assert check_params() == (np.float32(0), np.float32(0.5), np.float32(0.5), 2, 0)
    case = TC.random_clip(2, 3, seed=1)
    for kw, name in ((dict(max_age=8), "max_age"), (dict(max_age=-1), "max_age"), (dict(max_age=1.0), "max_age"),
                     (dict(t_min=0), "t_min"), (dict(t_min=2.5), "t_min"), (dict(sigma_l=float("nan")), "sigma_l"),
                     (dict(sigma_h=float("nan")), "sigma_h"), (dict(sigma_iou=float("nan")), "sigma_iou"), (dict(sigma_iou="x"), "sigma_iou")):
        with pytest.raises(ValueError, match=name):
            track_host(*case, **kw)
    with pytest.raises(ValueError, match="expected ids"):
        track_host(case[0], case[1], case[2][:, :, :3])


def test_synthetic_tracks_are_recovered_exactly():
    """The ground-truth rows of SyntheticTracks at score 0.9 give the dataset's own track partition in all 8 clips, per class
    and with all ids 0: 29 tracks, every row assigned."""
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("vid", num_videos=8, frames_per_video=32)
    T = ds.frames_per_video
    labels = [[ds.get_label(ds.sample_index(v, t) + 1) for t in range(T)] for v in range(ds.num_videos)]
    N = max(len(l) for clip in labels for l in clip)
    # the precondition: an object's boxes of consecutive frames overlap by at least sigma_iou (0.679 at the least here)
    low = 1.0
    for clip in labels:
        for a, b in zip(clip, clip[1:]):
            for ra in a:
                for rb in b[b[:, 5] == ra[5]]:
                    low = min(low, float(iou_matrix(ra[None, :4], rb[None, :4])[0, 0]))
    print("smallest consecutive-frame IoU of an object: %.3f" % low)
    assert low >= 0.5, "the dataset changed: an object moves further than the tracker's sigma_iou follows"
    total = 0
    for agnostic in (False, True):
        total = 0
        for clip in labels:
            ids, scores, bboxes = -np.ones((T, N, 1), np.float32), -np.ones((T, N, 1), np.float32), -np.ones((T, N, 4), np.float32)
            truth = -np.ones((T, N), np.int64)
            for t, l in enumerate(clip):
                n = len(l)
                ids[t, :n, 0], scores[t, :n, 0], bboxes[t, :n], truth[t, :n] = (0 if agnostic else l[:, 4]), 0.9, l[:, :4], l[:, 5]
            track, tlen, tscore = track_host(ids, scores, bboxes)
            assert np.array_equal(track >= 0, truth >= 0), "every row is assigned"
            pairs = set(zip(track[truth >= 0].tolist(), truth[truth >= 0].tolist()))
            n_truth = len(set(truth[truth >= 0].tolist()))
            assert len(pairs) == n_truth == len(set(p[0] for p in pairs)), "the partition is the dataset's"
            for tid, gid in pairs:
                assert (tlen[track == tid] == (truth == gid).sum()).all()
            total += n_truth
        assert total == 29


def test_clip_summary_counts_tracks_and_rows():
    track = np.array([[0, -1], [0, 2], [5, -1], [5, 5]])
    assert clip_summary(track, None, [0, 2, 2, 4]) == [(2, 3, 1.5), (0, 0, 0.0), (1, 3, 3.0)]


def test_library_exports_track_and_checks_its_arguments_before_any_launch():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # an entry point was added, nothing changed
    assert "vd_track" in L.SIGNATURES and len(L.SIGNATURES["vd_track"][1]) == 19
    assert (L.TRACK_MAX_ROWS, L.TRACK_MAX_ACTIVE, L.TRACK_WS_PER_ROW) == (128, 1024, 8)
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    good = dict(ids=P, scores=P, bboxes=P, clip_start=P, V=2, F=6, N=20, num_class=3, sl=0.0, sh=0.5, si=0.5, t_min=2, max_age=0,
                out_track=P, out_len=P, out_score=P, ws=P, ws_bytes=8 * 6 * 20)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_track(a["ids"], a["scores"], a["bboxes"], a["clip_start"], a["V"], a["F"], a["N"], a["num_class"], a["sl"],
                          a["sh"], a["si"], a["t_min"], a["max_age"], a["out_track"], a["out_len"], a["out_score"], a["ws"],
                          a["ws_bytes"], None)
        return rc, lib.vd_last_error()

    nan = float("nan")
    bad = [dict(ids=None), dict(scores=None), dict(bboxes=None), dict(out_track=None), dict(out_len=None), dict(out_score=None),
           dict(ws=None), dict(N=0), dict(N=129), dict(N=-1), dict(F=0), dict(V=0), dict(clip_start=None), dict(num_class=0),
           dict(sl=nan), dict(sh=nan), dict(si=nan), dict(t_min=0), dict(max_age=8), dict(max_age=-1),
           dict(ws_bytes=8 * 6 * 20 - 1), dict(ws_bytes=0), dict(bboxes=P + 4), dict(ws=P + 2), dict(ids=P + 2), dict(scores=P + 1),
           dict(clip_start=P + 2), dict(out_track=P + 2), dict(out_len=P + 1), dict(out_score=P + 3)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_track:"), (kw, err)


TRK = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--track"]


def test_detect_script_refuses_track_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    with pytest.raises(NotImplementedError, match="--track needs clips"):
        D.main(TRK)
    with pytest.raises(NotImplementedError, match="--track needs clips"):
        D.main(TRK + ["--metrics", "vid"])
    with pytest.raises(NotImplementedError, match="--track does not combine with several --dataset names"):
        D.main(["--random_init", "--dataset", "voc,coco", "--track", "--synthetic_videos", "2"])
    with pytest.raises(NotImplementedError, match="--track does not combine with --mult_out"):
        D.main(TRK + ["--stream", "--mult_out"])
    for extra, name in ((["--track_max_age", "8"], "--track_max_age"), (["--track_max_age", "-1"], "--track_max_age"),
                        (["--track_min_len", "0"], "--track_min_len"), (["--track_iou", "nan"], "--track_iou"),
                        (["--track_low", "nan"], "--track_low"), (["--track_high", "nan"], "--track_high")):
        with pytest.raises(NotImplementedError, match=name + " must"):
            D.main(TRK + ["--stream"] + extra)
    # with clips it gets as far as asking for the GPU
    for extra in (["--stream"], ["--synthetic_videos", "2"], ["--stream", "--seq_nms", "--track_max_age", "7"]):
        with pytest.raises(SystemExit):
            D.main(TRK + extra)


def test_track_flags_and_the_names_of_the_twins():
    import detect_yolo3 as D
    F = D.parse_flags(["--track"])
    assert F.track is True
    assert (F.track_iou, F.track_low, F.track_high, F.track_min_len, F.track_max_age) == (0.5, 0.0, 0.5, 2, 0)
    assert D.parse_flags([]).track is False and D.track_args(D.parse_flags([])) is None
    assert D.track_args(F) == dict(sigma_iou=0.5, sigma_l=0.0, sigma_h=0.5, t_min=2, max_age=0)
    from viddet_amd.track import DEFAULTS
    assert D.track_args(F) == DEFAULTS
    assert D.pred_dir("r", "p", trk=True) == os.path.join("r", "p", "pred_trk")
    assert D.pred_dir("r", "p", seq=True, trk=True) == os.path.join("r", "p", "pred_seq_trk")
    assert D.pred_dir("r", "p", True, trk=True) == os.path.join("r", "p", "pred_ag_trk")
    assert D.pred_dir("r", "p") == os.path.join("r", "p", "pred") and D.pred_dir("r", "p", seq=True) == os.path.join("r", "p", "pred_seq")
    assert D.result_name("tracks") == "tracks" and D.result_name("tracks", seq=True) == "tracks_seq"


def test_detect_video_refuses_a_bad_track_argument_on_a_cpu_net():
    import torch
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["a", "b"], device="cpu")
    x = torch.zeros(4, 3, 64, 64)
    with pytest.raises(ValueError, match="track takes sigma_l.*bogus"):
        net.detect_video(x, track={"bogus": 1})
    with pytest.raises(ValueError, match="max_age"):
        net.detect_video(x, track=dict(max_age=8))
    net.set_nms(post_nms=129)
    with pytest.raises(ValueError, match="post_nms=129"):
        net.detect_video(x, track=True)
