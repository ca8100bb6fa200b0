"""CPU: the definition of the stitching pass (viddet_amd.stitch.stitch_host), none of which touches a GPU.

Against the loop form of tests/stitch_oracle.py (the 7-state filter with its 7 x 7 matrices in float64, the links by enumeration)
on seeded clips that the oracle decides with a margin, on the closed forms of tests/stitch_cases.py, the cap of 512 participants,
hostile tables and several clips; then the plumbing: parameters, the option of detect_video, the ABI of vd_track_stitch and the
refusals of detect_yolo3.py --track_stitch."""
import numpy as np
import pytest

from tests import byte_cases as BC
from tests import smooth_cases as MC
from tests import sort_cases as SC
from tests import stitch_cases as TC
from tests.stitch_oracle import stitch_oracle
from viddet_amd.byte import byte_host
from viddet_amd.sort import sort_host
from viddet_amd.stitch import DEFAULTS, STITCH_MAX_GAP, STITCH_MAX_TRACKS, check_params, parse_option, stitch_host

# ------------------------------------------------------------------------------------------------ against the loop form
# Six walkers of one class in a field of 90 px, an occlusion of 3 to 9 frames cut out of each, SORT at max_age 1: 10 to 13
# tracks, several tails within reach of one head.  The seeds are those among 0..39 for which the ORACLE ALONE clears both
# margins and whose best matching has a rival (a margin below one pair, 2**27).  Measured on them (float64, deterministic):
#   seed            0       2       6       12      13      14       15      16       18      23      26      36
#   |iou - 0.3|     0.1516  0.1026  0.0216  0.2407  0.0173  0.0180   0.0480  0.0357   0.0118  0.0499  0.0134  0.0132
#   assign margin   508545  722518  528737  823736  687293  1046343  311278  1199293  494176  586065  628858  959691
# Asserted: 0.01 and 2**10 quanta (an IoU sum of 0.001).  The definition's float32 filter and IoU differ from the oracle's by
# some 1e-5 in the IoU of boxes of 30 to 60 px after at most 12 predictions, so neither decision can flip within the margins.
ORACLE_SEEDS = [0, 2, 6, 12, 13, 14, 15, 16, 18, 23, 26, 36]
IOU_MARGIN, ASSIGN_MARGIN = 0.01, 2 ** 10


def _crowd(seed):
    data = TC.cut_holes(SC.walkers(seed, T=24, objects=6, classes=1, miss=0.05, jitter=0.5, extent=90.0, speed=3.0, size=(30.0, 60.0)),
                        seed, lo=3, hi=9)
    return TC.tracked(data, num_class=2, **TC.KEEP_ALL)


@pytest.mark.parametrize("seed", ORACLE_SEEDS)
def test_host_equals_the_loop_form(seed):
    case = _crowd(seed)
    margins, stats = {}, {}
    strack, tlen, links = stitch_oracle(*case, num_class=2, max_gap=12, margins=margins)
    print("seed %d: |iou - sigma_iou| >= %.4f, best matching ahead by %d" % (seed, margins["iou"], margins["assign"]))
    assert margins["iou"] >= IOU_MARGIN, "an admissibility decision within 0.01 of sigma_iou"
    assert ASSIGN_MARGIN <= margins["assign"] < 2 ** 27, "the best matching beats the runner-up by less than 2**10 quanta, or has no rival"
    got = stitch_host(*case, num_class=2, max_gap=12, stats=stats)
    assert np.array_equal(got[0], strack) and np.array_equal(got[1], tlen)
    assert got[3].tolist() == [len(links)] == stats["links"] and len(links) >= 3 and stats["pairs"][0] > len(links)
    assert stats["tracks"][0] == len(np.unique(case[3][case[3] >= 0])) and got[4].tolist() == [0]


# ------------------------------------------------------------------------------------------------ closed forms
def test_one_hidden_object_is_linked_once_max_gap_reaches_its_gap():
    case = TC.hidden_one()
    assert np.unique(case[3]).tolist() == [-1, 0, 1] and (case[3][10:22] == -1).all()
    strack, tlen, tscore, stitches, overflow = stitch_host(*case, max_gap=12)
    assert stitches.tolist() == [0] and np.array_equal(strack, case[3]) and tlen.max() == 10
    stats = {}
    strack, tlen, tscore, stitches, overflow = stitch_host(*case, max_gap=13, stats=stats)
    seen = case[3][:, 0] >= 0
    assert stitches.tolist() == [1] and overflow.tolist() == [0] and stats == dict(tracks=[2], pairs=[1], links=[1])
    assert strack[seen, 0].tolist() == [0] * 20 and tlen[seen, 0].tolist() == [20] * 20 and (strack[~seen] == -1).all()
    assert (tlen[~seen] == 0).all() and (tscore[~seen] == -1).all() and (tscore[seen] == np.float32(0.9)).all()
    assert strack.dtype == tlen.dtype == stitches.dtype == overflow.dtype == np.int32 and tscore.dtype == np.float32
    assert stitch_host(*case, max_gap=13, sigma_iou=0.99)[3].tolist() == [0]        # the extrapolated tail is near, not on, the head


def test_two_objects_keep_their_ids_through_a_crossing():
    case = TC.crossing()
    assert case[3][0].tolist() == [0, 1] and case[3][20].tolist() == [2, 3]
    _, _, links = stitch_oracle(*case, max_gap=30)
    assert [(a, b) for _, a, b, _ in links] == [(0, 2), (1, 3)] and all(q > 0.9 for _, _, _, q in links)
    stats = {}
    strack, tlen, _, stitches, _ = stitch_host(*case, stats=stats)
    assert stitches.tolist() == [2] and stats["pairs"] == [2]                       # the wrong pairings are not admissible at all
    assert strack[20:].tolist() == [[0, 1]] * 10 and (tlen[20:] == 20).all()


def test_a_class_mismatch_gives_no_link():
    case = TC.other_class()
    strack, tlen, _, stitches, _ = stitch_host(*case, num_class=2)
    assert stitches.tolist() == [0] and np.array_equal(strack, case[3]) and tlen.max() == 10
    ids = np.where(case[0] >= 0, 0, case[0]).astype(np.float32)                     # the same rows of one class
    assert stitch_host(ids, *case[1:], num_class=2)[3].tolist() == [1]


def test_three_fragments_make_one_chain_with_the_first_id():
    case = TC.three_fragments()
    assert np.unique(case[3]).tolist() == [-1, 0, 1, 2]
    strack, tlen, tscore, stitches, _ = stitch_host(*case)
    on = case[3] >= 0
    assert stitches.tolist() == [2] and (strack[on] == 0).all() and (tlen[on] == 24).all()
    assert (tscore[on] == np.float32(0.9)).all()                                    # the chain's maximum: the middle fragment's
    assert stitch_host(*case, max_gap=5)[3].tolist() == [0]                         # the holes are 6 frames wide


def test_two_tails_compete_for_one_head():
    strack, tlen, tscore, stitches, _ = stitch_host(*TC.compete())
    assert stitches.tolist() == [1]
    assert strack.tolist() == [[0, 1]] * 3 + [[-1, -1]] * 2 + [[0, -1]] * 2        # the larger IoU wins, the loser stays
    assert tlen.tolist() == [[5, 3]] * 3 + [[0, 0]] * 2 + [[5, 0]] * 2
    assert tscore[0].tolist() == [np.float32(.9), np.float32(.8)] and tscore[5, 0] == np.float32(.9)


def test_a_nan_box_is_never_linked():
    for case in (TC.nan_head(), TC.nan_tail()):
        strack, tlen, _, stitches, _ = stitch_host(*case, max_gap=13)
        assert stitches.tolist() == [0] and np.array_equal(strack, case[3]) and tlen.max() == 10
        # iou_matrix's arithmetic gives a pair with a NaN side the IoU 0 (its `iw > 0` is false) or NaN: below every positive
        # threshold.  (At sigma_iou <= 0 every pair of a class within max_gap frames is admissible, disjoint boxes too.)
        assert stitch_host(*case, max_gap=13, sigma_iou=1e-30)[3].tolist() == [0]


@pytest.mark.parametrize("seed", range(4))
def test_with_nothing_admissible_the_three_arrays_are_the_trackers(seed):
    gen = dict(T=16, objects=8, jitter=2.0)
    for case, tracker in ((SC.walkers(seed, **gen), sort_host), (BC.dipped(seed, **gen), byte_host)):
        track, tlen, tscore, _ = tracker(*case, max_age=2)
        got = stitch_host(*case, track, sigma_iou=2.0)
        assert (track >= 0).sum() > 40 and got[3].tolist() == [0]
        assert np.array_equal(got[0], track) and np.array_equal(got[1], tlen) and TC.same_bits(got[2], tscore)


# ------------------------------------------------------------------------------------------------ the cap
def test_the_cap_of_512_participants():
    ids, scores, bboxes, track = TC.cap()
    assert track.shape == (5, 128) and np.array_equal(np.sort(track.ravel()), np.arange(640))
    stats = {}
    strack, tlen, tscore, stitches, overflow = stitch_host(ids, scores, bboxes, track, max_gap=2, stats=stats)
    assert overflow.tolist() == [128] == [640 - STITCH_MAX_TRACKS] and stats["tracks"] == [640]
    # tracks 512.. (frame 4) link nothing, although their boxes sit on frame 2's
    assert np.array_equal(strack[4], track[4]) and (tlen[4] == 1).all() and TC.same_bits(tscore[4], scores[4, :, 0])
    # the first 512 link as the uncapped rule says: the four frames alone hold exactly them
    alone = stitch_host(ids[:4], scores[:4], bboxes[:4], track[:4], max_gap=2)
    assert alone[4].tolist() == [0] and alone[3].tolist() == [256] == stitches.tolist()
    for k in range(3):
        assert TC.same_bits(np.asarray(alone[k], np.float32), np.asarray((strack, tlen, tscore)[k][:4], np.float32))
    assert np.array_equal(strack[2:4], track[:2]) and (tlen[:4] == 2).all()
    assert TC.same_bits(tscore[:2], np.maximum(scores[:2, :, 0], scores[2:4, :, 0]))
    assert stitch_host(ids, scores, bboxes, track, max_gap=1)[3].tolist() == [0]    # the frame between holds other boxes


# ------------------------------------------------------------------------------------------------ plumbing
@pytest.mark.parametrize("F,N", [(6, 65), (12, 128)], ids=["6x65", "12x128"])
def test_hostile_tables(F, N):
    case = MC.hostile(F, N)
    stats = {}
    strack, tlen, tscore, stitches, overflow = stitch_host(*case, sigma_iou=0.05, stats=stats)
    member = tlen > 0
    assert stats["tracks"][0] > 1 and stitches[0] == stats["links"][0] <= stats["pairs"][0] and overflow.tolist() == [0]
    assert ((strack >= 0) == member).all() and (tscore[~member] == -1).all() and np.isfinite(tscore).all()
    assert (case[0][..., 0][member] >= 0).all() and ((case[3][member] >= 0) & (case[3][member] < F * N)).all()
    ids_of = {}                                                                     # a chain's rows agree on its length
    for u, n in zip(strack[member], tlen[member]):
        assert ids_of.setdefault(int(u), int(n)) == n
    assert sum(ids_of.values()) == member.sum()


def test_several_clips_equal_each_clip_alone():
    ids, scores, bboxes, track, cs = TC.three_clips()
    stats = {}
    got = stitch_host(ids, scores, bboxes, track, clip_start=cs, num_class=2, max_gap=12, stats=stats)
    assert len(stats["tracks"]) == 3 and got[3].shape == got[4].shape == (3,) and got[4].tolist() == [0, 0, 128]
    for v, (a, b) in enumerate(zip(cs[:-1], cs[1:])):
        alone = stitch_host(ids[a:b], scores[a:b], bboxes[a:b], track[a:b], num_class=2, max_gap=12)
        assert np.array_equal(got[0][a:b], alone[0]) and np.array_equal(got[1][a:b], alone[1]) and TC.same_bits(got[2][a:b], alone[2])
        assert got[3][v] == alone[3][0] > 0 and got[4][v] == alone[4][0]
    offs = [0, cs[1], cs[1]] + cs[2:]                                               # an empty clip in the middle
    empty = stitch_host(ids, scores, bboxes, track, clip_start=offs, num_class=2, max_gap=12)
    assert np.array_equal(empty[0], got[0]) and empty[3].tolist() == [got[3][0], 0, got[3][1], got[3][2]]
    with pytest.raises(ValueError, match="clip_start"):
        stitch_host(ids, scores, bboxes, track, clip_start=[0, 12, 42])


def test_parameters_and_the_option():
    assert DEFAULTS == dict(max_gap=30, sigma_iou=0.3) and STITCH_MAX_TRACKS == 512 and STITCH_MAX_GAP == 32
    assert check_params(1, 0) == (1, np.float32(0)) and check_params(np.int64(32), np.float32(0.5)) == (32, np.float32(0.5))
    for bad in (0, 33, -1, 1.0, True, None, "3"):
        with pytest.raises(ValueError, match="stitch_host: max_gap must be an integer in \\[1, 32\\]"):
            check_params(bad, 0.3, "stitch_host")
    for bad in (float("nan"), None, "x", True):
        with pytest.raises(ValueError, match="stitch_host: sigma_iou must be a number"):
            check_params(30, bad, "stitch_host")
    assert parse_option(None, False, "detect_video") is None and parse_option(False, True, "detect_video") is None
    assert parse_option(True, True, "detect_video") == {}
    assert parse_option(dict(max_gap=3, sigma_iou=0.5), True, "detect_video") == dict(max_gap=3, sigma_iou=0.5)
    with pytest.raises(ValueError, match="detect_video: stitch needs track"):
        parse_option(True, False, "detect_video")
    with pytest.raises(ValueError, match="detect_video: stitch takes max_gap and sigma_iou, got rescore"):
        parse_option(dict(rescore="avg"), True, "detect_video")
    with pytest.raises(ValueError, match="detect_video with stitch: max_gap"):
        parse_option(dict(max_gap=33), True, "detect_video")
    with pytest.raises(ValueError, match="detect_video with stitch: sigma_iou"):
        parse_option(dict(sigma_iou=float("nan")), True, "detect_video")
    case = TC.compete()
    with pytest.raises(ValueError, match="max_gap"):
        stitch_host(*case, max_gap=0)
    with pytest.raises(ValueError, match="expected track"):
        stitch_host(case[0], case[1], case[2], case[3].astype(np.float32))
    with pytest.raises(ValueError, match="expected ids"):
        stitch_host(case[0], case[1], case[2][:, :, :3], case[3])
    with pytest.raises(ValueError, match="at most 128"):
        stitch_host(np.zeros((1, 129, 1)), np.zeros((1, 129, 1)), np.zeros((1, 129, 4)), np.zeros((1, 129), np.int32))


def test_detect_video_takes_the_option_and_open_video_does_not():
    import inspect
    from viddet_amd import live
    from viddet_amd.model import YOLOV3
    assert inspect.signature(YOLOV3.detect_video).parameters["stitch"].default is None
    assert inspect.signature(live.detect_video).parameters["stitch"].default is None
    assert "stitch" not in inspect.signature(YOLOV3.open_video).parameters


def test_library_exports_track_stitch_and_checks_its_arguments_before_any_launch():
    import os
    import re
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # entry points were added, nothing changed
    assert len(L.SIGNATURES["vd_track_stitch"][1]) == 19 and len(L.SIGNATURES["vd_track_stitch_ws_bytes"][1]) == 2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "viddet_hip.h")).read()
    assert "int vd_track_stitch(" in hdr and "int64_t vd_track_stitch_ws_bytes(int F, int N);" in hdr
    assert "vd_track_stitch.hip" in open(os.path.join(root, "viddet_amd", "csrc", "Makefile")).read()
    assert int(re.search(r"#define VD_TRACK_STITCH_WS_PER_ROW\s+(\d+)", hdr).group(1)) == L.TRACK_STITCH_WS_PER_ROW == 4 + 4 * (17 + 7)
    assert int(re.search(r"#define VD_TRACK_STITCH_MAX_TRACKS\s+(\d+)", hdr).group(1)) == L.STITCH_MAX_TRACKS == STITCH_MAX_TRACKS
    assert int(re.search(r"#define VD_TRACK_STITCH_MAX_GAP\s+(\d+)", hdr).group(1)) == L.STITCH_MAX_GAP == STITCH_MAX_GAP
    assert lib.vd_track_stitch_ws_bytes(6, 20) == 100 * 120 and lib.vd_track_stitch_ws_bytes((1 << 24) - 1, 128) == 100 * ((1 << 31) - 128)
    for F, N in ((0, 1), (1, 0), (1, 129), (1 << 24, 128)):
        assert lib.vd_track_stitch_ws_bytes(F, N) == -1
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    good = dict(ids=P, scores=P, bboxes=P, track=P, clip_start=P, V=2, F=6, N=20, num_class=3, max_gap=30, sigma_iou=0.3,
                out_track=P, out_len=P, out_score=P, out_stitches=P, out_overflow=P, ws=P, ws_bytes=100 * 120)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_track_stitch(a["ids"], a["scores"], a["bboxes"], a["track"], a["clip_start"], a["V"], a["F"], a["N"],
                                 a["num_class"], a["max_gap"], a["sigma_iou"], a["out_track"], a["out_len"], a["out_score"],
                                 a["out_stitches"], a["out_overflow"], a["ws"], a["ws_bytes"], None)
        return rc, lib.vd_last_error()

    bad = [dict(ids=None), dict(scores=None), dict(bboxes=None), dict(track=None), dict(out_track=None), dict(out_len=None),
           dict(out_score=None), dict(out_stitches=None), dict(out_overflow=None), dict(ws=None), dict(clip_start=None), dict(N=0),
           dict(N=129), dict(N=-1), dict(F=0), dict(V=0), dict(num_class=0), dict(F=1 << 24, N=128), dict(max_gap=33), dict(max_gap=0),
           dict(sigma_iou=float("nan")), dict(ws_bytes=100 * 120 - 1), dict(ws_bytes=0), dict(bboxes=P + 4), dict(ids=P + 2),
           dict(scores=P + 1), dict(track=P + 2), dict(clip_start=P + 1), dict(out_track=P + 3), dict(out_len=P + 1),
           dict(out_score=P + 2), dict(out_stitches=P + 2), dict(out_overflow=P + 1), dict(ws=P + 2)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_track_stitch:"), (kw, err)


STITCH = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--stream", "--track_stitch"]


def test_detect_script_refuses_track_stitch_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    flags = D.parse_flags([])
    assert flags.track_stitch is False and flags.track_stitch_gap is None and flags.track_stitch_iou is None
    assert D.stitch_args(flags) is None and D.stitch_args(D.parse_flags(["--track_stitch"])) == dict(max_gap=30, sigma_iou=0.3)
    assert D.stitch_args(D.parse_flags(["--track_stitch", "--track_stitch_gap", "3", "--track_stitch_iou", "0.5"])) == dict(max_gap=3, sigma_iou=0.5)
    with pytest.raises(NotImplementedError, match="--track_stitch needs --track"):
        D.main(STITCH)
    with pytest.raises(NotImplementedError, match="--track_stitch does not combine with --live"):
        D.main(STITCH + ["--track", "--live"])
    with pytest.raises(NotImplementedError, match="--track_stitch does not combine with --seq_nms"):
        D.main(STITCH + ["--track", "--seq_nms"])
    with pytest.raises(NotImplementedError, match="--track_stitch does not combine with --tubelet"):
        D.main(STITCH + ["--track", "--tubelet"])
    with pytest.raises(NotImplementedError, match="--track_stitch does not combine with --track_smooth"):
        D.main(STITCH + ["--track", "--track_smooth"])
    for gap in ("33", "0", "-1"):
        with pytest.raises(NotImplementedError, match="--track_stitch_gap must be an integer in \\[1, 32\\]"):
            D.main(STITCH + ["--track", "--track_stitch_gap", gap])
    with pytest.raises(NotImplementedError, match="--track_stitch_iou must be a number and not NaN"):
        D.main(STITCH + ["--track", "--track_stitch_iou", "nan"])
    for sub in (["--track_stitch_gap", "30"], ["--track_stitch_iou", "0.3"]):
        with pytest.raises(NotImplementedError, match="%s needs --track_stitch" % sub[0]):
            D.main(STITCH[:-1] + ["--track"] + sub)
    with pytest.raises(SystemExit, match="needs an MI355X"):               # and what is not refused gets as far as the GPU check
        D.main(STITCH + ["--track", "--track_method", "byte", "--track_stitch_gap", "32", "--track_stitch_iou", "0"])
    assert D.pred_dir("s", "p", tub="sti", trk=True).endswith("pred_sti_trk") and D.pred_dir("s", "p", True, tub="sti", trk=True).endswith("pred_ag_sti_trk")
    assert D.result_name("mot", tub="sti") == "mot_sti" and D.result_name("hota", True, tub="sti") == "hota_ag_sti"
    assert D.result_name("tracks", tub="sti") == "tracks_sti"
