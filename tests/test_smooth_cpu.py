"""CPU: the definition of the smoothing pass (viddet_amd.smooth.smooth_host), none of which touches a GPU.

Against the loop form of tests/smooth_oracle.py (the textbook 7-state filter and Rauch-Tung-Striebel smoother in float64), on the
closed forms of tests/smooth_cases.py, its forward pass against sort_host's and byte_host's filtered boxes, its effect on the
second differences of walker tracks; then the plumbing: clips, parameters, the option of detect_video, the ABI of
vd_track_smooth and the refusals of detect_yolo3.py --track_smooth."""
import numpy as np
import pytest

from tests import byte_cases as BC
from tests import smooth_cases as MC
from tests import sort_cases as SC
from tests.smooth_oracle import rts_segment, smooth_loop
from viddet_amd.byte import byte_host
from viddet_amd.smooth import DEFAULTS, check_params, parse_option, smooth_host
from viddet_amd.sort import kf_box, kf_start, measure, sort_host

# The largest coordinate difference between smooth_host (float32, decoupled) and the loop form (float64, 7 x 7) over
# smooth_cases.cv_tracks(): MEASURED 0.014477 px (coordinates up to 646; NumPy 2 on x86-64).  It is float32 rounding of the
# difference det = p00 * p11 - p01 * p01 and of the gains' numerators, which cancel to a few units out of 1e4 * 1e2.  The run is
# deterministic on the CPU: the factor 2 is slack for nothing but another NumPy build.
MEASURED = 0.014477
BOUND = 2 * MEASURED


# ------------------------------------------------------------------------------------------------ against the loop form
def test_host_equals_the_loop_form_on_jittered_constant_velocity_tracks():
    ids, scores, bboxes, track, cs = MC.cv_tracks()                        # 200 tracks, 2 to 40 frames, 0.5 px jitter, 15 % missing
    assert len(cs) == 201 and 600 < bboxes.max() < 700
    stats = {}
    sbox, slen = smooth_host(ids, scores, bboxes, track, clip_start=cs, stats=stats)
    want, wlen = smooth_loop(ids, scores, bboxes, track, clip_start=cs)
    assert np.array_equal(slen, wlen)
    assert sum(stats["members"]) == (slen > 0).sum() == (ids >= 0).sum() and sum(stats["segments"]) >= 195
    worst = np.abs(sbox.astype(np.float64) - want).max()
    print("worst coordinate difference %.6f px, bound %.6f" % (worst, BOUND))
    assert worst <= BOUND
    assert np.abs(sbox - bboxes).max() > 0.5                               # and it is no identity: boxes moved by more than the bound
    for g in (0, 2):                                                       # the cuts, and the segments on either side of them
        sbox, slen = smooth_host(ids, scores, bboxes, track, clip_start=cs, max_gap=g)
        want, wlen = smooth_loop(ids, scores, bboxes, track, clip_start=cs, max_gap=g)
        assert np.array_equal(slen, wlen) and np.abs(sbox.astype(np.float64) - want).max() <= BOUND


def test_float64_decoupled_form_equals_the_7x7_smoother():
    """the definition's arithmetic at float64 (sort.py's functions and rts_step follow their arrays' dtype): the covariance stays
    block diagonal through the backward pass too, so the two forms differ by float64 rounding only"""
    from viddet_amd.smooth import _predict_n, rts_step
    from viddet_amd.sort import kf_predict, kf_take, kf_update
    ids, scores, bboxes, track, cs = MC.cv_tracks(count=40, seed=5)
    worst = 0.0
    for a, b in zip(cs[:-1], cs[1:]):
        frames = [t for t in range(b - a) if track[a + t, 0] >= 0]
        if len(frames) < 2:
            continue
        box = bboxes[a:b, 0].astype(np.float64)[frames]
        post = [kf_start(measure(box[:1]))]
        for k in range(1, len(frames)):
            post.append(kf_update(_predict_n(post[-1], np.array([frames[k] - frames[k - 1]])), measure(box[k:k + 1])))
        S = dict(x=post[-1]["x"], xd=post[-1]["xd"], r=post[-1]["r"])
        out = [kf_box(S)]
        for k in range(len(frames) - 2, -1, -1):
            for j in range(frames[k + 1] - frames[k] - 1, -1, -1):
                f = _predict_n(post[k], np.array([j]))
                S = rts_step(S, f, kf_predict(f))
            out.append(kf_box(S))
        worst = max(worst, np.abs(np.concatenate(out[::-1]) - rts_segment(frames, box)[0]).max())
    assert worst < 1e-9, worst


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("frames", [list(range(6)), [0, 1, 4, 5, 6, 9]], ids=["dense", "holes"])
def test_a_stationary_box_with_power_of_two_sides_comes_back_bit_for_bit(frames):
    case = MC.still(frames)
    for g in (2, 7):
        sbox, slen = smooth_host(*case, max_gap=g)
        assert MC.same_bits(sbox, case[2])
        assert slen[:, 0].tolist() == [6 if t in frames else 0 for t in range(frames[-1] + 1)]


def test_one_outlier_is_pulled_back_and_its_neighbours_move_less():
    case = MC.outlier()
    sbox, slen = smooth_host(*case)
    x1, base = sbox[:, 0, 0], np.float32(MC.STILL[0])
    assert slen[:, 0].tolist() == [6] * 6
    assert base < x1[3] < base + 6
    for nb in (2, 4):
        assert base < x1[nb] < x1[3]                                       # towards the outlier ...
        assert x1[nb] - base < (base + 6) - x1[3]                          # ... by less than the outlier moves
    assert np.array_equal(sbox[:, 0, [1, 3]], case[2][:, 0, [1, 3]])       # y never moved: v and the sides are exact


def test_a_hole_wider_than_max_gap_cuts_the_track():
    ids, scores, bboxes, track = MC.holed()                                # frames 0..4 and 9..13
    sbox, slen = smooth_host(ids, scores, bboxes, track, max_gap=2)
    assert slen[:, 0].tolist() == [5] * 5 + [0] * 4 + [5] * 5
    head = smooth_host(ids[:5], scores[:5], bboxes[:5], track[:5], max_gap=2)
    tail = smooth_host(ids[9:], scores[9:], bboxes[9:], track[9:], max_gap=2)
    assert MC.same_bits(sbox[:5], head[0]) and MC.same_bits(sbox[9:], tail[0]) and MC.same_bits(sbox[5:9], bboxes[5:9])
    whole, wlen = smooth_host(ids, scores, bboxes, track, max_gap=4)       # a hole of 4 frames at max_gap 4: one segment
    assert wlen[:, 0].tolist() == [10] * 5 + [0] * 4 + [10] * 5 and not MC.same_bits(whole[:5], head[0])


def test_rows_that_keep_their_input_bits():
    ids, scores, bboxes, track, cs, slen = MC.keep_cases()
    stats = {}
    sbox, got = smooth_host(ids, scores, bboxes, track, clip_start=cs, stats=stats)
    assert np.array_equal(got, slen) and got.dtype == np.int32 and sbox.dtype == np.float32
    moved = (sbox.view(np.uint32) != bboxes.view(np.uint32)).any(axis=2)
    assert moved.tolist() == (slen == 2).tolist()
    assert stats["segments"] == [1, 1, 1] and stats["members"] == [1, 2, 1]
    assert MC.same_bits(stats["filtered"][[0, 3]], bboxes[[0, 3]])
    # a frame outside every clip: the definition takes offsets from 0 to F only, so the frame is cut off and kept by hand - the
    # device takes offsets as they are (tests/test_smooth_gpu.py)
    with pytest.raises(ValueError, match="clip_start"):
        smooth_host(ids, scores, bboxes, track, clip_start=[0, 1, 3])


def test_a_nan_box_keeps_the_input_wherever_it_reaches():
    ids, scores, bboxes, track = MC.nan_case()
    sbox, slen = smooth_host(ids, scores, bboxes, track)
    assert slen.tolist() == [[6, 6]] * 6
    # row 0: the NaN enters v's filter at frame 2 and stays in it; backwards it reaches frames 0 and 1 through the smoother.  v
    # is in every corner box through h and v, so the whole track keeps its input boxes; row 1 is smoothed as if alone
    assert MC.same_bits(sbox[:, 0], bboxes[:, 0])
    assert np.isnan(sbox).sum() == 1 and np.isnan(sbox[2, 0, 1])           # no NaN comes out that did not go in
    alone = smooth_host(ids[:, 1:], scores[:, 1:], bboxes[:, 1:], track[:, 1:] - 1)
    assert MC.same_bits(sbox[:, 1], alone[0][:, 0]) and not MC.same_bits(sbox[:, 1], bboxes[:, 1])
    for F, N in ((6, 65), (12, 128)):                                      # the hostile tables: zero heights, infinities, NaNs
        h = MC.hostile(F, N)
        sbox, _ = smooth_host(*h)
        bad = ~np.isfinite(sbox)
        assert np.array_equal(bad, ~np.isfinite(h[2])) and MC.same_bits(sbox[bad.any(axis=2)], h[2][bad.any(axis=2)])


# ------------------------------------------------------------------------------------------------ the forward pass
def _forward_equals(case, tracker, **kw):
    track, tlen, _, tbox = tracker(*case, max_age=3, t_min=1, sigma_h=0.0, **kw)
    stats = {}
    _, slen = smooth_host(*case, track, max_gap=3, stats=stats)
    on = track >= 0
    assert np.array_equal(slen[on], tlen[on]) and not slen[~on].any()      # gaps are at most max_age + 1: a track is one segment
    many = on & (tlen >= 2)
    assert many.any() and SC.same_tbox(stats["filtered"][many], tbox[many])
    one = on & (tlen == 1)                                                 # a track of one row is no segment to smooth: `filtered`
    if one.any():                                                          # is its input box, whose start state gives tbox
        assert MC.same_bits(stats["filtered"][one], case[2][one])
        assert SC.same_tbox(kf_box(kf_start(measure(case[2][one]))), tbox[one])
    return int(many.sum())


@pytest.mark.parametrize("seed", range(12))
def test_forward_pass_is_the_filter_of_sort_and_byte(seed):
    gen = dict(T=16, objects=8, jitter=2.0)
    assert _forward_equals(SC.walkers(seed, **gen), sort_host) > 40
    assert _forward_equals(BC.dipped(seed, **gen), byte_host) > 40


# ------------------------------------------------------------------------------------------------ effect
def test_smoothed_tracks_have_smaller_second_differences():
    """over all segments of three or more members of the walker clips above, at max_age 3 (gaps of up to 4 frames), on every
    three members in consecutive frames: the mean absolute second difference of the coordinates"""
    raw, smo = [], []
    for seed in range(12):
        case = SC.walkers(seed, T=16, objects=8, jitter=2.0)
        track = sort_host(*case, max_age=3, t_min=1, sigma_h=0.0)[0]
        sbox, slen = smooth_host(*case, track, max_gap=3)
        for u in np.unique(track[track >= 0]):
            t, i = np.nonzero(track == u)
            if len(t) < 3:
                continue
            assert (slen[t, i] == len(t)).all()
            for k in range(len(t) - 2):
                if t[k + 2] - t[k] == 2:
                    raw.append(MC.second_difference(case[2][t[k:k + 3], i[k:k + 3]]))
                    smo.append(MC.second_difference(sbox[t[k:k + 3], i[k:k + 3]]))
    raw, smo = float(np.mean(raw)), float(np.mean(smo))
    print("mean |second difference|: input %.3f, smoothed %.3f" % (raw, smo))
    assert smo < raw


# ------------------------------------------------------------------------------------------------ plumbing
def test_several_clips_equal_each_clip_alone():
    ids, scores, bboxes, track, cs = MC.three_clips()
    stats = {}
    sbox, slen = smooth_host(ids, scores, bboxes, track, clip_start=cs, num_class=2, stats=stats)
    assert len(stats["segments"]) == 3 and stats["filtered"].shape == bboxes.shape
    for a, b in zip(cs[:-1], cs[1:]):
        one = {}
        alone = smooth_host(ids[a:b], scores[a:b], bboxes[a:b], track[a:b], num_class=2, stats=one)
        assert MC.same_bits(sbox[a:b], alone[0]) and np.array_equal(slen[a:b], alone[1])
        assert MC.same_bits(stats["filtered"][a:b], one["filtered"])
    empty = smooth_host(ids, scores, bboxes, track, clip_start=[0, 6, 6, 46, 58], num_class=2)     # an empty clip in the middle
    assert MC.same_bits(empty[0], sbox) and np.array_equal(empty[1], slen)
    assert not MC.same_bits(smooth_host(ids, scores, bboxes, track, clip_start=cs, num_class=1)[0], sbox)   # class 1: no members


def test_parameters_and_the_option():
    assert DEFAULTS == dict(max_gap=7)
    assert check_params(0) == 0 and check_params(np.int64(7)) == 7
    for bad in (-1, 8, 1.0, True, None, "3"):
        with pytest.raises(ValueError, match="smooth_host: max_gap must be an integer in \\[0, 7\\]"):
            check_params(bad, "smooth_host")
    assert parse_option(None, False, "detect_video") is None and parse_option(False, True, "detect_video") is None
    assert parse_option(True, True, "detect_video") == {} and parse_option(dict(max_gap=3), True, "detect_video") == dict(max_gap=3)
    with pytest.raises(ValueError, match="detect_video: smooth needs track"):
        parse_option(True, False, "detect_video")
    with pytest.raises(ValueError, match="detect_video: smooth takes max_gap, got rescore"):
        parse_option(dict(rescore="avg"), True, "detect_video")
    with pytest.raises(ValueError, match="detect_video with smooth: max_gap"):
        parse_option(dict(max_gap=8), True, "detect_video")
    case = MC.still()
    with pytest.raises(ValueError, match="max_gap"):
        smooth_host(*case, max_gap=8)
    with pytest.raises(ValueError, match="expected track"):
        smooth_host(case[0], case[1], case[2], case[3].astype(np.float32))
    with pytest.raises(ValueError, match="expected ids"):
        smooth_host(case[0], case[1], case[2][:, :, :3], case[3])
    with pytest.raises(ValueError, match="at most 128"):
        smooth_host(np.zeros((1, 129, 1)), np.zeros((1, 129, 1)), np.zeros((1, 129, 4)), np.zeros((1, 129), np.int32))


def test_library_exports_track_smooth_and_checks_its_arguments_before_any_launch():
    import os
    import re
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # entry points were added, nothing changed
    assert len(L.SIGNATURES["vd_track_smooth"][1]) == 15 and len(L.SIGNATURES["vd_track_smooth_ws_bytes"][1]) == 2
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "viddet_hip.h")).read()
    assert int(re.search(r"#define VD_TRACK_SMOOTH_WS_PER_ROW\s+(\d+)", hdr).group(1)) == L.TRACK_SMOOTH_WS_PER_ROW == 12 + 4 * 17
    assert lib.vd_track_smooth_ws_bytes(6, 20) == 80 * 120 and lib.vd_track_smooth_ws_bytes((1 << 24) - 1, 128) == 80 * ((1 << 31) - 128)
    for F, N in ((0, 1), (1, 0), (1, 129), (1 << 24, 128)):
        assert lib.vd_track_smooth_ws_bytes(F, N) == -1
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    good = dict(ids=P, scores=P, bboxes=P, track=P, clip_start=P, V=2, F=6, N=20, num_class=3, max_gap=7, out_sbox=P, out_slen=P,
                ws=P, ws_bytes=80 * 120)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_track_smooth(a["ids"], a["scores"], a["bboxes"], a["track"], a["clip_start"], a["V"], a["F"], a["N"],
                                 a["num_class"], a["max_gap"], a["out_sbox"], a["out_slen"], a["ws"], a["ws_bytes"], None)
        return rc, lib.vd_last_error()

    bad = [dict(ids=None), dict(scores=None), dict(bboxes=None), dict(track=None), dict(out_sbox=None), dict(out_slen=None),
           dict(ws=None), dict(clip_start=None), dict(N=0), dict(N=129), dict(N=-1), dict(F=0), dict(V=0), dict(num_class=0),
           dict(F=1 << 24, N=128), dict(max_gap=8), dict(max_gap=-1), dict(ws_bytes=80 * 120 - 1), dict(ws_bytes=0),
           dict(bboxes=P + 4), dict(out_sbox=P + 8), dict(ids=P + 2), dict(scores=P + 1), dict(track=P + 2), dict(clip_start=P + 1),
           dict(out_slen=P + 3), dict(ws=P + 2)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_track_smooth:"), (kw, err)


SMOOTH = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--stream", "--track_smooth"]


def test_detect_script_refuses_track_smooth_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    assert D.parse_flags([]).track_smooth is False and D.parse_flags([]).track_smooth_gap == 7
    assert D.smooth_args(D.parse_flags([])) is None and D.smooth_args(D.parse_flags(["--track_smooth", "--track_smooth_gap", "3"])) == dict(max_gap=3)
    with pytest.raises(NotImplementedError, match="--track_smooth needs --track"):
        D.main(SMOOTH)
    with pytest.raises(NotImplementedError, match="--track_smooth does not combine with --live"):
        D.main(SMOOTH + ["--track", "--live"])
    with pytest.raises(NotImplementedError, match="--track_smooth does not combine with --seq_nms"):
        D.main(SMOOTH + ["--track", "--seq_nms"])
    with pytest.raises(NotImplementedError, match="--track_smooth does not combine with --tubelet"):
        D.main(SMOOTH + ["--track", "--tubelet"])
    for gap in ("8", "-1"):
        with pytest.raises(NotImplementedError, match="--track_smooth_gap must be an integer in \\[0, 7\\]"):
            D.main(SMOOTH + ["--track", "--track_smooth_gap", gap])
    with pytest.raises(SystemExit, match="needs an MI355X"):               # and what is not refused gets as far as the GPU check
        D.main(SMOOTH + ["--track", "--track_method", "sort", "--track_smooth_gap", "0"])
    assert D.pred_dir("s", "p", tub="smo", trk=True).endswith("pred_smo_trk") and D.pred_dir("s", "p", True, tub=True).endswith("pred_ag_tub")
    assert D.result_name("mot", tub="smo") == "mot_smo" and D.result_name("voc", True, tub="smo") == "voc_ag_smo"
    assert D.result_name("hota", False, True, tub="smo") == "hota_ag_met_smo" and D.result_name("vid", tub=True) == "vid_tub"
