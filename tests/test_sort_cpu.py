"""CPU: the definition of the SORT tracker (viddet_amd.sort.sort_host) against closed forms written out by hand and
against the paper's loop form (tests/sort_oracle.py: the full 7 x 7 filter in float64, the assignment by enumeration); the
decoupled filter against the 7 x 7 one in float64; then the `track=` option with `method`, the binding and the script's flags."""
import os

import numpy as np
import pytest

from tests import sort_cases as SC
from tests.sort_oracle import KalmanBox, sort_oracle
from viddet_amd import sort as S
from viddet_amd.sort import sort_host
from viddet_amd.track import track_host

# the decoupled float64 filter against the 7 x 7 one: the largest relative difference of a predicted box measured on this
# test's own inputs is 1.7e-14; the bound is 100 times that, and never looser than 1e-9
FILTER_MEASURED = 1.7e-14
FILTER_BOUND = min(100 * FILTER_MEASURED, 1e-9)

ORACLE_CASES = ([("sparse%d" % s, dict(), dict()) for s in (1, 3, 7, 8, 10, 21)] +
                [("sparse%d_age3" % s, dict(), dict(max_age=3, sigma_iou=0.4, num_class=2)) for s in (1, 3, 7, 8, 10, 21)] +
                [("dense%d" % s, dict(extent=120.0, classes=1, speed=4.0), dict(max_age=2)) for s in (0, 2, 4, 8, 10, 12, 21)])


@pytest.mark.parametrize("name,case,kw,track,tlen", SC.closed_form(), ids=[c[0] for c in SC.closed_form()])
def test_closed_forms(name, case, kw, track, tlen):
    got = sort_host(*case, **kw)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32 and got[3].dtype == np.float32
    assert got[3].shape == got[0].shape + (4,)
    assert got[0].tolist() == np.asarray(track).tolist()
    if tlen is not None:
        assert got[1].tolist() == np.asarray(tlen).tolist()
    off = got[0] < 0
    assert (got[1][off] == 0).all() and (got[2][off] == -1).all() and (got[3][off] == -1).all()
    sc = np.asarray(case[1], np.float32).reshape(got[0].shape)
    for u in np.unique(got[0][~off]):                                      # a track's maximum is the largest score among its rows
        assert (got[2][got[0] == u] == sc[got[0] == u].max()).all()


def test_the_gap_and_the_crossing_are_what_the_iou_tracker_loses():
    gap = SC.gap_case()
    track, tlen, _, tbox = sort_host(*gap, max_age=2, sigma_iou=0.5)
    assert len(np.unique(track[track >= 0])) == 1 and (tlen[track >= 0] == 4).all()
    assert abs(tbox[5, 0, 0] - 60.0) < 0.01                                # the filtered box sits on the returning one
    for si in (0.1, 0.3, 0.5):
        old = track_host(*gap, max_age=2, t_min=1, sigma_iou=si)[0]
        assert len(np.unique(old[old >= 0])) == 2                          # the last box overlaps the returning one with 0.053
    cross = [c for c in SC.closed_form() if c[0] == "cross"][0]
    assert track_host(*cross[1], **cross[2])[0].tolist() == [[0, 1], [0, 1], [0, 1]]            # the ids are swapped: rows changed
    assert sort_host(*cross[1], **cross[2])[0].tolist() == [[0, 1], [0, 1], [1, 0]]


def test_one_frame_tbox_is_the_box_of_z():
    """sqrt and divide alone: w = sqrt((w*h) * (w/h)), h = (w*h) / w in float32, one rounding each"""
    one = [c for c in SC.closed_form() if c[0] == "one_frame"][0]
    tbox = sort_host(*one[1], **one[2])[3][0]
    f = np.float32
    for b, got in zip(one[1][2][0], tbox):
        w, h = f(b[2] - b[0]), f(b[3] - b[1])
        u, v, s, r = f(b[0] + f(w / f(2))), f(b[1] + f(h / f(2))), f(w * h), f(w / h)
        bw = f(np.sqrt(f(s * r)))
        bh = f(s / bw)
        want = [f(u - f(bw / f(2))), f(v - f(bh / f(2))), f(u + f(bw / f(2))), f(v + f(bh / f(2)))]
        assert got.tolist() == want
        assert np.allclose(got, b, rtol=1e-5)


def test_two_clips_and_the_capacity_of_the_table():
    one = SC.walkers(3)
    case = [np.concatenate([a, a[:4]]) for a in one]
    both = sort_host(*case, clip_start=[0, 10, 10, 14], max_age=2)
    alone, head = sort_host(*one, max_age=2), sort_host(*[a[:4] for a in one], max_age=2)
    assert all(np.array_equal(b[:10], a, equal_nan=True) for b, a in zip(both, alone))
    assert all(np.array_equal(b[10:], a, equal_nan=True) for b, a in zip(both, head))
    stats = {}
    want = sort_host(*SC.capacity(False), max_age=7, t_min=1, stats=stats)
    assert stats["active"][:8].tolist() == [128 * (t + 1) for t in range(8)] and stats["active"].max() == 1024
    assert stats["closed"][:8].sum() == 0 and stats["closed"][8] == 128 and stats["closed"][9] == 128
    assert (want[0] == np.arange(1280).reshape(10, 128)).all() and (want[1] == 1).all()
    want = sort_host(*SC.capacity(True), max_age=7, t_min=1, stats=stats)
    assert stats["active"].tolist() == [128] * 10 and (want[0] == np.arange(128)[None, :]).all() and (want[1] == 10).all()
    want = sort_host(*SC.crowded(), t_min=1)
    assert (want[1] == 2).all() and sorted(want[0][1].tolist()) == list(range(128))              # every row took a track
    assert want[0][1].tolist() != list(range(128))


def test_parameters_are_checked():
    case = SC.gap_case()
    for kw, name in ((dict(max_age=8), "max_age"), (dict(max_age=-1), "max_age"), (dict(t_min=0), "t_min"),
                     (dict(sigma_iou=float("nan")), "sigma_iou"), (dict(sigma_l="x"), "sigma_l")):
        with pytest.raises(ValueError, match="sort_host: " + name):
            sort_host(*case, **kw)
    with pytest.raises(ValueError, match="expected ids"):
        sort_host(case[0], case[1], case[2][:, :, :3])
    with pytest.raises(ValueError, match="clip_start"):
        sort_host(*case, clip_start=[0, 3])
    assert S.DEFAULTS == dict(sigma_l=0.0, sigma_h=0.5, sigma_iou=0.3, t_min=2, max_age=1)


def _walks(seed, n=8, T=30):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        c = rng.uniform(100, 500, 2)
        wh = rng.uniform(16, 120, 2)
        boxes = []
        for _t in range(T):
            c = c + rng.uniform(-8, 8, 2)
            wh = np.maximum(wh * rng.uniform(0.95, 1.05, 2), 16.0)
            boxes.append(None if rng.uniform() < 0.2 and boxes else np.array([c[0] - wh[0] / 2, c[1] - wh[1] / 2, c[0] + wh[0] / 2, c[1] + wh[1] / 2]))
        out.append(boxes)
    return out


def test_the_decoupled_filter_is_the_7x7_filter_in_float64():
    worst = 0.0
    for walk in _walks(11):
        full = KalmanBox(walk[0])
        kf = S.kf_start(S.measure(np.asarray([walk[0]], dtype=np.float64)))
        assert kf["x"].dtype == np.float64
        for box in walk[1:]:
            want = full.predict()
            kf = S.kf_predict(kf)
            assert kf["x"][0, 2] > 0 and full.x[2] > 0                     # a negative area never occurs with these inputs
            got = S.kf_box(kf)[0]
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))))
            if box is not None:
                full.update(box)
                kf = S.kf_update(kf, S.measure(np.asarray([box], dtype=np.float64)))
        # the covariance too: the blocks of the 7 x 7 matrix are the decoupled filter's, everything else stays zero
        P = full.P
        blocks = np.zeros_like(P)
        for i in range(3):
            blocks[i, i], blocks[i, 4 + i], blocks[4 + i, i], blocks[4 + i, 4 + i] = kf["p00"][0, i], kf["p01"][0, i], kf["p01"][0, i], kf["p11"][0, i]
        blocks[3, 3] = kf["p"][0]
        assert np.allclose(P, blocks, rtol=1e-9, atol=1e-9)
    print("decoupled against 7x7, float64: the largest relative difference of a predicted box is %.3g" % worst)
    assert worst <= FILTER_BOUND


@pytest.mark.parametrize("name,gen,kw", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_the_definition_equals_the_paper_form(name, gen, kw):
    seed = int("".join(ch for ch in name.split("_")[0] if ch.isdigit()))
    case = SC.walkers(seed, **gen)
    assert case[2].shape[1] <= 6
    margins = {}
    track, tlen, _ = sort_oracle(*case, margins=margins, **kw)
    # the oracle decides every frame with room to spare, so float32 against float64 cannot flip a decision
    assert margins["iou"] >= 0.01, "an admissibility decision within 0.01 of sigma_iou"
    assert margins["assign"] >= 2 ** 10, "the best matching beats the runner-up by less than 2**10 quanta"
    got = sort_host(*case, **kw)
    assert np.array_equal(got[0], track) and np.array_equal(got[1], tlen)
    assert (track >= 0).sum() >= 30 and track.max() >= 4


def test_the_oracle_cases_are_contested():
    """some of the fixed seeds make the enumeration choose between matchings of equal size (a margin well below one pair)"""
    contested = 0
    for name, gen, kw in ORACLE_CASES:
        if name.startswith("dense"):
            margins = {}
            sort_oracle(*SC.walkers(int(name[5:]), **gen), margins=margins, **kw)
            contested += margins["assign"] < (1 << 26)
    assert contested >= 5


def test_parse_option_with_method():
    from viddet_amd.track import DEFAULTS, parse_option
    assert parse_option(None, 100, "w") is None and parse_option(False, 100, "w") is None
    assert parse_option(True, 100, "w") == (DEFAULTS, None, "iou")
    assert parse_option(dict(method="iou", max_age=2, clip=64), 100, "w") == (dict(DEFAULTS, max_age=2), 64, "iou")
    assert parse_option(dict(method="sort"), 100, "w") == (S.DEFAULTS, None, "sort")
    kw, clip, method = parse_option(dict(method="sort", sigma_iou=0.4, clip=32.0), 100, "w")
    assert kw == dict(S.DEFAULTS, sigma_iou=0.4) and clip == 32.0 and method == "sort"
    with pytest.raises(ValueError, match="w: track method must be 'iou' or 'sort', got 'deep'"):
        parse_option(dict(method="deep"), 100, "w")
    with pytest.raises(ValueError, match="w: track takes sigma_l, sigma_h, sigma_iou, t_min and max_age.*bogus"):
        parse_option(dict(method="sort", bogus=1), 100, "w")
    with pytest.raises(ValueError, match="max_age"):
        parse_option(dict(method="sort", max_age=8), 100, "w")
    with pytest.raises(ValueError, match="at most 128"):
        parse_option(dict(method="sort"), 129, "w")


def test_open_video_refuses_sort_on_a_cpu_net():
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["a", "b"], device="cpu")
    with pytest.raises(NotImplementedError, match="open_video with track method 'sort'"):
        net.open_video(track={"method": "sort"})
    with pytest.raises(ValueError, match="track method must be"):
        net.open_video(track={"method": "kalman"})


def test_binding_and_header_declare_the_entry_points():
    from viddet_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "viddet_hip.h")).read()
    assert "int vd_track_sort(" in hdr and "int64_t vd_track_sort_ws_bytes(int V, int F, int N);" in hdr
    assert len(L.SIGNATURES["vd_track_sort"][1]) == 20 and len(L.SIGNATURES["vd_track_sort_ws_bytes"][1]) == 3
    assert "#define VD_TRACK_SORT_WS_PER_ROW %d\n" % L.TRACK_SORT_WS_PER_ROW in hdr
    assert "#define VD_TRACK_SORT_WS_PER_CLIP %d\n" % L.TRACK_SORT_WS_PER_CLIP in hdr
    assert L.TRACK_SORT_WS_PER_CLIP == 2 * S.STATE_FLOATS * L.TRACK_MAX_ACTIVE * 4
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # entry points were added, nothing changed
    assert lib.vd_track_sort_ws_bytes(3, 10, 128) == 8 * 10 * 128 + 3 * L.TRACK_SORT_WS_PER_CLIP
    assert lib.vd_track_sort_ws_bytes(1, 10, 129) == -1 and lib.vd_track_sort_ws_bytes(0, 10, 1) == -1
    src = open(os.path.join(root, "viddet_amd", "csrc", "vd_track_sort.hip")).read()
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "vd_track_math.h"')
    assert "vd_track_sort.hip" in open(os.path.join(root, "viddet_amd", "csrc", "Makefile")).read()


TRK = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--track"]


def test_the_script_resolves_the_method_and_its_defaults():
    import detect_yolo3 as D
    F = D.parse_flags(["--track"])
    assert F.track_method == "iou" and (F.track_iou, F.track_max_age) == (0.5, 0)
    assert D.track_args(F) == dict(sigma_iou=0.5, sigma_l=0.0, sigma_h=0.5, t_min=2, max_age=0)
    F = D.parse_flags(["--track", "--track_method", "sort"])
    assert (F.track_iou, F.track_max_age) == (0.3, 1)
    assert D.track_args(F) == dict(S.DEFAULTS, method="sort")
    F = D.parse_flags(["--track", "--track_method", "sort", "--track_iou", "0.45", "--track_max_age", "0"])
    assert D.track_args(F) == dict(S.DEFAULTS, sigma_iou=0.45, max_age=0, method="sort")
    assert D.track_args(D.parse_flags(["--track_method", "sort"])) is None
    with pytest.raises(SystemExit):
        D.parse_flags(["--track", "--track_method", "deep"])


def test_the_script_refuses_sort_with_live_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    with pytest.raises(NotImplementedError, match="--track_method sort does not combine with --live"):
        D.main(TRK + ["--stream", "--live", "--track_method", "sort"])
    with pytest.raises(NotImplementedError, match="--track needs clips"):
        D.main(TRK + ["--track_method", "sort"])
    with pytest.raises(NotImplementedError, match="--track_max_age must"):
        D.main(TRK + ["--stream", "--track_method", "sort", "--track_max_age", "8"])
    # with clips it gets as far as asking for the GPU
    for extra in (["--stream"], ["--synthetic_videos", "2"]):
        with pytest.raises(SystemExit):
            D.main(TRK + ["--track_method", "sort"] + extra)
