"""CPU: the definition of the BYTE tracker (viddet_amd.byte.byte_host) against closed forms written out by hand,
against sort_host where the second association has nothing to do, and against the paper's loop form (tests/byte_oracle.py: the
full 7 x 7 filter in float64, both assignments by enumeration, the second over a compacted track list); then the `track=` option
with method 'byte', the binding and the script's flags."""
import os

import numpy as np
import pytest

from tests import byte_cases as BC
from tests import sort_cases as SC
from tests.byte_oracle import byte_oracle
from viddet_amd import byte as B
from viddet_amd.byte import byte_host
from viddet_amd.sort import sort_host

ORACLE_CASES = ([("sparse%d" % s, dict(), dict()) for s in (0, 2, 3, 6, 7, 12)] +
                [("sparse%d_age3" % s, dict(), dict(max_age=3, sigma_iou=0.3, sigma_iou2=0.4, num_class=2)) for s in (0, 2, 6, 7, 8, 12)] +
                [("dense%d" % s, dict(extent=120.0, classes=1, speed=4.0), dict(max_age=2)) for s in (1, 3, 5, 6, 7, 23, 25)])


@pytest.mark.parametrize("name,case,kw,track,tlen", BC.closed_form(), ids=[c[0] for c in BC.closed_form()])
def test_closed_forms(name, case, kw, track, tlen):
    got = byte_host(*case, **kw)
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


def test_the_dip_and_the_clutter_are_what_sort_loses():
    """the two options sort_host leaves: a high sigma_l breaks the track at the dip, a low one hands it to the clutter"""
    stats = {}
    track, tlen, _, _ = byte_host(*BC.dip_case(), stats=stats)
    assert track[:, 0].tolist() == [0] * 5 and (tlen == 5).all()
    assert stats["first"].tolist() == [0, 1, 0, 0, 1] and stats["second"].tolist() == [0, 0, 1, 1, 0]
    cut = sort_host(*BC.dip_case(), sigma_l=.5)[0]
    assert cut[2, 0] == -1 and cut[3, 0] == -1
    assert byte_host(*BC.clutter_case())[0].tolist() == [[0, -1], [0, -1], [-1, 0]]
    assert sort_host(*BC.clutter_case(), sigma_l=.1, sigma_iou=.2)[0].tolist() == [[0, -1], [0, -1], [0, -1]]


def test_no_low_rows_is_sort_at_that_sigma_l():
    """sigma_l > sigma_d leaves no low rows: sort_host at that sigma_l, with sigma_new = sigma_d (every candidate may start)"""
    for seed in (1, 3):
        case = SC.walkers(seed)
        got = byte_host(*case, sigma_l=0.7, sigma_d=0.5, sigma_new=0.5, sigma_iou=0.3, max_age=1)
        want = sort_host(*case, sigma_l=0.7)
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))
        assert (want[0] >= 0).any() and (np.asarray(case[1]).reshape(want[0].shape)[want[0] < 0] > 0.5).any()


@pytest.mark.parametrize("seed", [1, 3, 7, 8, 10, 21])
def test_reduction_to_sort(seed):
    """sigma_d = sigma_new = sigma_l: every candidate is a high row that may start a track, the second association is never
    entered, and what is left is sort_step"""
    for case, kw in ((SC.walkers(seed), dict(sigma_iou=0.3, max_age=1)),
                     (SC.walkers(seed, extent=120.0, classes=1, speed=4.0), dict(sigma_iou=0.4, max_age=3, sigma_l=0.6))):
        sl = kw.pop("sigma_l", 0.0)
        stats = {}
        got = byte_host(*case, sigma_l=sl, sigma_d=sl, sigma_new=sl, stats=stats, **kw)
        want = sort_host(*case, sigma_l=sl, **kw)
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))
        assert stats["second"].sum() == 0 and stats["first"].sum() > 0


def test_reduction_to_sort_on_the_crowded_pair():
    stats = {}
    got = byte_host(*SC.crowded(), sigma_l=0.0, sigma_d=0.0, sigma_new=0.0, sigma_iou=0.3, max_age=1, t_min=1, stats=stats)
    want = sort_host(*SC.crowded(), t_min=1)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))
    assert stats["first"].tolist() == [0, 128]


def test_the_crowded_pair_runs_both_associations_wide():
    stats = {}
    want = byte_host(*BC.crowded_pair(), stats=stats, **BC.CROWDED_KW)
    assert stats["first"].tolist() == [0, 64] and stats["second"].tolist() == [0, 63]
    assert (want[0][1] < 0).sum() == 1 and (want[0][1][0::2] >= 0).all()   # one low row found no track


def test_two_clips_and_the_capacity_of_the_table():
    one = BC.dipped(3)
    case = [np.concatenate([a, a[:4]]) for a in one]
    both = byte_host(*case, clip_start=[0, 10, 10, 14], max_age=2)
    alone, head = byte_host(*one, max_age=2), byte_host(*[a[:4] for a in one], max_age=2)
    assert all(np.array_equal(b[:10], a, equal_nan=True) for b, a in zip(both, alone))
    assert all(np.array_equal(b[10:], a, equal_nan=True) for b, a in zip(both, head))
    stats = {}
    want = byte_host(*BC.capacity_full(), max_age=7, t_min=1, stats=stats)
    assert stats["active"][:8].tolist() == [128 * (t + 1) for t in range(8)] and stats["active"].max() == 1024
    assert stats["second"].tolist() == [0] * 8 + [128, 0] and stats["first"].sum() == 0
    assert (want[0][8] == want[0][7]).all() and (want[1][7] == 2).all()
    want = byte_host(*BC.capacity_low(True), max_age=7, t_min=1, stats=stats)
    assert stats["active"].tolist() == [128] * 10 and (want[0] == np.arange(128)[None, :]).all() and (want[1] == 10).all()
    assert stats["second"].tolist() == [0, 128] * 5 and stats["first"].tolist() == [0, 0] + [128, 0] * 4
    want = byte_host(*BC.capacity_low(False), max_age=7, t_min=1, stats=stats)
    assert stats["active"].max() == 512 and stats["second"].sum() == 0 and (want[0][1::2] == -1).all()


def test_parameters_are_checked():
    case = BC.dip_case()
    for kw, name in ((dict(max_age=8), "max_age"), (dict(max_age=-1), "max_age"), (dict(t_min=0), "t_min"),
                     (dict(sigma_iou=float("nan")), "sigma_iou"), (dict(sigma_l="x"), "sigma_l"), (dict(sigma_d=float("nan")), "sigma_d"),
                     (dict(sigma_new=float("nan")), "sigma_new"), (dict(sigma_iou2=float("nan")), "sigma_iou2"),
                     (dict(sigma_d=None), "sigma_d")):
        with pytest.raises(ValueError, match="byte_host: " + name):
            byte_host(*case, **kw)
    with pytest.raises(ValueError, match="expected ids"):
        byte_host(case[0], case[1], case[2][:, :, :3])
    with pytest.raises(ValueError, match="clip_start"):
        byte_host(*case, clip_start=[0, 3])
    assert B.DEFAULTS == dict(sigma_l=0.1, sigma_d=0.5, sigma_new=0.6, sigma_iou=0.2, sigma_iou2=0.5, sigma_h=0.5, t_min=2, max_age=7)
    # no order among the thresholds is demanded
    byte_host(*case, sigma_l=0.9, sigma_d=0.2, sigma_new=0.1, sigma_iou=0.9, sigma_iou2=0.1)


@pytest.mark.parametrize("name,gen,kw", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_the_definition_equals_the_paper_form(name, gen, kw):
    seed = int("".join(ch for ch in name.split("_")[0] if ch.isdigit()))
    case = BC.dipped(seed, **gen)
    assert case[2].shape[1] <= 6
    margins = {}
    track, tlen, second = byte_oracle(*case, margins=margins, **kw)
    # the oracle decides every frame with room to spare, so float32 against float64 cannot flip a decision
    assert margins["iou"] >= 0.01, "an admissibility decision of the first association within 0.01 of sigma_iou"
    assert margins["iou2"] >= 0.01, "an admissibility decision of the second association within 0.01 of sigma_iou2"
    assert margins["det"] >= 0.01, "a score within 0.01 of sigma_d"
    assert margins["new"] >= 0.01, "an unmatched high row's score within 0.01 of sigma_new"
    assert margins["assign"] >= 2 ** 10, "the first association's best matching beats the runner-up by less than 2**10 quanta"
    assert margins["assign2"] >= 2 ** 10, "the second association's best matching beats the runner-up by less than 2**10 quanta"
    stats = {}
    got = byte_host(*case, stats=stats, **kw)
    assert np.array_equal(got[0], track) and np.array_equal(got[1], tlen)
    assert stats["second"].sum() == second
    assert (track >= 0).sum() >= 30 and track.max() >= 3


def test_the_oracle_cases_use_the_second_association():
    """at least a quarter of the chosen clips have a pair made in the second association (in fact every one has)"""
    with_pairs = sum(byte_oracle(*BC.dipped(int("".join(ch for ch in name.split("_")[0] if ch.isdigit())), **gen), **kw)[2] > 0
                     for name, gen, kw in ORACLE_CASES)
    assert 4 * with_pairs >= len(ORACLE_CASES)


def test_parse_option_with_method_byte():
    from viddet_amd.track import DEFAULTS, METHODS, parse_option
    assert METHODS == ("iou", "sort", "byte")
    assert parse_option(dict(method="byte"), 100, "w") == (B.DEFAULTS, None, "byte")
    kw, clip, method = parse_option(dict(method="byte", sigma_d=0.4, sigma_new=0.7, sigma_iou2=0.3, max_age=2, clip=32.0), 100, "w")
    assert kw == dict(B.DEFAULTS, sigma_d=0.4, sigma_new=0.7, sigma_iou2=0.3, max_age=2) and clip == 32.0 and method == "byte"
    assert parse_option(True, 100, "w") == (DEFAULTS, None, "iou")
    with pytest.raises(ValueError, match="w: track method must be 'iou' or 'sort', got 'deep'.*'byte'"):
        parse_option(dict(method="deep"), 100, "w")
    for method in ("iou", "sort"):                                         # the three keys are byte's alone
        with pytest.raises(ValueError, match="w: track takes sigma_l, sigma_h, sigma_iou, t_min and max_age .*got sigma_d"):
            parse_option(dict(method=method, sigma_d=0.4), 100, "w")
    with pytest.raises(ValueError, match="w: track takes sigma_l, sigma_h, sigma_iou, t_min and max_age, sigma_d, sigma_new, sigma_iou2.*bogus"):
        parse_option(dict(method="byte", bogus=1), 100, "w")
    with pytest.raises(ValueError, match="max_age"):
        parse_option(dict(method="byte", max_age=8), 100, "w")
    with pytest.raises(ValueError, match="sigma_new must not be NaN"):
        parse_option(dict(method="byte", sigma_new=float("nan")), 100, "w")
    with pytest.raises(ValueError, match="at most 128"):
        parse_option(dict(method="byte"), 129, "w")


def test_open_video_refuses_byte_on_a_cpu_net():
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["a", "b"], device="cpu")
    with pytest.raises(NotImplementedError, match="open_video with track method 'byte'"):
        net.open_video(track={"method": "byte"})


def test_binding_header_and_makefile_declare_the_entry_points():
    from viddet_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "viddet_hip.h")).read()
    assert "int vd_track_byte(" in hdr and "int64_t vd_track_byte_ws_bytes(int V, int F, int N);" in hdr
    assert len(L.SIGNATURES["vd_track_byte"][1]) == 23 and len(L.SIGNATURES["vd_track_byte_ws_bytes"][1]) == 3
    assert len(L.SIGNATURES["vd_track_byte"][1]) == len(L.SIGNATURES["vd_track_sort"][1]) + 3
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # entry points were added, nothing changed
    for V, F, N in ((3, 10, 128), (1, 1, 1), (64, 64, 100)):
        assert lib.vd_track_byte_ws_bytes(V, F, N) == lib.vd_track_sort_ws_bytes(V, F, N) == 8 * F * N + V * L.TRACK_SORT_WS_PER_CLIP
    assert lib.vd_track_byte_ws_bytes(1, 10, 129) == -1 and lib.vd_track_byte_ws_bytes(0, 10, 1) == -1
    assert lib.vd_track_byte_ws_bytes(1, 0, 1) == -1 and lib.vd_track_byte_ws_bytes(1, 10, 0) == -1
    assert lib.vd_track_byte_ws_bytes(1, 1 << 30, 2) == -1                 # F * N = 2^31
    csrc = os.path.join(root, "viddet_amd", "csrc")
    for name in ("vd_track_byte.hip", "vd_track_sort.hip"):                # one filter, included by both, after the pragma
        src = open(os.path.join(csrc, name)).read()
        assert src.index("#pragma clang fp contract(off)") < src.index('#include "vd_track_math.h"') < src.index('#include "vd_track_kf.h"')
        assert "struct Kf" not in src
    assert "struct Kf" in open(os.path.join(csrc, "vd_track_kf.h")).read()
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "vd_track_byte.hip" in make and "vd_track_kf.h" in make.split("%.o:")[1].splitlines()[0]


TRK = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--track"]


def test_the_script_resolves_the_method_and_its_defaults():
    import detect_yolo3 as D
    from viddet_amd.sort import DEFAULTS as SORT
    from viddet_amd.track import DEFAULTS as IOU
    F = D.parse_flags(["--track"])
    assert (F.track_iou, F.track_low, F.track_max_age) == (0.5, 0.0, 0) and (F.track_det, F.track_new, F.track_iou2) == (None,) * 3
    assert D.track_args(F) == IOU
    F = D.parse_flags(["--track", "--track_method", "sort"])
    assert (F.track_iou, F.track_low, F.track_max_age) == (0.3, 0.0, 1) and (F.track_det, F.track_new, F.track_iou2) == (None,) * 3
    assert D.track_args(F) == dict(SORT, method="sort")
    F = D.parse_flags(["--track", "--track_method", "byte"])
    assert (F.track_iou, F.track_low, F.track_max_age, F.track_det, F.track_new, F.track_iou2) == (0.2, 0.1, 7, 0.5, 0.6, 0.5)
    assert D.track_args(F) == dict(B.DEFAULTS, method="byte")
    F = D.parse_flags(["--track", "--track_method", "byte", "--track_low", "0.0", "--track_det", "0.4", "--track_new", "0.7",
                       "--track_iou2", "0.3", "--track_iou", "0.25", "--track_max_age", "3", "--track_high", "0.6", "--track_min_len", "3"])
    assert D.track_args(F) == dict(sigma_l=0.0, sigma_d=0.4, sigma_new=0.7, sigma_iou=0.25, sigma_iou2=0.3, sigma_h=0.6, t_min=3,
                                   max_age=3, method="byte")
    assert D.parse_flags(["--track", "--track_low", "0.3"]).track_low == 0.3
    assert D.track_args(D.parse_flags(["--track_method", "byte"])) is None
    with pytest.raises(SystemExit):
        D.parse_flags(["--track", "--track_method", "deep"])


def test_the_script_refuses_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    with pytest.raises(NotImplementedError, match="--track_method byte does not combine with --live"):
        D.main(TRK + ["--stream", "--live", "--track_method", "byte"])
    with pytest.raises(NotImplementedError, match="--track needs clips"):
        D.main(TRK + ["--track_method", "byte"])
    with pytest.raises(NotImplementedError, match="--track_max_age must"):
        D.main(TRK + ["--stream", "--track_method", "byte", "--track_max_age", "8"])
    with pytest.raises(NotImplementedError, match="--track_new must not be NaN"):
        D.main(TRK + ["--stream", "--track_method", "byte", "--track_new", "nan"])
    for method in ([], ["--track_method", "iou"], ["--track_method", "sort"]):
        for flag in ("--track_det", "--track_new", "--track_iou2"):
            with pytest.raises(NotImplementedError, match=flag + " belongs to --track_method byte"):
                D.main(TRK + ["--stream", flag, "0.4"] + method)
    # with clips it gets as far as asking for the GPU
    for extra in (["--stream"], ["--synthetic_videos", "2"], ["--stream", "--track_det", "0.4", "--track_new", "0.5", "--track_iou2", "0.3"]):
        with pytest.raises(SystemExit):
            D.main(TRK + ["--track_method", "byte"] + extra)
