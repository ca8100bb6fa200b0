"""CPU: the HOTA tracking metric's definition (viddet_amd/hota_metric.py): closed forms whose outputs are written
out by hand (tests/hota_cases.py), hota_match_host and hota_summary against the loop form of tests/hota_oracle.py on seeded
clips, the clip combination by hand, the metric class, the argument checks of vd_hota_match and the refusals of
detect_yolo3.py --metrics hota, none of which touches a GPU."""
import functools
import math

import numpy as np
import pytest

from tests import hota_cases as HC
from tests import hota_oracle as HO
from viddet_amd import hota_metric as H
from viddet_amd.mot_metric import masked_track

# the seeds of the clips held against the oracle: chosen so that the two margins asserted below hold
SEEDS = (1, 3, 4, 5, 6, 9, 10, 12)
# The rates against the oracle.  The definition's similarity is a float32 IoU and its scores are floored to 2**-20; neither
# moves a count (the margins are asserted), so a rate differs only through LocA's float32 terms and float64 roundings.  The
# largest absolute difference measured on these clips is 7.9e-8 (a LocA, seed 1: one float32 rounding of an IoU near 1); 100
# times it is allowed.
MEASURED, RATE_TOL = 7.9e-8, 7.9e-6


# ---- closed forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,arrays,kw,expect", HC.closed_forms(), ids=[c[0] for c in HC.closed_forms()])
def test_closed_form(name, arrays, kw, expect):
    records = H.hota_match_host(*arrays, **kw)
    match_kw = {k: v for k, v in kw.items() if k == "clip_start"}
    summary = H.hota_summary(records, arrays[2], masked_track(arrays[3], arrays[4], arrays[6], kw.get("num_class")), **match_kw)
    HC.check_expected(records, summary, expect)
    assert records[0].dtype == np.int32 and records[1].dtype == np.float32 and records[2].dtype == np.int32
    assert ((records[2] >= 0) & (records[2] <= 1 << 20)).all()


def test_the_alphas_and_the_side_one_half_falls_on():
    assert H.ALPHAS.dtype == np.float32 and len(H.ALPHAS) == 19
    assert np.float32(0.5) >= np.float32(0.05 * 10) and H.ALPHAS[9] == np.float32(0.5) and not np.float32(0.5) >= H.ALPHAS[10]
    assert H.ALPHAS.tolist() == [float(a) for a in HO.ALPHAS]


# ---- the matching and the summary against the loop form -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seeded(seed):
    arrays = HO.random_clip(seed, F=10, objects=3 + seed % 4)
    kw = dict(num_class=2, agnostic=bool(seed % 3 == 0), clip_start=[0, 10] if seed % 2 else [0, 4, 10])
    margins = {}
    want = HO.hota_oracle(*arrays, margins=margins, **kw)
    return arrays, kw, want, margins


@pytest.mark.parametrize("seed", SEEDS)
def test_definition_equals_the_oracle(seed):
    arrays, kw, (want_match, want_clips), margins = _seeded(seed)
    # a float32 or quantised decision cannot flip: no matched pair within 1e-4 of an alpha, no runner-up within 2**-10
    assert margins["alpha"] >= 1e-4, margins
    assert margins["assign"] >= 2.0 ** -10, margins
    records = H.hota_match_host(*arrays, **kw)
    track = masked_track(arrays[3], arrays[4], arrays[6], kw["num_class"])
    summary = H.hota_summary(records, arrays[2], track, kw["clip_start"])
    assert np.array_equal(records[0], want_match)
    assert int((want_match >= 0).sum()) > 15                                       # the clip is no empty exercise
    worst = 0.0
    for (t0, t1), got, want in zip(zip(kw["clip_start"][:-1], kw["clip_start"][1:]), summary["clips"], want_clips):
        ga, gp, cg, cp, a, p, sim = H.clip_tables(records, arrays[2].astype(np.int64), track.astype(np.int64), t0, t1)
        assert dict(zip(ga.tolist(), cg.tolist())) == want["cg"] and dict(zip(gp.tolist(), cp.tolist())) == want["cp"]
        assert (got["GT"], got["PRED"], got["gt_tracks"], got["pred_tracks"]) == (want["GT"], want["PRED"], len(want["cg"]), len(want["cp"]))
        assert got["TP"] == want["TP"] and got["FN"] == want["FN"] and got["FP"] == want["FP"]
        for k, alpha in enumerate(H.ALPHAS):
            mc = {}
            for x, y in zip(ga[a[sim >= alpha]].tolist(), gp[p[sim >= alpha]].tolist()):
                mc[x, y] = mc.get((x, y), 0) + 1
            assert mc == want["mc"][k]
        for name in H.PER_ALPHA:
            worst = max([worst, abs(got[name] - want[name])] + [abs(x - y) for x, y in zip(got[name + "@"], want[name + "@"])])
    print("seed %d: the largest |rate - oracle| = %.3g" % (seed, worst))
    assert worst <= RATE_TOL
    # msim is the float32 IoU of the pair the oracle matched, mscore its score in units of 2**-20, floored
    on = want_match >= 0
    assert np.array_equal(records[1] > 0, on) and (records[2][~on] == 0).all()


def test_two_clips_combine_by_hand():
    """clip 0 is one_track_answered_by_two (TP 6, AssA 1/2, DetA 1), clip 1 every_second_frame with a second, unanswered
    ground-truth track (TP 3 of GT 12, PRED 3): DetA = 3 / 12, AssA = 1/2"""
    from tests.mot_cases import A, B, build
    gt = [[(A, 0, 0)]] * 6 + [[(A, 0, 0), (B, 0, 1)]] * 6
    pred = [[(A, 0, 0.9, 1)]] * 3 + [[(A, 0, 0.9, 2)]] * 3 + [[(A, 0, 0.9, 1)], []] * 3
    arrays = build(gt, pred)
    records = H.hota_match_host(*arrays, clip_start=[0, 6, 12])
    s = H.hota_summary(records, arrays[2], masked_track(arrays[3], arrays[4], arrays[6]), [0, 6, 12])
    c0, c1, al = s["clips"][0], s["clips"][1], s["all"]
    assert (c0["DetA"], c0["AssA"], c0["TP"][0]) == (1.0, 0.5, 6) and (c1["DetA"], c1["AssA"], c1["TP"][0]) == (0.25, 0.5, 3)
    # counts summed: TP 9, GT 18, PRED 9: DetA = 9 / 18; AssA = (1/2 * 6 + 1/2 * 3) / 9; AssPr = (1 * 6 + 1 * 3) / 9
    assert al["TP"] == [9] * 19 and al["GT"] == 18 and al["PRED"] == 9 and al["FN"] == [9] * 19 and al["FP"] == [0] * 19
    assert al["DetA"] == 0.5 and abs(al["AssA"] - 0.5) < 1e-15 and abs(al["AssPr"] - 1.0) < 1e-15 and al["LocA"] == 1.0
    assert abs(al["HOTA"] - 0.5) < 1e-15 and al["gt_tracks"] == 3 and al["pred_tracks"] == 3 and al["frames"] == 12
    # unequal weights: make clip 1's AssA differ - its track answered by two ids on its three frames (mc 2 and 1)
    pred = [[(A, 0, 0.9, 1)]] * 6 + [[(A, 0, 0.9, 1)], [], [(A, 0, 0.9, 1)], [], [(A, 0, 0.9, 2)], []]
    arrays = build(gt, pred)
    s = H.hota_summary(H.hota_match_host(*arrays, clip_start=[0, 6, 12]), arrays[2], masked_track(arrays[3], arrays[4], arrays[6]), [0, 6, 12])
    # clip 0 perfect: AssA 1, TP 6; clip 1: mc = (2, 1), cg = 6, cp = (2, 1): AssA = (4 / 6 + 1 / 6) / 3 = 5/18, TP 3
    assert s["clips"][0]["AssA"] == 1.0 and abs(s["clips"][1]["AssA"] - 5 / 18) < 1e-15
    assert abs(s["all"]["AssA"] - (1.0 * 6 + 5 / 18 * 3) / 9) < 1e-15
    assert abs(s["all"]["HOTA"] - math.sqrt(0.5 * (6 + 5 / 6) / 9)) < 1e-15


# ---- the metric class ------------------------------------------------------------------------------------------------------
def _feed(metric, ds, shift=0.0, drop=()):
    for sid in ds.get_sample_ids():
        rows = ds.get_label(sid)
        keep = np.array([i for i in range(len(rows)) if (sid, i) not in drop], dtype=int)
        rows = rows[keep]
        metric.update([rows[None, :, :4] + shift], [rows[None, :, 4]], [np.ones((1, len(rows)))], None, None, None, sid=sid,
                      tracks=[rows[None, :, 5] + 100])


def test_the_metric_class_equals_the_functions_called_directly():
    from viddet_amd.data import SyntheticTracks
    from viddet_amd.mot_metric import pack_clips
    ds = SyntheticTracks("synthetic", num_videos=3, frames_per_video=8, num_class=4)
    m = H.HOTAMetric(ds)
    _feed(m, ds)
    names, values = m.get()
    got = dict(zip(names, values))
    assert names == list(H.RATES) + list(H.COUNTS)
    assert all(got[k] == "1.0000" for k in H.RATES) and got["frames"] == "24" and got["GT"] == got["PRED"]
    # shifted boxes, a dropped row: the class returns what the functions return on the packed arrays
    m.reset()
    _feed(m, ds, shift=3.0, drop={(1, 0), (5, 0)})
    out = m.get()
    arrays, cs = pack_clips(ds, m._results)
    records = H.hota_match_host(*arrays, clip_start=cs, num_class=len(ds.classes))
    direct = H.hota_summary(records, arrays[2], masked_track(arrays[3], arrays[4], arrays[6], len(ds.classes)), cs)
    assert m.summary == direct and out == H.format_summary(direct["all"]) and len(direct["clips"]) == 3
    assert 0.5 < direct["all"]["HOTA"] < 1.0 and direct["all"]["LocA"] < 1.0 and direct["all"]["FN"][0] == 2
    assert m.get() == out
    m.reset()
    assert dict(zip(*m.get()))["HOTA"] == "0.0000"
    with pytest.raises(NotImplementedError, match="no clips with ground-truth tracks"):
        from viddet_amd.data import SyntheticDetection
        H.HOTAMetric(SyntheticDetection("voc", num_samples=4))


def test_value_errors():
    arrays = list(HC.closed_forms()[0][1])
    with pytest.raises(ValueError, match="hota_match_host: expected gt_boxes"):
        H.hota_match_host(arrays[0][:, :, :3], *arrays[1:])
    with pytest.raises(ValueError, match="hota_match_host: expected track"):
        H.hota_match_host(*arrays[:6], arrays[6].astype(np.float32))
    with pytest.raises(ValueError, match="1 to 128"):
        H.hota_match_host(np.zeros((4, 129, 4), np.float32), np.zeros((4, 129), np.int32), np.zeros((4, 129), np.int32), *arrays[3:])
    with pytest.raises(ValueError, match="clip_start"):
        H.hota_match_host(*arrays, clip_start=[0, 2])
    records = H.hota_match_host(*arrays)
    with pytest.raises(ValueError, match="do not fit"):
        H.hota_summary(records, arrays[2][:, :0], arrays[6])
    with pytest.raises(ValueError, match="no candidate of the track table"):
        H.hota_summary(records, arrays[2], np.full_like(arrays[6], -1))


def test_device_metric_class_needs_the_gpu_and_chunks_whole_clips(monkeypatch):
    import torch
    from viddet_amd.device_hota_metric import DeviceHOTAMetric, clip_chunks, dense_ids
    cs = [0, 4, 8, 12]
    assert clip_chunks(cs, 2, 2, [2, 2, 2], [3, 3, 3], chunk_bytes=4 * 104) == [(0, 1, 2, 3), (1, 2, 2, 3), (2, 3, 2, 3)]
    assert clip_chunks(cs, 2, 2, [2, 1, 2], [3, 5, 0], chunk_bytes=8 * 104) == [(0, 2, 2, 5), (2, 3, 2, 1)]
    assert clip_chunks(cs, 2, 2, [2, 2, 2], [3, 3, 3], chunk_bytes=1) == [(0, 1, 2, 3), (1, 2, 2, 3), (2, 3, 2, 3)]   # never split
    assert clip_chunks(cs, 2, 2, [2, 2, 2], [3, 3, 3]) == [(0, 3, 2, 3)]
    # the workspace cap: a clip needs 8 * 2 * 3 + 4 * 2 + 4 * 3 = 68 bytes
    assert clip_chunks(cs, 2, 2, [2, 2, 2], [3, 3, 3], ws_bytes=2 * 68) == [(0, 2, 2, 3), (2, 3, 2, 3)]
    with pytest.raises(ValueError, match="clip 1 holds 2 ground-truth tracks and 4 prediction tracks"):
        clip_chunks(cs, 2, 2, [2, 2, 2], [3, 4, 3], ws_bytes=68)
    table = np.array([[7, -1, 30], [30, 7, 9], [5, -1, -1], [5, 5, 1000]])
    dense, counts = dense_ids(table, [0, 2, 2, 4])
    assert dense.tolist() == [[0, -1, 2], [2, 0, 1], [0, -1, -1], [0, 0, 1]] and counts == [3, 0, 2] and dense.dtype == np.int32

    class Stub:
        classes = ["a"]
        frames_per_video = 2
        get_sample_ids = lambda self: [1, 2]
        get_label = lambda self, sid: np.zeros((0, 6))
        image_size = lambda self, sid: (100, 100)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no host fallback"):
        DeviceHOTAMetric(Stub()).get()


# ---- the library's entry points --------------------------------------------------------------------------------------------
def test_library_exports_hota_match_and_checks_its_arguments_before_any_launch():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # entry points were added, nothing changed
    assert len(L.SIGNATURES["vd_hota_match"][1]) == 22 and len(L.SIGNATURES["vd_hota_ws_bytes"][1]) == 3
    assert L.HOTA_MAX_GT_IDS == 1024 == H.MAX_GT_ID and L.HOTA_MAX_FRAMES == H.MAX_FRAMES
    assert lib.vd_hota_ws_bytes(3, 20, 30) == 3 * (8 * 20 * 30 + 4 * 20 + 4 * 30)
    for shape in ((0, 20, 30), (3, 0, 30), (3, 20, 0), (3, 1025, 30), (2 ** 20, 1024, 2 ** 30)):
        assert lib.vd_hota_ws_bytes(*shape) == -1
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    need = lib.vd_hota_ws_bytes(2, 7, 9)
    good = dict(gt_boxes=P, gt_cls=P, gt_id=P, ids=P, scores=P, bboxes=P, track=P, clip_start=P, V=2, F=6, G=20, N=30, A=7, P=9,
                num_class=3, agnostic=0, match=P, msim=P, mscore=P, ws=P, ws_bytes=need)

    def call(**kw):
        rc = lib.vd_hota_match(*dict(good, **kw).values(), None)           # `good`'s keys are in the order of the arguments
        return rc, lib.vd_last_error()

    bad = [dict(gt_boxes=None), dict(gt_cls=None), dict(gt_id=None), dict(ids=None), dict(scores=None), dict(bboxes=None),
           dict(track=None), dict(match=None), dict(msim=None), dict(mscore=None), dict(ws=None), dict(G=0), dict(G=129),
           dict(N=0), dict(N=129), dict(F=0), dict(F=(1 << 22) + 1), dict(V=0), dict(A=0), dict(A=1025), dict(P=0), dict(P=-3),
           dict(clip_start=None), dict(num_class=0), dict(agnostic=2), dict(agnostic=-1), dict(ws_bytes=need - 1), dict(ws_bytes=0),
           dict(A=8), dict(P=10), dict(V=3), dict(gt_boxes=P + 4), dict(bboxes=P + 8), dict(ws=P + 4), dict(gt_cls=P + 2),
           dict(gt_id=P + 1), dict(ids=P + 2), dict(scores=P + 1), dict(track=P + 2), dict(clip_start=P + 2), dict(match=P + 2),
           dict(msim=P + 1), dict(mscore=P + 3)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_hota_match:"), (kw, err)


def test_ops_hota_match_names_the_argument_it_refuses():
    import torch
    from viddet_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    i32 = torch.int32
    ok = [z(2, 3, 4), z(2, 3, dt=i32), z(2, 3, dt=i32), z(2, 5), z(2, 5), z(2, 5, 4), z(2, 5, dt=i32)]
    for kw, what in ((dict(num_gt_id=0, num_track=1), "num_gt_id"), (dict(num_gt_id=1025, num_track=1), "num_gt_id"),
                     (dict(num_gt_id=1, num_track=0), "num_track"), (dict(num_gt_id=1, num_track=1, num_class=0), "num_class"),
                     (dict(num_gt_id=1, num_track=1, agnostic=1), "agnostic")):
        with pytest.raises(ValueError, match="hota_match: %s" % what):
            ops.hota_match(*ok, **kw)
    with pytest.raises(ValueError, match="G=129"):
        ops.hota_match(z(2, 129, 4), *ok[1:], num_gt_id=1, num_track=1)
    with pytest.raises(ValueError, match="N=129"):
        ops.hota_match(*ok[:5], z(2, 129, 4), ok[6], num_gt_id=1, num_track=1)
    with pytest.raises(ValueError, match="gt_boxes must be a contiguous float32 device tensor"):
        ops.hota_match(*ok, num_gt_id=1, num_track=1)                        # host tensors
    with pytest.raises(ValueError, match="beyond what is taken"):
        ops.hota_ws_bytes(2 ** 20, 1024, 2 ** 30)
    assert ops.hota_ws_bytes(3, 20, 30) == 3 * (8 * 20 * 30 + 4 * 20 + 4 * 30)


# ---- the script ------------------------------------------------------------------------------------------------------------
HOTA = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--metrics", "hota"]


def test_detect_script_refuses_hota_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    with pytest.raises(NotImplementedError, match="--metrics hota needs --track"):
        D.main(HOTA + ["--stream"])
    with pytest.raises(NotImplementedError, match="--metrics hota does not combine with several --dataset names"):
        D.main(HOTA + ["--track", "--stream", "--dataset", "voc,coco"])
    with pytest.raises(NotImplementedError, match="--metrics hota does not combine with --mult_out"):
        D.main(HOTA + ["--track", "--stream", "--mult_out"])
    with pytest.raises(NotImplementedError, match="--track needs clips"):
        D.main(HOTA + ["--track"])
    with pytest.raises(NotImplementedError, match="^--device_metric acts on --metrics vid, --metrics coco, --metrics mot and --metrics hota"):
        D.main(["--random_init", "--metrics", "voc", "--device_metric"])
    with pytest.raises(NotImplementedError, match="it needs --metrics vid or --metrics mot \\(or --metrics hota"):
        D.main(["--random_init", "--metrics", "voc", "--metric_agnostic"])
    # with --track and clips it gets as far as asking for the GPU: beside other metrics, with --device_metric, agnostic
    for extra in (["--stream"], ["--synthetic_videos", "2"], ["--stream", "--metrics", "voc,coco,vid,mot,hota"], ["--stream", "--device_metric"],
                  ["--stream", "--tubelet"], ["--stream", "--track_method", "sort"], ["--stream", "--metric_agnostic"],
                  ["--stream", "--model_agnostic"]):
        with pytest.raises(SystemExit):
            D.main(HOTA + ["--track"] + extra)


def test_the_script_s_file_names_and_flags_without_hota_are_unchanged():
    import detect_yolo3 as D
    assert D.result_name("hota") == "hota" and D.result_name("hota", seq=True) == "hota_seq" and D.result_name("hota", tub=True) == "hota_tub"
    assert D.result_name("hota", True, True) == "hota_ag" and D.result_name("hota", False, True, tub=True) == "hota_ag_met_tub"
    flags = D.parse_flags([])
    assert flags.metrics == ["voc", "coco"] and not flags.device_metric and not flags.metric_agnostic and not flags.track
    assert D.parse_flags(["--metrics", "mot,hota"]).metrics == ["mot", "hota"]


def test_the_script_scores_what_is_on_disk(tmp_path):
    """save_tracks' tail without a GPU: a tracked twin written from the ground truth itself reads back to HOTA 1; beside mot the
    run returns mot's result, alone its own; without hota nothing of it is written"""
    import os
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=6)
    w, h = ds.frame_size
    boxes, tracks = {}, {}
    for idx, sid in enumerate(ds.get_sample_ids()):
        rows = ds.get_label(sid)
        boxes[ds.sample_path(idx)] = [[int(r[4]), 0.9, r[0] / w, r[1] / h, r[2] / w, r[3] / h] for r in rows]
        tracks[ds.sample_path(idx)] = [int(r[5]) + 3 for r in rows]
    FLAGS = D.parse_flags(["--metrics", "hota", "--track", "--save_dir", str(tmp_path), "--save_prefix", "p"])
    names, values = D.save_tracks(FLAGS, ds, boxes, tracks)
    got = dict(zip(names, values))
    assert got["HOTA"] == got["DetA"] == got["AssA"] == "1.0000" and float(got["LocA"]) > 0.999
    text = open(os.path.join(str(tmp_path), "p", "hota.txt")).read()
    assert text == "".join("%s %s\n" % kv for kv in zip(names, values)) and text.startswith("HOTA 1.0000\n")
    assert sorted(os.listdir(os.path.join(str(tmp_path), "p"))) == ["hota.txt", "pred_trk", "tracks.txt"]
    FLAGS = D.parse_flags(["--metrics", "mot,hota", "--track", "--save_dir", str(tmp_path), "--save_prefix", "r"])
    both = D.save_tracks(FLAGS, ds, boxes, tracks, tub=True)
    assert both[0][0] == "MOTA"
    assert sorted(os.listdir(os.path.join(str(tmp_path), "r"))) == ["hota_tub.txt", "mot_tub.txt", "pred_tub_trk", "tracks_tub.txt"]
    assert open(os.path.join(str(tmp_path), "r", "hota_tub.txt")).read() == text
    FLAGS = D.parse_flags(["--metrics", "mot", "--track", "--save_dir", str(tmp_path), "--save_prefix", "q"])
    assert D.save_tracks(FLAGS, ds, boxes, tracks)[0][0] == "MOTA"
    assert sorted(os.listdir(os.path.join(str(tmp_path), "q"))) == ["mot.txt", "pred_trk", "tracks.txt"]
