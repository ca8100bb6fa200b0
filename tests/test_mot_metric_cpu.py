"""CPU: the MOT tracking metric's definition (viddet_amd/mot_metric.py): assign_host against brute force and
against scipy, mot_match_host and mot_summary against the loop form of tests/mot_oracle.py on random clips, closed forms whose
outputs are written out by hand (tests/mot_cases.py), the metric class, the argument checks of vd_mot_match and the refusals of
detect_yolo3.py --metrics mot, none of which touches a GPU."""
import functools

import numpy as np
import pytest

from tests import mot_cases as MC
from tests import mot_oracle as MO
from viddet_amd import mot_metric as M


# ---- the assignment --------------------------------------------------------------------------------------------------------
def _random_matrix(rng, k):
    R = int(rng.integers(1, 7))
    C = int(rng.integers(R, 8))
    if k % 3 == 0:
        cost = rng.choice(np.array([0, 5, 9], np.int64), (R, C))             # forced ties: three levels
    else:
        cost = rng.integers(-40, 60, (R, C)).astype(np.int64)
    if k % 2:
        cost[rng.random((R, C)) < 0.3] = M.FORBIDDEN
    return cost


def test_assign_host_equals_brute_force_on_200_small_matrices():
    rng = np.random.default_rng(2024)
    refused = tied = 0
    for k in range(200):
        cost = _random_matrix(rng, k)
        as_lists = [[None if c == M.FORBIDDEN else int(c) for c in row] for row in cost]
        best = MO.brute_assign(as_lists)
        if best is None:
            refused += 1
            with pytest.raises(ValueError, match="cannot be assigned"):
                M.assign_host(cost)
            with pytest.raises(ValueError):
                MO.assign_loops(as_lists)
            continue
        col = M.assign_host(cost)
        assert len(set(col.tolist())) == len(col) and (col >= 0).all() and (col < cost.shape[1]).all()
        assert int(cost[np.arange(len(col)), col].sum()) == best, k
        assert col.tolist() == MO.assign_loops(as_lists), k                   # the same assignment, not only the same value
        tied += k % 3 == 0
    assert refused >= 1 and tied > 50


def test_assign_host_equals_scipy_on_values():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(7)
    for k in range(50):
        R = int(rng.integers(1, 41))
        C = int(rng.integers(R, 61))
        cost = rng.integers(0, 1000 if k % 2 else 4, (R, C)).astype(np.int64)
        col = M.assign_host(cost)
        r, c = opt.linear_sum_assignment(cost)
        assert int(cost[np.arange(R), col].sum()) == int(cost[r, c].sum()), k


def test_assign_host_refuses_what_it_cannot_take():
    with pytest.raises(ValueError, match="integer matrix"):
        M.assign_host(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="integer matrix"):
        M.assign_host(np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="2\\*\\*40"):
        M.assign_host(np.full((1, 1), 1 << 41, np.int64))
    with pytest.raises(ValueError, match="row 2 cannot"):
        M.assign_host(np.zeros((3, 2), np.int64))
    assert M.assign_host(np.zeros((0, 3), np.int64)).shape == (0,)


# ---- the matching and the summary against the loop form -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cases():
    return MO.random_cases()


def _same(arrays, seen=None, **kw):
    got = M.mot_match_host(*arrays, **kw)
    want = MO.match_oracle(*arrays, seen=seen, **kw)
    for name, g, w in zip(("match", "miou", "flags", "adm"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name
    assert [g.dtype for g in got] == [np.int32, np.float32, np.int32, np.uint32]
    trk = M.masked_track(arrays[3], arrays[4], arrays[6], kw.get("num_class"))
    s, o = M.mot_summary(got, arrays[2], trk, kw.get("clip_start")), MO.summary_oracle(want, arrays[2], trk, kw.get("clip_start"))
    assert s == o                                                            # every figure, per clip and overall
    return got, s


def test_host_equals_the_loop_form_on_random_clips_which_hold_every_event():
    seen, frag, names = {}, 0, set()
    for name, arrays, kw in _cases():
        _, s = _same(arrays, seen, **kw)
        frag += s["all"]["Frag"]
        names.add(name.rsplit("_", 2)[0])
        assert len(s["clips"]) == (4 if "clip_start" in kw else 1)
    assert names == {"%dx%dx%d" % c for c in MO.SHAPES} | {"clips"}
    print(seen, frag)
    assert seen["carry"] > 0 and seen["assign22"] > 0 and seen["switch"] > 0 and frag > 0
    assert seen["gt_unmatched"] > 0 and seen["pred_unmatched"] > 0 and seen["brute"] > 0


@pytest.mark.parametrize("k", range(len(MO.tie_cases())), ids=[c[0] for c in MO.tie_cases()])
def test_host_equals_the_loop_form_where_equal_costs_abound(k):
    name, arrays, kw = MO.tie_cases()[k]
    seen = {}
    got, s = _same(arrays, seen, **kw)
    assert seen["assign22"] > 0 and s["all"]["TP"] > 0 and (seen["brute"] > 0) == (arrays[0].shape[1] <= 7)
    iou = [M.iou_matrix(arrays[0][t], arrays[5][t]) for t in range(len(arrays[0]))]
    assert all((i == 1).sum(axis=1).max() >= 2 for i in iou)                # a row with several exact hits in every frame: ties


def test_the_matching_does_not_read_the_rows_masked_track_blanks():
    _, arrays, kw = [c for c in _cases() if c[0] == "5x64x65_age7_cls"][0]
    arrays = [a.copy() for a in arrays]
    arrays[3][0, :5] = 7                                                     # a class beyond num_class: no candidates, track ids kept
    masked = list(arrays)
    masked[6] = M.masked_track(arrays[3], arrays[4], arrays[6], kw["num_class"])
    assert (masked[6] != arrays[6]).any()
    for a, b in zip(M.mot_match_host(*arrays, **kw), M.mot_match_host(*masked, **kw)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name,arrays,kw,expect", MC.closed_forms(), ids=[c[0] for c in MC.closed_forms()])
def test_closed_forms(name, arrays, kw, expect):
    got, s = _same(arrays, **kw)
    MC.check_expected(got, s, expect)


def test_arguments_are_checked_by_name():
    arrays = list(MC.build([[(MC.A, 0, 0)]], [[(MC.A, 0, 0.9, 0)]]))
    for thr in (0.0, -0.1, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="iou_thresh"):
            M.mot_match_host(*arrays, iou_thresh=thr)
    M.mot_match_host(*arrays, iou_thresh=1.0)
    bad = list(arrays)
    bad[6] = arrays[6].astype(np.float32)
    with pytest.raises(ValueError, match="track"):
        M.mot_match_host(*bad)
    bad = list(arrays)
    bad[1] = arrays[1][:, :0]
    with pytest.raises(ValueError, match="gt_cls"):
        M.mot_match_host(*bad)
    z = np.zeros((1, 129, 4), np.float32)
    with pytest.raises(ValueError, match="1 to 128"):
        M.mot_match_host(z, np.zeros((1, 129), np.int32), np.zeros((1, 129), np.int32), *arrays[3:])
    with pytest.raises(ValueError, match="clip_start"):
        M.mot_match_host(*arrays, clip_start=[0, 2])
    with pytest.raises(ValueError, match="do not fit"):
        M.mot_summary(M.mot_match_host(*arrays), arrays[2][:, :0], arrays[6])


# ---- the metric class ------------------------------------------------------------------------------------------------------
def _feed_ground_truth(metric, ds, drop=()):
    for sid in ds.get_sample_ids():
        rows = ds.get_label(sid)
        keep = np.array([i for i in range(len(rows)) if (sid, i) not in drop], dtype=int)
        rows = rows[keep]
        metric.update([rows[None, :, :4]], [rows[None, :, 4]], [np.ones((1, len(rows)))], None, None, None, sid=sid,
                      tracks=[rows[None, :, 5] + 100])


def test_the_ground_truth_fed_back_scores_one():
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("synthetic", num_videos=3, frames_per_video=12, num_class=4)
    m = M.MOTMetric(ds)
    _feed_ground_truth(m, ds)
    names, values = m.get()
    got = dict(zip(names, values))
    assert names == list(M.RATES) + list(M.COUNTS)
    assert got["MOTA"] == got["IDF1"] == got["MOTP"] == got["precision"] == got["recall"] == "1.0000"
    assert got["FN"] == got["FP"] == got["IDSW"] == got["Frag"] == "0" and got["frames"] == "36" and int(got["GT"]) > 36
    assert got["GT"] == got["PRED"] == got["TP"] == got["IDTP"] and got["MT"] == got["gt_tracks"]
    assert len(m.summary["clips"]) == 3 and all(c["MOTA"] == 1.0 for c in m.summary["clips"])
    # an image without a saved row is a frame without predictions: its ground truth counts as FN
    m.reset()
    first = len(ds.get_label(1))
    _feed_ground_truth(m, ds, drop={(1, i) for i in range(first)})
    got2 = dict(zip(*m.get()))
    assert int(got2["FN"]) == first and got2["GT"] == got["GT"] and int(got2["PRED"]) == int(got["PRED"]) - first
    assert m.get() == m.get()
    m.reset()
    assert dict(zip(*m.get()))["MOTA"] == "0.0000" and dict(zip(*m.get()))["FN"] == got["GT"]


class _Stub:
    """a set of one clip of two frames whose label rows the test chooses"""
    classes = ["a", "b"]
    frames_per_video = 2

    def __init__(self, labels):
        self.labels = labels

    def get_sample_ids(self):
        return [1, 2]

    def get_label(self, sid):
        return np.asarray(self.labels[sid - 1], dtype=np.float64).reshape(-1, 6)

    def image_size(self, sid):
        return 100, 100


def test_the_metric_names_the_sample_it_cannot_take():
    row = [0, 0, 10, 10, 0, 3]
    m = M.MOTMetric(_Stub([[row], [row]]))
    m.update([np.zeros((1, 129, 4))], [np.zeros((1, 129))], [np.ones((1, 129))], sid=2, tracks=[np.arange(129)[None]])
    with pytest.raises(ValueError, match="sample id 2 holds 129 prediction rows"):
        m.get()
    with pytest.raises(ValueError, match="sample id 1 holds 129 label rows"):
        M.MOTMetric(_Stub([[row[:5] + [i] for i in range(129)], [row]])).get()
    for bad in (1024, -1):
        with pytest.raises(ValueError, match="sample id 2 holds the ground-truth track id %d" % bad):
            M.MOTMetric(_Stub([[row], [row[:5] + [bad]]])).get()
    with pytest.raises(ValueError, match="sample id 2 holds a ground-truth track id that is no integer"):
        M.MOTMetric(_Stub([[row], [row[:5] + [1.5]]])).get()
    m = M.MOTMetric(_Stub([[row], [row]]))
    m.update([np.zeros((1, 1, 4))], [np.zeros((1, 1))], [np.ones((1, 1))], sid=1, tracks=[np.array([[2.5]])])
    with pytest.raises(ValueError, match="sample id 1 holds a track id that is no integer"):
        m.get()
    with pytest.raises(ValueError, match="tracks is missing"):
        m.update([np.zeros((1, 1, 4))], [np.zeros((1, 1))], [np.ones((1, 1))], sid=1)
    with pytest.raises(ValueError, match="iou_thresh"):
        M.MOTMetric(_Stub([[row], [row]]), iou_thresh=0.0)
    # 128 rows of either are taken
    m = M.MOTMetric(_Stub([[row[:5] + [i] for i in range(128)], [row]]))
    m.update([np.zeros((1, 128, 4))], [np.zeros((1, 128))], [np.ones((1, 128))], sid=2, tracks=[np.arange(128)[None]])
    assert dict(zip(*m.get()))["GT"] == "129"


def test_the_metric_refuses_sets_without_clips_and_window_sample_ids():
    from viddet_amd.data import SyntheticCombined, SyntheticDetection
    for ds in (SyntheticCombined(["voc", "coco"], num_samples=4), SyntheticDetection("voc", num_samples=4)):
        with pytest.raises(NotImplementedError, match="no clips with ground-truth tracks"):
            M.MOTMetric(ds)
    windows = _Stub([[], []])
    windows.get_sample_ids = lambda: [[1, 2], [2, 3]]
    with pytest.raises(NotImplementedError, match="--mult_out"):
        M.MOTMetric(windows)
    m = M.MOTMetric(_Stub([[], []]))
    with pytest.raises(NotImplementedError, match="one integer sample id"):
        m.update([np.zeros((1, 1, 4))], [np.zeros((1, 1))], [np.ones((1, 1))], sid=[1, 2], tracks=[np.zeros((1, 1))])


def test_device_metric_class_needs_the_gpu_and_chunks_whole_clips(monkeypatch):
    import torch
    from viddet_amd.device_mot_metric import DeviceMOTMetric, clip_chunks
    assert clip_chunks([0, 4, 8, 12], 2, 2, chunk_bytes=4 * 104) == [(0, 1), (1, 2), (2, 3)]
    assert clip_chunks([0, 4, 8, 12], 2, 2, chunk_bytes=8 * 104) == [(0, 2), (2, 3)]
    assert clip_chunks([0, 4, 8, 12], 2, 2, chunk_bytes=1) == [(0, 1), (1, 2), (2, 3)]      # a clip is never split
    assert clip_chunks([0, 4, 8, 12], 2, 2) == [(0, 3)]
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no host fallback"):
        DeviceMOTMetric(_Stub([[], []])).get()


# ---- the library's entry points --------------------------------------------------------------------------------------------
def test_library_exports_mot_match_and_checks_its_arguments_before_any_launch():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # entry points were added, nothing changed
    assert len(L.SIGNATURES["vd_mot_match"][1]) == 22 and len(L.SIGNATURES["vd_mot_match_ws_bytes"][1]) == 3
    assert L.MOT_MAX_ROWS == 128 == L.TRACK_MAX_ROWS and M.MAX_ROWS == 128
    assert lib.vd_mot_match_ws_bytes(6, 20, 30) == L.MOT_WS_PER_ROW * 6 * 50
    for shape in ((0, 20, 30), (6, 0, 30), (6, 20, 0), (6, 129, 30), (6, 20, 129)):
        assert lib.vd_mot_match_ws_bytes(*shape) == -1
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    need = lib.vd_mot_match_ws_bytes(6, 20, 30)
    good = dict(gt_boxes=P, gt_cls=P, gt_id=P, ids=P, scores=P, bboxes=P, track=P, clip_start=P, V=2, F=6, G=20, N=30, num_class=3,
                iou_thresh=0.5, agnostic=0, match=P, miou=P, flags=P, adm=P, ws=P, ws_bytes=need)

    def call(**kw):
        rc = lib.vd_mot_match(*dict(good, **kw).values(), None)            # `good`'s keys are in the order of the arguments
        return rc, lib.vd_last_error()

    bad = [dict(gt_boxes=None), dict(gt_cls=None), dict(gt_id=None), dict(ids=None), dict(scores=None), dict(bboxes=None),
           dict(track=None), dict(match=None), dict(miou=None), dict(flags=None), dict(adm=None), dict(ws=None), dict(G=0), dict(G=129),
           dict(N=0), dict(N=129), dict(F=0), dict(V=0), dict(clip_start=None), dict(num_class=0), dict(iou_thresh=0.0),
           dict(iou_thresh=-0.5), dict(iou_thresh=1.5), dict(iou_thresh=float("nan")), dict(agnostic=2), dict(agnostic=-1),
           dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(gt_boxes=P + 4), dict(bboxes=P + 8), dict(adm=P + 4), dict(ws=P + 2),
           dict(gt_cls=P + 2), dict(gt_id=P + 1), dict(ids=P + 2), dict(scores=P + 1), dict(track=P + 2), dict(clip_start=P + 2),
           dict(match=P + 2), dict(miou=P + 1), dict(flags=P + 3)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_mot_match:"), (kw, err)


# ---- the script ------------------------------------------------------------------------------------------------------------
MOT = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--metrics", "mot"]


def test_detect_script_refuses_mot_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    with pytest.raises(NotImplementedError, match="--metrics mot needs --track"):
        D.main(MOT + ["--stream"])
    with pytest.raises(NotImplementedError, match="--metrics mot does not combine with several --dataset names"):
        D.main(MOT + ["--track", "--stream", "--dataset", "voc,coco"])
    with pytest.raises(NotImplementedError, match="--metrics mot does not combine with --mult_out"):
        D.main(MOT + ["--track", "--stream", "--mult_out"])
    with pytest.raises(NotImplementedError, match="--track needs clips"):
        D.main(MOT + ["--track"])
    with pytest.raises(NotImplementedError, match="^--device_metric acts on --metrics vid"):
        D.main(["--random_init", "--metrics", "voc", "--device_metric"])
    with pytest.raises(NotImplementedError, match="--metric_agnostic without --model_agnostic"):
        D.main(["--random_init", "--metrics", "voc", "--metric_agnostic"])
    # with --track and clips it gets as far as asking for the GPU: beside other metrics, with --device_metric, agnostic
    for extra in (["--stream"], ["--synthetic_videos", "2"], ["--stream", "--metrics", "voc,coco,vid,mot"], ["--stream", "--device_metric"],
                  ["--stream", "--tubelet"], ["--stream", "--live"], ["--stream", "--metric_agnostic"], ["--stream", "--model_agnostic"]):
        with pytest.raises(SystemExit):
            D.main(MOT + ["--track"] + extra)


def test_the_script_s_dataset_and_file_names_with_mot():
    import detect_yolo3 as D
    assert D.result_name("mot") == "mot" and D.result_name("mot", seq=True) == "mot_seq" and D.result_name("mot", tub=True) == "mot_tub"
    assert D.result_name("mot", True, True) == "mot_ag" and D.result_name("mot", True, True, tub=True) == "mot_ag_tub"
    assert D.result_name("mot", False, True) == "mot_ag_met"
    assert D.parse_flags([]).metrics == ["voc", "coco"]                     # the default stays: a run without mot is as it was


def test_the_script_scores_what_is_on_disk(tmp_path):
    """save_tracks' tail without a GPU: a tracked twin written from the ground truth itself reads back to MOTA 1"""
    import os
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=6)
    FLAGS = D.parse_flags(["--metrics", "mot", "--track", "--save_dir", str(tmp_path), "--save_prefix", "p"])
    w, h = ds.frame_size
    boxes, tracks = {}, {}
    for idx, sid in enumerate(ds.get_sample_ids()):
        rows = ds.get_label(sid)
        boxes[ds.sample_path(idx)] = [[int(r[4]), 0.9, r[0] / w, r[1] / h, r[2] / w, r[3] / h] for r in rows]
        tracks[ds.sample_path(idx)] = [int(r[5]) + 3 for r in rows]
    names, values = D.save_tracks(FLAGS, ds, boxes, tracks)
    got = dict(zip(names, values))
    assert got["MOTA"] == "1.0000" and got["IDF1"] == "1.0000" and float(got["MOTP"]) > 0.999
    text = open(os.path.join(str(tmp_path), "p", "mot.txt")).read()
    assert text == "".join("%s %s\n" % kv for kv in zip(names, values)) and text.startswith("MOTA 1.0000\n")
    assert sorted(os.listdir(os.path.join(str(tmp_path), "p"))) == ["mot.txt", "pred_trk", "tracks.txt"]
    # without mot among the metrics nothing of it is written
    FLAGS = D.parse_flags(["--track", "--save_dir", str(tmp_path), "--save_prefix", "q"])
    assert D.save_tracks(FLAGS, ds, boxes, tracks) is None
    assert sorted(os.listdir(os.path.join(str(tmp_path), "q"))) == ["pred_trk", "tracks.txt"]
