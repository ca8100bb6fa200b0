"""CPU: the ImageNet VID motion metric (viddet_amd/vid_metric.py) against the reference's own outputs
(tests/golden/vid_golden.npz, written by tests/golden/make_vid_golden.py from metrics/imgnetvid.py), the record format of
vd_vid_match restated in NumPy (tests/vid_eval_oracle.py) through DeviceVIDDetectionMetric's host half, SyntheticTracks,
the C entry point's argument checks and the flags."""
import numpy as np
import pytest
import torch

from tests import vid_eval_oracle as E
from viddet_amd import vid_metric as V
from viddet_amd.data import SyntheticTracks, SyntheticVideo
from viddet_amd.device_vid_metric import DeviceVIDDetectionMetric, ap_from_records, pack_images


@pytest.fixture(scope="module")
def golden():
    return E.load_golden()


def _host(ds, results, agnostic=False):
    m = V.VIDDetectionMetric(ds, agnostic=agnostic)
    m._results = list(results)
    return m, m.get()


def _via_records(ds, results, C, agnostic=False, chunk_bytes=1 << 16):
    """the oracle's records -> AP through the device metric's host half"""
    chunks, all_motion = pack_images(ds, results, agnostic, chunk_bytes)
    recs = [E.match_records(det, gt, C=C) for det, gt in chunks]
    return ap_from_records(chunks, [r[:5] for r in recs], sum(r[5] for r in recs), sum(r[6] for r in recs), all_motion, E.MR, C), chunks


# ---- the golden fixture: the reference's own outputs ---------------------------------------------------------------------------
def test_golden_fixture_meets_its_conditions(golden):
    """scores pairwise distinct; every cell has a class with 0 < AP < 1; every fp rule, a matched detection outside its
    cell, a detection that loses its ground truth to a higher-scored one and a match below IoU 0.5 on a small ground truth"""
    g, ds = golden
    C = int(g["num_class"])
    assert len(np.unique(g["dets"][:, 2])) == len(g["dets"])
    assert ((g["ap"] > 0) & (g["ap"] < 1)).any(axis=2).all()
    (det, gt), = pack_images(ds, E.golden_results(g), chunk_bytes=1 << 40)[0]
    rec_gt, rec_tp, rec_fp, _, img_ngt, _, _ = E.match_records(det, gt, C=C)
    codes = (rec_fp.view(np.uint32)[..., None] >> (2 * np.arange(16))) & 3
    unmatched, matched = rec_gt == -1, rec_gt >= 0
    with_gt = unmatched & (img_ngt[:, None] > 0)
    assert (codes[with_gt] == 1).any() and (codes[with_gt] == 3).any()
    assert (codes[with_gt][:, [4, 8, 12]] == 0).any()                         # by ovmax_ig > ovmax_nig: these cells have no area gate
    assert (codes[unmatched & (img_ngt[:, None] == 0)] == 2).any()            # detections on a frame without ground truth
    assert (matched & (rec_tp.view(np.uint32) != 0xffff)).any()               # matched, but outside some cell
    assert (g["thr"] < 0.5).any()
    lost = small = False
    for b in range(det.shape[0]):
        gv = gt[b, :, 4] >= 0
        if gv.any():
            ov = V.overlaps(det[b, :, 2:6], gt[b, :, :4])
            ok = (ov >= V.gt_thresholds(gt[b, :, :4])) & (det[b, :, 0][:, None] == gt[b, :, 4][None]) & gv[None]
            lost |= bool((unmatched[b] & ok.any(axis=1)).any())
            small |= bool((ov[np.nonzero(matched[b])[0], rec_gt[b][matched[b]]] < 0.5).any())
    assert lost and small


def test_box_overlap_thresholds_and_vid_ap_equal_the_reference(golden):
    g, ds = golden
    got = np.array([float(V.box_overlap(p[:4], p[4:])) for p in g["pairs"]])
    assert np.array_equal(got, g["pair_iou"]) and (got > 0).sum() > 50 and (got == 0).sum() > 10
    assert np.array_equal(np.diag(V.overlaps(g["pairs"][:, :4], g["pairs"][:, 4:])), g["pair_iou"])
    thr = np.concatenate([V.gt_thresholds(ds.get_label(s)) for s in ds.get_sample_ids()])
    assert np.array_equal(thr, g["thr"])
    for i in range(3):
        assert V.vid_ap(g["ap_rec%d" % i], g["ap_prec%d" % i]) == g["ap_out%d" % i]


def test_motion_ious_of_the_fixture_are_the_functions(golden):
    g, ds = golden
    ids = ds.get_sample_ids()
    T = 24
    for v in range(len(ids) // T):
        clip = [ds.get_label(s) for s in ids[v * T:(v + 1) * T]]
        for s, m in zip(ids[v * T:(v + 1) * T], V.motion_ious(clip)):
            assert np.array_equal(np.asarray(m), np.asarray(ds.motion_ious[str(s)]), equal_nan=True)


@pytest.mark.parametrize("agnostic", [False, True])
def test_host_metric_equals_the_reference(golden, agnostic):
    g, ds = golden
    key = "_agnostic" if agnostic else ""
    m, (names, values) = _host(ds, E.golden_results(g), agnostic)
    assert np.array_equal(m.ap, g["ap" + key])                                # -1 entries included
    assert names == g["names" + key].tolist() and values == g["values" + key].tolist()


def test_update_filters_rows_as_the_reference_does(golden):
    g, ds = golden
    res = E.golden_results(g)
    a = V.VIDDetectionMetric(ds)
    rows = np.array([r for r in res if r[0] == res[0][0]])
    pad = np.array([[-1.0, 0.9, 0, 0, 5, 5], [1.0, 0.01, 0, 0, 5, 5]])      # no class; below the score threshold
    lab, sc, bb = np.concatenate([rows[:, 1], pad[:, 0]]), np.concatenate([rows[:, 2], pad[:, 1]]), np.concatenate([rows[:, 3:], pad[:, 2:]])
    a.update([bb[None]], [lab[None]], [sc[None]], None, None, None, sid=res[0][0])
    assert a._results == [r for r in res if r[0] == res[0][0]]
    a.reset()
    assert a.get() == (["mAP"], ["0.0"])


def test_calculate_ap_concatenates_in_image_order_skipping_none():
    tp = [None, np.array([1.0, 0.0]), None, np.array([1.0])]
    fp = [None, np.array([0.0, 1.0]), None, np.array([0.0])]
    lab = [None, np.array([0, 0]), None, np.array([0])]
    conf = [None, np.array([0.9, 0.2]), None, np.array([0.5])]
    ap = V.calculate_ap(tp, fp, [3, 2, 1], lab, conf, ["a", "b"], np.array([2.0, 0.0]))
    assert ap.tolist() == [1.0, -1.0]


# ---- motion_ious on hand-made clips -------------------------------------------------------------------------------------------
def test_motion_ious_by_hand():
    box = [10.0, 10.0, 50.0, 40.0]
    still = [np.array([box + [0.0, 3.0]]) for _ in range(5)]
    assert V.motion_ious(still) == [[1.0]] * 5
    once = [np.zeros((0, 6)), np.array([box + [1.0, 0.0]]), np.zeros((0, 6))]
    out = V.motion_ious(once)
    assert out[0] == [0.0] and out[2] == [0.0] and len(out[1]) == 1 and np.isnan(out[1][0])
    # the window is +-10 frames, cut at the clip's ends: a box that jumps away at frame 12 is seen from frame 2 on
    far = [200.0, 200.0, 240.0, 230.0]
    clip = [np.array([(box if t < 12 else far) + [0.0, 0.0]]) for t in range(14)]
    out = V.motion_ious(clip)
    assert out[0] == [1.0] and out[1] == [1.0]                                # frames 1..10 / 0,2..11 only
    assert out[2] == [11.0 / 12.0]                                            # frames 0..12 without 2: twelve, one of them away
    assert out[13] == [1.0 / 10.0]                                            # frames 3..12: only frame 12 is where it is
    untracked = [np.array([box + [0.0, -1.0]])]
    assert V.motion_ious(untracked) == [[0.0]]


# ---- the kernel's record format, restated: records -> AP equals the host metric -------------------------------------------------
@pytest.mark.parametrize("agnostic", [False, True])
def test_records_through_the_device_half_equal_the_host_metric_on_the_fixture(golden, agnostic):
    g, ds = golden
    res = E.golden_results(g)
    m, _ = _host(ds, res, agnostic)
    ap, chunks = _via_records(ds, res, 1 if agnostic else int(g["num_class"]), agnostic)
    assert len(chunks) > 1 and np.array_equal(ap, m.ap) and np.array_equal(ap, g["ap_agnostic" if agnostic else "ap"])


@pytest.mark.parametrize("B,N,M,C,one", [(3, 63, 65, 5, False), (4, 257, 64, 37, False), (3, 1, 1, 1, False), (3, 5, 0, 3, False),
                                         (2, 40, 30, 4, True)])
def test_records_through_the_device_half_equal_the_host_metric_on_random_sets(B, N, M, C, one):
    det, gt = E.random_case(B, N, M, C, 1, one_class=one)
    ds, res = E.dataset_from_case(det, gt, C)
    m, _ = _host(ds, res)
    ap, _ = _via_records(ds, res, C)
    assert np.array_equal(ap, m.ap)


def test_pack_images_names_the_sample_that_is_too_large():
    ds = E.ArrayDataset([1, 2], np.zeros((0, 7)), {"1": [0.0], "2": [0.0]}, 2)
    rows = [[2, 0, 0.5 + 1e-4 * i, 0, 0, 5, 5] for i in range(1025)]
    with pytest.raises(ValueError, match="sample id 2 holds 1025 detections"):
        pack_images(ds, rows)
    lab = np.array([[1, 0, 0, 5, 5, 0, i] for i in range(513)], np.float64)
    ds = E.ArrayDataset([1, 2], lab, {"1": [1.0] * 513, "2": [0.0]}, 2)
    with pytest.raises(ValueError, match="sample id 1 holds 513 label rows"):
        pack_images(ds, rows[:3])


# ---- SyntheticTracks ---------------------------------------------------------------------------------------------------------
def test_synthetic_tracks():
    a = SyntheticTracks("synthetic", num_videos=4, frames_per_video=24, window=3, step=1)
    b = SyntheticTracks("synthetic", num_videos=4, frames_per_video=24, window=3, step=1)
    ids = a.get_sample_ids()
    assert ids == list(range(1, 97)) and all(isinstance(i, int) for i in ids)
    assert all(np.array_equal(a.get_label(s), b.get_label(s)) for s in ids) and a.motion_ious == b.motion_ious
    assert a.motion_ious is a.motion_ious                                    # computed once
    mi = np.concatenate([np.asarray(a.motion_ious[str(s)]) for s in ids if len(a.get_label(s))])
    assert (mi < 0.7).any() and ((mi >= 0.7) & (mi <= 0.9)).any() and (mi > 0.9).any()
    assert a.wn_classes == a.classes and len(a.classes) == 20
    per_clip = [len(np.unique(np.concatenate([a.get_label(s)[:, 5] for s in ids[v * 24:(v + 1) * 24]]))) for v in range(4)]
    assert all(2 <= n <= 5 for n in per_clip)
    w, h = a.frame_size
    for s in ids:
        lab = a.get_label(s)
        assert lab.shape[1] == 6 and len(a.motion_ious[str(s)]) == max(1, len(lab))
        assert (lab[:, 0] >= 0).all() and (lab[:, 1] >= 0).all() and (lab[:, 2] <= w - 1).all() and (lab[:, 3] <= h - 1).all()
        assert (lab[:, 2] > lab[:, 0]).all() and (lab[:, 3] > lab[:, 1]).all()
    # the SyntheticVideo sample contract: the same pixels and windows, (n,6) labels whose column 5 is the `difficult` zero
    base = SyntheticVideo("synthetic", num_videos=4, frames_per_video=24, window=3, step=1)
    img, lab = a[30]
    assert np.array_equal(img, base[30][0]) and img.shape == (3, h, w, 3) and img.dtype == np.uint8
    assert np.array_equal(lab[:, :5], a.get_label(31)[:, :5]) and not lab[:, 5].any()
    assert np.array_equal(a.video_frames(2), base.video_frames(2)) and a.sample_path(30) == base.sample_path(30)


# ---- the library's argument checks, without a GPU ------------------------------------------------------------------------------
def test_library_entry_point_refuses_bad_arguments():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == L.ABI_VERSION                                       # an entry point was only added
    p = L.ptr(torch.zeros(64, dtype=torch.float64))
    q = L.ptr(torch.zeros(64, dtype=torch.int32))

    def call(B=1, N=1, M=1, C=4, det=p, gt=p, mr=p, ar=p, rec=q, npos=q, nout=q, img=q):
        return lib.vd_vid_match(det, B, N, gt, M, mr, ar, 0.5, 10.0, rec, rec, rec, img, img, npos, nout, C, None)

    for kw, text in ((dict(N=1025), b"N=1025"), (dict(M=513), b"M=513"), (dict(C=0), b"C=0"), (dict(B=-1), b"B, N, M"),
                     (dict(det=None), b"det"), (dict(gt=None), b"gt"), (dict(mr=None), b"motion_ranges"),
                     (dict(ar=None), b"area_ranges"), (dict(rec=None), b"rec_gt"), (dict(npos=None), b"npos"),
                     (dict(nout=None), b"nout"), (dict(img=None), b"img_nig")):
        assert call(**kw) != 0, kw
        err = lib.vd_last_error()
        assert err.startswith(b"vd_vid_match:") and text in err, (kw, err)
    assert call(B=0, N=7, M=3) == 0                                                    # no image: nothing is launched
    assert (L.VID_MATCH_MAX_DET, L.VID_MATCH_MAX_GT) == (1024, 512)


def test_ops_vid_match_names_the_argument_before_the_launch():
    from viddet_amd import ops
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(ValueError, match="det holds N=1025"):
        ops.vid_match(z(1, 1025, 6), z(1, 1, 6), z(4, 2), z(4, 2), 0.5, 10.0, i(1, 1025), i(1, 1025), i(1, 1025), i(1, 4), i(1), i(3), i(16, 3))
    with pytest.raises(ValueError, match="gt holds M=513"):
        ops.vid_match(z(1, 1, 6), z(1, 513, 6), z(4, 2), z(4, 2), 0.5, 10.0, i(1, 1), i(1, 1), i(1, 1), i(1, 4), i(1), i(3), i(16, 3))
    with pytest.raises(ValueError, match="det must be"):
        ops.vid_match(z(1, 1, 5), z(1, 1, 6), z(4, 2), z(4, 2), 0.5, 10.0, i(1, 1), i(1, 1), i(1, 1), i(1, 4), i(1), i(3), i(16, 3))


# ---- flags ----------------------------------------------------------------------------------------------------------------
def _flags(argv):
    import detect_yolo3 as D
    F = D.parse_flags(argv)
    F.window = [int(s) for s in F.window]
    return D, F


def test_flag_checks():
    D, F = _flags(["--metric_agnostic", "--metrics", "voc"])
    with pytest.raises(NotImplementedError, match="--metric_agnostic without --model_agnostic"):
        D.check_flags(F)
    D, F = _flags(["--metric_agnostic", "--metrics", "vid"])
    D.check_flags(F)
    assert F.metric_agnostic and not F.model_agnostic and D.result_name("vid", F.model_agnostic, F.metric_agnostic) == "vid_ag_met"
    assert D.result_name("vid", True, True) == "vid_ag" and D.result_name("vid") == "vid" and D.result_name("voc", True) == "voc_ag"
    D, F = _flags(["--metrics", "vid", "--dataset", "voc,coco"])
    with pytest.raises(NotImplementedError, match="--metrics vid does not combine with several --dataset"):
        D.check_flags(F)
    D, F = _flags(["--device_metric", "--metrics", "voc"])
    with pytest.raises(NotImplementedError, match="--device_metric acts on --metrics vid"):
        D.check_flags(F)
    assert D.parse_flags([]).device_metric is False and D.parse_flags([]).metrics == ["voc", "coco"]


def test_class_map_and_offset_raise(golden):
    _, ds = golden
    for cls in (V.VIDDetectionMetric, DeviceVIDDetectionMetric):
        with pytest.raises(NotImplementedError, match="class_map"):
            cls(ds, class_map=[0, 1, 2])
        with pytest.raises(NotImplementedError, match="offset"):
            cls(ds, offset=1)
        cls(ds, offset=0), cls(ds, offset=None)
    with pytest.raises(NotImplementedError, match="class_map"):
        V.vid_eval_motion(ds, [], V.MOTION_RANGES, V.AREA_RANGES, class_map=[0])


def test_evaluate_vid_unnormalises_to_the_source_frame():
    import detect_yolo3 as D
    ds = SyntheticTracks("synthetic", num_videos=1, frames_per_video=4)
    w, h = ds.frame_size
    m = V.VIDDetectionMetric(ds)
    m.get = lambda: (["n"], ["v"])
    preds = {ds.sample_path(2): [[3, 0.7, 0.25, 0.5, 0.75, 1.0], [1, 0.01, 0, 0, 1, 1], [0, 0.3, 0.0, 0.0, 0.5, 0.5]],
             ds.sample_path(0): [[2, 0.9, 0.1, 0.1, 0.2, 0.2]]}
    assert D.evaluate_vid(m, ds, preds) == (["n"], ["v"])
    assert m._results == [[1, 2, 0.9, 0.1 * w, 0.1 * h, 0.2 * w, 0.2 * h], [3, 3, 0.7, 0.25 * w, 0.5 * h, 0.75 * w, 1.0 * h],
                          [3, 0, 0.3, 0.0, 0.0, 0.5 * w, 0.5 * h]]
