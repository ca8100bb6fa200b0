"""CPU: the COCO detection metric (viddet_amd/coco_metric.py) against the literal loop form of the same algorithm
(tests/coco_oracle.py), closed-form cases with hand-derived numbers, the wrapper's behaviour, the flags, and the packing of the
device path."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import coco_oracle as O
from viddet_amd import coco_metric as M
from viddet_amd.data import SyntheticCombined, SyntheticDetection, SyntheticTracks, SyntheticVideo

AP3 = (51 + 50 * 2 / 3) / 101           # tp, fp, tp over two ground truths: precision 1 up to recall .5, 2/3 beyond


def _feed(metric, preds):
    for sid, boxes, labels, scores in preds:
        metric.update([boxes[None]], [labels[None]], [scores[None]], sid=sid)
    return metric


def _run(classes, labels, dets, **kw):
    """labels: per image rows x1,y1,x2,y2,cls; dets: per image rows x1,y1,x2,y2,cls,score (xyxy, as the network gives them)"""
    ds = O.ListDataset(classes, labels, **kw)
    m = M.COCODetectionMetric(ds, None)
    for sid, d in zip(ds.sample_ids, dets):
        d = np.asarray(d, dtype=np.float64).reshape(-1, 6)
        m.update([d[None, :, :4]], [d[None, :, 4]], [d[None, :, 5]], sid=sid)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        names, values = m.get()
    return m, names, values


# ---- against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 48), (480, 360)])
def test_metric_equals_the_loop_oracle(size):
    ds = SyntheticDetection("synthetic", num_samples=12, size=size, num_class=5)
    preds = O.seeded_predictions(ds, seed=size[0])
    scores = np.concatenate([p[3] for p in preds])
    assert len(np.unique(scores)) < len(scores) // 3                                   # duplicated scores
    m = _feed(M.COCODetectionMetric(ds, None), preds)
    names, values = m.get()
    ev = O.run(M.coco_ground_truth(ds), m._results)
    assert (names, values) == O.get_strings(ev, ds.classes)
    e = m._coco_eval
    assert e.eval['precision'].shape == (10, 101, 5, 4, 3) and e.eval['recall'].shape == (10, 5, 4, 3) and e.stats.shape == (12,)
    assert np.array_equal(e.eval['precision'], ev.eval['precision']) and np.array_equal(e.eval['recall'], ev.eval['recall'])
    assert np.array_equal(e.stats, ev.stats)
    assert 0 < e.stats[0] < 1 and 0 < e.stats[8] < 1


def test_ground_truth_is_build_coco_json_as_written(tmp_path):
    ds = SyntheticDetection("synthetic", num_samples=3, num_class=4)
    gt = M.coco_ground_truth(ds)
    rows = [r for i in range(3) for r in ds[i][1]]
    assert [a['id'] for a in gt['annotations']] == list(range(len(rows)))              # the first annotation has id 0
    for a, r in zip(gt['annotations'], rows):
        w, h = int(r[2]) - int(r[0]), int(r[3]) - int(r[1])                            # no +1 on this side
        assert a['bbox'] == [int(r[0]), int(r[1]), w, h] and a['area'] == int(w * h) and a['iscrowd'] == 0
        assert a['category_id'] == int(r[4])
    assert [im['id'] for im in gt['images']] == [0, 1, 2] and gt['images'][0]['width'] == 480 and gt['images'][0]['height'] == 360
    assert [c['id'] for c in gt['categories']] == [0, 1, 2, 3]
    path = M.COCODetectionMetric(ds, None).build_coco_json(str(tmp_path / "gt" / "gt.json"))
    with open(path) as f:
        assert json.load(f) == gt


def test_datasets_carry_what_the_metric_reads():
    a = SyntheticDetection("synthetic", num_samples=5, size=(64, 48))
    assert a.sample_ids == [0, 1, 2, 3, 4] and a.image_size(3) == (64, 48) and a.frame_size == (64, 48)
    v = SyntheticVideo("synthetic", num_videos=2, frames_per_video=3)
    assert v.sample_ids == list(range(6)) and v.image_size(0) == v.frame_size == (480, 360)
    t = SyntheticTracks("synthetic", num_videos=2, frames_per_video=3)
    assert t.sample_ids == t.get_sample_ids() == [1, 2, 3, 4, 5, 6] and t.image_size(1) == t.frame_size
    c = SyntheticCombined(["voc", "coco"], num_samples=4, classes_per_set=2)
    assert c.sample_ids == [0, 1, 2, 3] and c.image_size(0) == (480, 360)
    gt = M.coco_ground_truth(t)                                                        # labels by get_label(sid), ids 1-based
    assert [im['id'] for im in gt['images']] == t.sample_ids
    assert sum(len(t.get_label(s)) for s in t.sample_ids) == len(gt['annotations'])


# ---- closed-form cases -----------------------------------------------------------------------------------------------------
THROW = [300, 300, 340, 340, 1]          # the set's first annotation (id 0), of another category, so that no relevant id is 0


def _three(side):
    """two side x side ground truths; detections exactly on the first (.9), disjoint (.8), exactly on the second (.7)"""
    s = side
    labels = [[THROW, [10, 10, 10 + s, 10 + s, 0], [100, 100, 100 + s, 100 + s, 0]]]
    dets = [[[10, 10, 10 + s, 10 + s, 0, .9], [200, 200, 200 + s, 200 + s, 0, .8], [100, 100, 100 + s, 100 + s, 0, .7]]]
    return _run(["a", "b"], labels, dets)


def test_three_detections_two_ground_truths_50px():
    m, names, values = _three(50)
    e = m._coco_eval
    d, g = e.images[0]
    assert M.bbox_iou(d[0, :4], g[1, :4], [0])[0, 0] == 2500 / 2601                    # the +1 of the detection side
    p, r = e.eval['precision'], e.eval['recall']
    assert np.abs(p[:, :, 0, 0, 2].mean(axis=1) - AP3).max() < 1e-12 and abs(AP3 - 0.834983) < 1e-6
    assert np.array_equal(r[:, 0, 0, 2], np.ones(10))
    # category b holds the throw-away ground truth and no detection: precision 0, recall 0 - so the mean over both halves
    assert not p[:, :, 1, 0, 2].any() and not r[:, 1, 0, 2].any()
    assert abs(e.stats[0] - AP3 / 2) < 1e-12 and abs(e.stats[8] - 0.5) < 1e-12
    assert values[0].split("\n")[0] == "Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.417"
    assert values[0].split("\n")[8] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500"
    assert names[1:3] == ["a", "b"] and values[1:] == ["83.5", "0.0", "41.7"]
    assert names[0] == '~~~~ Summary metrics ~~~~\n' and names[-1] == '~~~~ MeanAP @ IoU=[0.50,0.95] ~~~~\n'


def test_three_detections_two_ground_truths_16px_lose_the_two_highest_thresholds():
    m, _, _ = _three(16)
    e = m._coco_eval
    d, g = e.images[0]
    assert M.bbox_iou(d[0, :4], g[1, :4], [0])[0, 0] == 256 / 289                      # 0.8858: below 0.90 and 0.95 only
    p, r = e.eval['precision'], e.eval['recall']
    for a in (0, 1):                                                                   # all, small
        ap = p[:, :, 0, a, 2].mean(axis=1)
        assert np.abs(ap[:8] - AP3).max() < 1e-12 and not ap[8:].any()
        assert np.array_equal(r[:, 0, a, 2], [1.0] * 8 + [0.0] * 2)
    assert (p[:, :, 0, 2:, :] == -1).all() and (r[:, 0, 2:, :] == -1).all()            # no medium or large ground truth


def test_three_detections_area_cells_50px():
    e = _three(50)[0]._coco_eval
    p = e.eval['precision']
    assert np.abs(p[:, :, 0, 2, 2].mean(axis=1) - AP3).max() < 1e-12                   # 2500 and 2601 are medium
    assert (p[:, :, 0, 1, :] == -1).all() and (p[:, :, 0, 3, :] == -1).all()


def test_the_first_annotation_of_the_set_is_never_a_true_positive():
    m, _, values = _run(["a"], [[[10, 10, 60, 60, 0]]], [[[10, 10, 60, 60, 0, .9]]])
    e = m._coco_eval
    assert e.images[0][1][0, 6] == 0                                                   # annotation id 0
    rank, bits, npig = e.records
    assert bits[0].tolist() == [[0, 0x3ff << 10, 0, 0x3ff << 10]] and npig.tolist() == [[1, 0, 1, 0]]   # unmatched; ignored only outside its area
    assert not e.eval['precision'][:, :, 0, 0, 2].any() and not e.eval['recall'][:, 0, 0, 2].any()     # a false positive
    assert values[1:] == ["0.0", "0.0"]
    # the same ground truth as the set's second annotation is found
    m, _, values = _run(["a", "b"], [[THROW, [10, 10, 60, 60, 0]]], [[[10, 10, 60, 60, 0, .9]]])
    e = m._coco_eval
    # (in `small` and `large` its ground truth is ignored by area: the detection takes it all the same, and is ignored with it)
    assert e.records[1][0].tolist() == [[0x3ff, 0xfffff, 0x3ff, 0xfffff]]
    assert np.abs(e.eval['precision'][:, :, 0, 0, 2] - 1).max() < 1e-12 and np.array_equal(e.eval['recall'][:, 0, 0, 2], np.ones(10))


def test_area_boundaries_are_inclusive():
    gt = np.array([[0, 0, 32, 32, 1024, 0, 5, 0], [0, 50, 96, 96, 9216, 0, 6, 0]], dtype=np.float64)
    _, _, npig = M.match_image(np.zeros((0, 6)), gt, 1)
    assert npig.tolist() == [[2, 1, 2, 1]]                                             # 1024: small and medium; 9216: medium and large
    det = np.array([[0, 0, 32, 32, .9, 0]], dtype=np.float64)                          # its own area 1024: inside small and medium
    _, bits, _ = M.match_image(det, gt, 1)
    assert bits.tolist() == [[0x3ff, 0x3ff, 0x3ff, 0xfffff]]                           # large: it takes the ignored one and is ignored with it
    m, _, _ = _run(["a", "b"], [[THROW, [0, 0, 32, 32, 0]]], [[]])
    r = m._coco_eval.eval['recall']
    assert (r[:, 0, 0:3, :] == 0).all() and (r[:, 0, 3, :] == -1).all()


def test_a_crowd_is_matched_by_several_detections_and_never_counted():
    gt = {'images': [{'id': 7, 'width': 640, 'height': 480, 'file_name': 'x'}],
          'categories': [{'id': 0, 'name': 'a'}],
          'annotations': [{'image_id': 7, 'id': 0, 'bbox': [500, 400, 10, 10], 'area': 100, 'category_id': 0, 'iscrowd': 0},
                          {'image_id': 7, 'id': 1, 'bbox': [0, 0, 100, 100], 'area': 10000, 'category_id': 0, 'iscrowd': 1},
                          {'image_id': 7, 'id': 2, 'bbox': [200, 200, 40, 40], 'area': 1600, 'category_id': 0, 'iscrowd': 0}]}
    res = [{'image_id': 7, 'category_id': 0, 'bbox': [10, 10, 20, 20], 'score': .9},
           {'image_id': 7, 'category_id': 0, 'bbox': [50, 50, 30, 30], 'score': .8},
           {'image_id': 7, 'category_id': 0, 'bbox': [200, 200, 40, 40], 'score': .7}]
    e = M.COCOEval(gt, res)
    e.evaluate(), e.accumulate()
    rank, bits, npig = e.records
    assert npig.tolist() == [[2, 1, 1, 0]]                                             # the crowd is in no range's count
    assert rank[0].tolist() == [0, 1, 2]
    assert bits[0][:, 0].tolist() == [0x3ff | 0x3ff << 10, 0x3ff | 0x3ff << 10, 0x3ff]  # both inside the crowd: matched and ignored
    ev = O.run(gt, res)
    assert np.array_equal(e.eval['precision'], ev.eval['precision']) and np.array_equal(e.eval['recall'], ev.eval['recall'])
    # the two ignored detections are neither true nor false positives: precision 1 up to the recall reached, 1 of 2
    p = e.eval['precision'][:, :, 0, 0, 2]
    assert np.abs(p[:, :51] - 1).max() < 1e-12 and not p[:, 51:].any() and (e.eval['recall'][:, 0, 0, 2] == 0.5).all()


def test_equal_ious_take_the_later_ground_truth():
    # the same box twice, as the set's annotations 0 and 1: taking the earlier would read as unmatched (id 0)
    m, _, _ = _run(["a"], [[[10, 10, 60, 60, 0], [10, 10, 60, 60, 0]]], [[[10, 10, 60, 60, 0, .9]]])
    assert m._coco_eval.records[1][0][0, 0] == 0x3ff
    # ... and a second detection is left with annotation 0
    m, _, _ = _run(["a"], [[[10, 10, 60, 60, 0], [10, 10, 60, 60, 0]]], [[[10, 10, 60, 60, 0, .9], [10, 10, 60, 60, 0, .8]]])
    assert m._coco_eval.records[1][0][:, 0].tolist() == [0x3ff, 0]


def test_an_iou_exactly_at_the_threshold_matches():
    m, _, _ = _run(["a", "b"], [[THROW, [0, 0, 10, 20, 0]]], [[[0, 0, 9, 9, 0, .9]]])  # 10x10 inside 10x20: 100 / 200
    e = m._coco_eval
    d, g = e.images[0]
    assert M.bbox_iou(d[:, :4], g[1:, :4], [0])[0, 0] == 0.5 == e.iouThrs[0]
    assert e.records[1][0][0, 0] == 1                                                  # matched at 0.50 only, never ignored in `all`


def test_max_dets_130_detections_of_one_category():
    grid = [[40 * (i % 10), 40 * (i // 10), 40 * (i % 10) + 20, 40 * (i // 10) + 20, 0] for i in range(20)]
    junk = lambda j: [600 + (j % 10), 200 + 2 * j, 610 + (j % 10), 210 + 2 * j, 0]
    on = {**{r: r for r in range(5)}, **{50 + r: 5 + r for r in range(5)}, **{110 + r: 10 + r for r in range(20 - 10)}}
    dets = [(grid[on[r]][:4] if r in on else junk(r)[:4]) + [0, 0.99 - 0.005 * r] for r in range(130)]
    order = np.random.default_rng(0).permutation(130)
    m, _, _ = _run(["a", "b"], [[THROW] + grid], [[dets[i] for i in order]], size=(800, 600))
    e = m._coco_eval
    rank = e.records[0][0]
    assert np.array_equal(rank, np.where(order < 100, order, -1))                      # only the top 100 take part
    assert not e.records[1][0][rank < 0].any()
    r = e.eval['recall'][0, 0, 0]                                                      # IoU 0.50, category a, all areas
    assert r.tolist() == [1 / 20, 5 / 20, 10 / 20]                                     # the first 1, 10, 100 detections
    assert abs(e.stats[6] - 0.9 * 0.05 / 2) < 1e-12                                    # 400 / 441: lost at 0.95; b: recall 0


# ---- the wrapper -----------------------------------------------------------------------------------------------------------
def test_a_category_without_ground_truth_prints_nan():
    _, names, values = _run(["a", "b", "c"], [[THROW, [10, 10, 60, 60, 0]]], [[[10, 10, 60, 60, 0, .9]]])
    assert names[1:4] == ["a", "b", "c"] and values[1:4] == ["100.0", "0.0", "nan"] and values[4] == "50.0"


def test_empty_results_give_the_dummy_row_and_an_empty_dataset_gives_map_0():
    ds = O.ListDataset(["a"], [[[10, 10, 60, 60, 0]], []], ids=[5, 3])
    m = M.COCODetectionMetric(ds, None)
    with pytest.warns(UserWarning, match="Recorded 0 out of 2 validation images"):
        names, values = m.get()
    assert m._results == [{'image_id': 3, 'category_id': 0, 'bbox': [0, 0, 0, 0], 'score': 0}]          # img_ids are sorted
    assert values[1:] == ["0.0", "0.0"]
    assert M.COCODetectionMetric(O.ListDataset(["a"], []), None).get() == (['mAP'], ['0.0'])


def test_score_thresh_label_filter_and_data_shape():
    ds = O.ListDataset(["a", "b"], [[[10, 10, 60, 60, 0]]], size=(640, 480))
    m = M.COCODetectionMetric(ds, None, score_thresh=0.3, data_shape=(240, 320))
    boxes = np.array([[[5., 10., 30., 40.], [1., 2., 3., 4.], [0., 0., 9., 9.]]])
    m.update(boxes, np.array([[1., -1., 0.]]), np.array([[.5, .9, .29]]))
    assert m._results == [{'image_id': 0, 'category_id': 1, 'bbox': [10.0, 20.0, 51.0, 61.0], 'score': 0.5}]   # x2 both ways, then +1
    assert boxes[0, 0].tolist() == [5., 10., 30., 40.]                                 # the caller's array is not written
    with pytest.raises(ValueError, match="data_shape"):
        M.COCODetectionMetric(ds, None, data_shape=416)


def test_sid_files_the_image_under_the_given_id_against_the_counter():
    ds = O.ListDataset(["a"], [[], [], []], ids=[10, 20, 30])
    box, lab, sc = np.array([[[0., 0., 9., 9.]]]), np.array([[0.]]), np.array([[.9]])
    m = M.COCODetectionMetric(ds, None)
    m.update(box, lab, sc, sid=30), m.update(box, lab, sc, sid=np.int64(20))
    assert [r['image_id'] for r in m._results] == [30, 20] and type(m._results[1]['image_id']) is int
    m = M.COCODetectionMetric(ds, None)
    m.update(box, lab, sc), m.update(box, lab, sc)                                     # the reference's counter
    assert [r['image_id'] for r in m._results] == [10, 20]
    m.reset()
    assert m._results == [] and m._current_id == 0


def test_the_json_is_written_and_removed_by_cleanup(tmp_path):
    ds = O.ListDataset(["a", "b"], [[THROW, [10, 10, 60, 60, 0]]])
    m = M.COCODetectionMetric(ds, str(tmp_path / "res"), use_time=False, cleanup=True)
    path = str(tmp_path / "res.json")
    assert m._filename == path and os.path.exists(path)
    m.update(np.array([[[10., 10., 60., 60.]]]), np.array([[0.]]), np.array([[.9]]), sid=0)
    m.get()
    with open(path) as f:
        assert json.load(f) == [{'image_id': 0, 'category_id': 0, 'bbox': [10.0, 10.0, 51.0, 51.0], 'score': 0.9}]
    del m
    assert not os.path.exists(path)
    keep = M.COCODetectionMetric(ds, str(tmp_path / "kept"), use_time=True)
    assert keep._filename.startswith(str(tmp_path / "kept_2")) and os.path.exists(keep._filename)
    name = keep._filename
    del keep
    assert os.path.exists(name)
    assert M.COCODetectionMetric(ds, None)._filename is None and os.listdir(str(tmp_path)) == [os.path.basename(name)]


def test_results_of_an_unknown_image_are_refused():
    ds = O.ListDataset(["a"], [[[10, 10, 60, 60, 0]]])
    m = M.COCODetectionMetric(ds, None)
    m.update(np.array([[[10., 10., 60., 60.]]]), np.array([[0.]]), np.array([[.9]]), sid=99)
    with pytest.raises(ValueError, match="do not correspond"):
        m.get()


# ---- flags and the script's glue -------------------------------------------------------------------------------------------
def _flags(argv):
    import detect_yolo3 as D
    F = D.parse_flags(argv)
    F.window = [int(s) for s in F.window]
    return D, F


def test_flag_checks():
    D, F = _flags(["--device_metric", "--metrics", "coco"])
    D.check_flags(F)
    D, F = _flags(["--device_metric", "--metrics", "voc,coco"])
    D.check_flags(F)
    D, F = _flags(["--device_metric", "--metrics", "voc"])
    with pytest.raises(NotImplementedError, match="^--device_metric acts on --metrics vid"):
        D.check_flags(F)
    F = D.parse_flags([])
    assert F.metrics == ["voc", "coco"] and F.device_metric is False
    assert D.result_name("coco") == "coco" and D.result_name("coco", True, True) == "coco_ag"
    assert "COCO metric are out of scope" not in D.__doc__ and "--metrics coco" in D.__doc__


def test_evaluate_by_sample_id_unnormalises_to_the_source_frame():
    import detect_yolo3
    assert detect_yolo3.evaluate_vid is detect_yolo3.evaluate_by_sample_id
    import detect_yolo3 as D
    ds = SyntheticDetection("synthetic", num_samples=3)
    w, h = ds.frame_size
    m = M.COCODetectionMetric(ds, None)
    m.get = lambda: (["n"], ["v"])
    preds = {ds.sample_path(2): [[3, 0.7, 0.25, 0.5, 0.75, 1.0], [1, 0.01, 0, 0, 1, 1]], ds.sample_path(0): [[2, 0.9, 0.1, 0.1, 0.2, 0.2]]}
    assert D.evaluate_by_sample_id(m, ds, preds) == (["n"], ["v"])
    x1, y1, x2, y2 = 0.1 * w, 0.1 * h, 0.2 * w, 0.2 * h
    assert m._results == [{'image_id': 0, 'category_id': 2, 'bbox': [x1, y1, x2 - (x1 - 1), y2 - (y1 - 1)], 'score': 0.9},
                          {'image_id': 2, 'category_id': 3, 'bbox': [0.25 * w, 0.5 * h, 0.75 * w - (0.25 * w - 1), h - (0.5 * h - 1)],
                           'score': 0.7}]


# ---- the device path's host halves -----------------------------------------------------------------------------------------
def _images(n_images=7, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_images):
        n, m = int(rng.integers(0, 9)), int(rng.integers(0, 5))
        det, gt = rng.uniform(0, 50, (n, 6)), rng.uniform(0, 50, (m, 8))
        det[:, 5], gt[:, 5] = rng.integers(0, 3, n), rng.integers(0, 3, m)
        out.append((det, gt))
    return out


def test_pack_images_chunks_and_pads():
    from viddet_amd.device_coco_metric import pack_images, unpack_records
    images = _images()
    ids = list(range(100, 100 + len(images)))
    one = pack_images(ids, images)
    assert len(one) == 1 and one[0][0].shape == (7, max(len(d) for d, _ in images), 6) and one[0][1].shape[2] == 8
    chunks = pack_images(ids, images, chunk_bytes=2 * (8 * 6 + 4 * 8) * 8)
    assert len(chunks) >= 3 and sum(c[0].shape[0] for c in chunks) == len(images)
    i = 0
    for det, gt in chunks:
        assert det.shape[0] * (det.shape[1] * 6 + gt.shape[1] * 8) * 8 <= 2 * (8 * 6 + 4 * 8) * 8 or det.shape[0] == 1
        for j in range(det.shape[0]):
            n, m = len(images[i][0]), len(images[i][1])
            assert np.array_equal(det[j, :n], images[i][0]) and np.array_equal(gt[j, :m], images[i][1])
            assert (det[j, n:, 5] == -1).all() and (gt[j, m:, 5] == -1).all() and not det[j, n:, :5].any()
            i += 1
    assert len(pack_images(ids, images, chunk_bytes=1)) == len(images)                  # one image is always taken
    assert pack_images([], []) == []
    # the records of the chunks, padded rows dropped, are the host's per-image records
    K = 3
    want = [M.match_image(d, g, K) for d, g in images]
    raw = [sum(w[2] for w in want).reshape(-1)]
    for det, gt in chunks:
        recs = [M.match_image(det[j], gt[j], K) for j in range(det.shape[0])]
        raw += [np.stack([r[0] for r in recs]).reshape(-1), np.stack([r[1] for r in recs]).reshape(-1)]
    ranks, bits, npig = unpack_records(chunks, images, np.concatenate(raw).astype(np.int32), K)
    assert all(np.array_equal(r, w[0]) and np.array_equal(b, w[1]) for r, b, w in zip(ranks, bits, want))
    assert np.array_equal(npig, sum(w[2] for w in want))


def test_pack_images_names_the_sample_with_too_many_rows():
    from viddet_amd.device_coco_metric import pack_images
    images = [(np.zeros((3, 6)), np.zeros((2, 8))), (np.zeros((1025, 6)), np.zeros((0, 8)))]
    with pytest.raises(ValueError, match="sample id 41 holds 1025 detections"):
        pack_images([40, 41], images)
    images = [(np.zeros((3, 6)), np.zeros((513, 8))), (np.zeros((1024, 6)), np.zeros((512, 8)))]
    with pytest.raises(ValueError, match="sample id 40 holds 513 label rows"):
        pack_images([40, 41], images)
    assert len(pack_images([41], images[1:])) == 1


def test_library_entry_point_refuses_bad_arguments():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == L.ABI_VERSION                                       # an entry point was only added
    p = L.ptr(torch.zeros(64, dtype=torch.float64))
    q = L.ptr(torch.zeros(64, dtype=torch.int32))

    def call(B=1, N=1, M=1, K=4, det=p, gt=p, thr=p, rng=p, rank=q, bits=q, npig=q):
        return lib.vd_coco_match(det, B, N, gt, M, thr, rng, rank, bits, npig, K, None)

    for kw, text in ((dict(N=1025), b"N=1025"), (dict(M=513), b"M=513"), (dict(K=0), b"K=0"), (dict(K=40000), b"K=40000"),
                     (dict(B=-1), b"B, N, M"), (dict(det=None), b"det"), (dict(gt=None), b"gt"), (dict(thr=None), b"iou_thrs"),
                     (dict(rng=None), b"area_rng"), (dict(rank=None), b"rec_rank"), (dict(bits=None), b"rec_bits"),
                     (dict(npig=None), b"npig")):
        assert call(**kw) != 0, kw
        err = lib.vd_last_error()
        assert err.startswith(b"vd_coco_match:") and text in err, (kw, err)
    assert call(B=0, N=7, M=3) == 0                                                    # no image: nothing is launched
    assert (L.COCO_MATCH_MAX_DET, L.COCO_MATCH_MAX_GT) == (1024, 512)


def test_ops_coco_match_names_the_argument_before_the_launch():
    from viddet_amd import ops
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(ValueError, match="det holds N=1025"):
        ops.coco_match(z(1, 1025, 6), z(1, 1, 8), z(10), z(4, 2), i(1, 1025), i(1, 1025, 4), i(3, 4))
    with pytest.raises(ValueError, match="gt holds M=513"):
        ops.coco_match(z(1, 1, 6), z(1, 513, 8), z(10), z(4, 2), i(1, 1), i(1, 1, 4), i(3, 4))
    with pytest.raises(ValueError, match="gt must be"):
        ops.coco_match(z(1, 1, 6), z(1, 1, 6), z(10), z(4, 2), i(1, 1), i(1, 1, 4), i(3, 4))
    with pytest.raises(ValueError, match="det must be a contiguous"):
        ops.coco_match(z(1, 1, 6), z(1, 1, 8), z(10), z(4, 2), i(1, 1), i(1, 1, 4), i(3, 4))       # host tensors


# ---- the per-image records, on the images the GPU tests launch ----------------------------------------------------------------
@pytest.mark.parametrize("case", O.edge_images(), ids=lambda c: c[0])
def test_match_image_equals_the_loop_oracle_on_the_edge_images(case):
    _, det, gt, K = case
    for got, want in zip(M.match_image(det, gt, K), O.records(det, gt, K)):
        assert got.dtype == np.int64 and np.array_equal(got, want)


def test_edge_images_hold_what_they_are_named_for():
    cases = {name: (d, g, K) for name, d, g, K in O.edge_images()}
    d, g, K = cases["padded rows"]
    for a in (d, g):
        pad = a[:, 5] < 0
        assert pad.any() and not pad.all() and (~pad[np.argmax(pad):]).any()           # padded rows in the middle
    d, g, K = cases["130 detections of one category"]
    rank, bits, _ = M.match_image(d, g, K)
    assert (d[:, 5] == 0).all() and (rank >= 0).sum() == 100 and not bits[rank < 0].any()
    d, g, K = cases["a tile larger than the staging buffer"]
    assert max(min((d[:, 5] == k).sum(), 100) * (g[:, 5] == k).sum() for k in range(K)) > 768
    d, g, K = cases["five categories: 0 and 4 share a wavefront"]
    assert {0, 4} <= set(d[:, 5]) and len(np.unique(d[:, 4])) < len(d) // 4 and g[:, 7].any()     # tied scores, crowds
    assert any((g[i, :4] == g[j, :4]).all() for i in range(len(g)) for j in range(i))                # tied IoUs
    assert {1024.0, 9216.0} <= set(g[:, 4])                                                          # area boundaries
    assert cases["annotation id 0"][1][0, 6] == 0
    d, g, K = cases["by hand"]
    rank, bits, npig = M.match_image(d, g, K)
    assert bits[:2, 0].tolist() == [0x3ff, 0]                  # equal IoUs: the later ground truth (id 1); the next is left with id 0
    assert bits[2, 0] == 1                                     # IoU exactly 0.5: matched at the first threshold only
    assert bits[3, 0] == bits[4, 0] == 0xfffff                 # the crowd, taken twice, ignored
    assert npig.tolist() == [[2, 0, 2, 0], [1, 1, 0, 0], [2, 1, 2, 1]] and rank.tolist() == [0, 1, 0, 1, 2, 0, 1, -1]
