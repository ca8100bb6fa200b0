"""GPU: vd_vid_match (viddet_amd/csrc/vd_vid_eval.hip) against its NumPy restatement bit for bit,
DeviceVIDDetectionMetric against the host metric, and detect_yolo3.py --metrics vid with and without --device_metric."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import vid_eval_oracle as E
from viddet_amd import vid_metric as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rec_gt", "rec_tp", "rec_fp", "img_nig", "img_ngt", "npos", "nout")


def _launch(det, gt, C, iou_thresh=0.5):
    from viddet_amd import ops
    dev = torch.device("cuda")
    B, N = det.shape[:2]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    i32 = lambda *s: torch.full(s, 0x55555555, dtype=torch.int32, device=dev)           # written whole: the fill must not survive
    out = [i32(B, N), i32(B, N), i32(B, N), i32(B, 4), i32(B), torch.zeros(C, dtype=torch.int32, device=dev),
           torch.zeros((16, C), dtype=torch.int32, device=dev)]
    ops.vid_match(up(det), up(gt), up(E.MR), up(E.AR), iou_thresh, 10.0, *out)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@functools.lru_cache(maxsize=None)
def _case(B, N, M, C, one_class=False):
    det, gt = E.random_case(B, N, M, C, 0, one_class=one_class)
    return det, gt, E.match_records(det, gt, C=C)


def _check(B, N, M, C, one_class=False):
    det, gt, want = _case(B, N, M, C, one_class)
    got = _launch(det, gt, C)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), \
            (name, B, N, M, C, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())
    return det, gt, got


@pytest.mark.parametrize("M", [0, 1, 64, 65, 512])
@pytest.mark.parametrize("N", [0, 1, 63, 65, 257, 1024])
def test_records_equal_the_oracle(N, M):
    _check(3, N, M, 5)


def test_case_holds_what_the_kernel_must_decide():
    """padded rows in the middle of both lists, a NaN motion IoU, a zero-area ground truth (thr = 0), every fp code, matches,
    detections that lose their ground truth to a higher-scored one"""
    det, gt, (rec_gt, rec_tp, rec_fp, *_rest) = _case(3, 257, 65, 5)
    for a, col in ((det, 0), (gt, 4)):
        pad = a[0, :, col] < 0
        assert pad.any() and not pad.all() and (~pad[np.argmax(pad):]).any()
    valid = gt[..., 4] >= 0
    assert np.isnan(gt[..., 5][valid]).any()
    assert (V.gt_thresholds(gt[0][valid[0]]) == 0).any()
    codes = (rec_fp.view(np.uint32)[..., None] >> (2 * np.arange(16))) & 3
    assert set(np.unique(codes[rec_gt == -1])) == {0, 1, 2, 3}
    assert (rec_gt >= 0).sum() > 20 and len(np.unique(rec_tp[rec_gt >= 0])) > 3
    ov = V.overlaps(det[0, :, 2:6], gt[0, :, :4])
    ok = (ov >= V.gt_thresholds(gt[0, :, :4])) & (det[0, :, 0][:, None] == gt[0, :, 4][None]) & valid[0][None]
    assert ((rec_gt[0] == -1) & ok.any(axis=1)).any()


def test_more_workgroups_than_compute_units():
    _check(300, 65, 64, 5)


def test_one_class_all_work_on_one_wavefront():
    _check(3, 257, 65, 1, one_class=True)
    _check(3, 257, 65, 5, one_class=True)


def test_many_classes():
    _check(3, 257, 65, 37)


def test_two_launches_write_the_same_bytes():
    det, gt, _ = _case(3, 1024, 512, 5)
    a, b = _launch(det, gt, 5), _launch(det, gt, 5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the metric class ----------------------------------------------------------------------------------------------------
def _both(ds, results, agnostic, **kw):
    from viddet_amd.device_vid_metric import DeviceVIDDetectionMetric
    host, dev = V.VIDDetectionMetric(ds, agnostic=agnostic), DeviceVIDDetectionMetric(ds, agnostic=agnostic, **kw)
    host._results, dev._results = list(results), list(results)
    h, d = host.get(), dev.get()
    assert h == d and np.array_equal(host.ap, dev.ap)
    return host, dev


@pytest.mark.parametrize("agnostic", [False, True])
def test_device_metric_equals_host_metric_on_the_golden_fixture(agnostic):
    g, ds = E.load_golden()
    host, dev = _both(ds, E.golden_results(g), agnostic, chunk_bytes=1 << 16)            # several chunks
    assert np.array_equal(dev.ap, g["ap_agnostic" if agnostic else "ap"])
    assert dev.get()[1] == g["values_agnostic" if agnostic else "values"].tolist()


@pytest.mark.parametrize("agnostic", [False, True])
def test_device_metric_equals_host_metric_on_synthetic_tracks(agnostic):
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("synthetic", num_videos=3, frames_per_video=16, num_class=4)
    rng = np.random.default_rng(3)
    w, h = ds.frame_size
    rows = []
    for sid in ds.get_sample_ids():
        for r in ds.get_label(sid):
            s = np.array([r[2] - r[0] + 1, r[3] - r[1] + 1] * 2)
            for _ in range(int(rng.integers(0, 3))):
                rows.append([sid, int(r[4]) if rng.random() < 0.8 else int(rng.integers(0, 4)), 0.0]
                            + (r[:4] + rng.normal(0, 0.1, 4) * s).tolist())
        xy = rng.uniform(0, (w - 30, h - 30))
        rows.append([sid, int(rng.integers(0, 4)), 0.0] + xy.tolist() + (xy + rng.uniform(10, 200, 2)).tolist())
    for r, s in zip(rows, rng.permutation(len(rows))):
        r[2] = 0.06 + 0.9 * (s + 0.5) / len(rows)
    host, _ = _both(ds, rows, agnostic)
    assert ((host.ap > 0) & (host.ap < 1)).any()


def test_device_metric_names_the_sample_with_too_many_rows():
    from viddet_amd.device_vid_metric import DeviceVIDDetectionMetric
    ds = E.ArrayDataset([1, 2], np.zeros((0, 7)), {"1": [0.0], "2": [0.0]}, 2)
    m = DeviceVIDDetectionMetric(ds)
    m._results = [[2, 0, 0.5 + 1e-4 * i, 0, 0, 5, 5] for i in range(1025)]
    with pytest.raises(ValueError, match="sample id 2 holds 1025 detections"):
        m.get()


# ---- the script ----------------------------------------------------------------------------------------------------------
def test_detect_script_writes_the_same_vid_txt_with_either_metric(tmp_path):
    """two runs as fresh child processes, each under its own time limit: host metric, then --device_metric"""
    texts = []
    for tag, extra in (("host", []), ("device", ["--device_metric"])):
        args = [sys.executable, os.path.join(ROOT, "detect_yolo3.py"), "--random_init", "--metrics", "vid", "--data_shape", "64",
                "--synthetic_videos", "2", "--synthetic_samples", "8", "--batch_size", "4", "--save_dir", str(tmp_path),
                "--save_prefix", tag, "--dataset", "voc"] + extra
        r = subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (tag, r.stdout[-1500:], r.stderr[-3000:])
        with open(os.path.join(str(tmp_path), tag, "vid.txt")) as f:
            texts.append(f.read())
    assert texts[0] == texts[1] and texts[0].startswith("~~~~ Summary metrics ~~~~") and "class19 " in texts[0]
