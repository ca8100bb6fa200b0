"""GPU: vd_coco_match (viddet_amd/csrc/vd_coco_eval.hip) against coco_metric.match_image integer for integer,
DeviceCOCODetectionMetric against the host metric, and detect_yolo3.py --metrics coco with and without --device_metric."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import coco_oracle as O
from viddet_amd import coco_metric as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(det, gt, K):
    """det (B,N,6), gt (B,M,8) -> rank (B,N), bits (B,N,4), npig (K,4)"""
    from viddet_amd import ops
    dev = torch.device("cuda")
    B, N = det.shape[:2]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    rank = torch.full((B, N), 0x55555555, dtype=torch.int32, device=dev)               # written whole: the fill must not survive
    bits = torch.full((B, N, 4), 0x55555555, dtype=torch.int32, device=dev)
    npig = torch.zeros((K, 4), dtype=torch.int32, device=dev)
    ops.coco_match(up(det), up(gt), up(M.IOU_THRS), up(M.AREA_RNG), rank, bits, npig)
    torch.cuda.synchronize()
    return rank.cpu().numpy(), bits.cpu().numpy(), npig.cpu().numpy()


def _check(images, K):
    """one launch over `images` padded to the widest; every image's records equal match_image's"""
    from viddet_amd.device_coco_metric import pack_images
    (det, gt), = pack_images(list(range(len(images))), images)
    rank, bits, npig = _launch(det, gt, K)
    want_npig = np.zeros((K, 4), np.int64)
    for i, (d, g) in enumerate(images):
        w_rank, w_bits, w_npig = M.match_image(d, g, K)
        n = len(d)
        assert np.array_equal(rank[i, :n], w_rank), (i, np.argwhere(rank[i, :n] != w_rank)[:5].tolist())
        assert np.array_equal(bits[i, :n], w_bits), (i, np.argwhere(bits[i, :n] != w_bits)[:5].tolist())
        assert (rank[i, n:] == -1).all() and not bits[i, n:].any()                     # padded rows
        want_npig += w_npig
    assert np.array_equal(npig, want_npig)
    return rank, bits, npig


@pytest.mark.parametrize("case", O.edge_images(), ids=lambda c: c[0])
def test_records_equal_the_host_on_the_edge_images(case):
    _, det, gt, K = case
    _check([(det, gt)], K)


def test_records_equal_the_host_in_one_padded_launch():
    """every edge image in ONE launch: each padded to the widest, so padded rows follow every list; K = 5"""
    _check([(d, g) for _, d, g, _ in O.edge_images()], 5)


@functools.lru_cache(maxsize=None)
def _big():
    return O.random_image(np.random.default_rng(4), 1024, 512, 5, pad=0.05)


def test_one_image_at_the_limits():
    det, gt = _big()
    assert det.shape == (1024, 6) and gt.shape == (512, 8)
    rank, _, _ = _check([(det, gt)], 5)
    assert (rank >= 0).sum() == 500                                                    # five categories, the first 100 each


def test_more_workgroups_than_compute_units():
    rng = np.random.default_rng(8)
    _check([O.random_image(rng, int(rng.integers(0, 20)), int(rng.integers(0, 9)), 7) for _ in range(300)], 7)


def test_two_launches_write_the_same_bytes():
    from viddet_amd.device_coco_metric import pack_images
    (det, gt), = pack_images([0, 1], [_big(), O.edge_images()[5][1:3]])
    a, b = _launch(det, gt, 5), _launch(det, gt, 5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the metric class ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 48), (480, 360)])
def test_device_metric_equals_host_metric(size):
    from viddet_amd.data import SyntheticDetection
    from viddet_amd.device_coco_metric import DeviceCOCODetectionMetric
    ds = SyntheticDetection("synthetic", num_samples=12, size=size, num_class=5)
    preds = O.seeded_predictions(ds, seed=size[0])
    host = M.COCODetectionMetric(ds, None)
    devs = [DeviceCOCODetectionMetric(ds, None), DeviceCOCODetectionMetric(ds, None, chunk_bytes=6000)]        # 12 images: three chunks
    for m in [host] + devs:
        for sid, boxes, labels, scores in preds:
            m.update([boxes[None]], [labels[None]], [scores[None]], sid=sid)
    want = host.get()
    assert 0 < host._coco_eval.stats[0] < 1
    for dev, chunks in zip(devs, (1, 3)):
        assert dev.get() == want
        assert dev.chunks == chunks and set(dev.timings) >= {"pack", "upload", "launch", "download", "accumulate"}
        for key in ("precision", "recall"):
            assert np.array_equal(dev._coco_eval.eval[key], host._coco_eval.eval[key])
        assert np.array_equal(dev._coco_eval.stats, host._coco_eval.stats)


def test_device_metric_names_the_sample_with_too_many_rows():
    from viddet_amd.device_coco_metric import DeviceCOCODetectionMetric
    ds = O.ListDataset(["a"], [[[10, 10, 60, 60, 0]], []], ids=[4, 9])
    m = DeviceCOCODetectionMetric(ds, None)
    m.update(np.tile(np.array([0., 0., 9., 9.]), (1, 1025, 1)), np.zeros((1, 1025)), np.full((1, 1025), .5), sid=9)
    with pytest.raises(ValueError, match="sample id 9 holds 1025 detections"):
        m.get()


# ---- the script ----------------------------------------------------------------------------------------------------------
def test_detect_script_writes_the_same_coco_txt_with_either_metric(tmp_path):
    """two runs as fresh child processes, each under its own time limit: host metric, then --device_metric"""
    texts = []
    for tag, extra in (("host", []), ("device", ["--device_metric"])):
        args = [sys.executable, os.path.join(ROOT, "detect_yolo3.py"), "--random_init", "--dataset", "voc", "--data_shape", "64",
                "--synthetic_samples", "8", "--batch_size", "4", "--metrics", "coco", "--save_dir", str(tmp_path),
                "--save_prefix", tag] + extra
        r = subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (tag, r.stdout[-1500:], r.stderr[-3000:])
        with open(os.path.join(str(tmp_path), tag, "coco.txt")) as f:
            texts.append(f.read())
        assert sorted(os.listdir(os.path.join(str(tmp_path), tag))) == ["coco.txt", "pred"]          # the JSON is cleaned up
    assert texts[0] == texts[1] and texts[0].startswith("~~~~ Summary metrics ~~~~") and "class19 " in texts[0]


def test_default_metrics_return_vocs_result_and_write_coco_txt(tmp_path):
    import detect_yolo3 as D
    names, values = D.main(["--random_init", "--dataset", "voc", "--data_shape", "64", "--synthetic_samples", "8", "--batch_size", "4",
                            "--save_dir", str(tmp_path), "--save_prefix", "d"])
    assert names[-1] == "mAP" and len(names) == 21 and isinstance(values[-1], float)                 # voc's tuple, as before
    with open(os.path.join(str(tmp_path), "d", "coco.txt")) as f:
        text = f.read()
    assert text.startswith("~~~~ Summary metrics ~~~~") and "class19 " in text and "~~~~ MeanAP @ IoU=[0.50,0.95] ~~~~" in text
