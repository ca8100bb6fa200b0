"""GPU: vd_yolo_targets and the paths that use it.

Kernel: against viddet_amd.targets.prefetch_targets on outputs pre-filled with NaN (an unwritten element shows).  The rule, for
every comparison of this file: objectness, centre, weight and class targets are bit-equal; scale targets are within one fp32
ulp - the device's fp64 log and the host's may differ in the last fp64 bit, which survives the cast to fp32 only on a rounding
boundary.  Each test prints how many scale elements are not bit-equal.

Paths: targets_on_device on loader batches against the host loader's columns (same rule), one training step on either set of
tensors, and train_yolov3.py --device_targets end to end in child processes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from viddet_amd import ops
from viddet_amd.data import (FeatureDataset, Loader, MixupDetection, SyntheticDetection, YOLO3NBVideoTrainTransform,
                             YOLO3VideoTrainTransform)
from viddet_amd.device_targets import num_rows, targets_on_device
from viddet_amd.targets import prefetch_targets
from viddet_amd.video import Rng

pytestmark = pytest.mark.gpu

NAMES = ("obj", "ctr", "scl", "wgt", "cls")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_kernel(gt, ids, mix, C, H, W):
    """gt (N,M,4), ids (N,M,1) or (N,M,C), mix (N,M) or None -> the five outputs as NumPy arrays, written into NaN"""
    gt, ids = np.ascontiguousarray(gt, np.float32), np.ascontiguousarray(ids, np.float32)
    N, M, idw = ids.shape
    P = num_rows(H, W)
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    out = [torch.full((N, P, c), float("nan"), dtype=torch.float32, device="cuda") for c in (1, 2, 2, 2, C)]
    ops.yolo_targets(d(gt), d(ids), idw, d(mix), N, M, C, H, W, *out)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def host(gt, ids, mix, C, H, W):
    return prefetch_targets(H, W, np.asarray(gt, np.float32), np.asarray(ids), C, None if mix is None else np.asarray(mix)[..., None])


def compare(got, want, what=""):
    """the rule of this file; returns the number of scale elements that are not bit-equal"""
    for name, g, w in zip(NAMES, got, want):
        g = np.asarray(g, np.float32)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert not np.isnan(g).any(), "%s %s: %d elements were not written" % (what, name, int(np.isnan(g).sum()))
        if name != "scl":
            bad = np.argwhere(_bits(g) != _bits(w))
            assert bad.size == 0, (what, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    g, w = np.asarray(got[2], np.float32), want[2]
    off = _bits(g) != _bits(w)
    assert np.all(np.abs(g - w) <= np.spacing(np.abs(w))), (what, "scl", g[off][:4], w[off][:4])
    print("%s: %d of %d scale elements not bit-equal" % (what, int(off.sum()), off.size))
    return int(off.sum())


def random_labels(rng, N, M, C, H, W, full=False):
    """`synthetic_batch`-style boxes with sizes scaled to the input (2 px .. 0.9 of the side: every layer's anchors are
    matched at 64 px), a random number of valid rows per image, the rest padded with -1"""
    c = rng.uniform(0.05, 0.95, (N, M, 2)) * (W, H)
    wh = rng.uniform(2, 0.9 * min(H, W), (N, M, 2)) * rng.choice([0.15, 1.0], (N, M, 1))
    gt = np.concatenate([np.clip(c - wh / 2, 0, (W - 1, H - 1)), np.clip(c + wh / 2, 0, (W - 1, H - 1))], axis=-1).astype(np.float32)
    ids = rng.integers(0, C, (N, M, 1)).astype(np.float32)
    for n in range(N):
        k = M if full or n == 0 else int(rng.integers(0, M + 1))
        gt[n, k:], ids[n, k:] = -1, -1
    return gt, ids


# ---- shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 8, 70, 300])
@pytest.mark.parametrize("C", [1, 3, 20, 285])
def test_kernel_matches_prefetch_targets_over_shapes(C, M):
    """64x64 (grids 2, 4, 8; P = 252) and 64x96 (P = 378: with C = 3 and N = 1 or 3 N*P*C is no multiple of 4), N in {1, 3};
    C = 285 is a class row longer than a workgroup, M = 70 more than a wave, M = 300 more than a workgroup.  At M = 70 and 300
    many gts share a row of the 252."""
    rng = np.random.default_rng(1000 * C + M)
    for H, W in ((64, 64), (64, 96)):
        for N in (1, 3):
            gt, ids = random_labels(rng, N, M, C, H, W)
            compare(run_kernel(gt, ids, None, C, H, W), host(gt, ids, None, C, H, W), "%dx%d N=%d C=%d M=%d" % (H, W, N, C, M))


@pytest.mark.parametrize("seed", range(16))
def test_kernel_matches_prefetch_targets_on_random_boxes(seed):
    rng = np.random.default_rng(seed)
    H, W = ((64, 64), (64, 96), (96, 64), (128, 128))[seed % 4]
    N, M, C = 1 + seed % 3, (5, 8, 33, 100)[seed // 4], (3, 7, 20, 80)[seed % 4]
    gt, ids = random_labels(rng, N, M, C, H, W)
    mix = rng.uniform(0, 1, (N, M)).astype(np.float32) if seed % 2 else None
    compare(run_kernel(gt, ids, mix, C, H, W), host(gt, ids, mix, C, H, W), "seed %d" % seed)


# ---- forced cases ---------------------------------------------------------------------------------------------------------
PAD = [-1., -1., -1., -1.]
BOX16 = [24., 24., 40., 40.]                  # 16x16: anchor (16,30) = stride 8, a = 1; centre (32,32) = a cell border


def _forced(gt, ids, C=3, H=64, W=64, mix=None, what=""):
    gt = np.asarray(gt, np.float32).reshape(1, -1, 4) if np.ndim(gt) == 2 else np.asarray(gt, np.float32)
    ids = np.asarray(ids, np.float32)
    ids = ids.reshape(gt.shape[0], gt.shape[1], -1)
    got, want = run_kernel(gt, ids, mix, C, H, W), host(gt, ids, mix, C, H, W)
    compare(got, want, what)
    return got, want


def test_later_gt_on_the_same_row_wins_every_column():
    """two and three gts on one cell and anchor with different classes (and slightly different sizes, so the other columns
    differ too): the last one's row stands and the earlier 1s are gone"""
    for k in (2, 3):
        gt = [[24. - i, 24., 40. + i, 40.] for i in range(k)] + [[4., 4., 60., 50.]]
        got, want = _forced(gt, list(range(k)) + [0], what="%d on one row" % k)
        p = 3 * (4 + 16) + (4 * 8 + 4) * 3 + 1
        assert got[0][0, p, 0] == 1.0 and got[4][0, p].tolist() == [1.0 if c == k - 1 else 0.0 for c in range(3)]
        assert int((got[0] == 1).sum()) == 2


def test_rows_behind_a_padded_row_are_ignored():
    got, _ = _forced([BOX16, PAD, [4., 4., 60., 50.], [2., 2., 12., 14.]], [0, -1, 1, 2], what="pad in the middle")
    assert int((got[0] == 1).sum()) == 1
    got, _ = _forced([[PAD, PAD, PAD], [BOX16, [4., 4., 60., 50.], PAD]], [[-1, -1, -1], [0, 1, -1]], what="an image of padded rows")
    assert np.all(got[0][0] == 0) and np.all(got[4][0] == -1) and int((got[0][1] == 1).sum()) == 2


def test_a_negative_or_nan_coordinate_ends_the_image():
    for bad in ([5., -0.5, 20., 20.], [5., 5., float("nan"), 20.], [-0.0001, 5., 20., 20.]):
        got, _ = _forced([BOX16, bad, [4., 4., 60., 50.]], [0, 1, 2], what="row %r" % (bad,))
        assert int((got[0] == 1).sum()) == 1


def test_centre_on_and_within_fp32_rounding_of_a_cell_edge():
    got, _ = _forced([BOX16], [0], C=1, what="cell border")
    p = 3 * (4 + 16) + (4 * 8 + 4) * 3 + 1
    assert got[0][0, p, 0] == 1.0 and got[1][0, p].tolist() == [0.0, 0.0]
    # tests/test_oracle_cpu.py::test_prefetch_targets_centre_within_fp32_rounding_of_a_cell_edge: x1 and x2 ARE 32 and 96 in fp32
    got, _ = _forced(np.array([[[31.9999995, 59.0, 95.9999995, 149.0]]]), [0], C=2, H=416, W=416, what="fp32 edge")
    p = 3 * 13 * 13 + (6 * 26 + 4) * 3 + 2
    assert got[0][0, p, 0] == 1.0 and np.allclose(got[1][0, p], [0.0, 0.5], atol=1e-7)


def test_degenerate_boxes():
    _forced([[10., 10., 10.5, 30.], [30., 30., 50., 30.25]], [0, 1], what="a width and a height below 1")
    _forced([[10., 10., 10., 10.], [40., 20., 40., 20.]], [2, 1], what="zero-area boxes")
    _forced([[30., 30., 20., 50.]], [1], what="x2 < x1")


def test_centre_on_the_right_and_bottom_edge_wraps_like_the_host():
    """A zero-width box has shape IoU 0 with every anchor, so it always matches anchor 0 (stride 32); the stride-16 and stride-8
    cases use boxes of their anchors' sizes centred ON the right edge (x2 beyond the image, every coordinate >= 0)."""
    H = W = 64
    _forced([[64., 10., 64., 20.]], [1], what="zero width, right edge, stride 32, row 0")          # -> cell (1, 0)
    _forced([[64., 40., 64., 50.]], [1], what="zero width, right edge, stride 32, last row")       # -> the stride-16 layer's row 0
    _forced([[64. - 15, 2., 64. + 15, 63.]], [2], what="right edge, stride 16")                    # anchor (30,61)
    _forced([[64. - 15, 33., 64. + 15, 94.]], [2], what="right edge, stride 16, last row")         # -> the stride-8 layer
    _forced([[64. - 5, 10., 64. + 5, 23.]], [0], what="right edge, stride 8")                      # anchor (10,13)
    _forced([[10., 64., 40., 64.]], [0], what="zero height, bottom edge, stride 32")


def test_a_row_outside_the_image_is_dropped_not_stored():
    """the stride-8 layer's last row, centre on the right edge: p = P + a.  The host raises IndexError; the device drops the gt:
    all five tensors are the host's without it."""
    edge = [64. - 5, 57., 64. + 5, 70.]                            # 10x13, centre (64, 63.5): cell y 7, cell x 8 of 8
    others = [BOX16, [4., 4., 60., 50.]]
    gt = np.asarray([others[0], edge, others[1]], np.float32)[None]
    ids = np.asarray([0, 1, 2], np.float32).reshape(1, 3, 1)
    with pytest.raises(IndexError):
        host(gt, ids, None, 3, 64, 64)
    want = host(gt[:, [0, 2]], ids[:, [0, 2]], None, 3, 64, 64)
    # the outputs in ONE allocation with guard words between and behind them: a store past an output's end shows
    P, C = num_rows(64, 64), 3
    sizes = [P * c for c in (1, 2, 2, 2, C)]
    buf = torch.full((sum(sizes) + 64 * 6,), float("nan"), dtype=torch.float32, device="cuda")
    outs, pos = [], 64
    for s in sizes:
        outs.append(buf[pos:pos + s])
        pos += s + 64
    d = lambda a: torch.from_numpy(a).cuda()
    ops.yolo_targets(d(gt), d(ids), 1, None, 1, 3, C, 64, 64, *outs)
    torch.cuda.synchronize()
    host_buf = buf.cpu().numpy()
    got, pos = [], 64
    for s, c in zip(sizes, (1, 2, 2, 2, C)):
        got.append(host_buf[pos:pos + s].reshape(1, P, c))
        assert np.isnan(host_buf[pos - 64:pos]).all() and np.isnan(host_buf[pos + s:pos + s + 64]).all()
        pos += s + 64
    compare(got, want, "dropped gt")
    # far outside: coordinates of 1e30 make a valid row (>= 0) whose cell is nowhere near the image
    got = run_kernel(np.asarray([[others[0], [1e30, 1e30, 2e30, 2e30], [1e30, 1., 2e30, 9.], others[1]]], np.float32),
                     np.asarray([0, 1, 1, 2], np.float32).reshape(1, 4, 1), None, C, 64, 64)
    compare(got, want, "far outside")


def test_mix_ratios_and_multi_hot_ids():
    rng = np.random.default_rng(5)
    N, M, C = 3, 8, 6
    gt, ids = random_labels(rng, N, M, C, 64, 96)
    mix = rng.uniform(0, 1, (N, M)).astype(np.float32)
    with_mix = run_kernel(gt, ids, mix, C, 64, 96)
    compare(with_mix, host(gt, ids, mix, C, 64, 96), "mix given")
    without = run_kernel(gt, ids, None, C, 64, 96)
    compare(without, host(gt, ids, None, C, 64, 96), "mix NULL")
    assert not np.array_equal(with_mix[0], without[0])
    hot = (rng.uniform(0, 1, (N, M, C)) < 0.4).astype(np.float32)
    compare(run_kernel(gt, hot, None, C, 64, 96), host(gt, hot, None, C, 64, 96), "multi-hot")
    # a class index outside [0, C) writes no 1 (targets_on_device refuses it on the host; the kernel must not store there)
    got = run_kernel([[BOX16, [4., 4., 60., 50.]]], [[[7.], [-3.]]], None, 3, 64, 64)
    want = list(host([[BOX16, [4., 4., 60., 50.]]], [[[0.], [0.]]], None, 3, 64, 64))
    want[4] = np.where(want[4] == 1, 0, want[4]).astype(np.float32)
    compare(got, want, "class index outside")


def test_two_launches_give_the_same_bits():
    rng = np.random.default_rng(9)
    gt, ids = random_labels(rng, 3, 300, 20, 64, 96, full=True)
    a, b = run_kernel(gt, ids, None, 20, 64, 96), run_kernel(gt, ids, None, 20, 64, 96)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- targets_on_device on loader batches ----------------------------------------------------------------------------------
SIZE, C, BS = 64, 3, 4


def _check_batch(hb_targets, hb_gt, labels, what):
    tg = targets_on_device(labels, SIZE, SIZE, C)
    torch.cuda.synchronize()
    assert all(t.is_cuda and t.dtype == torch.float32 for t in tg)
    gt = tg[0].cpu().numpy()
    assert gt.shape == hb_gt.shape and np.array_equal(_bits(gt), _bits(hb_gt)), what
    compare([t.cpu().numpy() for t in tg[1:]], hb_targets, what)
    return tg


def _pairs(ds, **kw):
    mk = lambda **k2: Loader(ds, YOLO3VideoTrainTransform(SIZE, SIZE, C, Rng.seeded(5), **dict(kw, **k2)), BS, train=True, seed=5)
    return zip(mk(), mk(device_targets=True))


def test_targets_on_device_single_frames():
    ds = SyntheticDetection("synthetic", num_samples=2 * BS, size=(80, 60), num_class=C, max_gt=6)
    for i, (hb, db) in enumerate(_pairs(ds)):
        assert np.array_equal(hb[0], db[0])
        _check_batch(hb[1:6], hb[6], db[1], "single frames, batch %d" % i)


def test_targets_on_device_per_frame_labels():
    ds = SyntheticDetection("synthetic", num_samples=BS, size=(80, 60), num_class=C, max_gt=6, window=3, mult_out=True)
    for hb, db in _pairs(ds):
        tg = _check_batch(hb[1:6], hb[6], db[1], "K = 3 with mult_out")
        assert tg[0].shape[:2] == (BS, 3) and tg[1].shape == (BS, 3, num_rows(SIZE, SIZE), 1)


def test_targets_on_device_mixup():
    base = SyntheticDetection("synthetic", num_samples=BS, size=(80, 60), num_class=C, max_gt=6)
    batches = []
    for kw in (dict(), dict(device_targets=True)):
        ds = MixupDetection(base, np.random.RandomState(1).beta, 1.5, 1.5, rng=np.random.RandomState(2))
        batches.append(next(iter(Loader(ds, YOLO3VideoTrainTransform(SIZE, SIZE, C, Rng.seeded(5), mixup=True, **kw), BS, train=True,
                                        seed=5))))
    hb, db = batches
    assert db[1].shape[-1] == 6 and np.any((hb[1] > 0) & (hb[1] < 1))
    _check_batch(hb[1:6], hb[6], db[1], "mixup")


def test_targets_on_device_features_loader(tmp_path):
    from tests.test_device_targets_cpu import _write_features
    base = SyntheticDetection("synthetic", num_samples=BS, size=(80, 60), num_class=C, max_gt=6)
    _write_features(base, tmp_path)
    ds = FeatureDataset(base, str(tmp_path))
    mk = lambda **kw: next(iter(Loader(ds, YOLO3NBVideoTrainTransform(1, SIZE, SIZE, C, **kw), BS, train=True, seed=5)))
    hb, db = mk(), mk(device_targets=True)
    assert len(db) == 4 and all(np.array_equal(a, b) for a, b in zip(hb[:3], db[:3]))
    _check_batch(hb[3:8], hb[8], db[3], "features loader")


# ---- one training step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_training_step_on_the_device_targets(storage, monkeypatch):
    """The network called once with the host columns uploaded and once with targets_on_device's tensors, from the same weights:
    the four losses within rtol = 1e-5 (one fp32 ulp of a scale target moves a loss term by parts in 10^7); if the six inputs
    were bit-equal, the losses and a seeded sample of gradients are bit-equal too."""
    from viddet_amd import model as M
    from viddet_amd.model import yolo3_darknet53
    monkeypatch.setenv("VD_AUTOTUNE", "0")
    M._TUNE_CACHE.clear()
    ds = SyntheticDetection("synthetic", num_samples=BS, size=(80, 60), num_class=C, max_gt=6)
    (hb, db), = list(_pairs(ds))
    x = torch.from_numpy(hb[0]).cuda()
    host_cols = [torch.from_numpy(b).cuda() for b in hb[1:7]]
    tg = targets_on_device(db[1], SIZE, SIZE, C)
    dev_cols = list(tg[1:]) + [tg[0]]
    same_inputs = all(torch.equal(a, b) for a, b in zip(host_cols, dev_cols))
    results = []
    for cols in (host_cols, dev_cols):
        net = yolo3_darknet53(["c%d" % i for i in range(C)])
        net.initialize(init="he", seed=9)
        if storage == "bf16":
            net.set_storage("bf16")
        out = net(x, cols[5], *cols[0:5])
        net.backward()
        torch.cuda.synchronize()
        params = net.collect_params()
        keys = sorted(k for k, _ in params.items() if k.endswith("weight"))
        pick = [keys[i] for i in np.random.default_rng(3).choice(len(keys), 6, replace=False)]
        results.append(([o.cpu().numpy() for o in out], [params[k].grad().cpu().numpy() for k in pick]))
    (la, ga), (lb, gb) = results
    for a, b in zip(la, lb):
        assert np.all(np.isfinite(a)) and np.allclose(a, b, rtol=1e-5, atol=0), (a, b)
    if same_inputs:
        print("%s: the six inputs were bit-equal -> losses and gradients compared bit for bit" % storage)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(la, lb))
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ga, gb))
    else:
        print("%s: a scale target differs in its last bit -> losses compared to rtol 1e-5 only" % storage)


# ---- the script -----------------------------------------------------------------------------------------------------------
def _run_script(tmp_path, prefix, extra):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["--batch_size", "4", "--data_shape", "64", "--epochs", "1", "--synthetic_samples", "8", "--save_prefix", prefix,
            "--log_interval", "1", "--no_random_shape", "--num_workers", "2"] + extra
    env = dict(os.environ, VD_AUTOTUNE="0")
    p = subprocess.run([sys.executable, os.path.join(root, "train_yolov3.py")] + args, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-1500:]
    pre = tmp_path / "models" / "experiments" / prefix
    log = (pre / "yolo3_darknet53_voc_train.log").read_text()
    lines = [ln for ln in log.splitlines() if "ObjLoss=" in ln and "Batch" in ln]
    assert len(lines) == 4, log
    vals = [[float(t.split("=")[1].rstrip(",")) for t in ln.split() if "Loss=" in t] for ln in lines]
    assert all(len(v) == 4 and all(np.isfinite(v)) and all(x >= 0 for x in v) for v in vals), lines
    assert (pre / "yolo3_darknet53_voc_0001.params").exists()
    return np.asarray(vals)


@pytest.mark.parametrize("extra", [[], ["--device_augment"]], ids=["alone", "device_augment"])
def test_train_script_with_device_targets(tmp_path, extra):
    """train_yolov3.py --device_targets end to end in a fresh child process (two epochs of two batches, worker processes on):
    exit status 0, finite losses, and the logged losses are those of the same run without the flag to one unit of the last
    printed digit"""
    want = _run_script(tmp_path, "host", extra)
    got = _run_script(tmp_path, "dt", extra + ["--device_targets"])
    print("logged losses without the flag:\n%s\nwith --device_targets:\n%s" % (want, got))
    assert np.all(np.abs(got - want) <= 1e-3 + 1e-9), (got, want)
