"""GPU: vd_augment_u8_nchw and the paths that use it.

Kernel: against tests/augment_oracle.py's host chain (colour operations in float32, filled canvas, slice, video.imresize,
reversed axis, to_tensor + normalise) on forced parameter sets.  The bound is derived per sample from its tables:
    2^-23 * V * (Ty + Tx + 12) * max_rows sum|w_y| * max_cols sum|w_x| / (255 * 0.224)
V = the largest absolute distorted level of the sample: a chain of Tx then Ty fmaf roundings on values bounded by V times the
weight sums, 12 more roundings for the colour affine, the weight casts and the normalise, through the steepest normalise
(1 / (255 * 0.224)).  tests/test_augment_cpu.py holds the NumPy restatement of the kernel to the same bound.

Paths: augment_on_device on a loader's batches against the host transform's pixel column, one training step on either batch,
and train_yolov3.py --device_augment end to end in a child process.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import augment_oracle as AO
from viddet_amd.augment import AugmentBatch, augment_on_device
from viddet_amd.data import Loader, SyntheticDetection, YOLO3VideoTrainTransform
from viddet_amd.video import Rng

pytestmark = pytest.mark.gpu

CASES = AO.forced_cases()


@pytest.fixture(scope="module")
def references():
    """case name -> (batch, frames, records, host pixels): computed once, never written to"""
    out = {}
    for case in CASES:
        batch, frames, recs = AO.build_case(case)
        want = AO.host_case(case, frames, recs)
        want.setflags(write=False)
        out[case["name"]] = (batch, frames, recs, want)
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_kernel_matches_the_host_chain(case, references):
    batch, frames, recs, want = references[case["name"]]
    got = augment_on_device(batch)
    again = augment_on_device(batch)
    torch.cuda.synchronize()
    assert got.shape == batch.shape and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(got, again), "two launches must give the same bits"
    got = got.cpu().numpy().reshape(want.shape)
    k = case["K"]
    for n, (f, r) in enumerate(zip(frames, recs)):
        tol = AO.tolerance(r, f)
        err = float(np.abs(got[n * k:(n + 1) * k] - want[n * k:(n + 1) * k]).max())
        print("%s sample %d: Ty=%d Tx=%d error %.3g bound %.3g" % (case["name"], n, r.idx_y.shape[1], r.idx_x.shape[1], err, tol))
        assert err <= tol, (case["name"], n, err, tol)


def test_entry_point_refuses_bad_arguments_without_launching():
    from viddet_amd import lib as L
    calls = AO.bad_argument_calls(L.load())
    assert len(calls) >= 28
    for kw, rc, err in calls:
        assert rc == -1, kw
        assert err.startswith(b"vd_augment_u8_nchw:"), (kw, err)
    torch.cuda.synchronize()                                       # nothing was launched: nothing can have faulted


# ---- paths ---------------------------------------------------------------------------------------------------------------
SIZES, C, BS = (32, 64), 4, 4


def _loaders(seed, ds):
    def mk(**kw):
        rng = Rng.seeded(seed)                                     # one generator pair for the whole list, as the script builds it
        return Loader(ds, [YOLO3VideoTrainTransform(s, s, C, rng, **kw) for s in SIZES], BS, train=True, seed=seed, interval=1)
    return mk(), mk(device_augment=True)


def test_loader_batches_match_the_host_pixel_column():
    """8 seeds of the random-shape loader: augment_on_device(batch) against the host transform's pixels, every sample within its
    own bound; every other column is the host loader's."""
    ds = SyntheticDetection("synthetic", num_samples=2 * BS, size=(61, 47), num_class=C, max_gt=3)
    shapes = set()
    for seed in range(8):
        host, dev = _loaders(seed, ds)
        # the records of the same stream, for the bound (the transforms of one loader share one generator pair)
        rng = Rng.seeded(seed)
        tfs = {s: YOLO3VideoTrainTransform(s, s, C, rng, device_augment=True) for s in SIZES}
        i = 0
        for hb, db in zip(host, dev):
            assert isinstance(db[0], AugmentBatch) and db[0].shape == hb[0].shape
            assert all(np.array_equal(a, b) for a, b in zip(hb[1:], db[1:]))
            got = augment_on_device(db[0]).cpu().numpy()
            shapes.add(got.shape[-1])
            for n in range(BS):
                img, label = ds[i]
                rec = tfs[db[0].H](img, label)[1]
                tol = AO.tolerance(rec, img[np.newaxis])
                err = float(np.abs(got[n] - hb[0][n]).max())
                assert err <= tol, (seed, i, err, tol, rec.params)
                i += 1
    assert shapes == set(SIZES)


def test_training_step_on_the_device_batch(monkeypatch):
    """one step of a small network on the device-augmented batch and on the host batch: the losses agree as a step agrees with
    its oracle in tests/test_model_gpu.py (2e-3 of max(1, |loss|))"""
    from viddet_amd import model as M
    from viddet_amd.model import yolo3_darknet53
    monkeypatch.setenv("VD_AUTOTUNE", "0")
    M._TUNE_CACHE.clear()
    ds = SyntheticDetection("synthetic", num_samples=BS, size=(80, 60), num_class=C, max_gt=3)
    mk = lambda **kw: next(iter(Loader(ds, YOLO3VideoTrainTransform(64, 64, C, Rng.seeded(5), **kw), BS, train=True, seed=5)))
    hb, db = mk(), mk(device_augment=True)
    losses = []
    for x, cols in ((torch.from_numpy(hb[0]).cuda(), hb[1:]), (augment_on_device(db[0]), db[1:])):
        net = yolo3_darknet53(["c%d" % i for i in range(C)])
        net.initialize(init="he", seed=9)
        dv = [torch.from_numpy(b).cuda() for b in cols]
        out = net(x, dv[5], *dv[0:5])
        net.backward()
        torch.cuda.synchronize()
        losses.append([o.cpu().numpy() for o in out])
    for a, b in zip(*losses):
        assert np.all(np.isfinite(a)) and np.all(np.abs(a - b) <= 2e-3 * np.maximum(1.0, np.abs(a))), (a, b)


def test_train_script_with_device_augment(tmp_path):
    """train_yolov3.py --device_augment end to end in a fresh child process: two epochs of two batches, worker processes on,
    finite losses in the log and the checkpoint written"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["--batch_size", "4", "--data_shape", "64", "--epochs", "1", "--synthetic_samples", "8", "--save_prefix", "da",
            "--log_interval", "1", "--no_random_shape", "--num_workers", "2", "--device_augment"]
    env = dict(os.environ, VD_AUTOTUNE="0")
    p = subprocess.run([sys.executable, os.path.join(root, "train_yolov3.py")] + args, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-1500:]
    pre = tmp_path / "models" / "experiments" / "da"
    log = (pre / "yolo3_darknet53_voc_train.log").read_text()
    lines = [ln for ln in log.splitlines() if "ObjLoss=" in ln and "Batch" in ln]
    assert len(lines) == 4, log
    for ln in lines:
        vals = [float(t.split("=")[1].rstrip(",")) for t in ln.split() if "Loss=" in t]
        assert len(vals) == 4 and all(np.isfinite(vals)) and all(v >= 0 for v in vals), ln
    assert (pre / "yolo3_darknet53_voc_0001.params").exists()
