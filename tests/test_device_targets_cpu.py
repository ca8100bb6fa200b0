"""CPU: the host half of --device_targets.

The transforms with device_targets=True take the draws of the host path in its order (same pixels, boxes and final generator
state) and carry the boxes as one label column; `prefetch_targets` on that column gives the host path's five target columns bit
for bit, which is what makes vd_yolo_targets' job (tests/test_device_targets_gpu.py) well defined.  Loader batches, the entry
point's refusals (nothing is launched), targets_on_device's host checks and the flag.
"""
import ctypes

import numpy as np
import pytest

from viddet_amd.augment import AugmentRecord
from viddet_amd.data import (FeatureDataset, Loader, MixupDetection, SyntheticDetection, YOLO3NBVideoTrainTransform,
                             YOLO3VideoTrainTransform)
from viddet_amd.targets import prefetch_targets
from viddet_amd.video import Rng

SIZE, C = 64, 4
SEEDS = range(32)


def _state(rng):
    s = rng.np.get_state()
    return (s[0], s[1].tobytes(), s[2:], rng.py.getstate())


def _host_targets_of(lab, mixup):
    """prefetch_targets on a label column (M,5|6) or (t,M,5|6) -> the host path's five columns"""
    frames = lab if lab.ndim == 3 else lab[np.newaxis]
    tg = prefetch_targets(SIZE, SIZE, frames[..., :4], frames[..., 4:5], C, frames[..., 5:6] if mixup else None)
    return tg if lab.ndim == 3 else tuple(t[0] for t in tg)


def _same(a, b):
    if isinstance(a, AugmentRecord):
        return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("color", "idx_y", "w_y", "idx_x", "w_x", "fill")) \
            and a.window == b.window and a.params == b.params
    return a.dtype == b.dtype and np.array_equal(a, b)


MODES = {
    "single": (dict(), dict()),
    "window3": (dict(window=3), dict()),
    "window3_mult_out": (dict(window=3, mult_out=True), dict()),
    "mixup": (dict(), dict(mixup=True)),
    "device_augment": (dict(), dict(device_augment=True)),
    "device_augment_window3_mult_out": (dict(window=3, mult_out=True), dict(device_augment=True)),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_train_transform_takes_the_host_paths_draws_and_boxes(mode):
    ds_kw, tf_kw = MODES[mode]
    ds = SyntheticDetection("synthetic", num_samples=len(SEEDS), size=(90, 70), num_class=C, max_gt=5, seed=11, **ds_kw)
    if tf_kw.get("mixup"):
        ds = MixupDetection(ds, np.random.RandomState(4).beta, 1.5, 1.5, rng=np.random.RandomState(5))
    lead = 2 if tf_kw.get("device_augment") else 1                 # pixel columns: frames (+ record)
    for seed in SEEDS:
        sample = ds[seed]
        ra, rb = Rng.seeded(seed), Rng.seeded(seed)
        host = YOLO3VideoTrainTransform(SIZE, SIZE, C, ra, **tf_kw)(*sample)
        dev = YOLO3VideoTrainTransform(SIZE, SIZE, C, rb, device_targets=True, **tf_kw)(*sample)
        assert len(host) == lead + 6 and len(dev) == lead + 1
        for a, b in zip(host[:lead], dev[:lead]):
            assert _same(a, b), (mode, seed)
        assert _state(ra) == _state(rb), (mode, seed)
        lab = dev[-1]
        assert lab.dtype == np.float32 and lab.shape[-1] == (6 if tf_kw.get("mixup") else 5)
        assert lab.ndim == (3 if ds_kw.get("mult_out") else 2)
        assert _same(host[-1], lab[..., :4]), (mode, seed)         # gt
        for a, b in zip(host[lead:lead + 5], _host_targets_of(lab, tf_kw.get("mixup"))):
            assert _same(a, b), (mode, seed)


def _write_features(ds, fdir):
    from viddet_amd.data import feature_file_id
    rng = np.random.default_rng(0)
    for i in range(len(ds)):
        for k, (ch, g) in enumerate(((8, 8), (8, 4), (8, 2)), 1):
            np.save(str(fdir / ("%s_F%d.npy" % (feature_file_id(ds.sample_path(i)), k))),
                    rng.standard_normal((ch, g, g)).astype(np.float32))


def test_features_transform_carries_the_resized_boxes(tmp_path):
    base = SyntheticDetection("synthetic", num_samples=len(SEEDS), size=(90, 70), num_class=C, max_gt=5, seed=12)
    _write_features(base, tmp_path)
    ds = FeatureDataset(base, str(tmp_path))
    for i in SEEDS:
        host = YOLO3NBVideoTrainTransform(1, SIZE, SIZE, C)(*ds[i])
        dev = YOLO3NBVideoTrainTransform(1, SIZE, SIZE, C, device_targets=True)(*ds[i])
        assert len(host) == 9 and len(dev) == 4
        assert all(_same(a, b) for a, b in zip(host[:3], dev[:3]))
        lab = dev[-1]
        assert lab.dtype == np.float32 and lab.shape[1] == 5 and _same(host[-1], lab[:, :4])
        for a, b in zip(host[3:8], _host_targets_of(lab, False)):
            assert _same(a, b), i


def test_loader_pads_ragged_label_rows_with_minus_one():
    ds = SyntheticDetection("synthetic", num_samples=8, size=(90, 70), num_class=C, max_gt=6, seed=13)
    mk = lambda **kw: Loader(ds, YOLO3VideoTrainTransform(SIZE, SIZE, C, Rng.seeded(3), **kw), 4, train=True, seed=3)
    ragged = False
    for hb, db in zip(mk(), mk(device_targets=True)):
        assert len(hb) == 7 and len(db) == 2
        x, lab = db
        assert _same(hb[0], x) and lab.dtype == np.float32 and lab.shape[0] == 4 and lab.shape[2] == 5
        assert _same(hb[6], lab[..., :4])
        pad = (lab[..., :4] < 0).all(axis=-1)
        assert np.all(lab[pad] == -1.0)
        ragged |= bool(pad.any())
        for a, b in zip(hb[1:6], prefetch_targets(SIZE, SIZE, lab[..., :4], lab[..., 4:5], C)):
            assert _same(a, b)
    assert ragged, "the dataset was meant to give batches with ragged M"


def test_loader_per_frame_labels_are_padded_per_frame():
    ds = SyntheticDetection("synthetic", num_samples=4, size=(90, 70), num_class=C, max_gt=6, seed=14, window=3, mult_out=True)
    mk = lambda **kw: next(iter(Loader(ds, YOLO3VideoTrainTransform(SIZE, SIZE, C, Rng.seeded(3), **kw), 4, train=True, seed=3)))
    hb, (x, lab) = mk(), mk(device_targets=True)
    assert _same(hb[0], x) and lab.ndim == 4 and lab.shape[:2] == (4, 3) and _same(hb[6], lab[..., :4])
    for b in range(4):
        for a, t in zip(hb[1:6], prefetch_targets(SIZE, SIZE, lab[b, ..., :4], lab[b, ..., 4:5], C)):
            assert _same(a[b], t)


def test_loader_worker_processes_give_the_host_runs_gt_column():
    ds = SyntheticDetection("synthetic", num_samples=8, size=(90, 70), num_class=C, max_gt=6, seed=15)
    out = []
    for kw in (dict(), dict(device_targets=True)):
        ld = Loader(ds, YOLO3VideoTrainTransform(SIZE, SIZE, C, Rng.seeded(1), **kw), 4, train=True, shuffle=True, seed=9,
                    num_workers=2)
        try:
            out.append(list(ld))
        finally:
            ld.close()
    assert len(out[0]) == len(out[1]) == 2
    for hb, db in zip(*out):
        assert len(db) == 2 and _same(hb[0], db[0]) and _same(hb[6], db[1][..., :4])
        for a, b in zip(hb[1:6], prefetch_targets(SIZE, SIZE, db[1][..., :4], db[1][..., 4:5], C)):
            assert _same(a, b)


def test_loader_random_shape_list():
    ds = SyntheticDetection("synthetic", num_samples=16, size=(90, 70), num_class=C, max_gt=4, seed=16)

    def mk(**kw):
        rng = Rng.seeded(2)
        return Loader(ds, [YOLO3VideoTrainTransform(s, s, C, rng, **kw) for s in (32, 64)], 4, train=True, seed=2, interval=1)
    shapes = set()
    for hb, db in zip(mk(), mk(device_targets=True)):
        assert len(db) == 2 and _same(hb[0], db[0]) and _same(hb[6], db[1][..., :4])
        s = db[0].shape[-1]
        shapes.add(s)
        for a, b in zip(hb[1:6], prefetch_targets(s, s, db[1][..., :4], db[1][..., 4:5], C)):
            assert _same(a, b)
    assert shapes == {32, 64}


def test_entry_point_refuses_bad_arguments_without_launching():
    from viddet_amd import lib as L
    lib = L.load()
    good = dict(gt=64, ids=64, idw=1, mix=None, N=1, M=2, C=3, H=64, W=64, obj=64, ctr=64, scl=64, wgt=64, cls=64)

    def call(**kw):
        a = dict(good, **kw)                                       # the addresses are only compared and tested for alignment
        rc = lib.vd_yolo_targets(a["gt"], a["ids"], a["idw"], a["mix"], a["N"], a["M"], a["C"], a["H"], a["W"], a["obj"], a["ctr"],
                                 a["scl"], a["wgt"], a["cls"], None)
        return rc, lib.vd_last_error()

    cases = [(dict([(k, None)]), b"NULL") for k in ("gt", "ids", "obj", "ctr", "scl", "wgt", "cls")]
    cases += [(dict(N=0), b"N=0"), (dict(M=0), b"M=0"), (dict(C=0), b"C=0"), (dict(N=-1), b"N=-1"),
              (dict(M=513), b"M=513"),
              (dict(H=16), b"H=16"), (dict(W=0), b"W=0"), (dict(H=72), b"H=72"), (dict(W=100), b"W=100"),
              (dict(idw=2), b"idw=2"), (dict(idw=0), b"idw=0"), (dict(idw=4, C=3), b"idw=4")]
    cases += [(dict([(k, 66)]), b"4-byte aligned") for k in ("obj", "ctr", "scl", "wgt", "cls")]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_yolo_targets:") and text in err, (kw, err)


def test_targets_on_device_checks_the_labels_on_the_host():
    from viddet_amd.device_targets import targets_on_device
    lab = np.full((2, 3, 5), -1.0, np.float32)
    lab[:, 0] = (4, 4, 30, 30, 1)
    lab[1, 1] = (8, 8, 20, 40, 2)
    for bad, text in ((float(C), "sample 1"), (-1.0, "sample 1"), (1.5, "sample 1")):
        l2 = lab.copy()
        l2[1, 1, 4] = bad
        with pytest.raises(ValueError, match=text):
            targets_on_device(l2, SIZE, SIZE, C)
    per_frame = np.stack([lab, lab], axis=1)                       # (B,t,M,5)
    per_frame[1, 1, 0, 4] = 7
    with pytest.raises(ValueError, match="sample 1 frame 1"):
        targets_on_device(per_frame, SIZE, SIZE, C)
    with pytest.raises(ValueError, match="513"):
        targets_on_device(np.zeros((1, 513, 5), np.float32), SIZE, SIZE, C)
    # an id behind the first padded row is never read by the host path: it is not an error
    l3 = lab.copy()
    l3[0, 2] = (1, 1, 9, 9, 99)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            targets_on_device(l3, SIZE, SIZE, C)


def test_flag():
    import train_yolov3 as T
    assert T.parse_flags([]).device_targets is False
    assert T.parse_flags(["--device_targets"]).device_targets is True
    assert T.parse_flags(["--device_targets", "--device_augment", "--num_workers", "2"]).device_augment is True
