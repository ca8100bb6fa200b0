"""CPU: the host half of the device augmentation - YOLO3VideoTrainTransform(device_augment=True) takes the host
path's decisions from the host path's draws, its records describe the host path's pixels (checked through the NumPy restatement
of vd_augment_u8_nchw within the GPU test's bound, before any GPU exists), the tap rule, the batch assembly and the refusals."""
import numpy as np
import pytest

from tests import augment_oracle as AO
from viddet_amd import video as V
from viddet_amd.augment import AugmentBatch, AugmentRecord, FILL_TAP, augment_record
from viddet_amd.data import Loader, SyntheticDetection, YOLO3VideoTrainTransform
from viddet_amd.video import Rng

SEEDS = range(64)
SRC, H, W, C = (64, 48), 32, 32, 5          # (width, height) of the synthetic source; target; classes


def _dataset(window, mult_out):
    return SyntheticDetection("synthetic", num_samples=8, size=SRC, num_class=C, max_gt=3, window=window, mult_out=mult_out)


def _pair(seed, **kw):
    return (YOLO3VideoTrainTransform(W, H, C, Rng.seeded(seed), **kw),
            YOLO3VideoTrainTransform(W, H, C, Rng.seeded(seed), device_augment=True, **kw))


def _same_state(a, b):
    sa, sb = a._rng.np.get_state(), b._rng.np.get_state()
    return (sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:] and a._rng.py.getstate() == b._rng.py.getstate())


@pytest.fixture(scope="module")
def runs():
    """seed -> (sample, host columns, device columns) for single frames; shared by the decision and the record test"""
    ds = _dataset(1, False)
    out = {}
    for s in SEEDS:
        host, dev = _pair(s)
        img, label = ds[s % len(ds)]
        out[s] = ((img, label), host(img, label), dev(img, label), _same_state(host, dev))
    return out


def test_same_decisions_single_frames(runs):
    n_exp = n_flip = 0
    interps, orders = set(), set()
    for s in SEEDS:
        (img, _), hc, dc, same = runs[s]
        assert same, s
        assert len(dc) == len(hc) + 1 and isinstance(dc[1], AugmentRecord)
        assert dc[0].dtype == np.uint8 and np.array_equal(dc[0], img)                  # the frames travel untouched
        for a, b in zip(hc[1:], dc[2:]):
            assert a.dtype == b.dtype and np.array_equal(a, b), s
        p = dc[1].params
        n_exp += p["expand"] is not None
        n_flip += p["flip"]
        interps.add(p["interp"])
        names = [n for n, _ in p["ops"] if n != "brightness"]
        if "contrast" in names and len(names) > 1:
            orders.add(names.index("contrast") == 0)
    # the seeds take every branch (a test that never expands or never flips would pass for nothing)
    assert 8 <= n_exp <= 56 and 8 <= n_flip <= 56, (n_exp, n_flip)
    assert interps == {0, 1, 2, 3, 4} and orders == {True, False}


@pytest.mark.parametrize("mult_out", [False, True])
def test_same_decisions_windows(mult_out):
    ds = _dataset(3, mult_out)
    for s in SEEDS:
        host, dev = _pair(s)
        img, label = ds[s % len(ds)]
        hc, dc = host(img, label), dev(img, label)
        assert _same_state(host, dev)
        assert dc[0].shape == (3, SRC[1], SRC[0], 3) and dc[1].window and hc[0].shape == (3, 3, H, W)
        assert len(dc) == 8
        for a, b in zip(hc[1:], dc[2:]):
            assert a.shape == b.shape and np.array_equal(a, b), s
        if mult_out:
            assert hc[1].shape[0] == 3 and hc[6].ndim == 3                              # per-frame targets and gt


def test_no_augment_keeps_its_meaning():
    ds = _dataset(1, False)
    flips = 0
    for s in range(16):
        host, dev = _pair(s, augment=False)
        img, label = ds[s % len(ds)]
        hc, dc = host(img, label), dev(img, label)
        assert _same_state(host, dev)
        p = dc[1].params
        assert p["ops"] == [] and p["expand"] is None and p["crop"] == (0, 0, SRC[0], SRC[1]) and p["interp"] == 1
        assert np.array_equal(dc[1].color, np.concatenate([np.eye(3).ravel(), np.zeros(3)]).astype(np.float32))
        flips += p["flip"]
        for a, b in zip(hc[1:], dc[2:]):
            assert np.array_equal(a, b)
    assert 0 < flips < 16


# ---- the switch off: the host path is the parent's, bit for bit -----------------------------------------------------------
def _old_random_expand(src, max_ratio=4, fill=0, keep_ratio=True, rng=None):
    """random_expand as it was before its draws were factored out"""
    if max_ratio <= 1:
        return src, (0, 0, src.shape[1], src.shape[0])
    k, h, w, c = src.shape
    ratio_x = rng.py.uniform(1, max_ratio)
    ratio_y = ratio_x if keep_ratio else rng.py.uniform(1, max_ratio)
    oh, ow = int(h * ratio_y), int(w * ratio_x)
    off_y = rng.py.randint(0, oh - h)
    off_x = rng.py.randint(0, ow - w)
    if np.isscalar(fill):
        dst = np.full((k, oh, ow, c), fill, dtype=src.dtype)
    else:
        fill = np.asarray(fill, dtype=src.dtype)
        dst = np.tile(fill.reshape(1, 1, 1, c), (k, oh, ow, 1))
    dst[:, off_y:off_y + h, off_x:off_x + w, :] = src
    return dst, (off_x, off_y, ow, oh)


def _old_random_color_distort(src, rng, brightness_delta=32, contrast_low=0.5, contrast_high=1.5, saturation_low=0.5,
                              saturation_high=1.5, hue_delta=18):
    """random_color_distort as it was before its draws were factored out"""
    src = np.asarray(src).astype(np.float32)

    def brightness(x):
        if rng.np.uniform(0, 1) > 0.5:
            x = x + np.float32(rng.np.uniform(-brightness_delta, brightness_delta))
        return x

    def contrast(x):
        if rng.np.uniform(0, 1) > 0.5:
            x = x * np.float32(rng.np.uniform(contrast_low, contrast_high))
        return x

    def saturation(x):
        if rng.np.uniform(0, 1) > 0.5:
            alpha = np.float32(rng.np.uniform(saturation_low, saturation_high))
            gray = (x * np.array([0.299, 0.587, 0.114], np.float32)).sum(axis=-1, keepdims=True)
            x = x * alpha + gray * (np.float32(1.0) - alpha)
        return x

    def hue(x):
        if rng.np.uniform(0, 1) > 0.5:
            alpha = rng.py.uniform(-hue_delta, hue_delta)
            x = np.dot(x, V.hue_matrix(alpha).astype(np.float32))
        return x

    src = brightness(src)
    if rng.np.randint(0, 2):
        src = hue(saturation(contrast(src)))
    else:
        src = contrast(hue(saturation(src)))
    return src.astype(np.float32)


def test_refactored_draw_functions_return_what_they_returned():
    frames = np.random.default_rng(5).integers(0, 256, (2, 21, 30, 3), dtype=np.uint8)
    for s in SEEDS:
        a, b = Rng.seeded(s), Rng.seeded(s)
        want, got = _old_random_color_distort(frames, a), V.random_color_distort(frames, rng=b)
        assert got.dtype == np.float32 and np.array_equal(want, got), s
        for keep in (True, False):
            we, wp = _old_random_expand(want, fill=[1.0, 2.0, 3.0], keep_ratio=keep, rng=a)
            ge, gp = V.random_expand(got, fill=[1.0, 2.0, 3.0], keep_ratio=keep, rng=b)
            assert wp == gp and np.array_equal(we, ge), s
        assert a.np.get_state()[1].tolist() == b.np.get_state()[1].tolist() and a.py.getstate() == b.py.getstate()
        # the parameter functions alone take the same draws
        c, d = Rng.seeded(s), Rng.seeded(s)
        ops = V.color_distort_params(c)
        assert np.array_equal(V.apply_color_ops(frames, ops), _old_random_color_distort(frames, d))
        assert V.expand_params(21, 30, c) == _old_random_expand(frames, rng=d)[1]
    same, (off_x, off_y, ow, oh) = V.random_expand(frames, max_ratio=1)
    assert same is frames and (off_x, off_y) == (0, 0)


def test_switch_off_is_the_host_chain_bit_for_bit(runs):
    """device_augment=False: the pixel column is the chain of host primitives on the decisions the record names - the
    parent's batches (the draws are the parent's: test_refactored_draw_functions_return_what_they_returned)."""
    for s in SEEDS:
        (img, _), hc, dc, _ = runs[s]
        assert np.array_equal(hc[0], AO.host_pixels(img[np.newaxis], dc[1].params, H, W)[0]), s


# ---- records -------------------------------------------------------------------------------------------------------------
def test_records_reproduce_the_host_pixels_within_the_bound(runs):
    worst = 0.0
    for s in SEEDS:
        (img, _), hc, dc, _ = runs[s]
        rec = dc[1]
        assert rec.color.dtype == np.float32 and rec.idx_y.dtype == np.int32 and rec.w_x.dtype == np.float32
        assert rec.idx_y.shape == rec.w_y.shape and rec.idx_y.shape[0] == H and rec.idx_x.shape[0] == W
        assert np.array_equal(rec.fill, AO.FILL)
        if rec.params["expand"] is None:
            assert rec.idx_y.min() >= 0 and rec.idx_x.min() >= 0                        # fill only where the expansion was drawn
        got = AO.kernel_sample(img[np.newaxis], rec.color, rec.idx_y, rec.w_y, rec.idx_x, rec.w_x, rec.fill)[0]
        tol = AO.tolerance(rec, img[np.newaxis])
        err = float(np.abs(got - hc[0]).max())
        worst = max(worst, err / tol)
        assert err <= tol, (s, err, tol, rec.params)
    print("worst error / bound over the seeds: %.3f" % worst)


@pytest.mark.parametrize("case", AO.forced_cases(), ids=lambda c: c["name"])
def test_forced_cases_within_the_bound(case):
    batch, frames, recs = AO.build_case(case)
    want, got = AO.host_case(case, frames, recs), AO.kernel_restatement(batch)
    k = case["K"]
    for n, (f, r) in enumerate(zip(frames, recs)):
        tol = AO.tolerance(r, f)
        err = float(np.abs(got[n * k:(n + 1) * k] - want[n * k:(n + 1) * k]).max())
        print("%s sample %d: error %.3g, bound %.3g" % (case["name"], n, err, tol))
        assert err <= tol, (case["name"], n, err, tol)


def test_forced_cases_cover_what_they_name():
    by = {c["name"]: AO.build_case(c) for c in AO.forced_cases()}
    assert by["interp0"][0].src_off.tolist() == [0, 5883] and by["interp0"][0].src_off[1] % 2 == 1
    b = by["taps32"][0]
    assert (b.Ty, b.Tx) == (32, 32) and by["taps32"][2][0].idx_x.shape[1] == 32 and by["taps32"][2][1].idx_y.shape[1] == 32
    assert by["unequal2"][0].Ty != by["unequal2"][0].Tx
    r_straddle, r_fill = by["expand1"][2]
    mixed = ((r_straddle.idx_x == FILL_TAP).any(axis=1) & (r_straddle.idx_x != FILL_TAP).any(axis=1))
    assert mixed.any() and (r_fill.idx_x == FILL_TAP).all() and (r_fill.idx_y == FILL_TAP).all()
    assert by["window2"][0].K == 2 and by["window2"][0].shape == (2, 2, 3, 32, 32)
    # a flip reverses the rows of the x tables and nothing else
    plain = augment_record(37, 53, 32, 32, interp=3)
    flipped = augment_record(37, 53, 32, 32, interp=3, flip=True)
    assert np.array_equal(plain.idx_x[::-1], flipped.idx_x) and np.array_equal(plain.w_x[::-1], flipped.w_x)
    assert np.array_equal(plain.idx_y, flipped.idx_y)


def test_bad_tables_stay_inside_the_sample():
    """The kernel's clamps, on the restatement (which asserts every index it reads): indices far outside either way read a
    wrong pixel or the fill, never outside the frames."""
    case = AO.forced_cases()[1]
    batch, frames, recs = AO.build_case(case)
    batch.idx_y[0, ::3] = 10 ** 6
    batch.idx_x[1, ::2] = -(10 ** 6)
    batch.idx_x[0, 1::2] = 2 ** 31 - 1
    out = AO.kernel_restatement(batch)
    assert np.all(np.isfinite(out))


def test_color_affine_is_the_float32_chain():
    x = np.random.default_rng(3).integers(0, 256, (1, 9, 11, 3), dtype=np.uint8)
    for ops in (AO.OPS_FULL_A, AO.OPS_FULL_B, [], AO.OPS_FULL_A[:1], AO.OPS_FULL_B[1:3]):
        M, b = V.color_affine(ops)
        want = V.apply_color_ops(x, ops).astype(np.float64)
        assert np.abs(x.astype(np.float64) @ M + b - want).max() <= 2.0 ** -23 * 8 * max(1.0, np.abs(want).max())


# ---- tap rule ------------------------------------------------------------------------------------------------------------
def test_tap_rule_is_decided_from_the_size():
    tf = YOLO3VideoTrainTransform(320, 320, C, Rng.seeded(0), device_augment=True)
    label = np.array([[10.0, 10.0, 100.0, 100.0, 1.0, 0.0]])
    with pytest.raises(ValueError, match="2600x40"):
        tf(np.zeros((40, 2600, 3), np.uint8), label)
    with pytest.raises(ValueError, match="40x2600"):                                   # either axis, windows too
        tf(np.zeros((2, 2600, 40, 3), np.uint8), label)
    for s in range(8):                                                                 # 1920 fits whatever is drawn (25 taps)
        tf = YOLO3VideoTrainTransform(320, 320, C, Rng.seeded(s), device_augment=True)
        out = tf(np.zeros((320, 1920, 3), np.uint8), label)
        assert out[1].idx_x.shape[1] <= 25
    with pytest.raises(ValueError, match="device_augment"):
        YOLO3VideoTrainTransform(32, 32, C, device_augment=True, mixup=True)
    with pytest.raises(ValueError, match="device_augment"):
        YOLO3VideoTrainTransform(32, 32, C, device_augment=True, device_normalize=True)


# ---- batch assembly ------------------------------------------------------------------------------------------------------
class TwoSizes:
    """frames of two source sizes in one dataset"""
    num_class = C

    def __len__(self):
        return 4

    def __getitem__(self, i):
        h0, w0 = ((37, 53), (50, 41))[i % 2]
        rng = np.random.default_rng(i)
        return rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8), np.array([[4.0, 5.0, 30.0, 31.0, float(i % C), 0.0]])


def test_collate_builds_one_batch_object():
    ds = TwoSizes()
    loader = Loader(ds, YOLO3VideoTrainTransform(W, H, C, Rng.seeded(7), device_augment=True), 4, train=True)
    batch = next(iter(loader))
    ab = batch[0]
    assert isinstance(ab, AugmentBatch) and len(batch) == 7 and all(isinstance(b, np.ndarray) for b in batch[1:])
    assert (ab.N, ab.K, ab.H, ab.W) == (4, 1, H, W) and ab.shape == (4, 3, H, W) and not ab.window
    assert ab.src_off.dtype == np.int64 and ab.src_off.tolist() == [0, 5883, 5883 + 6150, 2 * 5883 + 6150]
    assert ab.src_hw.dtype == np.int32 and ab.src_hw.tolist() == [[37, 53], [50, 41]] * 2
    assert ab.raw.dtype == np.uint8 and ab.raw.size == 2 * (5883 + 6150)
    assert ab.color.shape == (4, 12) and ab.idx_y.shape == (4, H, ab.Ty) and ab.w_x.shape == (4, W, ab.Tx)
    # the same draws sample by sample: the batch holds each record's tables, padded with zero-weight fill taps
    tf = YOLO3VideoTrainTransform(W, H, C, Rng.seeded(7), device_augment=True)
    recs = [tf(*ds[i])[1] for i in range(4)]
    assert ab.Ty == max(r.idx_y.shape[1] for r in recs) and ab.Tx == max(r.idx_x.shape[1] for r in recs)
    assert len({r.idx_x.shape[1] for r in recs}) > 1, "the seed should give the batch tables of different widths"
    for n, r in enumerate(recs):
        ty, tx = r.idx_y.shape[1], r.idx_x.shape[1]
        assert np.array_equal(ab.idx_y[n, :, :ty], r.idx_y) and np.array_equal(ab.w_x[n, :, :tx], r.w_x)
        assert np.all(ab.idx_x[n, :, tx:] == FILL_TAP) and np.all(ab.w_x[n, :, tx:] == 0)
        assert np.all(ab.idx_y[n, :, ty:] == FILL_TAP) and np.all(ab.w_y[n, :, ty:] == 0)
        h0, w0 = ab.src_hw[n]
        assert np.array_equal(ab.raw[ab.src_off[n]:ab.src_off[n] + h0 * w0 * 3].reshape(h0, w0, 3), ds[n][0])
    # padding changes no pixel of the restatement
    want = np.concatenate([AO.kernel_sample(ds[n][0][np.newaxis], r.color, r.idx_y, r.w_y, r.idx_x, r.w_x, r.fill)
                           for n, r in enumerate(recs)])
    assert np.array_equal(AO.kernel_restatement(ab), want)
    # one packed buffer: aligned sections that hold the arrays
    buf, lay = ab.packed()
    assert lay["src_off"][0] % 8 == 0 and all(off % 16 == 0 for off, _, _ in lay.values())
    for name, (off, dt, shape) in lay.items():
        a = getattr(ab, name)
        assert np.array_equal(buf[off:off + a.nbytes].view(dt).reshape(shape), a), name


def _same_batches(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for name in AugmentBatch.SECTIONS:
            assert np.array_equal(getattr(x[0], name), getattr(y[0], name)), name
        assert all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:]))


def test_worker_path_carries_the_record():
    ds = _dataset(1, False)
    out = []
    for nw in (2, 1):
        loader = Loader(ds, [YOLO3VideoTrainTransform(s, s, C, Rng.seeded(3), device_augment=True) for s in (32, 64)], 4,
                        train=True, shuffle=True, seed=11, interval=1, num_workers=nw)
        try:
            out.append(list(loader))
        finally:
            loader.close()
    assert len(out[0]) == 2 and isinstance(out[0][0][0], AugmentBatch)
    _same_batches(out[0], out[1])                                                      # whatever worker takes which sample
    assert {b[0].H for b in out[0]} <= {32, 64}


def test_script_refuses_by_name_before_gpu_work():
    import train_yolov3 as T
    common = ["--batch_size", "2", "--data_shape", "64", "--epochs", "1", "--synthetic_samples", "2", "--save_prefix", "0000",
              "--no_random_shape", "--device_augment"]
    with pytest.raises(NotImplementedError, match="--device_augment does not combine with --mixup"):
        T.main(common + ["--mixup"])
    with pytest.raises(NotImplementedError, match="--device_augment does not combine with --features_dir"):
        T.main(common + ["--features_dir", "nowhere"])
    assert T.parse_flags([]).device_augment is False and T.parse_flags(["--device_augment"]).device_augment is True


# ---- the library ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_augmentation():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == L.ABI_VERSION                                       # an entry point was only added
    assert callable(lib.vd_augment_u8_nchw) and len(L.SIGNATURES["vd_augment_u8_nchw"][1]) == 17


def test_augment_checks_its_arguments_before_any_launch():
    from viddet_amd import lib as L
    for kw, rc, err in AO.bad_argument_calls(L.load()):
        assert rc == -1, kw
        assert err.startswith(b"vd_augment_u8_nchw:"), (kw, err)
