"""CPU: the host side of the device resize - the tap tables handed to vd_resize_u8_nchw, the interp-9 rule
factored out of imresize, the raw-frame transform, the script's flag, and every refusal, all before any GPU work."""
import numpy as np
import pytest

from viddet_amd import video as V

CLASSES = ["a", "b"]
# (h0, w0, h, w) -> what interp 9 resolves to: both axes shrink -> area, both enlarge -> bicubic, mixed -> bilinear
BRANCHES = [((50, 70, 32, 32), 2), ((20, 24, 32, 64), 3), ((40, 24, 32, 32), 1), ((32, 70, 32, 32), 1), ((330, 330, 32, 32), 2)]


@pytest.mark.parametrize("shape,interp", BRANCHES)
def test_resize_tables_are_axis_taps_after_the_cast(shape, interp):
    h0, w0, h, w = shape
    used, iy, wy, ix, wx = V.resize_tables(h0, w0, h, w, 9)
    assert used == interp == V.resolve_interp(h0, w0, h, w, 9)
    for (idx, wt), n_in, n_out in (((iy, wy), h0, h), ((ix, wx), w0, w)):
        ri, rw = V._axis_taps(n_in, n_out, interp)
        assert idx.dtype == np.int32 and wt.dtype == np.float32 and idx.flags.c_contiguous and wt.flags.c_contiguous
        assert idx.shape == wt.shape == ri.shape and idx.shape[0] == n_out
        assert np.array_equal(idx, ri) and np.array_equal(wt, rw.astype(np.float32))
        assert idx.min() >= 0 and idx.max() < n_in
    # an explicit interpolation is taken as it is; what has no tap tables is refused
    assert V.resize_tables(h0, w0, h, w, 4)[0] == 4 and V.resize_tables(h0, w0, h, w, 4)[1].shape[1] == 8
    with pytest.raises(ValueError, match="resize_tables"):
        V.resize_tables(h0, w0, h, w, 0)


def _imresize_before_the_refactor(img, w, h, interp):
    """imresize with the interp-9 rule written out as it stood inside it"""
    h0, w0 = img.shape[:2]
    if interp == 9:
        interp = 2 if (h < h0 and w < w0) else (3 if (h > h0 and w > w0) else 1)
    return V.imresize(img, w, h, interp=interp)


@pytest.mark.parametrize("shape,interp", BRANCHES)
def test_imresize_is_unchanged_by_the_refactor(shape, interp):
    h0, w0, h, w = shape
    img = np.random.default_rng(h0 * w0).integers(0, 256, (h0, w0, 3), dtype=np.uint8)
    got = V.imresize(img, w, h, interp=9)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3)
    assert np.array_equal(got, _imresize_before_the_refactor(img, w, h, 9))
    # and it is the separable operator of the resolved interpolation: dense matrices, fp64, rounded as imresize rounds
    Wy, Wx = V._axis_weights(h0, h, interp), V._axis_weights(w0, w, interp)
    v = np.einsum("yr,rcx,oc->yox", Wy, img.astype(np.float64), Wx)
    ref = np.clip(np.rint(v), 0, 255)
    tie = np.abs(v - np.floor(v) - 0.5) < 1e-9                            # (the two summation orders may round a tie apart)
    assert np.array_equal(got[~tie], ref[~tie].astype(np.uint8)) and np.abs(got.astype(int) - ref).max() <= 1
    assert np.array_equal(V.imresize(img, w0, h0, interp=9), img)


def test_transform_with_device_resize_returns_the_raw_frames():
    from viddet_amd.data import YOLO3VideoInferenceTransform
    rng = np.random.default_rng(3)
    label = np.array([[5., 6., 40., 30., 1., 0.], [10., 2., 60., 44., 0., 0.]])
    on = YOLO3VideoInferenceTransform(64, 32, device_normalize=True, device_resize=True)
    off = YOLO3VideoInferenceTransform(64, 32, device_normalize=True)
    for shape in ((50, 70, 3), (3, 50, 70, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        x, bb, idx = on(img, label, 7)
        assert x.dtype == np.uint8 and x.shape == shape and x.tobytes() == img.tobytes() and idx == 7
        x0, bb0, _ = off(img, label, 7)
        assert x0.shape == shape[:-3] + (32, 64, 3)
        assert bb.dtype == bb0.dtype and np.array_equal(bb, bb0)
    with pytest.raises(ValueError, match="device_resize=True needs device_normalize"):
        YOLO3VideoInferenceTransform(64, 64, device_resize=True)
    with pytest.raises(ValueError, match="device_resize=True needs device_normalize"):
        YOLO3VideoInferenceTransform(64, 64, device_normalize=False, device_resize=True)


BASE = ["--random_init", "--data_shape", "64", "--device_resize"]


def test_detect_script_refuses_device_resize_with_several_datasets_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    with pytest.raises(NotImplementedError, match="--device_resize does not combine with several --dataset"):
        D.main(BASE + ["--dataset", "voc,coco"])


def test_detect_script_accepts_device_resize_up_to_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    join = ["--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early"]
    for extra in (["--dataset", "voc"], ["--dataset", "vid", "--stream"] + join, ["--dataset", "vid", "--precision", "bf16"] + join,
                  ["--dataset", "vid", "--stream", "--model_agnostic", "--window", "3,1", "--k_join_type", "cat", "--k_join_pos", "late"]):
        with pytest.raises(SystemExit):
            D.main(BASE + extra)
    F = D.parse_flags(["--device_resize"])
    assert F.device_resize is True and D.parse_flags([]).device_resize is False


def test_set_device_resize_refusals_before_any_gpu_work():
    import torch
    from viddet_amd.model import yolo3_darknet53, yolo3_no_backbone
    net = yolo3_darknet53(CLASSES, device="cpu")
    assert net._dev_resize is None
    for w, h in ((48, 64), (64, 50), (0, 64), (-32, 64)):
        with pytest.raises(ValueError, match="set_device_resize: width and height must be positive multiples of 32"):
            net.set_device_resize(w, h)
    with pytest.raises(ValueError, match="set_device_resize: interp 0"):
        net.set_device_resize(64, 64, interp=0)
    assert net._dev_resize is None
    with pytest.raises(NotImplementedError, match="set_device_resize with noback"):
        yolo3_no_backbone(CLASSES, device="cpu").set_device_resize(64, 64)
    net.set_device_resize(64, 96)
    assert net._dev_resize == (96, 64, 9)
    with pytest.raises(ValueError, match="set_device_resize is on: the network takes raw uint8 frames"):
        net(torch.zeros(2, 3, 96, 64))
    with pytest.raises(ValueError, match="set_device_resize is on"):
        net.detect_video(torch.zeros(4, 3, 96, 64))
    # more taps than the kernel takes (a 20x area shrink: 21 + 1), named before anything is built or uploaded
    with pytest.raises(ValueError, match="set_device_resize: a 1920x1280 -> 96x64 resize has Ty=21 / Tx=21"):
        net(torch.zeros(1, 1920, 1280, 3, dtype=torch.uint8))
    assert not net._programs
    # the tables are cached on the net per (H0, W0, H, W, interp)
    t = net._resize_tables(50, 70)
    assert net._resize_tables(50, 70) is t and set(net._resize_cache) == {(50, 70, 96, 64, 9)} and t['dev'] is None
    assert net._in_shape(torch.zeros(2, 50, 70, 3, dtype=torch.uint8)) == (2, 96, 64)
    net.set_device_resize(None)
    assert net._dev_resize is None and net._in_shape(torch.zeros(2, 50, 70, 3, dtype=torch.uint8)) == (2, 50, 70)
    assert net._in_shape(torch.zeros(2, 3, 96, 64)) == (2, 96, 64)


def test_library_exports_the_resize():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # an entry point was only added
    assert callable(lib.vd_resize_u8_nchw) and len(L.SIGNATURES["vd_resize_u8_nchw"][1]) == 15


def test_resize_checks_its_arguments_before_any_launch():
    from viddet_amd import lib as L
    lib = L.load()
    P = 4096                                                               # an aligned, never dereferenced address
    good = dict(in_=P, out=P, out_u8=None, N=2, H0=50, W0=70, H=32, W=32, iy=P, wy=P, Ty=3, ix=P, wx=P, Tx=4)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_resize_u8_nchw(a['in_'], a['out'], a['out_u8'], a['N'], a['H0'], a['W0'], a['H'], a['W'], a['iy'], a['wy'],
                                   a['Ty'], a['ix'], a['wx'], a['Tx'], None)
        return rc, lib.vd_last_error()

    bad = [dict(in_=None), dict(out=None), dict(iy=None), dict(wy=None), dict(ix=None), dict(wx=None),
           dict(Tx=17), dict(Ty=17), dict(Tx=0), dict(Ty=-1), dict(H=0), dict(W=0), dict(N=0), dict(H0=0), dict(W0=-3),
           dict(iy=P + 2), dict(wx=P + 1), dict(out=P + 2),
           dict(W0=70000, Tx=2)]                                           # one tile's source columns do not fit in LDS
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_resize_u8_nchw:"), (kw, err)
    assert b"Tx=17" in call(Tx=17)[1] and b"H=0" in call(H=0)[1] and b"NULL" in call(in_=None)[1]
    assert b"LDS" in call(W0=70000, Tx=2)[1]
