"""CPU: the host side of NV12 input - the colour conversion's one definition (video.NV12_MATRICES,
nv12_to_rgb, rgb_to_nv12) against a loop oracle and against the standards' real coefficients, the synthetic NV12 frames, the
transform, the script's flags and every refusal, all before any GPU work."""
import numpy as np
import pytest

from tests.nv12_oracle import nv12_to_rgb_loops
from viddet_amd import video as V

CLASSES = ["a", "b"]
PAIRS = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
# the standards' real coefficients, written out: luma gain, then (ru, rv, gu, gv, bu).  BT.601: Kr = 0.299, Kb = 0.114;
# BT.709: Kr = 0.2126, Kb = 0.0722; limited range = luma * 255/219, chroma * 255/224
REAL = {
    ("bt601", "limited"): (16, 1.164384, 0.0, 1.596027, -0.391762, -0.812968, 2.017232),
    ("bt601", "full"): (0, 1.0, 0.0, 1.402, -0.344136, -0.714136, 1.772),
    ("bt709", "limited"): (16, 1.164384, 0.0, 1.792741, -0.213249, -0.532909, 2.112402),
    ("bt709", "full"): (0, 1.0, 0.0, 1.5748, -0.187324, -0.468124, 1.8556),
}
# |integer result - rint(real formula)| <= 2: rounding each of the three coefficients of a channel to 1/256 moves the sum by at
# most 0.5 * (255 + 128 + 128) / 256 < 1.0 in all, and each side's own rounding (floor(v + 0.5) here, rint there) adds 0.5
BOUND = 2


def _real_rgb(frame, key):
    """rint of the fp64 real-coefficient formula, clipped"""
    off, gain, ru, rv, gu, gv, bu = REAL[key]
    hn, w0 = frame.shape
    h0 = hn * 2 // 3
    c = frame[:h0].astype(np.float64) - off
    uv = frame[h0:].astype(np.float64) - 128.0
    d = np.repeat(np.repeat(uv[:, 0::2], 2, axis=0), 2, axis=1)
    e = np.repeat(np.repeat(uv[:, 1::2], 2, axis=0), 2, axis=1)
    rgb = np.stack([gain * c + ru * d + rv * e, gain * c + gu * d + gv * e, gain * c + bu * d], axis=-1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.int64)


def test_table_entries_are_the_rounded_real_coefficients():
    assert set(V.NV12_MATRICES) == set(PAIRS)
    for key in PAIRS:
        entry = V.NV12_MATRICES[key]
        assert len(entry) == 7 and all(isinstance(c, int) for c in entry)
        assert entry[0] == REAL[key][0]
        assert list(entry[1:]) == [int(round(256 * c)) for c in REAL[key][1:]], key
        assert V.nv12_matrix(*key) is entry


@pytest.mark.parametrize("key", PAIRS, ids=["%s-%s" % k for k in PAIRS])
def test_nv12_to_rgb_equals_the_loop_oracle_and_is_within_two_levels_of_the_real_formula(key):
    rng = np.random.default_rng(PAIRS.index(key))
    frames = rng.integers(0, 256, (2, 36, 30), dtype=np.uint8)            # H0 = 24: all of 0..255 in both planes
    frames[0, :2, :] = np.arange(60, dtype=np.uint8).reshape(2, 30) * 4    # below-black .. above-white luma on one chroma row
    got = V.nv12_to_rgb(frames, *key)
    assert got.dtype == np.uint8 and got.shape == (2, 24, 30, 3)
    worst = 0
    for n in range(2):
        assert np.array_equal(got[n], nv12_to_rgb_loops(frames[n], V.NV12_MATRICES[key])), "differs from the loop oracle"
        worst = max(worst, int(np.abs(got[n].astype(np.int64) - _real_rgb(frames[n], key)).max()))
    print("%s %s: worst |integer - rint(real)| = %d grey levels" % (key + (worst,)))
    assert worst <= BOUND
    assert int((got == 0).sum()) > 0 and int((got == 255).sum()) > 0, "neither clip side was reached"
    # a single frame without a leading axis, and the default matrix
    assert np.array_equal(V.nv12_to_rgb(frames[1], *key), got[1])
    assert np.array_equal(V.nv12_to_rgb(frames), V.nv12_to_rgb(frames, "bt601", "limited"))


@pytest.mark.parametrize("key", PAIRS, ids=["%s-%s" % k for k in PAIRS])
def test_rgb_to_nv12_round_trip_on_block_constant_frames(key):
    rng = np.random.default_rng(10 + PAIRS.index(key))
    blocks = rng.integers(0, 256, (2, 20, 30, 3), dtype=np.uint8)
    blocks[0, 0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]]
    rgb = np.repeat(np.repeat(blocks, 2, axis=1), 2, axis=2)               # constant over each 2 x 2 block
    nv = V.rgb_to_nv12(rgb, *key)
    assert nv.dtype == np.uint8 and nv.shape == (2, 60, 60)
    back = V.nv12_to_rgb(nv, *key)
    worst = int(np.abs(back.astype(np.int64) - rgb).max())
    print("%s %s: round trip worst %d grey levels" % (key + (worst,)))
    assert worst <= BOUND
    if key[1] == "limited":                                               # black and white land on the standard's levels
        assert nv[0, 0, 0] == 16 and nv[0, 0, 2] == 235 and nv[0, 40, 0] == 128 and nv[0, 40, 1] == 128


def test_chroma_is_the_mean_of_the_block():
    rgb = np.zeros((2, 2, 3), np.uint8)
    rgb[0, 0], rgb[1, 1] = (255, 0, 0), (0, 0, 255)
    nv = V.rgb_to_nv12(rgb, "bt601", "full")
    one = [V.rgb_to_nv12(np.broadcast_to(p, (2, 2, 3)).copy(), "bt601", "full")[2].astype(float) for p in rgb.reshape(4, 3)]
    assert np.abs(nv[2].astype(float) - np.mean(one, axis=0)).max() <= 1.0


def test_refusals_of_the_conversion_by_name():
    ok = np.zeros((36, 30), np.uint8)
    for bad in (np.zeros((36, 31), np.uint8), np.zeros((35, 30), np.uint8), np.zeros((2, 37, 30), np.uint8)):
        with pytest.raises(ValueError, match=r"NV12 frames are \(.., H0\*3/2, W0\) with H0 and W0 even.*got %d rows.*W0 = %d"
                           % bad.shape[-2:]):
            V.nv12_to_rgb(bad)
    for shape in ((23, 30, 3), (24, 31, 3)):
        with pytest.raises(ValueError, match="NV12 needs an even frame size.*H0=%d W0=%d" % shape[:2]):
            V.rgb_to_nv12(np.zeros(shape, np.uint8))
    with pytest.raises(ValueError, match="nv12_to_rgb takes uint8 frames"):
        V.nv12_to_rgb(ok.astype(np.float32))
    with pytest.raises(ValueError, match="rgb_to_nv12 takes uint8 frames"):
        V.rgb_to_nv12(np.zeros((24, 30, 3), np.float32))
    for kw in (dict(matrix="bt2020"), dict(range="studio")):
        with pytest.raises(ValueError, match="NV12: unknown matrix / range"):
            V.nv12_to_rgb(ok, **kw)
        with pytest.raises(ValueError, match="NV12: unknown matrix / range"):
            V.rgb_to_nv12(np.zeros((24, 30, 3), np.uint8), **kw)


def test_identity_tables():
    iy, wy, ix, wx = V.identity_tables(4, 6)
    assert iy.dtype == ix.dtype == np.int32 and wy.dtype == wx.dtype == np.float32
    assert np.array_equal(iy[:, 0], np.arange(4)) and np.array_equal(ix[:, 0], np.arange(6))
    assert wy.shape == (4, 1) and wx.shape == (6, 1) and bool((wy == 1).all()) and bool((wx == 1).all())


# ------------------------------------------------------------------------------------------------ data
def test_synthetic_sets_hand_out_rgb_to_nv12_of_their_rgb_frames():
    from viddet_amd.data import SyntheticDetection, SyntheticVideo
    kw = dict(num_videos=2, frames_per_video=4, size=(50, 36))
    rgb, nv = SyntheticVideo(**kw), SyntheticVideo(frame_format="nv12", **kw)
    assert rgb.frame_format == "rgb" and nv.frame_format == "nv12"
    for v in range(2):
        clip = nv.video_frames(v)
        assert clip.shape == (4, 54, 50) and np.array_equal(clip, V.rgb_to_nv12(rgb.video_frames(v)))
    for idx in (0, 5):
        (a, la), (b, lb) = rgb[idx], nv[idx]
        assert np.array_equal(b, V.rgb_to_nv12(a)) and np.array_equal(la, lb)            # labels unchanged
        assert nv.sample_path(idx) == rgb.sample_path(idx)
    w_rgb, w_nv = SyntheticVideo(window=3, **kw), SyntheticVideo(window=3, frame_format="nv12", yuv_matrix="bt709",
                                                                 yuv_range="full", **kw)
    assert w_nv[1][0].shape == (3, 54, 50) and np.array_equal(w_nv[1][0], V.rgb_to_nv12(w_rgb[1][0], "bt709", "full"))
    d_rgb, d_nv = SyntheticDetection(num_samples=3, size=(50, 36), window=3), \
        SyntheticDetection(num_samples=3, size=(50, 36), window=3, frame_format="nv12")
    assert np.array_equal(d_nv[2][0], V.rgb_to_nv12(d_rgb[2][0])) and np.array_equal(d_nv[2][1], d_rgb[2][1])
    with pytest.raises(ValueError, match="frame_format 'yuv420' is neither"):
        SyntheticDetection(frame_format="yuv420")
    with pytest.raises(ValueError, match="NV12: unknown matrix / range"):
        SyntheticDetection(frame_format="nv12", yuv_matrix="bt2020")
    with pytest.raises(ValueError, match="NV12 needs an even frame size"):
        SyntheticDetection(size=(51, 36), frame_format="nv12")[0]


def test_transform_returns_nv12_frames_untouched_and_the_loader_collates_them():
    from viddet_amd.data import Loader, SyntheticDetection, YOLO3VideoInferenceTransform
    rng = np.random.default_rng(3)
    label = np.array([[5., 6., 40., 30., 1., 0.], [10., 2., 60., 44., 0., 0.]])
    on = YOLO3VideoInferenceTransform(64, 32, device_normalize=True, device_resize=True, frame_format="nv12")
    rgb = YOLO3VideoInferenceTransform(64, 32, device_normalize=True, device_resize=True)
    for lead in ((), (3,)):
        img = rng.integers(0, 256, lead + (75, 70), dtype=np.uint8)                      # H0 = 50, W0 = 70
        x, bb, idx = on(img, label, 7)
        assert x.dtype == np.uint8 and x.shape == img.shape and x.tobytes() == img.tobytes() and idx == 7
        _, bb0, _ = rgb(np.zeros(lead + (50, 70, 3), np.uint8), label, 7)                # boxes resized from (50, 70)
        assert bb.dtype == bb0.dtype and np.array_equal(bb, bb0)
    with pytest.raises(ValueError, match="frame_format='nv12' needs device_resize=True"):
        YOLO3VideoInferenceTransform(64, 64, device_normalize=True, frame_format="nv12")
    with pytest.raises(ValueError, match="frame_format 'i420' is neither"):
        YOLO3VideoInferenceTransform(64, 64, device_normalize=True, device_resize=True, frame_format="i420")
    with pytest.raises(ValueError, match="NV12 frames are"):
        on(np.zeros((76, 70), np.uint8), label)
    ds = SyntheticDetection(num_samples=4, size=(50, 36), window=3, frame_format="nv12")
    batches = list(Loader(ds, on, 2, train=False, last_batch="keep"))
    assert len(batches) == 2 and batches[0][0].shape == (2, 3, 54, 50) and batches[0][0].dtype == np.uint8
    assert np.array_equal(batches[1][0][1], ds[3][0]) and list(batches[1][2]) == [2, 3]


# ------------------------------------------------------------------------------------------------ script
BASE = ["--random_init", "--data_shape", "64"]


def test_detect_script_flags_and_refusals_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    F = D.parse_flags([])
    assert F.frame_format == "rgb" and F.yuv_matrix == "bt601" and F.yuv_range == "limited" and F.device_resize is False
    F = D.parse_flags(["--frame_format", "nv12", "--yuv_matrix", "bt709", "--yuv_range", "full"])
    assert (F.frame_format, F.yuv_matrix, F.yuv_range) == ("nv12", "bt709", "full")
    with pytest.raises(SystemExit):
        D.parse_flags(["--frame_format", "i420"])
    with pytest.raises(NotImplementedError, match="--frame_format nv12 needs --device_resize"):
        D.main(BASE + ["--frame_format", "nv12"])
    with pytest.raises(NotImplementedError, match="--frame_format nv12 does not combine with several --dataset"):
        D.main(BASE + ["--frame_format", "nv12", "--device_resize", "--dataset", "voc,coco"])
    join = ["--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early"]
    for extra in (["--dataset", "voc"], ["--dataset", "vid", "--stream"] + join, ["--dataset", "vid", "--precision", "bf16"] + join,
                  ["--dataset", "vid", "--stream", "--model_agnostic", "--window", "3,1", "--k_join_type", "cat", "--k_join_pos", "late"]):
        with pytest.raises(SystemExit):                                     # accepted up to the GPU check
            D.main(BASE + ["--frame_format", "nv12", "--device_resize"] + extra)


# ------------------------------------------------------------------------------------------------ network
def test_set_device_resize_nv12_refusals_before_any_gpu_work():
    import torch
    from viddet_amd.model import yolo3_darknet53, yolo3_no_backbone
    net = yolo3_darknet53(CLASSES, device="cpu")
    # RGB semantics are unchanged
    net.set_device_resize(64)
    assert net._dev_resize == (64, 64, 9) and net._dev_nv12 is None
    assert net._in_shape(torch.zeros(2, 50, 70, 3, dtype=torch.uint8)) == (2, 64, 64)
    net.set_device_resize(None)
    assert net._dev_resize is None and net._dev_nv12 is None
    with pytest.raises(NotImplementedError, match="set_device_resize with noback"):
        yolo3_no_backbone(CLASSES, device="cpu").set_device_resize(64, 64, source="nv12")
    for kw in (dict(matrix="bt2020"), dict(range="studio")):
        with pytest.raises(ValueError, match="set_device_resize: NV12: unknown matrix / range"):
            net.set_device_resize(64, 64, source="nv12", **kw)
    with pytest.raises(ValueError, match="set_device_resize: source 'yuv' is neither"):
        net.set_device_resize(64, 64, source="yuv")
    assert net._dev_resize is None and net._dev_nv12 is None
    net.set_device_resize(64, 96, source="nv12", matrix="bt709", range="full")
    assert net._dev_resize == (96, 64, 9) and net._dev_nv12 == V.NV12_MATRICES[("bt709", "full")]
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"source='nv12'\) is on: the network takes NV12 frames, uint8 .* got a float32 tensor"):
        net(torch.zeros(2, 54, 50))
    with pytest.raises(ValueError, match="got a float32 tensor"):
        net.detect_video(torch.zeros(4, 3, 96, 64))
    with pytest.raises(ValueError, match=r"NV12 frames are .* got 52 rows \(H0 = 52\*2/3\) of W0 = 50"):
        net(u8(2, 52, 50))
    with pytest.raises(ValueError, match=r"NV12 frames are .* got 54 rows \(H0 = 36\) of W0 = 51"):
        net(u8(2, 54, 51))
    with pytest.raises(ValueError, match=r"got packed RGB frames \(2, 36, 50, 3\)"):
        net(u8(2, 36, 50, 3))
    with pytest.raises(ValueError, match=r"expected an NV12 clip \(T,H0\*3/2,W0\) uint8, got \(4, 36, 50, 3\)"):
        net.detect_video(u8(4, 36, 50, 3))
    with pytest.raises(ValueError, match=r"expected NV12 frames \(B,H0\*3/2,W0\), got \(2, 3, 54, 50\)"):
        net(u8(2, 3, 54, 50))
    with pytest.raises(ValueError, match="set_device_resize: a 1920x1280 -> 96x64 resize has Ty=21 / Tx=21"):
        net(u8(1, 2880, 1280))
    assert not net._programs
    assert net._in_shape(u8(2, 54, 50)) == (2, 96, 64) and net._in_shape(u8(2, 3, 54, 50)) == (2, 96, 64)
    assert net._in_shape(u8(2, 144, 64)) == (2, 96, 64)                    # already at the target size: identity tables
    assert set(net._resize_cache) == {(50, 70, 64, 64, 9), (36, 50, 96, 64, 9), (96, 64, 96, 64, "identity")}   # (the first: the RGB call above)
    t = net._resize_cache[(96, 64, 96, 64, "identity")]
    assert t["dev"] is None and t["host"][0].shape == (96, 1) and t["host"][2].shape == (64, 1)
    # switching back restores RGB behaviour; off clears both
    net.set_device_resize(64, 96)
    assert net._dev_nv12 is None and net._in_shape(u8(2, 50, 70, 3)) == (2, 96, 64)
    net.set_device_resize(64, 96, source="nv12")
    net.set_device_resize(None)
    assert net._dev_resize is None and net._dev_nv12 is None and net._in_shape(u8(2, 50, 70, 3)) == (2, 50, 70)


# ------------------------------------------------------------------------------------------------ library
def test_library_declares_the_nv12_resize():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # an entry point was only added
    assert callable(lib.vd_resize_nv12_nchw) and len(L.SIGNATURES["vd_resize_nv12_nchw"][1]) == 26
    assert len(L.SIGNATURES["vd_resize_u8_nchw"][1]) == 15                 # the RGB entry point's argument list is untouched


def test_nv12_resize_checks_its_arguments_before_any_launch():
    from viddet_amd import lib as L
    lib = L.load()
    P = 4096                                                               # an aligned, never dereferenced address
    h0, w0, hn = 34, 50, 51
    good = dict(in_=P, in_bytes=2 * hn * w0, fs=hn * w0, pitch=w0, uv=h0 * w0, out=P, N=2, H0=h0, W0=w0, H=32, W=32, iy=P, wy=P, Ty=3,
                ix=P, wx=P, Tx=4)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_resize_nv12_nchw(a['in_'], a['in_bytes'], a['fs'], a['pitch'], a['uv'], a['out'], None, a['N'], a['H0'], a['W0'],
                                     a['H'], a['W'], a['iy'], a['wy'], a['Ty'], a['ix'], a['wx'], a['Tx'],
                                     *V.NV12_MATRICES[("bt601", "limited")], None)
        return rc, lib.vd_last_error()

    bad = [dict(in_=None), dict(out=None), dict(iy=None), dict(wy=None), dict(ix=None), dict(wx=None),
           dict(N=0), dict(H0=0), dict(W0=-2), dict(H=0), dict(W=0), dict(H0=33), dict(W0=49), dict(pitch=w0 - 1),
           dict(uv=h0 * w0 - 1), dict(fs=hn * w0 - 1), dict(in_bytes=2 * hn * w0 - 1),
           dict(Tx=17), dict(Ty=17), dict(Tx=0), dict(Ty=-1), dict(iy=P + 2), dict(wx=P + 1), dict(out=P + 2),
           # one tile's source columns do not fit in LDS
           dict(W0=70000, pitch=70000, uv=70000 * h0, fs=70000 * hn, in_bytes=2 * 70000 * hn, Tx=2)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_resize_nv12_nchw:"), (kw, err)
    assert b"Tx=17" in call(Tx=17)[1] and b"even" in call(W0=49)[1] and b"pitch=49" in call(pitch=w0 - 1)[1]
    assert b"uv_offset=1699" in call(uv=h0 * w0 - 1)[1] and b"frame_stride=2549" in call(fs=hn * w0 - 1)[1]
    assert b"in_bytes=5099" in call(in_bytes=2 * hn * w0 - 1)[1] and b"LDS" in call(**bad[-1])[1]


def test_shipped_tuning_table_is_still_the_one_that_is_found(monkeypatch):
    import os
    from viddet_amd import model as M
    monkeypatch.delenv("VD_TUNE_CACHE", raising=False)
    monkeypatch.delenv("VD_WGRAD_RESERVE", raising=False)
    p = M._TUNE_CACHE.path()
    assert os.path.basename(p) == "gfx950_d345f7eebb9a.json" and os.path.exists(p)
