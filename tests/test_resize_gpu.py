"""GPU: raw uint8 frames resized on the device (vd_resize.hip, YOLOV3.set_device_resize).

Kernel: vd_resize_u8_nchw against video.imresize on uint8.  With v the fp64 value of the resample before rounding (from
_axis_taps), the kernel's fp32 sums are within
    delta = 2^-23 * 255 * (Ty + Tx + 2) * max_rows sum|w_y| * max_cols sum|w_x|
of v (the rounding of the weights to fp32 plus the Ty + Tx fused adds, a factor 2 in hand), so the rounded grey level must
EQUAL imresize's wherever v is further than delta from a rounding tie, and differ by at most one level inside that band.
More than 99 % of a random frame's pixels must be held to equality, so that arm is not vacuous.  One case cannot meet that
through the band alone: (40, 24) -> (32, 32) is bilinear with scales 5/4 and 3/4, all of its weights are multiples of 1/8, so
v is a multiple of 1/64 and 1/64 of all pixels (measured on the CPU: 2.3 % of the random frame, 9.4 % of the ramp) are EXACT
ties, whatever the frame.  There, though, fp32 makes no error at all: 8 bits of grey level + 3 + 3 fractional bits fit the
24-bit significand, every product and partial sum is exact, the kernel's value IS v and rintf and np.rint both round half to
even.  Where the weights are such dyadic fractions (_exact_in_fp32) the test therefore holds every pixel, ties included, to
equality - more than the band asks - and the 99 % is counted over the pixels held to equality.
`out` is bit-equal to vd_preprocess_u8_nchw of `out_u8`, with or without out_u8, twice, and the source is not written.
Network: with the switch on, net(raw) is bit-identical to net(kernel's own resized frames) with it off - the device-resize
path differs from the existing one by the resample alone - for fp32 and bf16, k = 1 and k = 3, and through detect_video.
Script: detect_yolo3.py --device_resize, plain and --stream.
"""
import os

import numpy as np
import pytest
import torch

from oracle import yolo as Y
from viddet_amd import video as V

pytestmark = pytest.mark.gpu

# (H0, W0) -> (H, W): area; bicubic; mixed -> bilinear; a non-integer area scale with the tile border inside the frame;
# a strong shrink (12 taps per axis, the tile's row count cut to fit); one output tile wider than the source
PAIRS = [((50, 70), (32, 32), 2), ((20, 24), (32, 64), 3), ((40, 24), (32, 32), 1), ((97, 131), (32, 64), 2),
         ((330, 330), (32, 32), 2), ((3, 5), (32, 32), 3)]


def _tables(h0, w0, h, w):
    used, iy, wy, ix, wx = V.resize_tables(h0, w0, h, w, 9)
    return used, [torch.from_numpy(a).cuda() for a in (iy, wy, ix, wx)]


def _resize(x, h, w, tabs, want_u8=True):
    """vd_resize_u8_nchw on the device tensor x (N,H0,W0,3) -> (out, out_u8 | None)"""
    from viddet_amd import lib as L
    n, h0, w0, _ = x.shape
    iy, wy, ix, wx = tabs
    out = torch.full((n, 3, h, w), float("nan"), device="cuda")
    u8 = torch.full((n, h, w, 3), 77, dtype=torch.uint8, device="cuda") if want_u8 else None
    L.check(L.load().vd_resize_u8_nchw(x.data_ptr(), out.data_ptr(), u8.data_ptr() if want_u8 else None, n, h0, w0, h, w,
                                       iy.data_ptr(), wy.data_ptr(), iy.shape[1], ix.data_ptr(), wx.data_ptr(), ix.shape[1],
                                       L.stream_ptr()), "vd_resize_u8_nchw")
    return out, u8


def _preprocess(u8):
    from viddet_amd import lib as L
    n, h, w, _ = u8.shape
    out = torch.full((n, 3, h, w), float("nan"), device="cuda")
    L.check(L.load().vd_preprocess_u8_nchw(u8.data_ptr(), out.data_ptr(), n, h, w, L.stream_ptr()), "vd_preprocess_u8_nchw")
    return out


def _exact_in_fp32(wy, wx):
    """True where both weight tables are dyadic fractions k / 2^f with 8 + fy + fx <= 24 bits: the fp32 sums of grey levels
    are then exact (no product or partial sum needs more than the significand holds)"""
    def frac_bits(w):
        for f in range(13):
            if np.array_equal(w * 2.0 ** f, np.rint(w * 2.0 ** f)):
                return f
        return None
    fy, fx = frac_bits(wy), frac_bits(wx)
    return fy is not None and fx is not None and 8 + fy + fx <= 24


def _inputs(h0, w0):
    """two launches of N = 2: (random, horizontal ramp) and (constant 255, constant 0)"""
    rng = np.random.default_rng(1000 * h0 + w0)
    ramp = np.broadcast_to((np.arange(w0) * 255 // max(1, w0 - 1)).astype(np.uint8)[None, :, None], (h0, w0, 3))
    return [np.stack([rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8), ramp]),
            np.stack([np.full((h0, w0, 3), 255, np.uint8), np.zeros((h0, w0, 3), np.uint8)])]


@pytest.mark.parametrize("src,dst,interp", PAIRS, ids=["%dx%d-%dx%d" % (a + b) for a, b, _ in PAIRS])
def test_kernel_against_imresize(src, dst, interp):
    (h0, w0), (h, w) = src, dst
    used, tabs = _tables(h0, w0, h, w)
    assert used == interp
    (iy, wy), (ix, wx) = V._axis_taps(h0, h, used), V._axis_taps(w0, w, used)
    Ty, Tx = iy.shape[1], ix.shape[1]
    delta = 2.0 ** -23 * 255 * (Ty + Tx + 2) * np.abs(wy).sum(axis=1).max() * np.abs(wx).sum(axis=1).max()
    exact = _exact_in_fp32(wy, wx)
    assert exact == (src == (40, 24))
    for li, frames in enumerate(_inputs(h0, w0)):
        # the source sits one byte into its allocation: rows start at every phase of a dword, the first dword of the buffer
        # is put together from bytes
        store = torch.zeros(frames.size + 8, dtype=torch.uint8, device="cuda")
        x = store[1:1 + frames.size].view(frames.shape)
        x.copy_(torch.from_numpy(frames))
        keep = store.clone()
        out, u8 = _resize(x, h, w, tabs)
        out_b, _ = _resize(x, h, w, tabs, want_u8=False)
        out_c, u8_c = _resize(x, h, w, tabs)
        out_d, u8_d = _resize(torch.from_numpy(frames).cuda(), h, w, tabs)                # an aligned copy
        torch.cuda.synchronize()
        assert torch.equal(store, keep), "the source buffer was written"
        assert not bool(torch.isnan(out).any())
        assert torch.equal(out, _preprocess(u8)), "out is not vd_preprocess_u8_nchw(out_u8), bit for bit"
        assert torch.equal(out, out_b), "out_u8 = NULL changes out"
        assert torch.equal(out, out_c) and torch.equal(u8, u8_c), "two runs differ"
        assert torch.equal(out, out_d) and torch.equal(u8, u8_d), "the source's alignment changes the result"
        got = u8.cpu().numpy().astype(np.int64)
        for n in range(2):
            f64 = frames[n].astype(np.float64)
            v = V._resample_axis(V._resample_axis(f64, 1, ix, wx), 0, iy, wy)             # fp64, before rounding
            ref = V.imresize(frames[n], w, h, interp=9).astype(np.int64)
            outside = np.abs(v - np.floor(v) - 0.5) > delta
            # (imresize itself against v: both arms hold by construction)
            assert np.array_equal(ref[outside], np.clip(np.rint(v), 0, 255).astype(np.int64)[outside])
            d = np.abs(got[n] - ref)
            print("%s -> %s launch %d frame %d: Ty=%d Tx=%d delta=%.2e, %.3f%% of pixels in the tie band, %d differ from imresize"
                  % (src, dst, li, n, Ty, Tx, delta, 100.0 * (1 - outside.mean()), int((d > 0).sum())))
            assert np.array_equal(got[n][outside], ref[outside]), "a grey level outside the tie band differs from imresize"
            assert d.max() <= 1
            held = np.ones_like(outside) if exact else outside                            # pixels held to equality
            assert np.array_equal(got[n][held], ref[held]), "fp32 is exact on these weights, yet a grey level differs"
            if li == 0 and n == 0:                                                        # the random frame
                assert held.mean() > 0.99, "the exact-equality arm is (almost) vacuous"
        if li == 1:
            assert bool((u8[0] == 255).all()) and bool((u8[1] == 0).all())


# ------------------------------------------------------------------------------------------------ network
C, SIZE, RAW = 3, 64, (50, 70)


@pytest.fixture(scope="module")
def nets():
    from viddet_amd.model import yolo3_darknet53
    out = {}
    for k in (1, 3):
        kw = dict(k=3, k_join_type="max", k_join_pos="early") if k == 3 else {}
        net = yolo3_darknet53(["c%d" % i for i in range(C)], **kw)
        net.initialize(init="he", seed=7 + k, obj_bias=0.0)
        out[k] = net
    return out


def _resized_by_the_kernel(raw):
    """the kernel's own resized uint8 frames of raw (..., H0, W0, 3), in raw's leading shape"""
    _, tabs = _tables(RAW[0], RAW[1], SIZE, SIZE)
    flat = torch.from_numpy(raw.reshape((-1,) + raw.shape[-3:])).cuda()
    _, u8 = _resize(flat, SIZE, SIZE, tabs)
    return u8.view(raw.shape[:-3] + (SIZE, SIZE, 3))


def _outputs(net, res):
    torch.cuda.synchronize()
    return [t.clone() for t in res] + [net.last_rows.clone()]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("k", [1, 3])
def test_net_on_raw_frames_equals_net_on_the_kernels_resized_frames(nets, k, precision):
    net = nets[k]
    net.set_precision(precision)
    raw = np.random.default_rng(5 * k).integers(0, 256, ((2, 3) if k == 3 else (2,)) + RAW + (3,), dtype=np.uint8)
    pre = _resized_by_the_kernel(raw)
    try:
        net.set_device_resize(None)
        want = _outputs(net, net(pre))
        key = ('infer_bf16' if precision == 'bf16' else 'infer', 2, SIZE, SIZE)
        prog = net._programs[key]
        net.set_device_resize(SIZE, SIZE)
        got = _outputs(net, net(torch.from_numpy(raw).cuda()))
        assert net._programs[key] is prog and (RAW[0], RAW[1], SIZE, SIZE, 9) in net._resize_cache
        same = _outputs(net, net(pre))                                # a source the size of the target: no resample
        with pytest.raises(ValueError, match="set_device_resize is on"):
            net(torch.zeros((2, 3, 3, SIZE, SIZE) if k == 3 else (2, 3, SIZE, SIZE), device="cuda"))
        net.set_device_resize(None)
        after = _outputs(net, net(pre))
        assert net._programs[key] is prog, "the switch rebuilt the plan"
    finally:
        net.set_device_resize(None)
        net.set_precision("fp32")
    assert int((want[0] >= 0).sum()) > 4, "fixture produced (almost) no detections"
    for name, a, b, c, d in zip(("ids", "scores", "bboxes", "last_rows"), want, got, same, after):
        assert torch.equal(a, b), "%s: net(raw) differs from net(resized by the kernel)" % name
        assert torch.equal(a, c), "%s: a source of the target's size differs from the switch off" % name
        assert torch.equal(a, d), "%s: differs after set_device_resize(None)" % name


def test_detect_video_on_a_raw_clip(nets):
    net = nets[3]
    raw = np.random.default_rng(11).integers(0, 256, (7,) + RAW + (3,), dtype=np.uint8)
    pre = _resized_by_the_kernel(raw)
    try:
        net.set_device_resize(None)
        want = _outputs(net, net.detect_video(pre.cpu(), step=1, chunk=3))
        net.set_device_resize(SIZE, SIZE)
        got = _outputs(net, net.detect_video(torch.from_numpy(raw), step=1, chunk=3))        # uploaded chunk by chunk
        stats = dict(net.stream_stats)
    finally:
        net.set_device_resize(None)
    assert stats['prefix_frames'] == 7 and stats['suffix_frames'] == 7 and stats['chunks'] == 3
    assert int((want[0] >= 0).sum()) > 7
    for name, a, b in zip(("ids", "scores", "bboxes", "last_rows"), want, got):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ script
@pytest.mark.parametrize("extra", [[], ["--stream", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early"]],
                         ids=["batched", "stream"])
def test_detect_script_device_resize(tmp_path, capsys, extra):
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticDetection, SyntheticVideo, YOLO3VideoInferenceTransform
    out = D.main(["--random_init", "--dataset", "voc", "--data_shape", "64", "--batch_size", "4", "--synthetic_samples", "8",
                  "--device_resize", "--metrics", "voc", "--save_dir", str(tmp_path), "--save_prefix", "r"] + extra)
    ds = SyntheticVideo("voc", num_videos=2, frames_per_video=8, window=3, step=1) if extra else SyntheticDetection("voc", num_samples=8)
    pred = tmp_path / "r" / "pred"
    assert len(os.listdir(pred)) == len(ds)                                  # one prediction file per image
    preds = D.load_predictions(str(pred), ds)
    rows = np.array([b for v in preds.values() for b in v], dtype=np.float64).reshape(-1, 6)
    assert len(rows) > 10, "fixture produced (almost) no detections"
    assert rows[:, 2:6].min() >= 0.0 and rows[:, 2:6].max() <= 1.0           # boxes are divided by --data_shape
    metric = Y.VOCMApMetric(iou_thresh=0.5, class_names=ds.classes)
    tf = YOLO3VideoInferenceTransform(64, 64)
    for idx in range(len(ds)):
        img, label = ds[idx]
        _, gt, _ = tf(img, label, idx)
        p = np.asarray(preds.get(ds.sample_path(idx), np.zeros((0, 6))), dtype=np.float64).reshape(-1, 6)
        metric.update([p[:, 2:6]], [p[:, 0]], [p[:, 1]], [gt[:, :4] / 64], [gt[:, 4]], [gt[:, 5]])
    _, map_r = metric.get()
    names, values = out
    printed = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("mAP=")]
    assert len(printed) == 1
    assert np.isclose(float(printed[0].split("=")[1]), map_r, rtol=0, atol=1e-4, equal_nan=True)      # printed with 4 decimals
    assert np.isclose(values[-1], map_r, rtol=0, atol=1e-6, equal_nan=True)
