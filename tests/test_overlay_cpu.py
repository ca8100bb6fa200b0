"""The overlay's definition (viddet_amd/overlay.py) held to independent forms on the CPU: the loop painter of
tests/overlay_loop.py, PIL's rectangle outline, a float64 point-to-segment distance, '%.2f', glyphs written out here; its
symmetries and edge cases; the library's exports and argument refusals; the script's flags."""
import numpy as np
import pytest

from tests import overlay_cases as OC
from tests.overlay_loop import overlay_loop
from viddet_amd import overlay as O
from viddet_amd.video import nv12_to_rgb, rgb_to_nv12


@pytest.mark.parametrize("name", sorted(OC.CASES))
@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_host_equals_the_loop_painter(name, fmt):
    c = OC.case(name)
    frames = c["frames"] if fmt == "rgb" else rgb_to_nv12(OC.even(c["frames"]))
    args, kw = OC.call_args(c, fmt)
    out, painted = O.overlay_host(frames, *args, **kw)
    ref, ref_painted = overlay_loop(frames, *args, **kw)
    assert out.dtype == np.uint8 and out.shape == frames.shape and painted.dtype == np.int32
    assert np.array_equal(out, ref)
    assert np.array_equal(painted, ref_painted) and painted.sum() > 0


def _grid(h, w):
    return np.arange(w)[None, :], np.arange(h)[:, None]


def test_rings_equal_pil_rectangles():
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    X, Y = _grid(40, 56)
    n = 0
    for _ in range(400):
        t = int(rng.integers(1, 6))
        x0, y0 = int(rng.integers(0, 40)), int(rng.integers(0, 28))
        x1, y1 = x0 + int(rng.integers(0, 30)), y0 + int(rng.integers(0, 24))
        x1, y1 = min(x1, 55), min(y1, 39)
        if x1 - x0 + 1 < 2 * t or y1 - y0 + 1 < 2 * t:           # both sides >= 2 t pixels: smaller boxes come out filled here
            continue
        img = Image.new("L", (56, 40), 0)
        ImageDraw.Draw(img).rectangle([x0, y0, x1, y1], outline=255, width=t)
        assert np.array_equal(O.on_ring(X, Y, (x0, y0, x1, y1), t), np.asarray(img) > 0), (x0, y0, x1, y1, t)
        n += 1
    assert n > 100


def test_segment_agrees_with_a_float64_distance():
    rng = np.random.default_rng(1)
    X, Y = _grid(48, 48)
    for _ in range(200):
        t = int(rng.integers(1, 9))
        a, b = rng.integers(0, 48, 2), rng.integers(0, 48, 2)
        if (a == b).all():
            assert not O.on_segment(X, Y, a, b, t).any()          # a zero-length segment holds nothing
            continue
        d = (b - a).astype(np.float64)
        vx, vy = X - float(a[0]), Y - float(a[1])
        u = (vx * d[0] + vy * d[1]) / (d @ d)
        dist = np.abs(vx * d[1] - vy * d[0]) / np.sqrt(d @ d)
        want = (u >= 0) & (u <= 1) & (dist <= t / 2)
        sure = np.abs(dist - t / 2) > 1e-6
        got = O.on_segment(X, Y, a, b, t)
        assert np.array_equal(got[sure], want[sure])


def test_axis_aligned_segments_are_rectangles_and_the_mask_follows_transposes_and_mirrors():
    X, Y = _grid(32, 32)
    for t in range(1, 9):
        got = O.on_segment(X, Y, (5, 10), (20, 10), t)
        want = (X >= 5) & (X <= 20) & (2 * np.abs(Y - 10) <= t)
        assert np.array_equal(got, want)
        assert np.array_equal(O.on_segment(X, Y, (10, 5), (10, 20), t), want.T)
    rng = np.random.default_rng(2)
    for _ in range(50):
        t = int(rng.integers(1, 9))
        a, b = rng.integers(0, 32, 2), rng.integers(0, 32, 2)
        m = O.on_segment(X, Y, a, b, t)
        assert np.array_equal(O.on_segment(X, Y, a[::-1], b[::-1], t), m.T)
        assert np.array_equal(O.on_segment(X, Y, (31 - a[0], a[1]), (31 - b[0], b[1]), t), m[:, ::-1])
        assert np.array_equal(O.on_segment(X, Y, (a[0], 31 - a[1]), (b[0], 31 - b[1]), t), m[::-1])
        assert np.array_equal(O.on_segment(X, Y, b, a, t), m)
        box = (min(a[0], b[0]), min(a[1], b[1]), max(a[0], b[0]), max(a[1], b[1]))
        r = O.on_ring(X, Y, box, t)
        assert np.array_equal(O.on_ring(X, Y, (box[1], box[0], box[3], box[2]), t), r.T)
        assert np.array_equal(O.on_ring(X, Y, (31 - box[2], box[1], 31 - box[0], box[3]), t), r[:, ::-1])


def test_label_text_prints_the_score_as_percent_2f():
    for k in range(100):
        s = np.float32(k / 100 + 0.003)
        assert O.label_text(3, s) == b"3 " + ("%.2f" % s).encode()
    assert O.label_text(2, 0.5, 17, ("a", "b", "cat")) == b"#17 cat 0.50"
    assert O.label_text(5, 0.5, -1, ("a", "b", "cat")) == b"5 0.50"          # beyond the table: the decimal id
    assert O.label_text(1, None, None, ("a", "bird")) == b"bird"              # ground truth: the name alone
    assert O.label_text(0, 123.0) == b"0 9.99" and O.label_text(0, -1.0) == b"0 0.00"
    long = O.label_text(0, 0.25, 2147483647, ("a" * 15,))
    assert long == b"#2147483647 " + b"a" * 15 + b" 0.25" and len(long) == 32
    assert len(O.label_text(0, 0.25, 2147483647, None)) == 18


GLYPHS = {
    "A": [".###.", "#...#", "#...#", "#...#", "#####", "#...#", "#...#"],
    "8": [".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."],
    "#": [".#.#.", ".#.#.", "#####", ".#.#.", "#####", ".#.#.", ".#.#."],
}


@pytest.mark.parametrize("ch", sorted(GLYPHS))
def test_a_glyph_equals_its_pattern_and_scale_repeats_pixels(ch):
    assert O.FONT_5X7.shape == (95, 7) and O.FONT_5X7.dtype == np.uint8 and int(O.FONT_5X7.max()) < 32
    want = np.array([[c == "#" for c in row] for row in GLYPHS[ch]])
    text = ch.encode()
    tag = O.tag_box(3, 20, 1, 1)
    assert tag == (3, 11, 9, 19)                                  # 6 + 1 wide, 9 high, above the box
    X, Y = _grid(32, 32)
    one = O.glyph_pixel(X, Y, tag, text, 1) & O.in_tag(X, Y, tag)
    assert np.array_equal(one[12:19, 4:9], want) and one.sum() == want.sum()
    for s in (2, 3, 4):
        tag_s = O.tag_box(0, 0, 1, s)
        assert tag_s == (0, 0, 7 * s - 1, 9 * s - 1)              # no room above: the tag starts at the box's top
        Xs, Ys = _grid(9 * s, 7 * s)
        big = O.glyph_pixel(Xs, Ys, tag_s, text, s)
        tag_1 = O.tag_box(0, 0, 1, 1)
        X1, Y1 = _grid(9, 7)
        small = O.glyph_pixel(X1, Y1, tag_1, text, 1)
        assert np.array_equal(big, np.repeat(np.repeat(small, s, axis=0), s, axis=1))


def test_nv12_result_converts_to_the_rgb_result_on_whole_blocks():
    """On frames that are nv12_to_rgb of the source, at every pixel whose 2 x 2 block is all painted (in one colour: the block
    has one chroma pair) or all untouched: the NV12 result, converted, is the RGB result - a painted colour having gone
    through the NV12 round trip once, as the palette of NV12 frames has."""
    c = OC.case("rgb_L3")
    nv = rgb_to_nv12(c["frames"])
    rgb = nv12_to_rgb(nv)
    args, kw = OC.call_args(c)
    out_nv, p_nv = O.overlay_host(nv, *args, fmt="nv12", **kw)
    out_rgb, p_rgb = O.overlay_host(rgb, *args, **kw)
    assert np.array_equal(p_nv, p_rgb)
    rec, rec_gt = O.overlay_records(*args, kw["track"], kw["gt"], kw["clip_start"], size=rgb.shape[1:3], **c["params"])
    n = 0
    for f in range(rgb.shape[0]):
        idx = O.resolve_records(rec[f], rec_gt[f], rgb.shape[1:3], c["params"].get("thickness", 2), c["params"].get("scale", 1))
        on = (idx >= 0).reshape(idx.shape[0] // 2, 2, idx.shape[1] // 2, 2)
        whole = on.all(axis=(1, 3)) | ~on.any(axis=(1, 3))
        # an all-painted block must also be of one colour for its one chroma pair to stand for all four pixels
        same = (idx.reshape(on.shape) == idx[0::2, 0::2][:, None, :, None]).all(axis=(1, 3))
        ok = np.repeat(np.repeat(whole & same, 2, axis=0), 2, axis=1)
        want = nv12_to_rgb(rgb_to_nv12(out_rgb[f]))               # a painted colour goes through the NV12 round trip once
        want = np.where((idx >= 0)[..., None], want, rgb[f])
        assert np.array_equal(nv12_to_rgb(out_nv[f])[ok], want[ok])
        n += int(ok.sum())
    assert n > 1000 and p_nv.sum() > 0


def _one(frames, rows, **kw):
    """rows: [(class, score, box, track)] of ONE frame -> overlay_host on it"""
    ids = np.array([[r[0] for r in rows]], np.float32)
    sc = np.array([[r[1] for r in rows]], np.float32)
    bb = np.array([[r[2] for r in rows]], np.float32)
    tr = np.array([[r[3] for r in rows]], np.int32)
    return O.overlay_host(frames, ids, sc, bb, tr, **kw)


def test_layer_order_tag_over_ring_over_trail_over_ground_truth():
    pal = O.default_palette()
    F = np.full((2, 64, 64, 3), 7, np.uint8)                      # a background that is no colour of the picture
    # row 1's tag (above its box at y 30) crosses row 0's ring; row 0's ring crosses row 1's trail; the trail crosses a gt ring
    ids = np.array([[0, 1], [0, 1]], np.float32)[..., None]
    sc = np.full((2, 2, 1), 0.9, np.float32)
    bb = np.array([[[50, 50, 60, 60], [2, 40, 20, 60]], [[10, 10, 40, 27], [30, 30, 60, 60]]], np.float32)
    tr = np.array([[5, 9], [5, 9]], np.int32)
    gt = np.array([[[0, 0, 1, 1, -1]], [[20, 35, 50, 62, 0]]], np.float32)
    out, painted = O.overlay_host(F, ids, sc, bb, tr, gt, thickness=2, trail=1, color_by="class")
    f = out[1]
    c0, c1, green = tuple(pal[0]), tuple(pal[1]), (0, 255, 0)
    assert tuple(f[26, 30]) in (c1, (0, 0, 0), (255, 255, 255))   # row 1's tag (y 21..29 from x 30) lies over row 0's ring (y 26, 27)
    assert tuple(f[26, 12]) == c0                                 # row 0's ring where no tag is
    # row 1's trail runs from its centre (45, 45) to (11, 50) of frame 0; the gt ring's left edge x 20, 21 crosses it
    assert tuple(f[48, 25]) == c1 and tuple(f[48, 20]) == c1      # trail over ground truth
    assert tuple(f[40, 20]) == green and tuple(f[62, 30]) == green
    # row 0's trail from (25, 18) to (55, 55) passes under row 1's ring at its top-left corner (30, 30) .. : the ring wins
    assert tuple(f[30, 35]) == c1
    assert painted[1] == (f != 7).any(-1).sum() and painted[0] == (out[0] != 7).any(-1).sum() > 0


def test_tag_flips_inside_at_the_top_edge_and_is_cut_at_the_frames_edges():
    F = np.zeros((1, 40, 40, 3), np.uint8)
    out, painted = _one(F, [(0, 0.9, (30, 3, 39, 20), -1)], thickness=1)
    assert O.tag_box(30, 3, 6, 1) == (30, 3, 66, 11)
    assert (out[0, 3:12, 30:40] != 0).any(-1).all()               # the tag's background, inside the box, cut at x = 39
    assert not (out[0, :3] != 0).any()
    out, _ = _one(F, [(0, 0.9, (5, 9, 20, 20), -1)], thickness=1)
    assert (out[0, 0:9, 5:20] != 0).any(-1).all() and O.tag_box(5, 9, 6, 1)[1] == 0


def test_threshold_nan_and_negative_ids():
    F = np.zeros((1, 40, 40, 3), np.uint8)
    box = (5, 15, 20, 30)
    th = np.float32(0.3)
    assert _one(F, [(0, th, box, -1)], thresh=0.3)[1][0] > 0                          # exactly at the threshold: drawn
    assert _one(F, [(0, np.nextafter(th, np.float32(0)), box, -1)], thresh=0.3)[1][0] == 0
    assert _one(F, [(-1, 0.9, box, -1)])[1][0] == 0
    assert _one(F, [(0, 0.9, (5, np.nan, 20, 30), -1)])[1][0] == 0
    assert _one(F, [(0, 0.9, (5, 15, np.inf, 30), -1)])[1][0] == 0
    assert _one(F, [(0, 0.9, (21, 15, 20, 30), -1)])[1][0] == 0
    assert _one(F, [(0, np.nan, box, -1)])[1][0] == 0
    out, painted = _one(F.copy() + 7, [(-1, 0.9, box, -1)])
    assert (out == 7).all() and painted[0] == 0                                       # no valid row: the frame unchanged


def test_a_trail_skips_a_missing_frame_and_stops_at_a_clip_boundary():
    F_ = 5
    ids = np.zeros((F_, 2, 1), np.float32)
    sc = np.full((F_, 2, 1), 0.9, np.float32)
    bb = np.zeros((F_, 2, 4), np.float32)
    for f in range(F_):
        bb[f, 0] = [10 * f, 10, 10 * f + 8, 18]
        bb[f, 1] = [40, 30, 50, 40]
    tr = np.array([[3, -1], [3, -1], [-1, 3], [3, -1], [3, -1]], np.int32)
    tr[2] = [-1, -1]                                              # frame 2: the track is missing
    kw = dict(size=(64, 64), trail=4)
    rec, _ = O.overlay_records(ids, sc, bb, tr, **kw)
    assert rec["nv"][:, 0].tolist() == [1, 2, 0, 3, 4] and (rec["nv"][:, 1] == 0).all()
    assert rec["vx"][4, 0, :4].tolist() == [[44, 14], [34, 14], [14, 14], [4, 14]]    # newest first, frame 2 skipped
    rec, _ = O.overlay_records(ids, sc, bb, tr, clip_start=[0, 3, 5], **kw)
    assert rec["nv"][:, 0].tolist() == [1, 2, 0, 1, 2]            # frame 3 starts a clip
    rec, _ = O.overlay_records(ids, sc, bb, tr, size=(64, 64), trail=1)
    assert rec["nv"][:, 0].tolist() == [1, 2, 0, 1, 2]            # L = 1 looks one frame back, and frame 2 holds nothing
    tr[1] = [3, 3]                                                # two rows of one track: the lowest row is the vertex
    rec, _ = O.overlay_records(ids, sc, bb, tr, **kw)
    assert rec["vx"][3, 0, 1].tolist() == [14, 14]
    # an invalid row is no vertex
    sc[1, 0] = 0.1
    rec, _ = O.overlay_records(ids, sc, bb, tr, **kw)
    assert rec["vx"][3, 0, 1].tolist() == [45, 35]


def test_colour_follows_the_track_and_untracked_rows_keep_the_class_colour():
    pal = O.default_palette()
    F = np.zeros((1, 40, 40, 3), np.uint8)
    rows = [(2, 0.9, (5, 15, 20, 30), 300), (2, 0.8, (22, 15, 36, 30), -1)]
    out, _ = _one(F, rows, thickness=1, trail=0)
    assert tuple(out[0, 30, 10]) == tuple(pal[300 % 256]) and tuple(out[0, 30, 30]) == tuple(pal[2])
    out, _ = _one(F, rows, thickness=1, trail=0, color_by="class")
    assert tuple(out[0, 30, 10]) == tuple(pal[2])
    assert pal.shape == (256, 3) and len({tuple(c) for c in pal}) == 255 and (pal.sum(1) > 0).all()
    assert np.array_equal(pal, O.default_palette())               # a fixed table
    assert O.glyph_colour((255, 255, 255)) == O.COL_BLACK and O.glyph_colour((0, 0, 200)) == O.COL_WHITE


def test_parameters_are_checked_by_name():
    c = OC.case("rgb_L0")
    args, kw = OC.call_args(c)
    for bad, name in ((dict(thickness=0), "thickness"), (dict(thickness=9), "thickness"), (dict(scale=5), "scale"),
                      (dict(scale=True), "scale"), (dict(trail=17), "trail"), (dict(trail=-1), "trail"),
                      (dict(color_by="id"), "color_by"), (dict(fmt="yuv"), "fmt"), (dict(matrix="bt2020"), "matrix"),
                      (dict(class_names=["a" * 16]), "class_names"), (dict(class_names=["café"]), "class_names"),
                      (dict(palette=np.zeros((16, 3), np.uint8)), "palette"), (dict(thresh=float("nan")), "thresh")):
        with pytest.raises(ValueError, match=name):
            O.overlay_host(c["frames"], *args, **dict(kw, **bad))
    with pytest.raises(ValueError, match="at most 128"):
        O.overlay_host(np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 129)), np.zeros((1, 129)), np.zeros((1, 129, 4)))
    with pytest.raises(ValueError, match="8192"):
        O.overlay_host(np.zeros((1, 1, 8193, 3), np.uint8), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1, 4)))
    with pytest.raises(ValueError, match="even"):
        O.overlay_host(np.zeros((1, 9, 7), np.uint8), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1, 4)), fmt="nv12")
    with pytest.raises(ValueError, match="uint8"):
        O.overlay_host(np.zeros((1, 8, 8, 3), np.float32), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1, 4)))


def _declared(prefix):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "viddet_hip.h")) as f:
        return sorted(set(re.findall(r"^(?:int|int64_t)\s+(%s\w*)\(" % prefix, f.read(), re.M)))


def test_library_exports_overlay_and_checks_its_arguments_before_any_launch():
    import ctypes
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION            # entry points were added, nothing changed
    names = _declared("vd_overlay")
    assert names == ["vd_overlay", "vd_overlay_stages", "vd_overlay_ws_bytes"]
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert n in L.SIGNATURES and getattr(raw, n) is not None
    assert len(L.SIGNATURES["vd_overlay"][1]) == 34 and len(L.SIGNATURES["vd_overlay_stages"][1]) == 35
    assert L.OVERLAY_MAX_ROWS == O.MAX_ROWS == 128 and L.OVERLAY_WS_PER_ROW == O.REC_DTYPE.itemsize == 128
    assert lib.vd_overlay_ws_bytes(6, 20, 3) == 128 * 6 * 23 and lib.vd_overlay_ws_bytes(6, 20, 0) == 128 * 6 * 20
    for bad in ((0, 20, 0), (6, 0, 0), (6, 129, 0), (6, 20, 129), (6, 20, -1)):
        assert lib.vd_overlay_ws_bytes(*bad) == -1
    P = 1 << 20                                                   # an aligned, never dereferenced address
    Q = 1 << 24
    good = dict(frames=P, out=Q, frame_stride=48 * 64 * 3, pitch=64 * 3, uv_offset=0, fmt=0, F=6, H0=48, W0=64, ids=P, scores=P,
                bboxes=P, track=P, gt=P, gt_stride=6, clip_start=P, V=2, N=20, G=3, Hn=64, Wn=64, thresh=0.5, thickness=2, scale=1,
                trail=8, by_track=1, names=P, n_names=4, palette=P, font=P, painted=P, ws=P, ws_bytes=128 * 6 * 23)
    nv = dict(fmt=1, pitch=64, uv_offset=64 * 48, frame_stride=64 * 72)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vd_overlay(*a.values(), None), lib.vd_last_error()   # `good`'s keys are in the order of the arguments

    bad = [dict(frames=None), dict(out=None), dict(ids=None), dict(scores=None), dict(bboxes=None), dict(palette=None),
           dict(font=None), dict(painted=None), dict(ws=None), dict(gt=None), dict(clip_start=None), dict(N=0), dict(N=129),
           dict(G=129), dict(G=-1), dict(F=0), dict(V=0), dict(gt_stride=4), dict(thickness=0), dict(thickness=9), dict(scale=0),
           dict(scale=5), dict(trail=-1), dict(trail=17), dict(by_track=2), dict(H0=8193, frame_stride=1 << 30),
           dict(W0=8193, pitch=3 * 8193, frame_stride=1 << 30), dict(H0=0), dict(Hn=0), dict(thresh=float("nan")), dict(fmt=2),
           dict(pitch=64 * 3 - 1), dict(frame_stride=48 * 64 * 3 - 1), dict(ws_bytes=128 * 6 * 23 - 1), dict(ws_bytes=0),
           dict(bboxes=P + 4), dict(ws=P + 8), dict(ids=P + 2), dict(scores=P + 1), dict(track=P + 2), dict(gt=P + 2),
           dict(clip_start=P + 1), dict(palette=P + 2), dict(font=P + 1), dict(painted=P + 2), dict(names=None), dict(n_names=0),
           dict(out=P + 1), dict(out=P + 6 * 48 * 64 * 3 - 1), dict(out=P - 5),          # out overlaps frames other than exactly
           dict(nv, H0=47), dict(nv, W0=63), dict(nv, pitch=62), dict(nv, uv_offset=64 * 48 - 1), dict(nv, frame_stride=64 * 72 - 1)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_overlay:"), (kw, err)
    for stages in (0, 4, -1):
        assert lib.vd_overlay_stages(*good.values(), stages, None) == -1 and b"stages" in lib.vd_last_error()


def test_ops_overlay_refuses_its_arguments_without_touching_the_gpu():
    import torch
    from viddet_amd import ops
    fr = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    ids, sc, bb = torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="device tensor"):
        ops.overlay(fr, ids, sc, bb)
    with pytest.raises(ValueError, match="thickness"):
        ops.overlay(fr, ids, sc, bb, thickness=9)
    with pytest.raises(ValueError, match="uint8"):
        ops.overlay(fr.float(), ids, sc, bb)
    with pytest.raises(ValueError, match="RGB frames are"):
        ops.overlay(fr[..., 0], ids, sc, bb)
    with pytest.raises(ValueError, match="even"):
        ops.overlay(torch.zeros(2, 9, 7, dtype=torch.uint8), ids, sc, bb, fmt="nv12")
    with pytest.raises(ValueError, match="at most 128"):
        ops.overlay(fr, torch.zeros(2, 129), torch.zeros(2, 129), torch.zeros(2, 129, 4))
    with pytest.raises(ValueError, match="2 frames but rows of 3"):
        ops.overlay(fr, torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3, 3, 4))
    with pytest.raises(ValueError, match="1-D NV12 surface"):
        ops.overlay(fr, ids, sc, bb, pitch=64)


VIS = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--visualise"]


def test_detect_script_takes_and_refuses_visualise_by_name_before_the_gpu_check(monkeypatch):
    import os
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    with pytest.raises(NotImplementedError, match="--visualise needs --stream"):
        D.main(VIS)
    with pytest.raises(NotImplementedError, match="--visualise does not combine with --live"):
        D.main(VIS + ["--stream", "--live"])
    with pytest.raises(NotImplementedError, match="--visualise.*one --dataset"):
        D.main(["--random_init", "--dataset", "vid,voc", "--data_shape", "64", "--visualise", "--stream"])
    for extra in (["--vis_thickness", "3"], ["--vis_scale", "2"], ["--vis_trail", "4"], ["--vis_every", "2"]):
        with pytest.raises(NotImplementedError, match=extra[0] + " needs --visualise"):
            D.main(["--random_init", "--dataset", "vid", "--data_shape", "64", "--stream"] + extra)
    for extra, name in ((["--vis_thickness", "9"], "--vis_thickness"), (["--vis_scale", "0"], "--vis_scale"),
                        (["--vis_trail", "17"], "--vis_trail"), (["--vis_every", "0"], "--vis_every")):
        with pytest.raises(NotImplementedError, match=name + " must"):
            D.main(VIS + ["--stream"] + extra)
    for flag, value in (("--per_frame_metric", []), ("--worst_video_path", ["x"])):
        with pytest.raises(NotImplementedError, match="outside the yolo3_darknet53 hot path"):
            D.main(VIS[:-1] + ["--stream", flag] + value)
    # with --stream it gets as far as asking for the GPU
    for extra in ([], ["--track"], ["--track", "--track_smooth", "--display_gt", "--vis_trail", "0", "--vis_every", "3"],
                  ["--display_gt", "False"]):
        with pytest.raises(SystemExit):
            D.main(VIS + ["--stream"] + extra)
    F = D.parse_flags(["--visualise"])
    a = D.visualise_args(F)                                       # (a --vis_* flag that was not given parses as None)
    assert F.visualise is True and a["params"] == dict(thresh=0.5, thickness=2, scale=1, trail=8) and a["every"] == 1 and a["display_gt"]
    assert a["dir"] == os.path.join(F.save_dir, F.save_prefix, "vis") and a["yuv"] is None
    a = D.visualise_args(D.parse_flags(["--visualise", "--vis_thickness", "3", "--vis_scale", "2", "--vis_trail", "0", "--vis_every",
                                        "4", "--display_gt", "False", "--detection_threshold", "0.25"]))
    assert a["params"] == dict(thresh=0.25, thickness=3, scale=2, trail=0) and a["every"] == 4 and a["display_gt"] is False
    assert D.parse_flags([]).visualise is False and D.visualise_args(D.parse_flags([])) is None


def test_detect_video_refuses_a_bad_overlay_argument_on_a_cpu_net():
    import torch
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["a", "b"], device="cpu")
    with pytest.raises(ValueError, match="overlay needs uint8 frames"):
        net.detect_video(torch.zeros(4, 3, 64, 64), overlay=True)
    u8 = torch.zeros(4, 64, 64, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="overlay does not take bogus"):
        net.detect_video(u8, overlay={"bogus": 1})
    with pytest.raises(ValueError, match="thickness"):
        net.detect_video(u8, overlay=dict(thickness=9))
    with pytest.raises(ValueError, match="inplace.*device"):
        net.detect_video(u8, overlay=dict(inplace=True))
    with pytest.raises(TypeError):
        net.open_video(overlay=True)                              # a live session has no such argument
