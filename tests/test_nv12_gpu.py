"""GPU: NV12 frames converted, resized and normalised in one launch (vd_resize.hip k_resize_nv12_nchw,
YOLOV3.set_device_resize(source='nv12')).

Kernel: `out` and `out_u8` of vd_resize_nv12_nchw are bit-equal (torch.equal) to vd_resize_u8_nchw on video.nv12_to_rgb of
the same planes - the conversion is exact integer arithmetic and everything behind it is the RGB kernel's arithmetic - for
the four (matrix, range) pairs, shrinking / growing / many-tile / identity shapes, every interpolation, a pitched surface
between guard bytes whose value must not matter, and a first byte at an address that is 1 mod 4.  The tiles' first source
column and first source row are computed here from the tap tables and must be odd somewhere: that is where the pairing
of a pixel with its chroma can go wrong.
Network: net(NV12) under source='nv12' is bit-identical to net(nv12_to_rgb(NV12)) under source='rgb', fp32 and bf16, k = 1
and k = 3, from the host, from a pitched device surface (no repack: the kernel is handed the surface's own pointer and
pitch), and through detect_video; the plans are those of the target size and survive the switch.
Script: detect_yolo3.py --stream --device_resize --frame_format nv12.
"""
import os

import numpy as np
import pytest
import torch

from viddet_amd import video as V

pytestmark = pytest.mark.gpu

PAIRS = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
# (H0, W0) -> (H, W): shrinking (area); mixed (bicubic: both grow); growing; several tiles per frame; identity
SHAPES = [((34, 50), (32, 32)), ((36, 64), (64, 96)), ((24, 20), (64, 64)), ((150, 202), (64, 96)), ((64, 96), (64, 96))]


def _tables(h0, w0, h, w, interp=9):
    """host tables (identity: one tap of weight 1) and their uploads"""
    host = V.identity_tables(h, w) if (h0, w0) == (h, w) else V.resize_tables(h0, w0, h, w, interp)[1:]
    return host, [torch.from_numpy(a).cuda() for a in host]


def _planes(n, h0, w0, seed):
    """random NV12 frames over all of 0..255: both clip sides and below-black / above-white luma occur"""
    return np.random.default_rng(seed).integers(0, 256, (n, h0 * 3 // 2, w0), dtype=np.uint8)


def _rgb_ref(frames, h, w, tabs, key):
    """vd_resize_u8_nchw on nv12_to_rgb of the frames -> (out, out_u8)"""
    from viddet_amd import lib as L
    x = torch.from_numpy(V.nv12_to_rgb(frames, *key)).cuda()
    n, h0, w0, _ = x.shape
    iy, wy, ix, wx = tabs
    out = torch.full((n, 3, h, w), float("nan"), device="cuda")
    u8 = torch.full((n, h, w, 3), 77, dtype=torch.uint8, device="cuda")
    L.check(L.load().vd_resize_u8_nchw(x.data_ptr(), out.data_ptr(), u8.data_ptr(), n, h0, w0, h, w, iy.data_ptr(), wy.data_ptr(),
                                       iy.shape[1], ix.data_ptr(), wx.data_ptr(), ix.shape[1], L.stream_ptr()), "vd_resize_u8_nchw")
    return out, u8


def _nv12(ptr, in_bytes, fstride, pitch, uv_off, n, h0, w0, h, w, tabs, key, want_u8=True):
    """vd_resize_nv12_nchw on n frames at device address ptr -> (out, out_u8 | None)"""
    from viddet_amd import lib as L
    iy, wy, ix, wx = tabs
    out = torch.full((n, 3, h, w), float("nan"), device="cuda")
    u8 = torch.full((n, h, w, 3), 77, dtype=torch.uint8, device="cuda") if want_u8 else None
    L.check(L.load().vd_resize_nv12_nchw(ptr, in_bytes, fstride, pitch, uv_off, out.data_ptr(), u8.data_ptr() if want_u8 else None,
                                         n, h0, w0, h, w, iy.data_ptr(), wy.data_ptr(), iy.shape[1], ix.data_ptr(), wx.data_ptr(),
                                         ix.shape[1], *V.NV12_MATRICES[key], L.stream_ptr()), "vd_resize_nv12_nchw")
    return out, u8


def _nv12_packed(frames, h, w, tabs, key, want_u8=True):
    """the frames as one contiguous device tensor: pitch W0, no slack"""
    n, hn, w0 = frames.shape
    x = torch.from_numpy(frames).cuda()
    res = _nv12(x.data_ptr(), x.numel(), hn * w0, w0, (hn * 2 // 3) * w0, n, hn * 2 // 3, w0, h, w, tabs, key, want_u8)
    torch.cuda.synchronize()
    return res


def _tile_origins(host, h0, w0, h, w):
    """(first source rows, first source columns) of the kernel's tiles, from the tables: the kernel's tile is TH x TW = 16 x 64
    output pixels for every shape of this file (pick_geo_nv12 takes its largest tile whenever the staged rows fit in 64 KB of
    LDS; at these sizes they do, the assert restates its byte count), and a tile's first row / column is the smallest index
    its slice of the table holds"""
    iy, _, ix, _ = host
    TH, TW, Ty, Tx = 16, 64, iy.shape[1], ix.shape[1]
    cmax, rmax = min(-(-TW * w0 // w) + Tx + 1, w0), min(-(-TH * h0 // h) + Ty + 1, h0)
    fixed = rmax * TW * 3 * 4 + (TW * Tx + TH * Ty) * 8 + 64
    row = ((cmax + 6) // 4 + (cmax * 3 + 3) // 4) * 4 + (cmax + 8) // 4 * 4                # one Y + one RGB row, one UV row
    assert fixed + 2 * row <= 64 * 1024, "the 16 x 64 tile does not fit: restate pick_geo_nv12 for this shape"
    rows = [int(iy[o:o + TH].min()) for o in range(0, h, TH)]
    cols = [int(ix[o:o + TW].min()) for o in range(0, w, TW)]
    return rows, cols


@pytest.fixture(scope="module")
def shape_runs():
    """every shape once under bt601 / limited, both kernels: [(src, dst, host tables, frames, nv12 result, rgb result)]"""
    runs = []
    for si, ((h0, w0), (h, w)) in enumerate(SHAPES):
        host, tabs = _tables(h0, w0, h, w)
        frames = _planes(2, h0, w0, 100 + si)
        runs.append(((h0, w0), (h, w), host, frames, _nv12_packed(frames, h, w, tabs, PAIRS[0]), _rgb_ref(frames, h, w, tabs, PAIRS[0])))
    torch.cuda.synchronize()
    return runs


@pytest.mark.parametrize("si", range(len(SHAPES)), ids=["%dx%d-%dx%d" % (a + b) for a, b in SHAPES])
def test_kernel_is_bit_equal_to_the_rgb_kernel_on_converted_frames(shape_runs, si):
    src, dst, host, frames, (out, u8), (out_r, u8_r) = shape_runs[si]
    assert not bool(torch.isnan(out).any())
    assert torch.equal(u8, u8_r), "out_u8 differs from vd_resize_u8_nchw on nv12_to_rgb: %d bytes" % int((u8 != u8_r).sum())
    assert torch.equal(out, out_r), "out differs from vd_resize_u8_nchw on nv12_to_rgb"
    if src == dst:                                                        # identity: the converted frame itself
        assert np.array_equal(u8.cpu().numpy(), V.nv12_to_rgb(frames))
    assert int((u8 == 0).sum()) > 0 and int((u8 == 255).sum()) > 0        # both clip sides reached the output


def test_some_tile_starts_on_an_odd_source_column_and_some_on_an_odd_source_row(shape_runs):
    odd_row = odd_col = False
    for src, dst, host, *_ in shape_runs:
        rows, cols = _tile_origins(host, *src, *dst)
        print("%s -> %s: tiles' first source rows %s, first source columns %s" % (src, dst, rows, cols))
        odd_row |= any(r % 2 for r in rows)
        odd_col |= any(c % 2 for c in cols)
    assert odd_col, "no tile's first source column is odd: the chroma pair of an odd first column is not exercised"
    assert odd_row, "no tile's first source row is odd: a batch that starts on the second row of a chroma row is not exercised"


@pytest.mark.parametrize("key", PAIRS, ids=["%s-%s" % k for k in PAIRS])
def test_every_matrix_and_range(key):
    (h0, w0), (h, w) = (36, 64), (64, 96)
    _, tabs = _tables(h0, w0, h, w)
    frames = _planes(2, h0, w0, 7)
    out, u8 = _nv12_packed(frames, h, w, tabs, key)
    out_r, u8_r = _rgb_ref(frames, h, w, tabs, key)
    assert torch.equal(u8, u8_r) and torch.equal(out, out_r)
    other = PAIRS[(PAIRS.index(key) + 1) % 4]
    assert not torch.equal(u8, _rgb_ref(frames, h, w, tabs, other)[1]), "the comparison does not tell the matrices apart"


@pytest.mark.parametrize("interp", [1, 2, 3, 4])
@pytest.mark.parametrize("src,dst", [((34, 50), (32, 32)), ((24, 20), (64, 64))], ids=["shrink", "grow"])
def test_every_interpolation(src, dst, interp):
    _, tabs = _tables(*src, *dst, interp=interp)
    frames = _planes(2, *src, 20 + interp)
    out, u8 = _nv12_packed(frames, *dst, tabs, PAIRS[0])
    out_r, u8_r = _rgb_ref(frames, *dst, tabs, PAIRS[0])
    assert torch.equal(u8, u8_r) and torch.equal(out, out_r)


@pytest.mark.parametrize("start", [16, 1], ids=["aligned", "1mod4"])
def test_pitched_surface_between_guard_bytes(start):
    """pitch = W0 + 6, slack behind every UV plane, guard bytes around and between the frames - all of it allocated, and
    in_bytes ends at the last chroma byte: the result depends on none of them.  start = 1: the first frame byte sits at an
    address that is 1 mod 4 (a view one byte into the buffer)"""
    (h0, w0), (h, w), n = (34, 50), (32, 32), 2
    hn, pitch, uv_off = h0 * 3 // 2, w0 + 6, (w0 + 6) * h0 + 24                         # a gap between the planes too
    fstride = uv_off + pitch * (h0 // 2) + 10
    in_bytes = (n - 1) * fstride + uv_off + pitch * (h0 // 2 - 1) + w0
    _, tabs = _tables(h0, w0, h, w)
    frames = _planes(n, h0, w0, 31)
    want = _rgb_ref(frames, h, w, tabs, PAIRS[0])
    results = []
    for guard in (0xA5, 0x5A):
        host = np.full(start + n * fstride + 64, guard, dtype=np.uint8)
        for i in range(n):
            f0 = start + i * fstride
            for r in range(h0):
                host[f0 + r * pitch:f0 + r * pitch + w0] = frames[i, r]
            for r in range(h0 // 2):
                host[f0 + uv_off + r * pitch:f0 + uv_off + r * pitch + w0] = frames[i, h0 + r]
        store = torch.from_numpy(host).cuda()
        assert store.data_ptr() % 4 == 0 and (store.data_ptr() + start) % 4 == start % 4
        a = _nv12(store.data_ptr() + start, in_bytes, fstride, pitch, uv_off, n, h0, w0, h, w, tabs, PAIRS[0])
        b = _nv12(store.data_ptr() + start, in_bytes, fstride, pitch, uv_off, n, h0, w0, h, w, tabs, PAIRS[0])
        c = _nv12(store.data_ptr() + start, in_bytes, fstride, pitch, uv_off, n, h0, w0, h, w, tabs, PAIRS[0], want_u8=False)
        torch.cuda.synchronize()
        assert np.array_equal(store.cpu().numpy(), host), "the input buffer was written"
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "two runs differ"
        assert torch.equal(a[0], c[0]), "out_u8 = NULL changes out"
        results.append(a)
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), "the guard value shows"
    assert torch.equal(results[0][1], want[1]) and torch.equal(results[0][0], want[0])


def test_argument_checks_return_minus_one_and_launch_nothing():
    from viddet_amd import lib as L
    lib = L.load()
    (h0, w0), (h, w), n = (34, 50), (32, 32), 2
    _, (iy, wy, ix, wx) = _tables(h0, w0, h, w)
    x = torch.from_numpy(_planes(n, h0, w0, 1)).cuda()
    out = torch.full((n, 3, h, w), float("nan"), device="cuda")
    u8 = torch.full((n, h, w, 3), 77, dtype=torch.uint8, device="cuda")
    hn = h0 * 3 // 2
    good = dict(in_=x.data_ptr(), in_bytes=x.numel(), fs=hn * w0, pitch=w0, uv=h0 * w0, out=out.data_ptr(), out_u8=u8.data_ptr(),
                N=n, H0=h0, W0=w0, H=h, W=w, iy=iy.data_ptr(), wy=wy.data_ptr(), Ty=iy.shape[1], ix=ix.data_ptr(), wx=wx.data_ptr(),
                Tx=ix.shape[1])

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_resize_nv12_nchw(a['in_'], a['in_bytes'], a['fs'], a['pitch'], a['uv'], a['out'], a['out_u8'], a['N'], a['H0'],
                                     a['W0'], a['H'], a['W'], a['iy'], a['wy'], a['Ty'], a['ix'], a['wx'], a['Tx'],
                                     *V.NV12_MATRICES[PAIRS[0]], L.stream_ptr())
        return rc, lib.vd_last_error()

    bad = [dict(in_=None), dict(out=None), dict(iy=None), dict(wy=None), dict(ix=None), dict(wx=None),
           dict(N=0), dict(H0=0), dict(W0=-2), dict(H=0), dict(W=0),
           dict(H0=33), dict(W0=49),                                           # odd sizes
           dict(pitch=w0 - 1), dict(pitch=0),
           dict(uv=h0 * w0 - 1),                                               # the UV plane inside the Y plane
           dict(fs=hn * w0 - 1),                                               # a frame shorter than its two planes
           dict(in_bytes=n * hn * w0 - 1),                                     # the last chroma byte is outside the buffer
           dict(in_bytes=0),
           dict(Tx=17), dict(Ty=17), dict(Tx=0), dict(Ty=-1),
           dict(iy=iy.data_ptr() + 2), dict(wx=wx.data_ptr() + 1), dict(out=out.data_ptr() + 2)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_resize_nv12_nchw:"), (kw, err)
    assert b"Tx=17" in call(Tx=17)[1] and b"H=0" in call(H=0)[1] and b"NULL" in call(in_=None)[1]
    assert b"even" in call(H0=33)[1] and b"pitch" in call(pitch=w0 - 1)[1] and b"uv_offset" in call(uv=h0 * w0 - 1)[1]
    assert b"frame_stride" in call(fs=hn * w0 - 1)[1] and b"in_bytes" in call(in_bytes=0)[1]
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((u8 == 77).all()), "a refused call launched"
    # the exact rule: the buffer may end at the last frame's last chroma byte (pitch W0 + 2: 2 bytes short of a whole pitch)
    rc, err = call(pitch=w0 + 2, uv=h0 * (w0 + 2), fs=hn * (w0 + 2), N=1, in_bytes=hn * (w0 + 2) - 2 - 1)
    assert rc == -1 and b"in_bytes" in err
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ network
C, SIZE, RAW = 3, 64, (36, 50)
HN = RAW[0] * 3 // 2


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


def _outputs(net, res):
    torch.cuda.synchronize()
    return [t.clone() for t in res] + [net.last_rows.clone()]


NAMES = ("ids", "scores", "bboxes", "last_rows")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("k", [1, 3])
def test_net_on_nv12_equals_net_on_converted_frames(nets, k, precision, monkeypatch):
    from viddet_amd import lib as L
    net = nets[k]
    net.set_precision(precision)
    lead = (2, 3) if k == 3 else (2,)
    nv = np.random.default_rng(5 * k).integers(0, 256, lead + (HN, RAW[1]), dtype=np.uint8)
    rgb = torch.from_numpy(V.nv12_to_rgb(nv))
    calls = []
    real = L.load().vd_resize_nv12_nchw
    try:
        net.set_device_resize(SIZE, SIZE)
        want = _outputs(net, net(rgb))
        key = ('infer_bf16' if precision == 'bf16' else 'infer', 2, SIZE, SIZE)
        prog = net._programs[key]
        recs = list(prog[0].recs)
        net.set_device_resize(SIZE, SIZE, source='nv12')
        got = _outputs(net, net(torch.from_numpy(nv)))                                    # contiguous, from the host
        # a pitched surface already on the device: (.., HN, P)[..., :W0]; the kernel must be handed its pointer and pitch
        surf = torch.full(lead + (HN, RAW[1] + 6), 0xA5, dtype=torch.uint8, device="cuda")
        view = surf[..., :RAW[1]]
        view.copy_(torch.from_numpy(nv))
        monkeypatch.setattr(L.load(), "vd_resize_nv12_nchw", lambda *a: (calls.append(a), real(*a))[1])
        pitched = _outputs(net, net(view))
        monkeypatch.setattr(L.load(), "vd_resize_nv12_nchw", real)
        with pytest.raises(ValueError, match="got packed RGB frames"):
            net(rgb)
        net.set_device_resize(SIZE, SIZE)                                                 # back to RGB on the same net
        back = _outputs(net, net(rgb))
        assert net._programs[key] is prog and prog[0].recs == recs, "the switch rebuilt the plan"
        assert net._dev_nv12 is None
    finally:
        net.set_device_resize(None)
        net.set_precision("fp32")
    assert int((want[0] >= 0).sum()) > 4, "fixture produced (almost) no detections"
    for name, a, b, c, d in zip(NAMES, want, got, pitched, back):
        assert torch.equal(a, b), "%s: net(NV12) differs from net(nv12_to_rgb(NV12))" % name
        assert torch.equal(a, c), "%s: the pitched device surface differs from the contiguous host frames" % name
        assert torch.equal(a, d), "%s: differs after switching back to source='rgb'" % name
    assert len(calls) == 1 and calls[0][0] == view.data_ptr(), "the pitched surface was repacked"
    assert calls[0][3] == RAW[1] + 6 and calls[0][2] == HN * (RAW[1] + 6) and calls[0][4] == RAW[0] * (RAW[1] + 6)


def test_net_on_nv12_frames_of_the_target_size_goes_through_the_kernel(nets):
    net = nets[1]
    nv = np.random.default_rng(9).integers(0, 256, (2, SIZE * 3 // 2, SIZE), dtype=np.uint8)
    try:
        net.set_device_resize(None)
        want = _outputs(net, net(torch.from_numpy(V.nv12_to_rgb(nv))))                     # plain uint8 frames at 64 x 64
        net.set_device_resize(SIZE, SIZE, source='nv12')
        got = _outputs(net, net(torch.from_numpy(nv)))
        assert net._resize_cache[(SIZE, SIZE, SIZE, SIZE, 'identity')]['dev'] is not None
    finally:
        net.set_device_resize(None)
    for name, a, b in zip(NAMES, want, got):
        assert torch.equal(a, b), name


def _plan_programs(plan):
    """the Program objects of one entry of net._programs (a tuple (prog, bufs, ..) or a dict of a plan's parts)"""
    parts = plan.values() if isinstance(plan, dict) else plan
    return [p for p in parts if hasattr(p, 'recs') and hasattr(p, 'run')]


def test_detect_video_on_an_nv12_clip(nets):
    net = nets[3]
    nv = np.random.default_rng(11).integers(0, 256, (7, HN, RAW[1]), dtype=np.uint8)
    rgb = torch.from_numpy(V.nv12_to_rgb(nv))
    try:
        net.set_device_resize(SIZE, SIZE)
        windows = torch.from_numpy(np.random.default_rng(12).integers(0, 256, (3, 3) + RAW + (3,), dtype=np.uint8))
        net(windows)                                                                       # the windowed plan at batch 3
        want = _outputs(net, net.detect_video(rgb, step=1, chunk=3))
        held = dict(net._programs)
        recs = {k: [list(p.recs) for p in _plan_programs(v)] for k, v in held.items()}
        assert ('stream', 3, SIZE, SIZE, 5) in held and ('infer', 3, SIZE, SIZE) in held
        net.set_device_resize(SIZE, SIZE, source='nv12')
        got = _outputs(net, net.detect_video(torch.from_numpy(nv), step=1, chunk=3))       # uploaded chunk by chunk
        stats = dict(net.stream_stats)
        net(torch.from_numpy(np.ascontiguousarray(nv[:3])).unsqueeze(0).expand(3, 3, HN, RAW[1]))
        assert set(net._programs) == set(held), "an NV12 call built another plan"
        for k, v in held.items():
            assert net._programs[k] is v, k
            assert [list(p.recs) for p in _plan_programs(v)] == recs[k], k
    finally:
        net.set_device_resize(None)
    assert stats['prefix_frames'] == 7 and stats['suffix_frames'] == 7
    assert int((want[0] >= 0).sum()) > 7
    for name, a, b in zip(NAMES, want, got):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ script
def test_detect_script_stream_on_nv12_frames(tmp_path):
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticVideo
    from viddet_amd.model import yolo3_darknet53
    join = ["--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early"]
    base = ["--random_init", "--dataset", "voc", "--data_shape", "64", "--batch_size", "4", "--synthetic_samples", "6",
            "--synthetic_videos", "2", "--stream", "--device_resize", "--metrics", "voc", "--save_dir", str(tmp_path)] + join
    D.main(base + ["--frame_format", "nv12", "--save_prefix", "n"])
    D.main(base + ["--frame_format", "rgb", "--save_prefix", "r"])
    files = sorted(os.listdir(tmp_path / "n" / "pred"))
    assert len(files) == 12 and files == sorted(os.listdir(tmp_path / "r" / "pred"))         # one file per frame, the same set
    ds = SyntheticVideo("voc", num_videos=2, frames_per_video=6, window=3, step=1, frame_format="nv12")
    preds = D.load_predictions(str(tmp_path / "n" / "pred"), ds)

    # the same detections from detect_stream on the converted frames, with an identically seeded net (initialize's own seed)
    class Converted:
        classes, num_videos, sample_index, sample_path = ds.classes, ds.num_videos, ds.sample_index, ds.sample_path

        def __len__(self):
            return len(ds)

        def video_frames(self, v):
            return V.nv12_to_rgb(ds.video_frames(v))

    net = yolo3_darknet53(ds.classes, pretrained_base=False, k=3, k_join_type="max", k_join_pos="early")
    net.initialize(init="he", obj_bias=-2.0)
    net.set_device_resize(64, 64)
    boxes = D.detect_stream(net, Converted(), 64, 1, 4, device_resize=True)
    assert sum(len(v) for v in preds.values()) > 10, "fixture produced (almost) no detections"
    assert set(preds) == set(boxes)
    for path, rows in boxes.items():
        # (a prediction file holds "{}".format of every number: save_predictions)
        assert preds[path] == [[int(r[0])] + [float("{}".format(t)) for t in r[1:]] for r in rows], path
