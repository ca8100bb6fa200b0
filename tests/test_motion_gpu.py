"""GPU: camera-motion compensation on the device equals its definition on bytes.  vd_motion_sig
(ops.motion_signature) against viddet_amd.motion.signature_host over the cells, sizes, formats and surfaces; vd_motion_match
(ops.motion_match) against match_host on motion, sad and the running sum; vd_motion_shift (ops.motion_shift) against
stabilise_host / restore_host; then through net.detect_video(track={..., 'gmc': ...}) and detect_yolo3.py --track_gmc."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import motion_cases as MC
from tests import sort_cases as SC
from viddet_amd import motion as M

pytestmark = pytest.mark.gpu


def _bytes(t):
    return t.cpu().contiguous().view(torch.uint8).numpy().reshape(-1)


def _sig(frames, keep, **kw):
    """two runs of ops.motion_signature on device frames `frames` -> the signature; `keep`: the whole surface, which must stay"""
    from viddet_amd import ops
    before = keep.clone()
    runs = [ops.motion_signature(frames, **kw) for _ in range(2)]
    torch.cuda.synchronize()
    assert runs[0].dtype == torch.uint16 and np.array_equal(_bytes(runs[0]), _bytes(runs[1])), "two runs differ"
    assert torch.equal(keep, before), "the frames were written"
    return runs[0].cpu().numpy()


def _frames(F, h, w, seed, full=False):
    if full:
        return np.full((F, h, w, 3), 255, np.uint8)
    return np.random.RandomState(seed).randint(0, 256, (F, h, w, 3)).astype(np.uint8)


# ------------------------------------------------------------------ the signature
@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("cell", M.CELLS)
def test_signature_rgb(cell, F):
    sizes = [(96, 128, False), (37, 53, False)] + ([(16, 16, True)] if cell == 16 else [])
    for h, w, full in sizes:
        fr = _frames(F, h, w, cell + F, full)
        x = torch.from_numpy(fr).cuda()
        want = M.signature_host(fr, cell)
        assert np.array_equal(_sig(x, x, cell=cell), want), (h, w)
        if full:
            assert (want == 65280).all()
        # a base that is no multiple of 16: the narrow path on the same pixels
        store = torch.zeros(fr.size + 3, dtype=torch.uint8, device="cuda")
        y = store[3:].view(fr.shape)
        y.copy_(x)
        assert np.array_equal(_sig(y, store, cell=cell), want), (h, w, "unaligned")


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("cell", M.CELLS)
def test_signature_nv12(cell, F):
    """NV12 needs even sizes: 38 x 54 stands for 37 x 53 (tails on both axes at cell >= 4, rows not 16-byte aligned)"""
    from viddet_amd import ops
    sizes = [(96, 128, False), (38, 54, False)] + ([(16, 16, True)] if cell == 16 else [])
    for h, w, full in sizes:
        nv = MC.to_nv12_luma(_frames(F, h, w, cell + F, full), seed=cell)
        want = M.signature_host(nv, cell, "nv12")
        rows = h * 3 // 2
        x = torch.from_numpy(nv).cuda()
        assert np.array_equal(_sig(x, x, cell=cell, fmt="nv12"), want), (h, w)
        # the view [..., :W0] of a surface with pitch W0 + 24 whose padding is 0xFF
        store = torch.full((F, rows, w + 24), 0xFF, dtype=torch.uint8, device="cuda")
        store[..., :w] = x
        assert np.array_equal(_sig(store[..., :w], store, cell=cell, fmt="nv12"), want), (h, w, "pitched")
        # the same as a 1-D surface
        flat = store.reshape(-1)
        assert np.array_equal(_sig(flat, flat, cell=cell, fmt="nv12", H0=h, W0=w, pitch=w + 24), want), (h, w, "1-D")
        out = torch.zeros(F, h // cell, w // cell, dtype=torch.uint16, device="cuda")
        assert ops.motion_signature(x, cell=cell, fmt="nv12", out=out) is out and np.array_equal(out.cpu().numpy(), want)


# ------------------------------------------------------------------ the match
def _match(sig, clip_start=None, **kw):
    from viddet_amd import ops
    want = M.match_host(sig, clip_start, **kw)
    d = torch.from_numpy(sig).cuda()
    keep = d.clone()
    runs = [ops.motion_match(d, clip_start, **kw) for _ in range(2)]
    torch.cuda.synchronize()
    got = runs[0]
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int64 and got[2].dtype == torch.int32
    assert np.array_equal(got[0].cpu().numpy(), want[0]), "motion"
    assert np.array_equal(got[1].cpu().numpy(), want[1]), "sad"
    assert np.array_equal(got[2].cpu().numpy(), M.cumulate(want[0], clip_start)), "cum"
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two runs differ"
    assert np.array_equal(_bytes(d), _bytes(keep)), "the signature was written"
    return want


@pytest.mark.parametrize("Gh,Gw,radius", [(24, 32, 1), (24, 32, 8), (24, 32, 11), (33, 33, 16)])
def test_match_equals_the_definition(Gh, Gw, radius):
    sig = MC.signatures(12, Gh, Gw, seed=radius)
    for gate in (1.0, 0.75):
        assert _match(sig, radius=radius, gate=gate)[0].any() or gate < 1.0
        want = _match(sig, [0, 1, 3, 12], radius=radius, gate=gate, cell=8)          # clips of 1, 2 and 9 frames
        assert not want[0][[0, 1, 3]].any()
    _match(sig[:1], radius=radius)                                                     # one frame: nothing to match


def test_match_flat_shake_and_uncorrelated():
    from viddet_amd import ops
    flat = np.full((4, 24, 32), 1234, np.uint16)
    assert not _match(flat, gate=1.0)[0].any()                                         # every SAD ties: the tie rule gives 0
    rows = flat.copy()
    rows[:, ::2] = 900
    assert not _match(rows, gate=1.0)[0].any()
    assert np.array_equal(_match(M.signature_host(MC.shake_clip()))[0], MC.MOTION)
    u = M.signature_host(MC.uncorrelated())
    assert not _match(u, gate=0.75)[0].any() and _match(u, gate=1.0)[0].any()
    # device offsets are taken as they are; the last frame lies outside every clip and comes out as zeros
    sig = MC.signatures(6, 24, 32, seed=4)
    cs = torch.tensor([0, 2, 5], dtype=torch.int32, device="cuda")
    got = ops.motion_match(torch.from_numpy(sig).cuda(), cs, gate=1.0)
    want = M.match_host(sig[:5], [0, 2, 5], gate=1.0)
    z = np.zeros((1, 2))
    assert np.array_equal(got[0].cpu().numpy(), np.concatenate([want[0], z])) and np.array_equal(got[1].cpu().numpy(), np.concatenate([want[1], z]))
    assert np.array_equal(got[2].cpu().numpy(), np.concatenate([M.cumulate(want[0], [0, 2, 5]), z]))
    ws = torch.full((8 * 6 * 17 * 17,), 0xFF, dtype=torch.uint8, device="cuda")        # a reused workspace
    again = ops.motion_match(torch.from_numpy(sig).cuda(), cs, gate=1.0, ws=ws)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


# ------------------------------------------------------------------ the shift
def test_shift_equals_the_definition():
    from viddet_amd import ops
    rng = np.random.RandomState(2)
    F, N = 9, 37
    boxes = rng.uniform(-50, 500, (F, N, 4)).astype(np.float32)
    boxes[1, 2, 0], boxes[3, 0, 3] = np.nan, np.inf
    ids = rng.randint(-1, 3, (F, N, 1)).astype(np.float32)
    ids[2, 1, 0] = np.nan
    track = rng.randint(-1, 4, (F, N)).astype(np.int32)
    motion = rng.randint(-4000, 4001, (F, 2)).astype(np.int32)                          # offsets of thousands of pixels
    sx, sy = float(np.float32(416) / np.float32(1280)), float(np.float32(416) / np.float32(720))
    d_ids, d_track, d_boxes = torch.from_numpy(ids).cuda(), torch.from_numpy(track).cuda(), torch.from_numpy(boxes).cuda()
    keep = d_boxes.clone()
    for cs in (None, [0, 3, 9]):
        cum = torch.from_numpy(M.cumulate(motion, cs)).cuda()
        got = ops.motion_shift(d_ids, d_boxes, cum, sx, sy, -1)
        assert np.array_equal(_bytes(got), M.stabilise_host(ids, boxes, motion, cs, sx, sy).view(np.uint8).reshape(-1)), "stabilise"
        got = ops.motion_shift(d_track, d_boxes, cum, sx, sy, 1)
        assert np.array_equal(_bytes(got), M.restore_host(track, boxes, motion, cs, sx, sy).view(np.uint8).reshape(-1)), "restore"
    zero = torch.zeros(F, 2, dtype=torch.int32, device="cuda")
    assert np.array_equal(_bytes(ops.motion_shift(d_ids, d_boxes, zero, sx, sy, -1)), _bytes(d_boxes))
    assert np.array_equal(_bytes(d_boxes), _bytes(keep)), "the input was written"


# ------------------------------------------------------------------ arguments
def test_argument_checks_return_minus_one():
    from viddet_amd import lib as L
    from viddet_amd import ops
    lib, p = L.load(), L.ptr
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    fr = torch.zeros(2, 96, 128, 3, dtype=torch.uint8, device="cuda")
    sig = torch.zeros(2, 24, 32, dtype=torch.uint16, device="cuda")

    def call_sig(frames=p(fr), fs=96 * 384, pitch=384, fmt=0, F=2, H0=96, W0=128, cell=4, out=p(sig)):
        return lib.vd_motion_sig(frames, fs, pitch, fmt, F, H0, W0, cell, out, L.stream_ptr())

    assert call_sig() == 0
    for kw in (dict(frames=None), dict(out=None), dict(fmt=2), dict(cell=3), dict(cell=32), dict(F=0), dict(H0=2), dict(W0=0),
               dict(W0=20000), dict(pitch=383), dict(fs=95 * 384), dict(out=off(sig, 1))):
        assert call_sig(**kw) == -1 and lib.vd_last_error().decode().startswith("vd_motion_sig: "), kw
    motion = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    sad = torch.zeros(2, 2, dtype=torch.int64, device="cuda")
    cum = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    need = 8 * 2 * 17 * 17
    assert lib.vd_motion_match_ws_bytes(2, 8) == need and lib.vd_motion_match_ws_bytes(2, 17) == -1
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    cs = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")

    def call_match(s=p(sig), c=None, V=1, F=2, Gh=24, Gw=32, cell=4, R=8, gate=0.75, m=p(motion), sd=p(sad), cm=p(cum), w=p(ws), nb=need):
        return lib.vd_motion_match(s, c, V, F, Gh, Gw, cell, R, gate, m, sd, cm, w, nb, L.stream_ptr())

    assert call_match() == 0 and call_match(c=p(cs), V=2) == 0
    for kw in (dict(s=None), dict(m=None), dict(sd=None), dict(cm=None), dict(w=None), dict(V=2), dict(V=0), dict(F=0), dict(cell=5),
               dict(R=0), dict(R=17), dict(R=12), dict(Gh=16), dict(Gw=5000), dict(gate=0.0), dict(gate=1.5), dict(gate=float("nan")),
               dict(nb=need - 1), dict(w=off(ws, 4)), dict(sd=off(sad, 4)), dict(m=off(motion, 2)), dict(s=off(sig, 1))):
        assert call_match(**kw) == -1 and lib.vd_last_error().decode().startswith("vd_motion_match: "), kw
    ids = torch.zeros(2, 4, device="cuda")
    bx, out = torch.zeros(2, 4, 4, device="cuda"), torch.zeros(2, 4, 4, device="cuda")

    def call_shift(k=p(ids), it=0, b=p(bx), c=p(cum), F=2, N=4, sign=-1, o=p(out)):
        return lib.vd_motion_shift(k, it, b, c, F, N, 1.0, 1.0, sign, o, L.stream_ptr())

    assert call_shift() == 0
    for kw in (dict(k=None), dict(b=None), dict(c=None), dict(o=None), dict(it=2), dict(sign=0), dict(sign=2), dict(F=0), dict(N=0),
               dict(o=p(bx)), dict(b=off(bx, 4)), dict(o=off(out, 8)), dict(k=off(ids, 2))):
        assert call_shift(**kw) == -1 and lib.vd_last_error().decode().startswith("vd_motion_shift: "), kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="motion_signature: frames must be a device tensor"):
        ops.motion_signature(fr.cpu())
    with pytest.raises(ValueError, match="motion_signature: frames must be a uint8"):
        ops.motion_signature(fr.float())
    with pytest.raises(ValueError, match="motion_signature: cell must be"):
        ops.motion_signature(fr, cell=3)
    with pytest.raises(ValueError, match="motion_signature: RGB frames must be contiguous"):
        ops.motion_signature(fr[:, :, ::2])
    with pytest.raises(ValueError, match="motion_signature: a 1-D NV12 surface needs"):
        ops.motion_signature(fr.reshape(-1), fmt="nv12")
    with pytest.raises(ValueError, match="motion_match: radius=16 needs"):
        ops.motion_match(sig, radius=16)
    with pytest.raises(ValueError, match="motion_match: sig must be"):
        ops.motion_match(sig.to(torch.int32))
    with pytest.raises(ValueError, match="motion_match: clip_start must be"):
        ops.motion_match(sig, [0, 1])
    with pytest.raises(ValueError, match="motion_match: ws must be"):
        ops.motion_match(sig, ws=ws[:-8])
    with pytest.raises(ValueError, match="motion_shift: sign must be"):
        ops.motion_shift(ids, bx, cum, 1.0, 1.0, 0)
    with pytest.raises(ValueError, match="motion_shift: ids_or_track must be"):
        ops.motion_shift(ids.double(), bx, cum, 1.0, 1.0, 1)


# ------------------------------------------------------------------ through the stack
def _same_tracks(net, want, what):
    for name, g, w in zip(("track", "tlen", "tscore"), net.last_tracks, want):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), what + name
    if len(want) == 4:
        assert SC.same_tbox(net.last_track_boxes.cpu().numpy(), want[3]), what + "tbox"
    else:
        assert net.last_track_boxes is None


@pytest.mark.parametrize("k", [1, 3], ids=["k1", "k3_early_max"])
def test_detect_video_with_gmc(k):
    """A 12-frame 96 x 128 SyntheticPan clip at a network size of 64 x 64, chunk 5 (a padded last chunk)."""
    from viddet_amd.appearance import app_sort_host
    from viddet_amd.byte import byte_host
    from viddet_amd.data import SyntheticPan
    from viddet_amd.model import yolo3_darknet53
    from viddet_amd.sort import sort_host
    from viddet_amd.track import track_host
    from viddet_amd.video import rgb_to_nv12
    kw_net = dict(k=3, k_join_type="max", k_join_pos="early") if k == 3 else {}
    net = yolo3_darknet53(["c%d" % i for i in range(3)], **kw_net)
    net.initialize(init="he", obj_bias=1.0)                                # objectness up: rows exist
    net.set_device_resize(64, 64)
    ds = SyntheticPan("vid", num_videos=1, frames_per_video=12, size=(128, 96), pan=24, cell=4)
    frames = ds.video_frames(0)
    want_motion, want_sad = M.motion_host(frames)
    assert np.array_equal(M.cumulate(want_motion), -ds.camera_path(0)) and want_motion.any()
    sx, sy = np.float32(64) / np.float32(128), np.float32(64) / np.float32(96)
    x = torch.from_numpy(frames).cuda()
    kw = dict(sigma_h=0.0, max_age=2, clip=64)
    par = {k_: v for k_, v in kw.items() if k_ != "clip"}

    def expect(host, rows, motion, **more):
        st = M.stabilise_host(rows[0], np.clip(rows[2], 0, 64), motion, None, sx, sy)
        out = host(rows[0], rows[1], st, num_class=3, **par, **more)
        return out if len(out) == 3 else out[:3] + (M.restore_host(out[0], out[3], motion, None, sx, sy),)

    for method, host in (("sort", sort_host), ("iou", track_host), ("byte", byte_host)):
        trk = dict(kw, method=method)
        plain = [t.clone() for t in net.detect_video(x, chunk=5, track=trk)]
        assert net.last_motion is None
        plain_tracks = net.last_tracks[0].clone()
        assert (plain[0] >= 0).sum() > 10, "fixture produced (almost) no detections"
        for src in ((x, torch.from_numpy(frames)) if method == "sort" else (x,)):
            got = [t.clone() for t in net.detect_video(src, chunk=5, track=dict(trk, gmc=True))]
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(plain, got)), "gmc changed what the call returns"
            motion, sad = net.last_motion
            assert np.array_equal(motion.cpu().numpy(), want_motion) and np.array_equal(sad.cpu().numpy(), want_sad)
            rows = [t.cpu().numpy() for t in got]
            _same_tracks(net, expect(host, rows, want_motion), method + ": ")
        assert torch.equal(x.cpu(), torch.from_numpy(frames)), "the frames were written"
        if method == "sort":
            assert not torch.equal(plain_tracks, net.last_tracks[0]), "the camera's motion changed no id"
    # the parameters reach the kernels; stitch runs in the stabilised frame
    net.detect_video(x, chunk=5, track=dict(kw, method="sort", gmc=dict(cell=8, radius=3, gate=1.0)), stitch=True)
    m8 = M.motion_host(frames, cell=8, radius=3, gate=1.0)
    assert np.array_equal(net.last_motion[0].cpu().numpy(), m8[0]) and np.array_equal(net.last_motion[1].cpu().numpy(), m8[1])
    assert net.last_stitch is not None
    # with appearance: the fused cost on the stabilised boxes
    got = net.detect_video(x, chunk=5, track=dict(kw, method="sort", gmc=True, appearance=dict(sigma_app=0.5, sigma_prox=0.05)))
    rows = [t.cpu().numpy() for t in got]
    emb = net.last_embeddings.cpu().numpy()
    _same_tracks(net, expect(lambda *a, **b: app_sort_host(a[0], a[1], a[2], emb, **b), rows, want_motion, sigma_app=0.5, sigma_prox=0.05), "app: ")
    # composes with seq_nms (ahead, on image coordinates) and overlay
    got = net.detect_video(x, chunk=5, track=dict(kw, method="sort", gmc=True), seq_nms=True, overlay=True)
    rows = [t.cpu().numpy() for t in got]
    _same_tracks(net, expect(sort_host, rows, want_motion), "seq_nms: ")
    assert net.last_overlay is not None
    # NV12
    if k == 1:
        net.set_device_resize(64, 64, source="nv12")
        nv = rgb_to_nv12(frames, "bt601", "limited")
        want_nv = M.motion_host(nv, fmt="nv12")
        for src in (torch.from_numpy(nv).cuda(), torch.from_numpy(nv)):
            plain = [t.clone() for t in net.detect_video(src, chunk=5, track=dict(kw, method="sort"))]
            got = net.detect_video(src, chunk=5, track=dict(kw, method="sort", gmc=True))
            assert all(torch.equal(a, b) for a, b in zip(plain, got))
            assert np.array_equal(net.last_motion[0].cpu().numpy(), want_nv[0]) and np.array_equal(net.last_motion[1].cpu().numpy(), want_nv[1])
            _same_tracks(net, expect(sort_host, [t.cpu().numpy() for t in got], want_nv[0]), "nv12: ")
        net.set_device_resize(64, 64)
    # a following call without it: None again
    net.detect_video(x, chunk=5, track=dict(kw, method="sort"))
    assert net.last_motion is None


def test_detect_video_refuses_by_name():
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["a", "b"])
    x = torch.zeros(4, 96, 128, 3, dtype=torch.uint8)
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="detect_video: gmc beside smooth"):
        net.detect_video(x, track=dict(method="sort", gmc=True), smooth=True)
    with pytest.raises(ValueError, match="detect_video: gmc beside tubelet"):
        net.detect_video(x, track=dict(method="sort", gmc=True), tubelet=True)
    with pytest.raises(ValueError, match="detect_video: gmc needs uint8 frames"):
        net.detect_video(torch.zeros(4, 3, 64, 64), track=dict(gmc=True))
    with pytest.raises(ValueError, match="detect_video with gmc: radius=16 needs"):
        net.detect_video(x, track=dict(gmc=dict(radius=16)))
    with pytest.raises(ValueError, match="detect_video with gmc: cell must be"):
        net.detect_video(x, track=dict(gmc=dict(cell=3)))
    with pytest.raises(NotImplementedError, match="open_video with track's gmc"):
        net.open_video(track=dict(gmc=True))
    assert torch.cuda.memory_allocated() == before, "refused before any GPU work"


def _run_script(tmp_path, prefix, *more):
    import detect_yolo3 as D
    D.main(["--random_init", "--dataset", "vid", "--synthetic_samples", "8", "--synthetic_videos", "2", "--data_shape", "64",
            "--device_resize", "--batch_size", "3", "--save_dir", str(tmp_path), "--save_prefix", prefix, "--stream", "--track",
            "--track_method", "sort", "--track_high", "0", "--track_max_age", "2", *more])
    return tmp_path / prefix


def _tree(root):
    import os
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_detect_script_track_gmc(tmp_path):
    """--synthetic_pan 24: motion.txt holds the definition's values on every clip's frames, which undo the camera's path.
    --synthetic_pan 0: SyntheticVideo's frames have no common motion, the gate leaves every frame unmoved, and every other file
    equals the run without the flag byte for byte."""
    from viddet_amd.data import SyntheticPan
    q = _run_script(tmp_path, "pan", "--track_gmc", "--synthetic_pan", "24")
    ds = SyntheticPan("vid", num_videos=2, frames_per_video=8, pan=24, cell=4)
    want = []
    for v in range(2):
        motion, sad = M.motion_host(ds.video_frames(v))
        assert np.array_equal(M.cumulate(motion), -ds.camera_path(v)) and motion.any()
        want += ["%d %d %d %d %d %d" % (v, t, motion[t, 0], motion[t, 1], sad[t, 0], sad[t, 1]) for t in range(8)]
    assert open(q / "motion.txt").read().splitlines() == want
    assert sum(len(b) for f, b in _tree(q).items() if f.startswith("pred_trk")) > 0, "fixture produced no detections"
    plain = _tree(_run_script(tmp_path, "a"))
    gmc = _tree(_run_script(tmp_path, "b", "--track_gmc"))
    lines = gmc.pop("motion.txt").decode().splitlines()
    assert len(lines) == 16 and all(l.split()[2:4] == ["0", "0"] for l in lines), "the gate let a frame move"
    assert any(int(l.split()[4]) > 0 for l in lines)
    assert "motion.txt" not in plain and gmc == plain
