"""vd_overlay against its definition on the GPU: ops.overlay is torch.equal to viddet_amd.overlay.overlay_host
on the frames and on `painted`, in place and out of place - the seeded cases of tests/overlay_cases.py (the dword path at
48 x 64, the byte path at 37 x 51, two clips), 128 rows + 128 ground-truth rows + trails of 16 (the batched walk), NV12
contiguous and pitched, the thinnest and thickest outlines, the smallest and largest text, a frame with nothing to draw; each
launch of vd_overlay_stages against the definition's records; then net.detect_video(overlay=...)."""
import numpy as np
import pytest
import torch

from tests import overlay_cases as OC
from viddet_amd import overlay as O
from viddet_amd.video import rgb_to_nv12

pytestmark = pytest.mark.gpu


def _dev(c):
    d = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("ids", "scores", "bboxes", "track")}
    d["gt"] = None if c["gt"] is None else torch.from_numpy(c["gt"]).cuda()
    return d


def _check(c, fmt="rgb", frames=None):
    """both forms of ops.overlay on a case against overlay_host; returns the host's (out, painted)"""
    from viddet_amd import ops
    if frames is None:
        frames = c["frames"] if fmt == "rgb" else rgb_to_nv12(OC.even(c["frames"]))
    args, kw = OC.call_args(c, fmt)
    want, want_painted = O.overlay_host(frames, *args, **kw)
    d = _dev(c)
    kw = dict(kw, track=d["track"], gt=d["gt"])
    src = torch.from_numpy(frames).cuda()
    keep = src.clone()
    out, painted = ops.overlay(src, d["ids"], d["scores"], d["bboxes"], **kw)          # out of place: every pixel written
    torch.cuda.synchronize()
    assert out.data_ptr() != src.data_ptr() and torch.equal(src, keep)
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and torch.equal(painted.cpu(), torch.from_numpy(want_painted))
    out2, painted2 = ops.overlay(src, d["ids"], d["scores"], d["bboxes"], out=src, **kw)   # in place
    torch.cuda.synchronize()
    assert out2 is src and torch.equal(src.cpu(), torch.from_numpy(want)) and torch.equal(painted2.cpu(), torch.from_numpy(want_painted))
    assert painted.dtype == torch.int32 and tuple(painted.shape) == (frames.shape[0],)
    return want, want_painted


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_device_equals_host_on_the_seeded_cases(name):
    c = OC.case(name)
    _, painted = _check(c)
    assert painted.sum() > 0
    if c["frames"].shape[2] % 4 == 0:
        # the byte path on the same picture: an odd width cut out of the frames
        c2 = dict(c, frames=np.ascontiguousarray(c["frames"][:, :, :-1]))
        _check(c2)


def test_the_batched_walk_128_rows_128_ground_truth_rows_and_trails_of_16():
    F, N = 18, 128
    c = OC.make_case(11, F, (96, 128), N, G=128, net_size=(64, 64), tracked=2.0, broken=False, trail=16, thickness=1)
    c["track"] = np.tile(np.arange(N, dtype=np.int32) * 3, (F, 1))        # every row tracked, in every frame: 16 segments a row
    c["gt"][..., 4] = np.abs(c["gt"][..., 4])                             # and every ground-truth row present
    c["gt"][..., :4] = np.clip(c["bboxes"][:, ::-1, :] * 0.9, 0, None)
    rec, rec_gt = O.overlay_records(c["ids"], c["scores"], c["bboxes"], c["track"], c["gt"], size=(96, 128), **c["params"])
    assert (rec["nv"][-1] == 17).all() and rec["valid"].all() and rec_gt["valid"].all()
    _, painted = _check(c)
    assert painted[-1] > 1000


@pytest.mark.parametrize("name", ["rgb_L3", "rgb_L0"])
def test_nv12_contiguous_and_pitched(name):
    from viddet_amd import ops
    c = OC.make_case(**dict(OC.CASES[name], size=(32, 48)))
    nv = rgb_to_nv12(c["frames"])
    want, want_painted = _check(c, "nv12", nv)
    # the same frames on a pitched surface: 64 bytes a row, three rows of gap ahead of the UV plane, a tail behind every frame
    F, h0, w0, pitch = nv.shape[0], 32, 48, 64
    uv_offset, stride = pitch * (h0 + 3), pitch * (h0 + 3 + h0 // 2) + 32
    surf = np.full(F * stride, 0xA5, np.uint8)
    for f in range(F):
        for y in range(h0):
            surf[f * stride + y * pitch:f * stride + y * pitch + w0] = nv[f, y]
        for y in range(h0 // 2):
            o = f * stride + uv_offset + y * pitch
            surf[o:o + w0] = nv[f, h0 + y]
    want_surf = surf.copy()
    for f in range(F):
        for y in range(h0):
            want_surf[f * stride + y * pitch:f * stride + y * pitch + w0] = want[f, y]
        for y in range(h0 // 2):
            o = f * stride + uv_offset + y * pitch
            want_surf[o:o + w0] = want[f, h0 + y]
    args, kw = OC.call_args(c, "nv12")
    d = _dev(c)
    kw = dict(kw, track=d["track"], gt=d["gt"], H0=h0, W0=w0, pitch=pitch, uv_offset=uv_offset, frame_stride=stride)
    src = torch.from_numpy(surf).cuda()
    out = torch.full_like(src, 0xA5)
    got, painted = ops.overlay(src, d["ids"], d["scores"], d["bboxes"], out=out, **kw)
    torch.cuda.synchronize()
    assert got is out and torch.equal(out.cpu(), torch.from_numpy(want_surf))          # no byte between rows and planes touched
    assert torch.equal(painted.cpu(), torch.from_numpy(want_painted)) and torch.equal(src.cpu(), torch.from_numpy(surf))
    ops.overlay(src, d["ids"], d["scores"], d["bboxes"], out=src, **kw)
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), torch.from_numpy(want_surf))
    # a strided view of a pitched surface without a gap goes through its strides
    wide = torch.full((F, h0 * 3 // 2, pitch), 0x5A, dtype=torch.uint8, device="cuda")
    wide[..., :w0] = torch.from_numpy(nv).cuda()
    view = wide[..., :w0]
    del kw["H0"], kw["W0"], kw["pitch"], kw["uv_offset"], kw["frame_stride"]
    got, _ = ops.overlay(view, d["ids"], d["scores"], d["bboxes"], out=view, **kw)
    torch.cuda.synchronize()
    assert torch.equal(view.cpu(), torch.from_numpy(want)) and bool((wide[..., w0:] == 0x5A).all())
    # an odd-aligned surface (the byte path of NV12): the frames one byte into a buffer
    buf = torch.zeros(nv.size + 1, dtype=torch.uint8, device="cuda")
    off = buf[1:].view(nv.shape)
    off.copy_(torch.from_numpy(nv))
    ops.overlay(off, d["ids"], d["scores"], d["bboxes"], out=off, **kw)
    torch.cuda.synchronize()
    assert torch.equal(off.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("t,s", [(1, 1), (8, 1), (1, 4), (8, 4)])
def test_thickness_and_scale_at_their_ends(t, s):
    c = OC.make_case(21, 3, (48, 64), 6, G=2, trail=3, thickness=t, scale=s, class_names=OC.NAMES)
    _check(c)
    c = OC.make_case(22, 3, (37, 51), 6, G=2, trail=3, thickness=t, scale=s)
    _check(c)


def test_a_frame_with_no_valid_row_comes_out_unchanged():
    c = OC.make_case(31, 3, (48, 64), 6, trail=2)
    c["ids"][1] = -1.0                                                    # frame 1: nothing to draw
    want, painted = _check(c)
    assert painted[1] == 0 and np.array_equal(want[1], c["frames"][1]) and painted[0] > 0 and painted[2] > 0
    c = OC.make_case(32, 2, (37, 51), 5)
    c["scores"][:] = 0.1                                                  # and a whole call of them
    want, painted = _check(c)
    assert (painted == 0).all() and np.array_equal(want, c["frames"])


def test_each_stage_against_the_definitions_records():
    from viddet_amd import ops
    c = OC.case("rgb_L3")
    args, kw = OC.call_args(c)
    F, h0, w0 = c["frames"].shape[:3]
    N, G = c["bboxes"].shape[1], c["gt"].shape[1]
    rec, rec_gt = O.overlay_records(*args, kw["track"], kw["gt"], kw["clip_start"], size=(h0, w0), **c["params"])
    want_ws = np.concatenate([rec.reshape(-1), rec_gt.reshape(-1)]).view(np.uint8)
    d = _dev(c)
    kw = dict(kw, track=d["track"], gt=d["gt"])
    src = torch.from_numpy(c["frames"]).cuda()
    ws = torch.full((128 * F * (N + G) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    out, painted = ops.overlay(src, d["ids"], d["scores"], d["bboxes"], ws=ws, stages=1, **kw)
    torch.cuda.synchronize()
    got = ws.cpu().numpy()
    assert np.array_equal(got[:want_ws.size], want_ws) and (got[want_ws.size:] == 0xEE).all()      # the records, bit for bit
    assert (painted.cpu() == 0).all()                             # stage 1 resets the count
    # stage 2 alone paints whatever records the workspace holds: the definition's, uploaded
    want, want_painted = O.paint_records(c["frames"], rec, rec_gt, **c["params"])
    ws2 = torch.from_numpy(want_ws.copy()).cuda()
    got_out, got_painted = ops.overlay(src, d["ids"], d["scores"], d["bboxes"], ws=ws2, stages=2, **kw)
    torch.cuda.synchronize()
    assert torch.equal(got_out.cpu(), torch.from_numpy(want)) and torch.equal(got_painted.cpu(), torch.from_numpy(want_painted))
    full_out, full_painted = ops.overlay(src, d["ids"], d["scores"], d["bboxes"], **kw)
    torch.cuda.synchronize()
    assert torch.equal(full_out, got_out) and torch.equal(full_painted.cpu(), torch.from_numpy(want_painted))


def test_detect_video_with_overlay():
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c0", "c1"])
    net.initialize(init="he", obj_bias=1.0)                               # objectness up: rows exist
    net.set_device_resize(64, 64)
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (6, 40, 52, 3), dtype=np.uint8)         # a source size of its own: the boxes are scaled
    x = torch.from_numpy(frames).cuda()
    trk = dict(sigma_iou=0.1, sigma_h=0.0, t_min=1, max_age=2)
    plain = [t.clone() for t in net.detect_video(x, chunk=3, track=trk)]
    assert net.last_overlay is None
    assert (plain[0] >= 0).sum() > 10, "fixture produced (almost) no detections"
    gt = np.array([[[4, 4, 40, 50, 1, 0], [-1] * 6]] * 6, np.float32)
    opt = dict(thresh=float(plain[1][plain[0] >= 0].median()), trail=3, class_names=("cat", "dog"), gt=gt)
    got = [t.clone() for t in net.detect_video(x, chunk=3, track=trk, overlay=opt)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(plain, got)) and torch.equal(x.cpu(), torch.from_numpy(frames))
    out, painted = net.last_overlay
    kw = {k: v for k, v in opt.items() if k != "gt"}
    want, want_painted = O.overlay_host(frames, *[t.cpu().numpy() for t in got], track=net.last_tracks[0].cpu().numpy(), gt=gt,
                                        net_size=(64, 64), **kw)
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and torch.equal(painted.cpu(), torch.from_numpy(want_painted))
    assert want_painted.min() > 0
    # behind the tubelet pass: the rows it returns, under its track table; host frames are painted on their upload
    got = net.detect_video(torch.from_numpy(frames), chunk=3, track=trk, tubelet=True, overlay=True)
    out, painted = net.last_overlay
    want, want_painted = O.overlay_host(frames, *[t.cpu().numpy() for t in got], track=net.last_tubelet[1].cpu().numpy(),
                                        net_size=(64, 64))
    assert out.is_cuda and torch.equal(out.cpu(), torch.from_numpy(want)) and torch.equal(painted.cpu(), torch.from_numpy(want_painted))
    # without track: class colours, no trails; in place on device frames
    y = x.clone()
    got = net.detect_video(y, chunk=3, overlay=dict(inplace=True))
    want, _ = O.overlay_host(frames, *[t.cpu().numpy() for t in got], net_size=(64, 64))
    assert net.last_overlay[0] is y and torch.equal(y.cpu(), torch.from_numpy(want)) and net.last_tracks is None
    net.detect_video(x, chunk=3)
    assert net.last_overlay is None
    # NV12 frames: the palette follows set_device_resize(source='nv12')'s matrix and range
    net.set_device_resize(64, 64, source="nv12", matrix="bt709", range="full")
    nv = rgb_to_nv12(frames, "bt709", "full")
    z = torch.from_numpy(nv).cuda()
    got = net.detect_video(z, chunk=3, track=trk, overlay=dict(trail=2))
    want, want_painted = O.overlay_host(nv, *[t.cpu().numpy() for t in got], track=net.last_tracks[0].cpu().numpy(), net_size=(64, 64),
                                        trail=2, fmt="nv12", matrix="bt709", range="full")
    out, painted = net.last_overlay
    assert out.data_ptr() != z.data_ptr() and torch.equal(z.cpu(), torch.from_numpy(nv))
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and torch.equal(painted.cpu(), torch.from_numpy(want_painted))
    assert want_painted.sum() > 0
