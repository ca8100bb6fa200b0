"""CPU: the definition of camera-motion compensation (viddet_amd/motion.py) against loop oracles
(tests/motion_oracle.py) and closed forms: a shaking camera over a canvas, frames without a common motion, flat frames, and
what the stabilised frame does for the trackers."""
import numpy as np
import pytest

from tests import motion_cases as MC
from tests import motion_oracle as MO
from viddet_amd import motion as M
from viddet_amd.byte import byte_host
from viddet_amd.sort import sort_host
from viddet_amd.track import track_host


@pytest.mark.parametrize("radius", [1, 8, 11])
def test_match_host_equals_the_loop_oracle(radius):
    sig = MC.signatures(5, 24, 32, seed=radius)
    for cs in (None, [0, 2, 5]):
        for gate in (0.75, 1.0):
            got = M.match_host(sig, cs, radius, gate)
            want = MO.match_oracle(sig, cs, radius, gate)
            assert got[0].dtype == np.int32 and got[1].dtype == np.int64
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (cs, gate)
    assert M.match_host(sig, None, radius, 1.0)[0].any(), "nothing moved"
    got = M.match_host(sig, [0, 2, 5], radius, 1.0)
    assert not got[0][[0, 2]].any() and not got[1][[0, 2]].any(), "first frames of clips"


@pytest.mark.parametrize("fmt,shape", [("rgb", (2, 11, 21, 3)), ("nv12", (2, 18, 22))])
@pytest.mark.parametrize("cell", M.CELLS)
def test_signature_host_equals_the_loop_oracle(cell, fmt, shape):
    if cell > 8:
        shape = (shape[0], 48, 38) + shape[3:] if fmt == "nv12" else (shape[0], 33, 37, 3)
    fr = np.random.RandomState(cell).randint(0, 256, shape).astype(np.uint8)
    got = M.signature_host(fr, cell, fmt)
    assert got.dtype == np.uint16 and np.array_equal(got, MO.signature_oracle(fr, cell, fmt))


def test_the_largest_word():
    assert (M.signature_host(np.full((1, 16, 16, 3), 255, np.uint8), 16) == 65280).all()


@pytest.mark.parametrize("kind", ["blocks", "pixels"])
def test_shake_clip_closed_form(kind):
    fr = MC.shake_clip(kind)
    motion, sad = M.motion_host(fr, cell=4, radius=8)
    assert np.array_equal(motion, MC.MOTION) and not sad[:, 0].any() and sad[1:, 1].all()
    assert np.array_equal(M.cumulate(motion), -MC.CAM)
    two = np.concatenate([fr, fr[:5]])
    motion2, _ = M.motion_host(two, clip_start=[0, 12, 17])
    assert np.array_equal(motion2, np.concatenate([MC.MOTION, MC.MOTION[:5]]))
    nv = MC.to_nv12_luma(fr)
    assert np.array_equal(M.motion_host(nv, fmt="nv12")[0], MC.MOTION)


def test_uncorrelated_frames_are_gated():
    fr = MC.uncorrelated()
    motion, sad = M.motion_host(fr)
    print("sad_best / sad_zero:", (sad[1:, 0] / sad[1:, 1]).round(3).tolist())
    assert (4 * sad[1:, 0] > 3 * sad[1:, 1]).all(), "the fixture's own frames pass the gate"
    assert not motion.any()
    assert M.motion_host(fr, gate=1.0)[0].any()


def test_flat_frames_give_zero_motion_by_the_tie_rule():
    motion, sad = M.motion_host(np.full((4, 96, 128, 3), 77, np.uint8), gate=1.0)
    assert not motion.any() and not sad.any()
    sig = np.full((3, 24, 32), 500, np.uint16)
    sig[:, ::2] = 900                                                      # every even dy ties at 0: the shortest wins
    motion, sad = M.match_host(sig, gate=1.0)
    assert not motion.any() and not sad[:, 0].any()


def test_the_trackers_on_the_shake_clip():
    ids, scores, boxes = MC.two_objects()
    alt = lambda a, b: [a, b] * (MC.T // 2)
    plain = sort_host(ids, scores, boxes)[0]
    assert plain[:, 0].tolist() == alt(0, 2) and plain[:, 1].tolist() == alt(1, 3)
    assert len(set(byte_host(ids, scores, boxes)[0][:, 0].tolist())) > 2
    iou = track_host(ids, scores, boxes, sigma_iou=0.5, max_age=1)[0]
    assert iou[:, 0].tolist() == alt(0, 2) and (iou[:, 1] == -1).all()
    motion, _ = M.motion_host(MC.shake_clip())
    st = M.stabilise_host(ids, boxes, motion, None, 1.0, 1.0)
    assert np.array_equal(st[:, 0], np.tile(np.float32([44, 28, 84, 68]), (MC.T, 1)))
    for link, kw in ((sort_host, {}), (byte_host, {}), (track_host, dict(sigma_iou=0.5, max_age=1))):
        out = link(ids, scores, st, **kw)
        assert out[0].tolist() == [[0, 1]] * MC.T, link.__name__
        if len(out) == 4:                                                  # the filtered boxes back in image coordinates
            back = M.restore_host(out[0], out[3], motion, None, 1.0, 1.0)
            assert np.abs(back[:, 0] - boxes[:, 0]).max() < 1e-3


def test_stabilise_and_restore():
    rng = np.random.RandomState(2)
    F, N = 7, 5
    boxes = rng.uniform(-50, 500, (F, N, 4)).astype(np.float32)
    boxes[1, 2, 0], boxes[3, 0, 3] = np.nan, np.inf
    ids = rng.randint(-1, 3, (F, N, 1)).astype(np.float32)
    ids[2, 1, 0] = np.nan
    track = rng.randint(-1, 4, (F, N)).astype(np.int32)
    zero = np.zeros((F, 2), np.int32)
    for out in (M.stabilise_host(ids, boxes, zero, None, 1.0, 1.0), M.restore_host(track, boxes, zero, [0, 3, 7], 0.5, 2.0)):
        assert out.dtype == np.float32 and np.array_equal(out.view(np.int32), boxes.view(np.int32)), "zero motion moves bits"
    motion = rng.randint(-4000, 4001, (F, 2)).astype(np.int32)
    sx, sy = np.float32(416) / np.float32(1280), np.float32(416) / np.float32(720)
    for cs in (None, [0, 3, 7]):
        with np.errstate(invalid="ignore"):
            m_ids = (ids >= 0).reshape(F, N)
        got = M.stabilise_host(ids, boxes, motion, cs, sx, sy)
        want = MO.shift_oracle(m_ids, boxes, motion, cs, sx, sy, -1)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        got = M.restore_host(track, boxes, motion, cs, sx, sy)
        want = MO.shift_oracle(track >= 0, boxes, motion, cs, sx, sy, 1)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(M.cumulate(motion, [0, 3, 7])[3], motion[3])


def test_arguments():
    sig = np.zeros((2, 16, 40), np.uint16)
    with pytest.raises(ValueError, match="radius"):
        M.match_host(sig, radius=8)
    with pytest.raises(ValueError, match="radius"):
        M.match_host(np.zeros((2, 40, 16), np.uint16), radius=8)
    for kw, word in ((dict(radius=0), "radius"), (dict(radius=17), "radius"), (dict(gate=0.0), "gate"), (dict(gate=1.5), "gate"),
                     (dict(gate=float("nan")), "gate"), (dict(cell=3), "cell"), (dict(radius=True), "radius")):
        with pytest.raises(ValueError, match="match_host: " + word):
            M.match_host(np.zeros((2, 40, 40), np.uint16), **kw)
    with pytest.raises(ValueError, match="cell must be"):
        M.signature_host(np.zeros((1, 8, 8, 3), np.uint8), cell=5)
    with pytest.raises(ValueError, match="uint8"):
        M.signature_host(np.zeros((1, 8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="clip_start"):
        M.match_host(np.zeros((3, 40, 40), np.uint16), clip_start=[0, 2])
    # the option of detect_video
    assert M.split_gmc(dict(method="sort", gmc=True)) == (dict(method="sort"), True)
    assert M.split_gmc(True) == (True, None) and M.split_gmc(dict(method="sort"))[1] is None
    po = M.parse_option
    assert po(None, True, False, False, "w") is None and po(False, False, True, True, "w") is None
    assert po(True, True, False, False, "w") == dict(cell=4, radius=8, gate=0.75)
    assert po(dict(cell=8, radius=3), True, False, False, "w") == dict(cell=8, radius=3, gate=0.75)
    for args, word in (((True, False, False, False), "gmc needs track"), ((True, True, True, False), "gmc beside smooth"),
                       ((True, True, False, True), "gmc beside tubelet"), ((dict(cells=4), True, False, False), "gmc takes cell, radius and gate"),
                       ((dict(cell=5), True, False, False), "cell must be"), ((dict(radius=40), True, False, False), "radius must be"),
                       ((dict(gate=2), True, False, False), "gate must be")):
        with pytest.raises(ValueError, match="w.*" + word):
            po(*args, "w")


def test_synthetic_pan_labels_follow_the_camera():
    from viddet_amd.data import SyntheticPan, SyntheticTracks
    kw = dict(num_videos=2, frames_per_video=12, size=(128, 96))
    ds, world = SyntheticPan("vid", pan=24, cell=4, **kw), SyntheticTracks("vid", **kw)
    moved = False
    for v in range(2):
        cam = ds.camera_path(v)
        assert cam.shape == (12, 2) and not cam[0].any() and (cam % 4 == 0).all() and np.abs(np.diff(cam, axis=0)).max() <= 24
        moved |= bool(np.abs(np.diff(cam, axis=0)).max() > 0)
        frames = ds.video_frames(v)
        assert frames.shape == (12, 96, 128, 3) and frames.dtype == np.uint8
        motion, sad = M.motion_host(frames, radius=8)
        assert np.array_equal(M.cumulate(motion), -cam) and not sad[:, 0].any(), "frames are crops of one canvas"
        for t in range(12):
            w = world.get_label(world.sample_index(v, t) + 1)
            got = ds.get_label(ds.sample_index(v, t) + 1)
            want = w.copy()
            want[:, [0, 2]] = np.clip(w[:, [0, 2]] - cam[t, 0], 0, 127)
            want[:, [1, 3]] = np.clip(w[:, [1, 3]] - cam[t, 1], 0, 95)
            want = want[(want[:, 2] > want[:, 0]) & (want[:, 3] > want[:, 1])]
            assert np.array_equal(got, want), (v, t)
            img, label = ds[ds.sample_index(v, t)]
            assert np.array_equal(img, frames[t]) and np.array_equal(label[:, :5], got[:, :5]) and not label[:, 5].any()
    assert moved
    again = SyntheticPan("vid", pan=24, cell=4, **kw)
    assert np.array_equal(again.video_frames(1), ds.video_frames(1)), "seeded"
    with pytest.raises(ValueError, match="SyntheticPan needs"):
        SyntheticPan("vid", pan=2, cell=4, **kw)


GMC = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--stream", "--track", "--track_gmc"]


def test_detect_script_refuses_track_gmc_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    flags = D.parse_flags([])
    assert flags.track_gmc is False and flags.synthetic_pan == 0
    assert flags.track_gmc_cell is None and flags.track_gmc_radius is None and flags.track_gmc_gate is None
    assert D.gmc_args(flags) is None and "gmc" not in D.track_args(D.parse_flags(["--track"]))
    assert D.gmc_args(D.parse_flags(["--track_gmc"])) == dict(cell=4, radius=8, gate=0.75)
    given = D.parse_flags(["--track", "--track_gmc", "--track_gmc_cell", "8", "--track_gmc_radius", "3", "--track_gmc_gate", "0.5"])
    assert D.track_args(given)["gmc"] == dict(cell=8, radius=3, gate=0.5)
    with pytest.raises(NotImplementedError, match="--track_gmc needs --track"):
        D.main([a for a in GMC if a != "--track"])
    with pytest.raises(NotImplementedError, match="--track_gmc needs --stream"):
        D.main([a for a in GMC if a != "--stream"] + ["--synthetic_videos", "2"])
    with pytest.raises(NotImplementedError, match="--track_gmc does not combine with --live"):
        D.main(GMC + ["--live"])
    with pytest.raises(NotImplementedError, match="--track_gmc does not combine with --track_smooth"):
        D.main(GMC + ["--track_smooth"])
    with pytest.raises(NotImplementedError, match="--track_gmc does not combine with --tubelet"):
        D.main(GMC + ["--tubelet"])
    with pytest.raises(NotImplementedError, match="--track_gmc does not combine with --seq_nms"):
        D.main(GMC + ["--seq_nms"])
    with pytest.raises(NotImplementedError, match="--track_gmc_cell must be 2, 4, 8 or 16, got 3"):
        D.main(GMC + ["--track_gmc_cell", "3"])
    with pytest.raises(NotImplementedError, match="--track_gmc_radius must be an integer in \\[1, 16\\]"):
        D.main(GMC + ["--track_gmc_radius", "17"])
    for v in ("0", "1.5", "nan"):
        with pytest.raises(NotImplementedError, match="--track_gmc_gate must be a number in \\(0, 1\\]"):
            D.main(GMC + ["--track_gmc_gate", v])
    for sub in (["--track_gmc_cell", "4"], ["--track_gmc_radius", "8"], ["--track_gmc_gate", "0.75"]):
        with pytest.raises(NotImplementedError, match="%s needs --track_gmc" % sub[0]):
            D.main(GMC[:-1] + sub)
    with pytest.raises(NotImplementedError, match="--synthetic_pan takes"):
        D.main(GMC + ["--synthetic_pan", "-4"])
    for more in ([], ["--track_method", "sort"], ["--track_method", "byte"], ["--track_stitch"], ["--synthetic_pan", "24"],
                 ["--track_method", "sort", "--track_app"], ["--track_gmc_cell", "8", "--track_gmc_radius", "3", "--track_gmc_gate", "1"]):
        with pytest.raises(SystemExit, match="needs an MI355X"):           # and what is not refused gets as far as the GPU check
            D.main(GMC + more)
