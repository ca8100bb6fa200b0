"""GPU: the tubelet pass on the device (vd_tubelet, ops.tubelet) equals its definition
(viddet_amd.tubelet.tubelet_host, itself held to a loop form in tests/test_tubelet_cpu.py) bit for bit - all six outputs with
torch.equal - on the closed forms and the random clips of tests/tubelet_cases.py under every parameter combination, on several
clips in one launch, with a workspace of the caller's; then through net.detect_video(track=..., tubelet=...) and
detect_yolo3.py --track --tubelet."""
import os

import numpy as np
import pytest
import torch

from tests import stream_oracle as SO
from tests import tubelet_cases as UC
from viddet_amd.track import track_host
from viddet_amd.tubelet import tubelet_host

pytestmark = pytest.mark.gpu
NAMES = ("ids", "scores", "bboxes", "perm", "track_out", "dropped")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check(data, track, clip_start=None, num_class=1, ws=None, **kw):
    from viddet_amd import ops
    host = [np.ascontiguousarray(a, dtype=np.float32) for a in data] + [np.ascontiguousarray(track, dtype=np.int32)]
    stats = {}
    want = tubelet_host(*host, clip_start=clip_start, num_class=num_class, stats=stats, **kw)
    ins = [torch.from_numpy(a).cuda() for a in host]
    keep = [t.clone() for t in ins]
    got = ops.tubelet(*ins, clip_start=clip_start, num_class=num_class, ws=ws, **kw)
    torch.cuda.synchronize()
    for name, g, w in zip(NAMES, got, want):
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), name
        assert torch.equal(_bits(g.cpu()), _bits(w)), (name, kw)           # the bits: -0.0 is not 0.0 here
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ins, keep)), "an input was written"
    return want, stats, got


@pytest.mark.parametrize("T,N,max_age", UC.RANDOM, ids=["%dx%d_age%d" % c for c in UC.RANDOM])
def test_device_equals_host_on_random_clips(T, N, max_age):
    ids, scores, bboxes, track = UC.random_case(T, N, max_age)
    filled = 0
    for kw in UC.PARAMS:
        _, stats, _ = _check((ids, scores, bboxes), track, **kw)
        filled = max(filled, stats["filled"][0])
    if T >= 5 and max_age >= 2:
        assert filled > 0


@pytest.mark.parametrize("name,data,track,kw,expect", UC.closed_form(), ids=[c[0] for c in UC.closed_form()])
def test_closed_forms(name, data, track, kw, expect):
    kw = dict(kw)
    cs, nc = kw.pop("clip_start", None), kw.pop("num_class", 1)
    _, _, got = _check(data, track, clip_start=cs, num_class=nc, **kw)
    UC.check_expected([g.cpu().numpy() for g in got], expect)
    for more in UC.PARAMS:
        _check(data, track, clip_start=cs, num_class=nc, **dict(kw, **more))


def test_three_clips_in_one_launch_equal_three_launches_and_a_workspace_is_reused():
    from viddet_amd import lib as L
    from viddet_amd import ops
    ids, scores, bboxes, track, cs = UC.three_clips()
    F, N = track.shape
    ws = torch.full((L.TUBELET_WS_PER_ROW * F * N,), 0xA5, dtype=torch.uint8, device="cuda")   # whatever a last call left behind
    for kw in (dict(), dict(rescore="max", max_gap=3, drop_untracked=True), dict(rescore=None)):
        want, stats, got = _check((ids, scores, bboxes), track, clip_start=cs, **kw)
        assert all(f > 0 for f in stats["filled"]) or kw.get("max_gap") == 0
        _, _, again = _check((ids, scores, bboxes), track, clip_start=cs, ws=ws, **kw)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again))
        for a, b in zip(cs[:-1], cs[1:]):
            _, _, alone = _check((ids[a:b], scores[a:b], bboxes[a:b]), track[a:b], ws=ws, **kw)
            assert all(torch.equal(_bits(g[a:b]), _bits(o)) for g, o in zip(got, alone))
    # offsets on the device are taken as they are; an empty clip in the middle
    dv = [torch.from_numpy(a).cuda() for a in (ids, scores, bboxes, track)]
    dcs = torch.tensor([0, 5, 5, 45, 51], dtype=torch.int32, device="cuda")
    want = tubelet_host(ids, scores, bboxes, track, clip_start=[0, 5, 5, 45, 51], num_class=1)
    got = ops.tubelet(*dv, clip_start=dcs)
    assert all(torch.equal(_bits(g.cpu()), _bits(torch.from_numpy(w))) for g, w in zip(got, want))
    # the launches one by one (vd_tubelet_stages), over one workspace: members, chain, then clear and frames
    ops.tubelet(*dv, clip_start=dcs, ws=ws, stages=2)
    ops.tubelet(*dv, clip_start=dcs, ws=ws, stages=4)
    staged = ops.tubelet(*dv, clip_start=dcs, ws=ws, stages=1 | 8)
    assert all(torch.equal(_bits(g), _bits(s)) for g, s in zip(got, staged))
    with pytest.raises(Exception, match="stages"):
        ops.tubelet(*dv, stages=16)
    with pytest.raises(ValueError, match="ws must be"):
        ops.tubelet(*dv, ws=ws[:-1])
    with pytest.raises(ValueError, match="clip_start"):
        ops.tubelet(*dv, clip_start=[0, 6, 12])
    with pytest.raises(ValueError, match="max_gap"):
        ops.tubelet(*dv, max_gap=8)
    with pytest.raises(ValueError, match="rescore"):
        ops.tubelet(*dv, rescore="mean")
    with pytest.raises(ValueError, match="drop_untracked"):
        ops.tubelet(*dv, drop_untracked=1)
    with pytest.raises(ValueError, match="track must be"):
        ops.tubelet(dv[0], dv[1], dv[2], dv[3].float())
    with pytest.raises(ValueError, match="scores must be"):
        ops.tubelet(dv[0], dv[1].cpu(), dv[2], dv[3])
    with pytest.raises(ValueError, match="num_class"):
        ops.tubelet(*dv, num_class=0)
    z = torch.zeros(2, 129, 1, device="cuda")
    with pytest.raises(ValueError, match="at most 128"):
        ops.tubelet(z, z, torch.zeros(2, 129, 4, device="cuda"), torch.zeros(2, 129, dtype=torch.int32, device="cuda"))


def test_several_classes():
    case = UC.random_clip(9, 40, classes=3, seed=3)
    track = track_host(*case, num_class=3, max_age=3, t_min=1, sigma_h=0.0)[0]
    _, stats, _ = _check(case, track, num_class=3)
    assert stats["filled"][0] > 0
    _check(case, track, num_class=2)                                       # class 2 is no candidate: its rows are not present


def _mk(k):
    from viddet_amd.model import yolo3_darknet53
    if k == 1:
        net = yolo3_darknet53(["c%d" % i for i in range(SO.C)])
        net.initialize(init="he", obj_bias=1.0)                            # objectness up: rows exist
        return net
    net = yolo3_darknet53(["c%d" % i for i in range(SO.C)], k=SO.K, k_join_type="max", k_join_pos="early")
    P = SO.params("max", "early")
    for name, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[name].astype(np.float32)))
    return net


@pytest.mark.parametrize("k,precision", [(3, "fp32"), (3, "bf16"), (1, "fp32")], ids=["k3_fp32", "k3_bf16", "k1_fp32"])
def test_detect_video_with_tubelet(k, precision):
    from viddet_amd import ops
    net = _mk(k)
    net.set_precision(precision)
    x = torch.from_numpy(SO.clip_frames()).cuda()
    trk = dict(sigma_iou=0.1, sigma_h=0.0, t_min=1, max_age=2)
    plain = [t.clone() for t in net.detect_video(x, chunk=3)] + [net.last_rows.clone()]
    assert net.last_tubelet is None and net.last_tracks is None
    assert (plain[0] >= 0).sum() > 10, "fixture produced (almost) no detections"
    # with track alone: what the call returned before, the tracks beside it
    tracked = [t.clone() for t in net.detect_video(x, chunk=3, track=trk)]
    links = [t.clone() for t in net.last_tracks]
    assert net.last_tubelet is None and net.last_pre_tubelet is None
    assert all(torch.equal(a, b) for a, b in zip(plain[:3], tracked)) and torch.equal(net.last_rows, plain[3])
    assert all(torch.equal(a, b) for a, b in zip(links, ops.track(*plain[:3], num_class=SO.C, **trk)))
    for arg, kw in ((True, {}), (dict(rescore="max", max_gap=1, drop_untracked=True), dict(rescore="max", max_gap=1, drop_untracked=True)),
                    (dict(rescore=None), dict(rescore=None))):
        got = [t.clone() for t in net.detect_video(x, chunk=3, track=trk, tubelet=arg)]
        torch.cuda.synchronize()
        pre = net.last_pre_tubelet
        assert all(torch.equal(a, b) for a, b in zip(pre, plain[:3])) and all(torch.equal(a, b) for a, b in zip(net.last_tracks, links))
        want = tubelet_host(*[t.cpu().numpy() for t in pre], net.last_tracks[0].cpu().numpy(), num_class=SO.C, **kw)
        for name, g, w in zip(NAMES, got + list(net.last_tubelet), want):
            assert torch.equal(_bits(g.cpu()), _bits(torch.from_numpy(w))), name
        perm = want[3]
        want_rows = np.where(perm >= 0, np.take_along_axis(plain[3].cpu().numpy(), np.maximum(perm, 0), axis=1), -1)
        assert np.array_equal(net.last_rows.cpu().numpy(), want_rows)
        print("k %d %s %r: rows %d -> %d, filled %d" % (k, precision, kw, (plain[0] >= 0).sum(), (want[0] >= 0).sum(), (perm == -2).sum()))
    # half of the rows below sigma_l: untracked rows to drop, which leaves room for fills
    low = dict(trk, sigma_l=float(plain[1][plain[0] >= 0].median()))
    got = [t.clone() for t in net.detect_video(x, chunk=3, track=low, tubelet=dict(drop_untracked=True))]
    want = tubelet_host(*[t.cpu().numpy() for t in net.last_pre_tubelet], net.last_tracks[0].cpu().numpy(), num_class=SO.C, drop_untracked=True)
    for name, g, w in zip(NAMES, got + list(net.last_tubelet), want):
        assert torch.equal(_bits(g.cpu()), _bits(torch.from_numpy(w))), name
    assert 0 < (want[0] >= 0).sum() < (plain[0] >= 0).sum()
    print("k %d %s sigma_l at the median: rows %d -> %d, filled %d" % (k, precision, (plain[0] >= 0).sum(), (want[0] >= 0).sum(), (want[3] == -2).sum()))
    # track's clip: the pass runs on the clipped boxes the tracker saw
    got = net.detect_video(x, chunk=3, track=dict(trk, clip=SO.SIZE), tubelet=True)
    clipped = plain[2].clamp(0, SO.SIZE)
    assert torch.equal(net.last_pre_tubelet[2], clipped)
    want = tubelet_host(plain[0].cpu().numpy(), plain[1].cpu().numpy(), clipped.cpu().numpy(), net.last_tracks[0].cpu().numpy(), num_class=SO.C)
    assert all(torch.equal(_bits(g.cpu()), _bits(torch.from_numpy(w))) for g, w in zip(got, want[:3]))
    if k == 3 and precision == "fp32":
        # behind Seq-NMS: the pass runs on the rescored, re-sorted rows the tracker saw
        got = net.detect_video(x, chunk=3, seq_nms=True, track=trk, tubelet=True)
        seq = ops.seq_nms(*plain[:3], num_class=SO.C)
        assert all(torch.equal(a, b) for a, b in zip(net.last_pre_tubelet, seq[:3]))
        want = tubelet_host(*[t.cpu().numpy() for t in seq[:3]], net.last_tracks[0].cpu().numpy(), num_class=SO.C)
        assert all(torch.equal(_bits(g.cpu()), _bits(torch.from_numpy(w))) for g, w in zip(got, want[:3]))
    # a call without it afterwards: as it was
    after = list(net.detect_video(x, chunk=3)) + [net.last_rows]
    torch.cuda.synchronize()
    assert net.last_tubelet is None and all(torch.equal(a, b) for a, b in zip(plain, after))


@pytest.mark.parametrize("path", [["--stream"], []], ids=["stream", "windowed"])
def test_detect_script_tubelet(tmp_path, path):
    """--stream --track --track_max_age 2 --tubelet (and the windowed path on --synthetic_videos alone) writes byte for byte
    every file the run without --tubelet writes, plus the _tub files; pred_tub holds the valid rows of the in-memory result,
    pred_tub_trk the same lines with the track id."""
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticTracks
    T, W = 5, 64
    common = ["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
              "--synthetic_samples", str(T), "--synthetic_videos", "2", "--data_shape", str(W), "--batch_size", "2",
              "--metrics", "vid,coco", "--save_dir", str(tmp_path), "--track", "--track_high", "0", "--track_max_age", "2"] + path
    D.main(common + ["--save_prefix", "p"])
    D.main(common + ["--save_prefix", "q", "--tubelet"])
    p, q = tmp_path / "p", tmp_path / "q"
    made = sorted(os.listdir(p))
    assert sorted(os.listdir(q)) == sorted(made + ["pred_tub", "pred_tub_trk", "tracks_tub.txt", "vid_tub.txt", "coco_tub.txt"])
    for name in made:                                                      # everything a run without --tubelet writes, byte for byte
        if os.path.isdir(p / name):
            assert sorted(os.listdir(p / name)) == sorted(os.listdir(q / name))
            for f in os.listdir(p / name):
                assert open(p / name / f).read() == open(q / name / f).read(), (name, f)
        else:
            assert open(p / name).read() == open(q / name).read(), name
    assert "vid.txt" in made and "coco.txt" in made and "pred" in made and "pred_trk" in made
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=T, window=3, step=1)
    order = [os.path.split(ds.sample_path(i))[1].split(".")[0] + ".txt" for i in range(2 * T)]
    assert sorted(os.listdir(q / "pred_tub")) == sorted(order) == sorted(os.listdir(q / "pred_tub_trk"))
    # the in-memory result: tubelet_host on the rows `pred_trk` holds (--data_shape 64: the saved box * 64 is the box, exactly)
    lines = [open(q / "pred_trk" / f).read().splitlines() for f in order]
    N = max(1, max(len(l) for l in lines))
    assert sum(len(l) for l in lines) > 10, "fixture produced (almost) no detections"
    ids, scores, bboxes = -np.ones((2 * T, N, 1), np.float32), -np.ones((2 * T, N, 1), np.float32), -np.ones((2 * T, N, 4), np.float32)
    track = -np.ones((2 * T, N), np.int32)
    for t, l in enumerate(lines):
        for i, line in enumerate(l):
            v = line.split(",")
            ids[t, i, 0], scores[t, i, 0], track[t, i] = int(v[1]), np.float32(v[2]), int(v[7])
            bboxes[t, i] = np.asarray([np.float32(c) for c in v[3:7]], np.float32) * np.float32(W)
    want = tubelet_host(ids, scores, bboxes, track, clip_start=[0, T, 2 * T])
    for t, f in enumerate(order):
        tub, twin = open(q / "pred_tub" / f).read().splitlines(), open(q / "pred_tub_trk" / f).read().splitlines()
        n = int((want[0][t] >= 0).sum())
        assert len(tub) == n == len(twin), f
        assert twin == ["%s,%d" % (l, want[4][t, i]) for i, l in enumerate(tub)], f
        for i, line in enumerate(tub):
            v = line.split(",")
            assert int(v[1]) == int(want[0][t, i, 0]) and np.float32(v[2]) == want[1][t, i, 0], (f, i)
    print("rows %d -> %d, filled %d" % ((ids >= 0).sum(), (want[0] >= 0).sum(), (want[3] == -2).sum()))
