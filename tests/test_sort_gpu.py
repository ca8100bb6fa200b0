"""GPU: SORT on the device (vd_track_sort, ops.track_sort) equals its definition (viddet_amd.sort.sort_host, itself
held to the paper's loop form in tests/test_sort_cpu.py) bit for bit - track, tlen and tscore with torch.equal, tbox on its bytes
wherever the definition's value is no NaN and a NaN wherever it is - on the closed forms, on clips that cross the 64-row boundary,
fill the table of active tracks and the assignment, hold degenerate boxes and span several clips; then through
net.detect_video(track={'method': 'sort'}) and detect_yolo3.py --track --track_method sort."""
import numpy as np
import pytest
import torch

from tests import sort_cases as SC
from viddet_amd.sort import sort_host
from viddet_amd.track import track_host

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    for name, g, w in zip(("track", "tlen", "tscore"), got, want):
        assert g.dtype == torch.from_numpy(w).dtype and tuple(g.shape) == w.shape, what + name
        assert torch.equal(g.cpu(), torch.from_numpy(w)), what + name
    assert got[3].dtype == torch.float32 and SC.same_tbox(got[3].cpu().numpy(), want[3]), what + "tbox"


def _check(case, num_class, clip_start=None, **kw):
    from viddet_amd import ops
    host = [np.ascontiguousarray(a, dtype=np.float32) for a in case]
    stats = {}
    want = sort_host(*host, clip_start=clip_start, num_class=num_class, stats=stats, **kw)
    ins = [torch.from_numpy(a).cuda() for a in host]
    keep = [t.clone() for t in ins]
    runs = [ops.track_sort(*ins, clip_start=clip_start, num_class=num_class, **kw) for _ in range(2)]
    torch.cuda.synchronize()
    _same(runs[0], want)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(runs[0], runs[1])), "two runs differ"
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ins, keep)), "an input was written"
    return want, stats


@pytest.mark.parametrize("name,case,kw,track,tlen", SC.closed_form(), ids=[c[0] for c in SC.closed_form()])
def test_closed_forms(name, case, kw, track, tlen):
    kw = dict(kw)
    want, _ = _check(case, kw.pop("num_class", 1), **kw)
    assert want[0].tolist() == np.asarray(track).tolist()


@pytest.mark.parametrize("T,N", SC.GPU_SIZES, ids=["%dx%d" % s for s in SC.GPU_SIZES])
@pytest.mark.parametrize("max_age", [0, 1, 7])
def test_device_equals_host_over_the_sizes(T, N, max_age):
    case = SC.random_clip(T, N, seed=7 * T + N, spread=40.0 + N, fill=1.0 if N < 4 else 0.8)
    want, _ = _check(case, 1, max_age=max_age, t_min=1 if T == 1 else 2, sigma_h=0.05 if N < 4 else 0.5)
    assert (want[0] >= 0).any()
    if N > 64 and T > 1:
        # a row at or above the lane boundary that JOINED a track (a row of a kept track, not the track's first)
        first = np.full(int(want[0].max()) + 1, T)
        for t in range(T - 1, -1, -1):
            first[want[0][t][want[0][t] >= 0]] = t
        joined = (want[0] >= 0) & (np.arange(T)[:, None] > first[np.maximum(want[0], 0)])
        assert joined[:, 64:].any(), "no matched row above the lane boundary"
    if T >= 3:                                                             # the same rows as clips: every one starts afresh
        cut, _ = _check(case, 1, clip_start=[0, T // 3, T // 3, T], max_age=max_age, t_min=1, sigma_h=0.05)
        assert all(np.array_equal(a[T // 3:], b, equal_nan=True)
                   for a, b in zip(cut, sort_host(*[a[T // 3:] for a in case], num_class=1, max_age=max_age, t_min=1, sigma_h=0.05)))


def test_classes_and_every_parameter_off_its_default():
    case = SC.random_clip(7, 40, classes=3, seed=3, absent=(1,))
    want, _ = _check(case, 3)
    assert (want[0] >= 0).any()
    _check(case, 3, sigma_l=0.3, sigma_h=0.7, sigma_iou=0.35, t_min=3, max_age=2)
    cut, _ = _check(case, 2)                                               # fewer classes than ids: the rows above are no candidates
    assert (cut[0][case[0][:, :, 0] >= 2] == -1).all()


@pytest.mark.parametrize("extend", [False, True], ids=["grow", "extend"])
def test_the_table_of_active_tracks_at_its_capacity(extend):
    """F = 10, N = 128, max_age = 7.  Boxes disjoint from frame to frame: the table reaches exactly 1024 in the 8th frame and the
    first closures fall in the 9th.  The twin: all 128 tracks are matched in every frame."""
    want, stats = _check(SC.capacity(extend), 1, max_age=7, t_min=1)
    if extend:
        assert stats["active"].tolist() == [128] * 10 and (want[1] == 10).all()
    else:
        assert stats["active"].max() == 1024 and stats["closed"][8] == 128 and (want[1] == 1).all()


def test_a_crowded_frame_pair():
    """128 admissible rows against 128 tracks, most rows with a dozen admissible cells, the rows in a shuffled order"""
    want, _ = _check(SC.crowded(), 1, t_min=1)
    assert (want[1] == 2).all() and want[0][1].tolist() != list(range(128))
    _check(SC.crowded(seed=6), 1, t_min=1, sigma_iou=0.6, max_age=0)       # fewer admissible cells: some rows take their dummy


def test_clips_of_unequal_length_a_frame_outside_and_a_reused_workspace():
    from viddet_amd import lib as L
    from viddet_amd import ops
    one = SC.random_clip(6, 24, classes=2, seed=13, fill=1.0)
    case = [np.concatenate([a, a[:4]]) for a in one]                       # the same boxes on both sides of the boundary
    want, _ = _check(case, 2, clip_start=[0, 6, 6, 10], max_age=1)          # V = 3, the middle clip empty
    alone = sort_host(*one, num_class=2, max_age=1)
    assert all(np.array_equal(a[:6], b, equal_nan=True) for a, b in zip(want, alone))
    dv = [torch.from_numpy(a).cuda() for a in case]
    cs = torch.tensor([0, 6, 6, 10], dtype=torch.int32, device="cuda")     # offsets already on the device are taken as they are
    _same(ops.track_sort(*dv, clip_start=cs, num_class=2, max_age=1), want, "device offsets: ")
    need = L.TRACK_SORT_WS_PER_ROW * 10 * 24 + L.TRACK_SORT_WS_PER_CLIP * 3
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")        # a workspace of the caller's, full of NaN bytes
    _same(ops.track_sort(*dv, clip_start=cs, num_class=2, max_age=1, ws=ws), want, "ws: ")
    _same(ops.track_sort(*dv, clip_start=cs, num_class=2, max_age=1, ws=ws), want, "ws again: ")
    # device offsets that leave the last frame outside every clip: its rows come out as -1 / 0 / -1 / -1
    short = torch.tensor([0, 6, 9], dtype=torch.int32, device="cuda")
    got = ops.track_sort(*dv, clip_start=short, num_class=2, max_age=1)
    head = sort_host(*[a[:9] for a in case], clip_start=[0, 6, 9], num_class=2, max_age=1)
    tail = (np.full((1, 24), -1, np.int32), np.zeros((1, 24), np.int32), np.full((1, 24), -1, np.float32), np.full((1, 24, 4), -1, np.float32))
    _same(got, [np.concatenate([h, t]) for h, t in zip(head, tail)], "a frame outside: ")
    with pytest.raises(ValueError, match="track_sort: clip_start"):
        ops.track_sort(*dv, clip_start=[0, 6, 12], num_class=2)
    with pytest.raises(ValueError, match="track_sort: max_age"):
        ops.track_sort(*dv, max_age=8)
    with pytest.raises(ValueError, match="track_sort: ws must be"):
        ops.track_sort(*dv, clip_start=cs, ws=ws[:-1])
    with pytest.raises(ValueError, match="track_sort: bboxes must be"):
        ops.track_sort(dv[0], dv[1], dv[2][:, :, :3])
    with pytest.raises(ValueError, match="track_sort: scores must be a contiguous float32 device tensor"):
        ops.track_sort(dv[0], dv[1].cpu(), dv[2])
    with pytest.raises(ValueError, match="at most 128"):
        ops.track_sort(torch.zeros(2, 129, 1, device="cuda"), torch.zeros(2, 129, 1, device="cuda"), torch.zeros(2, 129, 4, device="cuda"))


def test_detect_video_with_sort():
    from viddet_amd import ops
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(3)])
    net.initialize(init="he", obj_bias=1.0)                                # objectness up: rows exist
    x = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (7, 3, 64, 64)).astype(np.float32)).cuda()
    plain = [t.clone() for t in net.detect_video(x, chunk=3)]
    assert net.last_tracks is None and net.last_track_boxes is None
    assert (plain[0] >= 0).sum() > 10, "fixture produced (almost) no detections"
    kw = dict(sigma_h=0.0, max_age=2)
    got = [t.clone() for t in net.detect_video(x, chunk=3, track=dict(kw, method="sort"))]
    tracks, tbox = net.last_tracks, net.last_track_boxes
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(plain, got)), "track changed what the call returns"
    assert isinstance(tracks, tuple) and len(tracks) == 3
    want = sort_host(*[t.cpu().numpy() for t in plain], num_class=3, **kw)
    _same(tuple(tracks) + (tbox,), want)
    _same(ops.track_sort(*plain, num_class=3, **kw), want)
    print("tracked rows %d of %d" % ((want[0] >= 0).sum(), (plain[0] >= 0).sum()))
    assert (want[0] >= 0).any()
    # the method's own defaults; clip: the boxes are clipped ahead of the filter
    net.detect_video(x, chunk=3, track=dict(method="sort"))
    _same(tuple(net.last_tracks) + (net.last_track_boxes,), sort_host(*[t.cpu().numpy() for t in plain], num_class=3))
    net.detect_video(x, chunk=3, track=dict(kw, method="sort", clip=64))
    _same(tuple(net.last_tracks) + (net.last_track_boxes,),
          sort_host(plain[0].cpu().numpy(), plain[1].cpu().numpy(), plain[2].clamp(0, 64).cpu().numpy(), num_class=3, **kw))
    # the tubelet pass takes the table as it takes the IOU tracker's
    net.detect_video(x, chunk=3, track=dict(kw, method="sort"), tubelet=True)
    assert all(torch.equal(a, b) for a, b in zip(net.last_tracks, tracks))
    direct = ops.tubelet(*plain, tracks[0], num_class=3)
    assert all(torch.equal(a, b) for a, b in zip(net.last_tubelet, direct[3:6]))
    # track=True is the IOU tracker still, with no boxes beside it; a call without track resets both
    net.detect_video(x, chunk=3, track=True)
    assert net.last_track_boxes is None
    old = track_host(*[t.cpu().numpy() for t in plain], num_class=3)
    assert all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(net.last_tracks, old))
    after = net.detect_video(x, chunk=3)
    torch.cuda.synchronize()
    assert net.last_tracks is None and net.last_track_boxes is None and all(torch.equal(a, b) for a, b in zip(plain, after))
    with pytest.raises(NotImplementedError, match="open_video with track method 'sort'"):
        net.open_video(track=dict(method="sort"))


@pytest.mark.parametrize("path", [["--stream"], []], ids=["stream", "windowed"])
def test_detect_script_track_method_sort(tmp_path, path):
    """--track --track_method sort on two synthetic clips, through net.detect_video (--stream) and through the windowed path:
    every line of `pred_trk` is the line of `pred` plus the id sort_host gives on the rows `pred` holds (--data_shape 64: a power
    of two, so the saved box / 64 gives the box back exactly, and a float32 prints round-trip); tracks.txt counts them."""
    import os
    import detect_yolo3 as D
    from viddet_amd.track import clip_summary
    T, W = 5, 64
    D.main(["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
            "--synthetic_samples", str(T), "--synthetic_videos", "2", "--data_shape", str(W), "--batch_size", "2", "--save_dir",
            str(tmp_path), "--save_prefix", "q", "--track", "--track_method", "sort", "--track_high", "0", "--track_max_age", "2"] + path)
    q = tmp_path / "q"
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=T, window=3, step=1)
    order = [os.path.split(ds.sample_path(i))[1].split(".")[0] + ".txt" for i in range(2 * T)]
    assert sorted(os.listdir(q / "pred_trk")) == sorted(order)
    rows = []
    for f in order:
        with open(q / "pred" / f) as fh:
            rows.append([line.rstrip().split(",") for line in fh])
    N = max(1, max(len(r) for r in rows))
    assert sum(len(r) for r in rows) > 10, "fixture produced (almost) no detections"
    ids, scores, bboxes = -np.ones((2 * T, N, 1), np.float32), -np.ones((2 * T, N, 1), np.float32), -np.ones((2 * T, N, 4), np.float32)
    for t, r in enumerate(rows):
        for i, v in enumerate(r):
            ids[t, i, 0], scores[t, i, 0], bboxes[t, i] = int(v[1]), np.float32(v[2]), np.asarray([np.float32(c) for c in v[3:7]]) * np.float32(W)
    want = sort_host(ids, scores, bboxes, clip_start=[0, T, 2 * T], sigma_h=0.0, max_age=2)        # sigma_iou 0.3: the method's default
    assert (want[0] >= 0).any()
    for t, f in enumerate(order):
        plain_lines = open(q / "pred" / f).read().splitlines()
        assert open(q / "pred_trk" / f).read().splitlines() == ["%s,%d" % (l, want[0][t, i]) for i, l in enumerate(plain_lines)], f
    lines = ["{} {} {} {:.4f}".format(v, n, r, m) for v, (n, r, m) in enumerate(clip_summary(want[0], want[1], [0, T, 2 * T]))]
    assert open(q / "tracks.txt").read().splitlines() == lines
