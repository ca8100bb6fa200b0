"""GPU: the tracker on the device (vd_track, ops.track) equals its definition (viddet_amd.track.track_host, itself
held to a loop form in tests/test_track_cpu.py) bit for bit - all three outputs with torch.equal - on clips that tie, break,
cross the 64-lane boundary of the rows, fill the table of active tracks and span several clips and classes; then through
net.detect_video(track=...) and detect_yolo3.py --track."""
import os

import numpy as np
import pytest
import torch

from tests import track_cases as TC
from viddet_amd.track import clip_summary, track_host

pytestmark = pytest.mark.gpu


def _check(case, num_class, clip_start=None, **kw):
    from viddet_amd import ops
    host = [np.ascontiguousarray(a, dtype=np.float32) for a in case]
    stats = {}
    want = track_host(*host, clip_start=clip_start, num_class=num_class, stats=stats, **kw)
    ins = [torch.from_numpy(a).cuda() for a in host]
    keep = [t.clone() for t in ins]
    runs = [ops.track(*ins, clip_start=clip_start, num_class=num_class, **kw) for _ in range(2)]
    torch.cuda.synchronize()
    for name, g, g2, w in zip(("track", "tlen", "tscore"), runs[0], runs[1], want):
        assert g.dtype == torch.from_numpy(w).dtype and tuple(g.shape) == w.shape, name
        assert torch.equal(g.cpu(), torch.from_numpy(w)), name
        assert torch.equal(g, g2), name + ": two runs differ"
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ins, keep)), "an input was written"   # the bytes: a NaN stays
    return want, stats


@pytest.mark.parametrize("T,N", TC.SIZES, ids=["%dx%d" % s for s in TC.SIZES])
@pytest.mark.parametrize("max_age", [0, 1, 7])
def test_device_equals_host_over_the_sizes(T, N, max_age):
    case = TC.random_clip(T, N, seed=7 * T + N, spread=40.0 + N, fill=1.0 if N < 4 else 0.8)
    want, _ = _check(case, 1, max_age=max_age, t_min=1 if T == 1 else 2, sigma_h=0.05 if N < 4 else 0.5)
    assert (want[0] >= 0).any()
    if N > 64 and T > 1:
        # a row at or above the lane boundary that JOINED a track (a row of a kept track, not the track's first)
        first = np.full(int(want[0].max()) + 1, T)
        for t in range(T - 1, -1, -1):
            first[want[0][t][want[0][t] >= 0]] = t
        joined = (want[0] >= 0) & (np.arange(T)[:, None] > first[np.maximum(want[0], 0)])
        assert joined[:, 64:].any(), "no matched row above the lane boundary"


@pytest.mark.parametrize("extend", [False, True], ids=["grow", "extend"])
def test_the_table_of_active_tracks_at_its_capacity(extend):
    """F = 10, N = 128, max_age = 7.  Boxes disjoint from frame to frame: the table reaches exactly 1024 in the 8th frame and the
    first closures fall in the 9th (track_host's own bookkeeping).  The twin: all 128 tracks extend in every frame."""
    from viddet_amd import lib as L
    want, stats = _check(TC.capacity(extend), 1, max_age=7, t_min=1)
    if extend:
        assert stats["active"].tolist() == [128] * 10 and stats["closed"].sum() == 0
        assert (want[0] == np.arange(128)[None, :]).all() and (want[1] == 10).all()
    else:
        assert stats["active"][:8].tolist() == [128 * (t + 1) for t in range(8)] and stats["active"][7] == L.TRACK_MAX_ACTIVE
        assert stats["active"].max() == L.TRACK_MAX_ACTIVE
        assert stats["closed"][:8].sum() == 0 and stats["closed"][8] == 128 and stats["closed"][9] == 128
        assert (want[0] == np.arange(1280).reshape(10, 128)).all() and (want[1] == 1).all()


@pytest.mark.parametrize("name,case,kw,track,tlen", TC.closed_form(), ids=[c[0] for c in TC.closed_form()])
def test_closed_forms(name, case, kw, track, tlen):
    kw = dict(kw)
    want, _ = _check(case, kw.pop("num_class", 1), **kw)
    assert want[0].tolist() == np.asarray(track).tolist()


@pytest.mark.parametrize("classes,absent", [(1, ()), (3, (1,)), (20, (0, 7, 19))])
def test_classes_are_independent_and_may_be_absent(classes, absent):
    case = TC.random_clip(7, 40, classes=classes, seed=classes, absent=absent)
    want, _ = _check(case, classes)
    assert (want[0] >= 0).any()
    if classes == 20:                                                      # fewer classes than ids: the rows above are no candidates
        cut, _ = _check(case, 5)
        assert (cut[0][case[0][:, :, 0] >= 5] == -1).all() and (cut[0] >= 0).any()
    _check(case, classes, **TC.OFF_DEFAULT)


def test_clips_of_unequal_length_with_an_empty_one():
    from viddet_amd import ops
    one = TC.random_clip(6, 24, classes=2, seed=13, fill=1.0)
    case = [np.concatenate([a, a[:4]]) for a in one]                       # the same boxes on both sides of the boundary
    want, _ = _check(case, 2, clip_start=[0, 6, 6, 10], max_age=1)          # V = 3, the middle clip empty
    alone = track_host(*one, num_class=2, max_age=1)
    assert all(np.array_equal(a[:6], b) for a, b in zip(want, alone))
    dv = [torch.from_numpy(a).cuda() for a in case]
    cs = torch.tensor([0, 6, 6, 10], dtype=torch.int32, device="cuda")     # offsets already on the device are taken as they are
    got = ops.track(*dv, clip_start=cs, num_class=2, max_age=1)
    assert all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want))
    ws = torch.empty(8 * 10 * 24, dtype=torch.uint8, device="cuda")         # a workspace of the caller's
    got = ops.track(*dv, clip_start=cs, num_class=2, max_age=1, ws=ws)
    assert all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want))
    with pytest.raises(ValueError, match="clip_start"):
        ops.track(*dv, clip_start=[0, 6, 12], num_class=2)
    with pytest.raises(ValueError, match="max_age"):
        ops.track(*dv, max_age=8)
    with pytest.raises(ValueError, match="ws must be"):
        ops.track(*dv, ws=ws[:-1])
    with pytest.raises(ValueError, match="at most 128"):
        ops.track(torch.zeros(2, 129, 1, device="cuda"), torch.zeros(2, 129, 1, device="cuda"), torch.zeros(2, 129, 4, device="cuda"))


def test_detect_video_with_track():
    from viddet_amd import ops
    from viddet_amd.model import yolo3_darknet53
    from viddet_amd.seq_nms import seq_nms_host
    net = yolo3_darknet53(["c%d" % i for i in range(3)])
    net.initialize(init="he", obj_bias=1.0)                                # objectness up: rows exist
    x = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (7, 3, 64, 64)).astype(np.float32)).cuda()
    plain = [t.clone() for t in net.detect_video(x, chunk=3)]
    assert net.last_tracks is None
    assert (plain[0] >= 0).sum() > 10, "fixture produced (almost) no detections"
    kw = dict(sigma_h=0.0, max_age=1)
    got = [t.clone() for t in net.detect_video(x, chunk=3, track=kw)]
    tracks = net.last_tracks
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(plain, got)), "track changed what the call returns"
    direct = ops.track(*plain, num_class=3, **kw)
    want = track_host(*[t.cpu().numpy() for t in plain], num_class=3, **kw)
    for g, d, w in zip(tracks, direct, want):
        assert torch.equal(g, d) and torch.equal(g.cpu(), torch.from_numpy(w))
    print("tracked rows %d of %d" % ((want[0] >= 0).sum(), (plain[0] >= 0).sum()))
    assert (want[0] >= 0).any()
    # True: the defaults; clip: the boxes are clipped ahead of the IoUs
    net.detect_video(x, chunk=3, track=True)
    assert all(torch.equal(g, d) for g, d in zip(net.last_tracks, ops.track(*plain, num_class=3)))
    net.detect_video(x, chunk=3, track=dict(kw, clip=64))
    assert all(torch.equal(g, d) for g, d in zip(net.last_tracks, ops.track(plain[0], plain[1], plain[2].clamp(0, 64), num_class=3, **kw)))
    # with seq_nms too: the tracker runs on the rescored, re-sorted rows that are returned
    seq = [t.clone() for t in net.detect_video(x, chunk=3, seq_nms=True, track=kw)]
    tracks = net.last_tracks
    sw = seq_nms_host(*[t.cpu().numpy() for t in plain], num_class=3)
    assert all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(seq, sw[:3]))
    assert all(torch.equal(g, d) for g, d in zip(tracks, ops.track(*seq, num_class=3, **kw)))
    assert all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(tracks, track_host(*sw[:3], num_class=3, **kw)))
    # a call without track: as it was, and last_tracks is reset
    after = net.detect_video(x, chunk=3)
    torch.cuda.synchronize()
    assert net.last_tracks is None and all(torch.equal(a, b) for a, b in zip(plain, after))


def _parse(path, trk=False):
    rows = []
    with open(path) as f:
        for line in f:
            v = line.rstrip().split(",")
            assert len(v) == (8 if trk else 7)
            rows.append((v[0], int(v[1]), np.float32(v[2]), [np.float32(t) for t in v[3:7]]) + ((int(v[7]),) if trk else ()))
    return rows


@pytest.mark.parametrize("seq", [[], ["--seq_nms"]], ids=["plain", "seq_nms"])
@pytest.mark.parametrize("path", [["--stream"], []], ids=["stream", "windowed"])
def test_detect_script_track(tmp_path, path, seq):
    """--track on two synthetic clips, through net.detect_video (--stream) and through the windowed path: `pred` (and `pred_seq`)
    and the metric files are byte-equal to the run without it; every line of `pred_trk` is the line of `pred` plus the id
    track_host gives on the rows `pred` holds (--data_shape 64: a power of two, so the saved box / 64 gives the box back
    exactly, and a float32 prints round-trip); tracks.txt counts them."""
    import detect_yolo3 as D
    T, W = 5, 64
    common = ["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
              "--synthetic_samples", str(T), "--synthetic_videos", "2", "--data_shape", str(W), "--batch_size", "2",
              "--metrics", "vid,coco", "--save_dir", str(tmp_path)] + path + seq
    kw = dict(sigma_h=0.0, max_age=1)
    D.main(common + ["--save_prefix", "p"])
    D.main(common + ["--save_prefix", "q", "--track", "--track_high", "0", "--track_max_age", "1"])
    p, q = tmp_path / "p", tmp_path / "q"
    sets = [("pred", "pred_trk", "tracks.txt")] + ([("pred_seq", "pred_seq_trk", "tracks_seq.txt")] if seq else [])
    made = sorted(os.listdir(p))
    assert sorted(os.listdir(q)) == sorted(made + [s[1] for s in sets] + [s[2] for s in sets])
    for name in made:                                                      # everything a run without --track writes, byte for byte
        if os.path.isdir(p / name):
            assert sorted(os.listdir(p / name)) == sorted(os.listdir(q / name))
            for f in os.listdir(p / name):
                assert open(p / name / f).read() == open(q / name / f).read(), (name, f)
        else:
            assert open(p / name).read() == open(q / name).read(), name
    assert "vid.txt" in made and "coco.txt" in made and "pred" in made
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=T, window=3, step=1)
    order = [os.path.split(ds.sample_path(i))[1].split(".")[0] + ".txt" for i in range(2 * T)]
    for pred, twin, summary in sets:
        assert sorted(os.listdir(q / twin)) == sorted(order)
        rows = [_parse(q / pred / f) for f in order]
        N = max(1, max(len(r) for r in rows))
        assert sum(len(r) for r in rows) > 10, "fixture produced (almost) no detections"
        ids, scores, bboxes = -np.ones((2 * T, N, 1), np.float32), -np.ones((2 * T, N, 1), np.float32), -np.ones((2 * T, N, 4), np.float32)
        for t, r in enumerate(rows):
            for i, (_, id_, s, b) in enumerate(r):
                ids[t, i, 0], scores[t, i, 0], bboxes[t, i] = id_, s, np.asarray(b, np.float32) * np.float32(W)
        want = track_host(ids, scores, bboxes, clip_start=[0, T, 2 * T], **kw)
        assert (want[0] >= 0).any()
        for t, f in enumerate(order):
            plain_lines = open(q / pred / f).read().splitlines()
            twin_lines = open(q / twin / f).read().splitlines()
            assert twin_lines == ["%s,%d" % (l, want[0][t, i]) for i, l in enumerate(plain_lines)], f
        lines = ["{} {} {} {:.4f}".format(v, n, r, m) for v, (n, r, m) in enumerate(clip_summary(want[0], want[1], [0, T, 2 * T]))]
        assert open(q / summary).read().splitlines() == lines
