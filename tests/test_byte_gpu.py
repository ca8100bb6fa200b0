"""GPU: BYTE on the device (vd_track_byte, ops.track_byte) equals its definition (viddet_amd.byte.byte_host, itself
held to the paper's loop form in tests/test_byte_cpu.py) bit for bit - track, tlen and tscore with torch.equal, tbox on its bytes
wherever the definition's value is no NaN and a NaN wherever it is - on the closed forms, on clips whose scores straddle the three
score thresholds and that cross the 64-row boundary, fill the table of active tracks and run both assignments wide, and span
several clips; then through net.detect_video(track={'method': 'byte'}) and detect_yolo3.py --track --track_method byte."""
import os

import numpy as np
import pytest
import torch

from tests import byte_cases as BC
from viddet_amd.byte import byte_host

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    for name, g, w in zip(("track", "tlen", "tscore"), got, want):
        assert g.dtype == torch.from_numpy(w).dtype and tuple(g.shape) == w.shape, what + name
        assert torch.equal(g.cpu(), torch.from_numpy(w)), what + name
    assert got[3].dtype == torch.float32 and BC.same_tbox(got[3].cpu().numpy(), want[3]), what + "tbox"


def _check(case, num_class, clip_start=None, **kw):
    from viddet_amd import ops
    host = [np.ascontiguousarray(a, dtype=np.float32) for a in case]
    stats = {}
    want = byte_host(*host, clip_start=clip_start, num_class=num_class, stats=stats, **kw)
    ins = [torch.from_numpy(a).cuda() for a in host]
    keep = [t.clone() for t in ins]
    runs = [ops.track_byte(*ins, clip_start=clip_start, num_class=num_class, **kw) for _ in range(2)]
    torch.cuda.synchronize()
    _same(runs[0], want)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(runs[0], runs[1])), "two runs differ"
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ins, keep)), "an input was written"
    return want, stats


@pytest.mark.parametrize("name,case,kw,track,tlen", BC.closed_form(), ids=[c[0] for c in BC.closed_form()])
def test_closed_forms(name, case, kw, track, tlen):
    kw = dict(kw)
    want, _ = _check(case, kw.pop("num_class", 1), **kw)
    assert want[0].tolist() == np.asarray(track).tolist()


@pytest.mark.parametrize("T,N", BC.GPU_SIZES, ids=["%dx%d" % s for s in BC.GPU_SIZES])
@pytest.mark.parametrize("max_age", [0, 1, 7])
def test_device_equals_host_over_the_sizes(T, N, max_age):
    """random_clip's scores come from a ladder of 12 values from 0.05 to 0.95: they straddle sigma_l, sigma_d and sigma_new"""
    case = BC.random_clip(T, N, seed=7 * T + N, spread=40.0 + N, fill=1.0 if N < 4 else 0.8)
    sc = case[1][case[0] >= 0]
    if N >= 63:
        assert (sc < 0.1).any() and ((sc >= 0.1) & (sc < 0.5)).any() and ((sc >= 0.5) & (sc < 0.6)).any() and (sc >= 0.6).any()
    kw = dict(max_age=max_age, t_min=1 if T == 1 else 2, sigma_h=0.05 if N < 4 else 0.5)
    if N < 4:
        kw.update(sigma_new=0.05, sigma_d=0.3)                             # the few rows there are may start tracks
    want, stats = _check(case, 1, **kw)
    assert (want[0] >= 0).any() or T == 1
    if N >= 63:
        assert stats["first"].sum() > 0 and stats["second"].sum() > 0
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
                   for a, b in zip(cut, byte_host(*[a[T // 3:] for a in case], num_class=1, max_age=max_age, t_min=1, sigma_h=0.05)))


@pytest.mark.parametrize("classes", [2, 3])
def test_classes_and_every_parameter_off_its_default(classes):
    case = BC.random_clip(7, 40, classes=classes, seed=3, absent=(1,) if classes == 3 else ())
    want, stats = _check(case, classes)
    assert (want[0] >= 0).any() and stats["second"].sum() > 0
    off, stats = _check(case, classes, sigma_l=0.2, sigma_d=0.45, sigma_new=0.7, sigma_iou=0.35, sigma_iou2=0.3, sigma_h=0.8, t_min=3,
                        max_age=2)
    assert (off[0] >= 0).any() and stats["second"].sum() > 0 and not np.array_equal(off[0], want[0])
    _check(case, classes, sigma_l=0.6, sigma_d=0.3, sigma_new=0.1)         # sigma_l above sigma_d: no low rows
    cut, _ = _check(case, classes - 1)                                     # fewer classes than ids: the rows above are no candidates
    assert (cut[0][case[0][:, :, 0] >= classes - 1] == -1).all()


@pytest.mark.parametrize("which", ["grow", "extend", "full"])
def test_the_table_of_active_tracks_at_its_capacity(which):
    """F = 10, N = 128, max_age = 7, every second frame's scores low (grow: disjoint boxes, nothing admissible; extend: all 128
    tracks matched by the second association in every odd frame); full: the table reaches 1024 in the 8th frame and the 9th
    frame's 128 low rows meet it in the second association."""
    case = dict(grow=lambda: BC.capacity_low(False), extend=lambda: BC.capacity_low(True), full=BC.capacity_full)[which]()
    want, stats = _check(case, 1, max_age=7, t_min=1)
    if which == "extend":
        assert stats["active"].tolist() == [128] * 10 and (want[1] == 10).all() and stats["second"].tolist() == [0, 128] * 5
    elif which == "grow":
        assert stats["active"].max() == 512 and stats["second"].sum() == 0 and (want[0][1::2] == -1).all()
    else:
        assert stats["active"].max() == 1024 and stats["second"].tolist() == [0] * 8 + [128, 0] and stats["closed"][8] == 128


def test_a_crowded_frame_pair():
    """64 high and 64 low rows against 128 tracks, most rows with a dozen admissible cells, the rows in a shuffled order: both
    associations displace earlier rows along their augmenting paths"""
    want, stats = _check(BC.crowded_pair(), 1, **BC.CROWDED_KW)
    assert stats["first"][1] >= 32 and stats["second"][1] >= 32
    assert want[0][1].tolist() != sorted(want[0][1].tolist())


def test_clips_of_unequal_length_a_frame_outside_and_a_reused_workspace():
    from viddet_amd import lib as L
    from viddet_amd import ops
    one = BC.random_clip(6, 24, classes=2, seed=13, fill=1.0)
    case = [np.concatenate([a, a[:4]]) for a in one]                       # the same boxes on both sides of the boundary
    want, stats = _check(case, 2, clip_start=[0, 6, 6, 10], max_age=1)      # V = 3, the middle clip empty
    assert stats["second"].sum() > 0
    alone = byte_host(*one, num_class=2, max_age=1)
    assert all(np.array_equal(a[:6], b, equal_nan=True) for a, b in zip(want, alone))
    dv = [torch.from_numpy(a).cuda() for a in case]
    cs = torch.tensor([0, 6, 6, 10], dtype=torch.int32, device="cuda")     # offsets already on the device are taken as they are
    _same(ops.track_byte(*dv, clip_start=cs, num_class=2, max_age=1), want, "device offsets: ")
    need = L.TRACK_SORT_WS_PER_ROW * 10 * 24 + L.TRACK_SORT_WS_PER_CLIP * 3
    assert need == L.load().vd_track_byte_ws_bytes(3, 10, 24)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")        # a workspace of the caller's, full of NaN bytes
    _same(ops.track_byte(*dv, clip_start=cs, num_class=2, max_age=1, ws=ws), want, "ws: ")
    _same(ops.track_byte(*dv, clip_start=cs, num_class=2, max_age=1, ws=ws), want, "ws again: ")
    # device offsets that leave the last frame outside every clip: its rows come out as -1 / 0 / -1 / -1
    short = torch.tensor([0, 6, 9], dtype=torch.int32, device="cuda")
    got = ops.track_byte(*dv, clip_start=short, num_class=2, max_age=1)
    head = byte_host(*[a[:9] for a in case], clip_start=[0, 6, 9], num_class=2, max_age=1)
    tail = (np.full((1, 24), -1, np.int32), np.zeros((1, 24), np.int32), np.full((1, 24), -1, np.float32), np.full((1, 24, 4), -1, np.float32))
    _same(got, [np.concatenate([h, t]) for h, t in zip(head, tail)], "a frame outside: ")
    with pytest.raises(ValueError, match="track_byte: clip_start"):
        ops.track_byte(*dv, clip_start=[0, 6, 12], num_class=2)
    with pytest.raises(ValueError, match="track_byte: max_age"):
        ops.track_byte(*dv, max_age=8)
    with pytest.raises(ValueError, match="track_byte: sigma_d must not be NaN"):
        ops.track_byte(*dv, sigma_d=float("nan"))
    with pytest.raises(ValueError, match="track_byte: ws must be"):
        ops.track_byte(*dv, clip_start=cs, ws=ws[:-1])
    with pytest.raises(ValueError, match="track_byte: bboxes must be"):
        ops.track_byte(dv[0], dv[1], dv[2][:, :, :3])
    with pytest.raises(ValueError, match="track_byte: scores must be a contiguous float32 device tensor"):
        ops.track_byte(dv[0], dv[1].cpu(), dv[2])
    with pytest.raises(ValueError, match="at most 128"):
        ops.track_byte(torch.zeros(2, 129, 1, device="cuda"), torch.zeros(2, 129, 1, device="cuda"), torch.zeros(2, 129, 4, device="cuda"))


def test_detect_video_with_byte():
    from viddet_amd import ops
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(3)])
    net.initialize(init="he", obj_bias=1.0)                                # objectness up: rows exist
    x = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (7, 3, 64, 64)).astype(np.float32)).cuda()
    plain = [t.clone() for t in net.detect_video(x, chunk=3)]
    assert net.last_tracks is None and net.last_track_boxes is None
    sc = plain[1][plain[0] >= 0]
    assert sc.numel() > 10, "fixture produced (almost) no detections"
    # the split at the rows' median score: half of them are high rows, half low; a track starts a little above it
    sd = float(sc.median())
    kw = dict(sigma_l=0.0, sigma_d=sd, sigma_new=sd, sigma_h=0.0, max_age=2)
    got = [t.clone() for t in net.detect_video(x, chunk=3, track=dict(kw, method="byte"))]
    tracks, tbox = net.last_tracks, net.last_track_boxes
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(plain, got)), "track changed what the call returns"
    assert isinstance(tracks, tuple) and len(tracks) == 3
    stats = {}
    want = byte_host(*[t.cpu().numpy() for t in plain], num_class=3, stats=stats, **kw)
    _same(tuple(tracks) + (tbox,), want)
    _same(ops.track_byte(*plain, num_class=3, **kw), want)
    print("tracked rows %d of %d, pairs %d + %d" % ((want[0] >= 0).sum(), (plain[0] >= 0).sum(), stats["first"].sum(), stats["second"].sum()))
    assert (want[0] >= 0).any()
    # the method's own defaults; clip: the boxes are clipped ahead of the filter
    net.detect_video(x, chunk=3, track=dict(method="byte"))
    _same(tuple(net.last_tracks) + (net.last_track_boxes,), byte_host(*[t.cpu().numpy() for t in plain], num_class=3))
    net.detect_video(x, chunk=3, track=dict(kw, method="byte", clip=64))
    _same(tuple(net.last_tracks) + (net.last_track_boxes,),
          byte_host(plain[0].cpu().numpy(), plain[1].cpu().numpy(), plain[2].clamp(0, 64).cpu().numpy(), num_class=3, **kw))
    # the tubelet pass takes the table as it takes SORT's
    net.detect_video(x, chunk=3, track=dict(kw, method="byte"), tubelet=True)
    assert all(torch.equal(a, b) for a, b in zip(net.last_tracks, tracks))
    direct = ops.tubelet(*plain, tracks[0], num_class=3)
    assert all(torch.equal(a, b) for a, b in zip(net.last_tubelet, direct[3:6]))
    # a call without track is unchanged and resets both
    after = net.detect_video(x, chunk=3)
    torch.cuda.synchronize()
    assert net.last_tracks is None and net.last_track_boxes is None and all(torch.equal(a, b) for a, b in zip(plain, after))
    with pytest.raises(NotImplementedError, match="open_video with track method 'byte'"):
        net.open_video(track=dict(method="byte"))


def _tree(root):
    return [os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files]


def test_detect_script_track_method_byte(tmp_path):
    """--track --track_method byte --tubelet --metrics mot,hota on two synthetic clips: every line of `pred_trk` is the line of
    `pred` plus the id byte_host gives on the rows `pred` holds (--data_shape 64: a power of two, so the saved box / 64 gives
    the box back exactly, and a float32 prints round-trip); tracks.txt counts them; mot.txt and hota.txt and the _tub files are
    written.  A run without byte writes what it wrote before: the IOU tracker's ids at its own defaults (--track_low left out
    is 0.0 there), the same files."""
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticTracks
    from viddet_amd.track import clip_summary, track_host
    T, W = 5, 64
    base = ["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
            "--synthetic_samples", str(T), "--synthetic_videos", "2", "--data_shape", str(W), "--batch_size", "2", "--save_prefix", "q",
            "--track", "--track_high", "0", "--metrics", "mot,hota"]
    D.main(base + ["--save_dir", str(tmp_path / "i")])
    q, qi = tmp_path / "b" / "q", tmp_path / "i" / "q"
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=T, window=3, step=1)
    order = [os.path.split(ds.sample_path(i))[1].split(".")[0] + ".txt" for i in range(2 * T)]
    rows = []
    for f in order:
        with open(qi / "pred" / f) as fh:
            rows.append([line.rstrip().split(",") for line in fh])
    N = max(1, max(len(r) for r in rows))
    assert sum(len(r) for r in rows) > 10, "fixture produced (almost) no detections"
    ids, scores, bboxes = -np.ones((2 * T, N, 1), np.float32), -np.ones((2 * T, N, 1), np.float32), -np.ones((2 * T, N, 4), np.float32)
    for t, r in enumerate(rows):
        for i, v in enumerate(r):
            ids[t, i, 0], scores[t, i, 0], bboxes[t, i] = int(v[1]), np.float32(v[2]), np.asarray([np.float32(c) for c in v[3:7]]) * np.float32(W)
    # the split at the median score of the rows the untrained heads let through: half of them high rows, half low
    sd = repr(float(np.median(scores[ids >= 0])))
    D.main(base + ["--save_dir", str(tmp_path / "b"), "--track_method", "byte", "--track_low", "0", "--track_det", sd, "--track_new", sd,
                   "--track_max_age", "2", "--tubelet"])
    assert sorted(os.listdir(q / "pred_trk")) == sorted(order) == sorted(os.listdir(qi / "pred_trk"))
    for f in order:
        assert open(q / "pred" / f, "rb").read() == open(qi / "pred" / f, "rb").read()             # the detections do not depend on it
    cs = [0, T, 2 * T]
    stats = {}
    want = byte_host(ids, scores, bboxes, clip_start=cs, sigma_l=0.0, sigma_d=float(sd), sigma_new=float(sd), sigma_h=0.0, max_age=2,
                     stats=stats)
    print("pairs of the two associations: %d + %d" % (stats["first"].sum(), stats["second"].sum()))
    old = track_host(ids, scores, bboxes, clip_start=cs, sigma_h=0.0)                              # sigma_l 0.0, sigma_iou 0.5, max_age 0
    assert (want[0] >= 0).any() and (old[0] >= 0).any()
    for root, res in ((q, want), (qi, old)):
        for t, f in enumerate(order):
            plain_lines = open(root / "pred" / f).read().splitlines()
            assert open(root / "pred_trk" / f).read().splitlines() == ["%s,%d" % (l, res[0][t, i]) for i, l in enumerate(plain_lines)], f
        lines = ["{} {} {} {:.4f}".format(v, n, r, m) for v, (n, r, m) in enumerate(clip_summary(res[0], res[1], cs))]
        assert open(root / "tracks.txt").read().splitlines() == lines
        for name in ("mot.txt", "hota.txt"):
            assert len(open(root / name).read().splitlines()) > 3, name
    byte_files, iou_files = set(_tree(q)), set(_tree(qi))
    new = byte_files - iou_files                                           # what --tubelet adds; nothing else differs in name
    assert iou_files <= byte_files and {"tracks_tub.txt", "mot_tub.txt", "hota_tub.txt"} <= new
    assert any(k.startswith("pred_tub_trk" + os.sep) for k in new) and any(k.startswith("pred_tub" + os.sep) for k in new)
    assert all("tub" in k for k in new)
