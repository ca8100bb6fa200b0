"""GPU: the smoothing pass on the device (vd_track_smooth, ops.smooth) equals its definition
(viddet_amd.smooth.smooth_host, itself held to a textbook loop form in tests/test_smooth_cpu.py) bit for bit - sbox on its uint32
view, slen with torch.equal - on tables of sort_host at the wave and row boundaries, on the closed forms, on hostile tables, on
the deepest serial chain and on several clips in one launch with a dirtied workspace of the caller's; then through
net.detect_video(track=..., smooth=...) and detect_yolo3.py --track --track_smooth."""
import os

import numpy as np
import pytest
import torch

from tests import smooth_cases as MC
from tests import stream_oracle as SO
from viddet_amd.smooth import smooth_host

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check(case, clip_start=None, num_class=1, ws=None, gaps=MC.GAPS):
    from viddet_amd import ops
    host = [np.ascontiguousarray(a, dtype=np.float32) for a in case[:3]] + [np.ascontiguousarray(case[3], dtype=np.int32)]
    ins = [torch.from_numpy(a).cuda() for a in host]
    keep = [t.clone() for t in ins]
    out = []
    for g in gaps:
        stats = {}
        want = smooth_host(*host, clip_start=clip_start, num_class=num_class, max_gap=g, stats=stats)
        got = ops.smooth(*ins, clip_start=clip_start, num_class=num_class, max_gap=g, ws=ws)
        torch.cuda.synchronize()
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
        assert torch.equal(got[1].cpu(), torch.from_numpy(want[1])), ("slen", g)
        assert torch.equal(_bits(got[0].cpu()), _bits(torch.from_numpy(want[0]))), ("sbox", g)   # the bits: NaNs and -0.0 too
        out.append((want, stats, got))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ins, keep)), "an input was written"
    return out


@pytest.mark.parametrize("F,N,max_age", MC.SORT_TABLES, ids=["%dx%d_age%d" % c for c in MC.SORT_TABLES])
def test_device_equals_host_on_tables_of_sort(F, N, max_age):
    case = MC.sort_table(F, N, max_age)
    out = _check(case, num_class=2)
    if F >= 6:
        want, stats, _ = out[-1]
        assert (want[1] >= 2).any() and not MC.same_bits(want[0], case[2])          # something was smoothed
        if max_age == 7:
            assert stats["segments"][0] < out[0][1]["segments"][0]                 # max_gap 0 cuts tracks that max_gap 7 keeps
    _check(case, num_class=1, gaps=[7])                                             # class 1 is no candidate: its rows are no members


CLOSED = [("still", MC.still()), ("still_holes", MC.still([0, 1, 4, 5, 6, 9])), ("outlier", MC.outlier()), ("holed", MC.holed()),
          ("nan", MC.nan_case())]


@pytest.mark.parametrize("name,case", CLOSED, ids=[c[0] for c in CLOSED])
def test_closed_forms(name, case):
    out = _check(case)
    if name.startswith("still"):
        assert all(MC.same_bits(g[0].cpu().numpy(), case[2]) for _, _, g in out)
    if name == "still_holes":
        assert [w[1][:, 0].tolist() for w, _, _ in out] == [[2, 2, 0, 0, 3, 3, 3, 0, 0, 1], [6, 6, 0, 0, 6, 6, 6, 0, 0, 6],
                                                           [6, 6, 0, 0, 6, 6, 6, 0, 0, 6]]
    if name == "nan":
        got = out[-1][2][0].cpu().numpy()
        assert np.isnan(got).sum() == 1 and np.isnan(got[2, 0, 1])


def test_rows_that_keep_their_bits():
    ids, scores, bboxes, track, cs, slen = MC.keep_cases()
    for want, _, got in _check((ids, scores, bboxes, track), clip_start=cs):
        assert np.array_equal(got[1].cpu().numpy(), slen)
        moved = (got[0].cpu().numpy().view(np.uint32) != bboxes.view(np.uint32)).any(axis=2)
        assert moved.tolist() == (slen == 2).tolist()


@pytest.mark.parametrize("F,N", [(6, 65), (12, 128)], ids=["6x65", "12x128"])
def test_hostile_tables(F, N):
    case = MC.hostile(F, N)
    want, stats, _ = _check(case)[-1]
    assert (want[1] >= 2).any() and stats["members"][0] < (case[0] >= 0).sum()
    half = F // 2
    _check(case, clip_start=[0, half, F])                                           # an id is an id inside its clip only


def test_long_thin_clip():
    case = MC.long_thin()
    assert case[2].shape == (40, 2, 4)
    out = _check(case)
    assert [int(w[1].max()) for w, _, _ in out] == [9, 12, 27]                      # the longest segment at max_gap 0, 2 and 7


def test_three_clips_in_one_launch_equal_three_launches_and_a_workspace_is_reused():
    from viddet_amd import lib as L
    from viddet_amd import ops
    ids, scores, bboxes, track, cs = MC.three_clips()
    F, N = track.shape
    ws = torch.full((L.TRACK_SMOOTH_WS_PER_ROW * F * N,), 0xA5, dtype=torch.uint8, device="cuda")   # whatever a last call left behind
    fresh = _check((ids, scores, bboxes, track), clip_start=cs)
    again = _check((ids, scores, bboxes, track), clip_start=cs, ws=ws)
    for (_, _, a), (_, _, b) in zip(fresh, again):
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])
    for a, b in zip(cs[:-1], cs[1:]):
        alone = _check((ids[a:b], scores[a:b], bboxes[a:b], track[a:b]), ws=ws)
        for (_, _, g), (_, _, o) in zip(fresh, alone):
            assert torch.equal(_bits(g[0][a:b]), _bits(o[0])) and torch.equal(g[1][a:b], o[1])
    # offsets on the device are taken as they are: an empty clip in the middle, and the last frame in no clip - it keeps its bits
    dv = [torch.from_numpy(a).cuda() for a in (ids, scores, bboxes, track)]
    dcs = torch.tensor([0, 6, 6, 46, F - 1], dtype=torch.int32, device="cuda")
    want = smooth_host(ids[:F - 1], scores[:F - 1], bboxes[:F - 1], track[:F - 1], clip_start=[0, 6, 6, 46, F - 1], num_class=1)
    sbox, slen = ops.smooth(*dv, clip_start=dcs, ws=ws)
    assert MC.same_bits(sbox[:F - 1].cpu().numpy(), want[0]) and np.array_equal(slen[:F - 1].cpu().numpy(), want[1])
    assert MC.same_bits(sbox[F - 1].cpu().numpy(), bboxes[F - 1]) and not slen[F - 1].any()
    # the launches one by one (vd_track_smooth_stages), over one workspace: members, links, then clear and segments
    ops.smooth(*dv, clip_start=dcs, ws=ws, stages=2)
    ops.smooth(*dv, clip_start=dcs, ws=ws, stages=4)
    staged = ops.smooth(*dv, clip_start=dcs, ws=ws, stages=1 | 4 | 8)              # links writes the rows' default output
    assert torch.equal(_bits(staged[0]), _bits(sbox)) and torch.equal(staged[1], slen)
    with pytest.raises(Exception, match="stages"):
        ops.smooth(*dv, stages=16)
    with pytest.raises(ValueError, match="ws must be"):
        ops.smooth(*dv, ws=ws[:-1])
    with pytest.raises(ValueError, match="clip_start"):
        ops.smooth(*dv, clip_start=[0, 6, 12])
    with pytest.raises(ValueError, match="max_gap"):
        ops.smooth(*dv, max_gap=8)
    with pytest.raises(ValueError, match="track must be"):
        ops.smooth(dv[0], dv[1], dv[2], dv[3].float())
    with pytest.raises(ValueError, match="scores must be"):
        ops.smooth(dv[0], dv[1].cpu(), dv[2], dv[3])
    with pytest.raises(ValueError, match="num_class"):
        ops.smooth(*dv, num_class=0)
    z = torch.zeros(2, 129, 1, device="cuda")
    with pytest.raises(ValueError, match="at most 128"):
        ops.smooth(z, z, torch.zeros(2, 129, 4, device="cuda"), torch.zeros(2, 129, dtype=torch.int32, device="cuda"))


def _mk():
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(SO.C)], k=SO.K, k_join_type="max", k_join_pos="early")
    P = SO.params("max", "early")
    for name, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[name].astype(np.float32)))
    return net


def test_detect_video_with_smooth():
    from viddet_amd import ops
    net = _mk()
    x = torch.from_numpy(SO.clip_frames()).cuda()
    trk = dict(method="sort", sigma_iou=0.1, sigma_h=0.0, t_min=1, max_age=2)
    plain = [t.clone() for t in net.detect_video(x, chunk=3, track=trk)] + [net.last_rows.clone()]
    links = [t.clone() for t in net.last_tracks]
    tbox = net.last_track_boxes.clone()
    assert net.last_smooth is None and net.last_pre_smooth is None
    assert (plain[0] >= 0).sum() > 10, "fixture produced (almost) no detections"
    for arg, kw in ((True, {}), (dict(max_gap=0), dict(max_gap=0))):
        got = [t.clone() for t in net.detect_video(x, chunk=3, track=trk, smooth=arg)]
        torch.cuda.synchronize()
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and torch.equal(net.last_rows, plain[3])
        assert torch.equal(net.last_pre_smooth, plain[2])
        assert all(torch.equal(a, b) for a, b in zip(net.last_tracks, links)) and torch.equal(_bits(net.last_track_boxes), _bits(tbox))
        sbox, slen = ops.smooth(plain[0], plain[1], net.last_pre_smooth, links[0], num_class=SO.C, **kw)
        assert torch.equal(_bits(got[2]), _bits(sbox)) and torch.equal(net.last_smooth, slen)
        want = smooth_host(plain[0].cpu().numpy(), plain[1].cpu().numpy(), plain[2].cpu().numpy(), links[0].cpu().numpy(), num_class=SO.C, **kw)
        assert MC.same_bits(got[2].cpu().numpy(), want[0]) and np.array_equal(slen.cpu().numpy(), want[1])
        assert net.last_tubelet is None
        print("%r: %d rows, %d in segments of two or more, %d moved" % (kw, (plain[0] >= 0).sum(), (want[1] >= 2).sum(),
                                                                        (want[0] != plain[2].cpu().numpy()).any(axis=2).sum()))
    # track's clip: the pass runs on the clipped boxes the tracker saw
    got = net.detect_video(x, chunk=3, track=dict(trk, clip=SO.SIZE), smooth=True)
    clipped = plain[2].clamp(0, SO.SIZE)
    assert torch.equal(net.last_pre_smooth, clipped)
    sbox, _ = ops.smooth(plain[0], plain[1], clipped, net.last_tracks[0], num_class=SO.C)
    assert torch.equal(_bits(got[2]), _bits(sbox))
    # the tubelet pass behind it gets the smoothed boxes
    got = [t.clone() for t in net.detect_video(x, chunk=3, track=trk, smooth=True, tubelet=True)]
    sbox, slen = ops.smooth(plain[0], plain[1], plain[2], links[0], num_class=SO.C)
    assert torch.equal(_bits(net.last_pre_tubelet[2]), _bits(sbox)) and torch.equal(net.last_pre_smooth, plain[2])
    tub = ops.tubelet(plain[0], plain[1], sbox, links[0], num_class=SO.C)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, tub[:3]))
    with pytest.raises(ValueError, match="smooth needs track"):
        net.detect_video(x, chunk=3, smooth=True)
    with pytest.raises(ValueError, match="max_gap"):
        net.detect_video(x, chunk=3, track=trk, smooth=dict(max_gap=8))
    # a call without it afterwards: as it was
    after = list(net.detect_video(x, chunk=3, track=trk)) + [net.last_rows]
    torch.cuda.synchronize()
    assert net.last_smooth is None and net.last_pre_smooth is None and all(torch.equal(a, b) for a, b in zip(plain, after))


@pytest.mark.parametrize("path", [["--stream"], []], ids=["stream", "windowed"])
def test_detect_script_track_smooth(tmp_path, path):
    """--stream --track --track_method sort --track_smooth --metrics voc,mot,hota (and the windowed path on --synthetic_videos
    alone) writes byte for byte every file the run without --track_smooth writes, plus the _smo files; pred_smo's lines are
    pred's with other coordinates - those of smooth_host on the rows `pred_trk` holds - and pred_smo_trk's end in pred_trk's ids."""
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticTracks
    T, W = 5, 64
    common = ["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
              "--synthetic_samples", str(T), "--synthetic_videos", "2", "--data_shape", str(W), "--batch_size", "2",
              "--metrics", "voc,mot,hota", "--save_dir", str(tmp_path), "--track", "--track_method", "sort", "--track_high", "0",
              "--track_max_age", "2"] + path
    D.main(common + ["--save_prefix", "p"])
    D.main(common + ["--save_prefix", "q", "--track_smooth"])
    p, q = tmp_path / "p", tmp_path / "q"
    made = sorted(os.listdir(p))
    assert sorted(os.listdir(q)) == sorted(made + ["pred_smo", "pred_smo_trk", "tracks_smo.txt", "mot_smo.txt", "hota_smo.txt"])
    for name in made:                                                      # everything a run without the flag writes, byte for byte
        if os.path.isdir(p / name):
            assert sorted(os.listdir(p / name)) == sorted(os.listdir(q / name))
            for f in os.listdir(p / name):
                assert open(p / name / f).read() == open(q / name / f).read(), (name, f)
        else:
            assert open(p / name).read() == open(q / name).read(), name
    assert "mot.txt" in made and "hota.txt" in made and "pred" in made and "pred_trk" in made
    assert open(q / "tracks_smo.txt").read() == open(q / "tracks.txt").read()
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=T, window=3, step=1)
    order = [os.path.split(ds.sample_path(i))[1].split(".")[0] + ".txt" for i in range(2 * T)]
    assert sorted(os.listdir(q / "pred_smo")) == sorted(order) == sorted(os.listdir(q / "pred_smo_trk"))
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
    sbox, slen = smooth_host(ids, scores, bboxes, track, clip_start=[0, T, 2 * T])
    want = np.clip(sbox, 0, W) / W
    moved = 0
    for t, f in enumerate(order):
        plain, smo = open(q / "pred" / f).read().splitlines(), open(q / "pred_smo" / f).read().splitlines()
        twin = open(q / "pred_smo_trk" / f).read().splitlines()
        assert len(plain) == len(smo) == len(twin) == len(lines[t]), f
        assert twin == ["%s,%d" % (l, track[t, i]) for i, l in enumerate(smo)], f
        for i, (a, b) in enumerate(zip(plain, smo)):
            a, b = a.split(","), b.split(",")
            assert a[:3] == b[:3], (f, i)                                  # the path, the class and the score: untouched
            assert [np.float32(c) for c in b[3:7]] == want[t, i].tolist(), (f, i)
            moved += a[3:7] != b[3:7]
    assert moved > 0 and (slen >= 2).any()
    print("rows %d, in segments of two or more %d, moved %d" % ((ids >= 0).sum(), (slen >= 2).sum(), moved))
