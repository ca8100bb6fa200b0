"""GPU: the stitching pass on the device (vd_track_stitch, ops.stitch) equals its definition
(viddet_amd.stitch.stitch_host, itself held to a loop form in tests/test_stitch_cpu.py) bit for bit on all five outputs - the
float one on its int32 view - on tables of sort_host with occlusion holes at the wave and row boundaries, on the closed forms,
the cap case, hostile tables, the two widest cases and several clips in one launch with a dirtied workspace of the caller's;
then through net.detect_video(track=..., stitch=...) and detect_yolo3.py --track --track_stitch."""
import os

import numpy as np
import pytest
import torch

from tests import smooth_cases as MC
from tests import stitch_cases as TC
from tests import stream_oracle as SO
from viddet_amd.stitch import stitch_host

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check(case, clip_start=None, num_class=1, ws=None, **kw):
    from viddet_amd import ops
    host = [np.ascontiguousarray(a, dtype=np.float32) for a in case[:3]] + [np.ascontiguousarray(case[3], dtype=np.int32)]
    ins = [torch.from_numpy(a).cuda() for a in host]
    keep = [t.clone() for t in ins]
    stats = {}
    want = stitch_host(*host, clip_start=clip_start, num_class=num_class, stats=stats, **kw)
    got = ops.stitch(*ins, clip_start=clip_start, num_class=num_class, ws=ws, **kw)
    torch.cuda.synchronize()
    assert [g.dtype for g in got] == [torch.int32, torch.int32, torch.float32, torch.int32, torch.int32]
    for name, g, w in zip(("strack", "tlen", "tscore", "stitches", "overflow"), got, want):
        assert torch.equal(_bits(g.cpu()), _bits(torch.from_numpy(w))), (name, kw)      # the bits of tscore: -0.0 too
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ins, keep)), "an input was written"
    return want, stats, got


@pytest.mark.parametrize("F,N", TC.HOLED_SIZES, ids=["%dx%d" % c for c in TC.HOLED_SIZES])
def test_device_equals_host_on_tables_of_sort_with_holes(F, N):
    case = TC.holed(F, N)
    want, stats, _ = _check(case, num_class=2)
    if F >= 6:
        assert want[3][0] > 0 and stats["pairs"][0] >= stats["links"][0] == want[3][0]        # something was linked
        few = _check(case, num_class=2, max_gap=3)[0]
        assert 0 < few[3][0] < want[3][0]                                                     # max_gap arrives
        few = _check(case, num_class=2, sigma_iou=0.7)[0]
        assert 0 < few[3][0] <= want[3][0]                                                    # and sigma_iou
        _check(TC.holed(F, N, max_age=7), num_class=2, max_gap=32)
    off = _check(case, num_class=2, sigma_iou=2.0)[0]                                         # nothing admissible: the tracker's ids
    assert np.array_equal(off[0], np.where(off[1] > 0, case[3], -1)) and off[3][0] == 0
    none = _check(case, num_class=1)[0]                                                       # class 1 is no candidate
    assert (none[0] == -1).sum() > (want[0] == -1).sum() or F == 1


CLOSED = [("hidden_12", TC.hidden_one, dict(max_gap=12), 0), ("hidden_13", TC.hidden_one, dict(max_gap=13), 1),
          ("crossing", TC.crossing, {}, 2), ("other_class", TC.other_class, {}, 0), ("three_fragments", TC.three_fragments, {}, 2),
          ("compete", TC.compete, {}, 1), ("nan_head", TC.nan_head, {}, 0), ("nan_tail", TC.nan_tail, {}, 0)]


@pytest.mark.parametrize("name,case,kw,links", CLOSED, ids=[c[0] for c in CLOSED])
def test_closed_forms(name, case, kw, links):
    want, _, got = _check(case(), num_class=2, **kw)
    assert int(got[3][0]) == links == want[3][0]
    if name == "compete":
        assert got[0].cpu().tolist() == [[0, 1]] * 3 + [[-1, -1]] * 2 + [[0, -1]] * 2


def test_the_cap():
    want, stats, got = _check(TC.cap(), max_gap=2)
    assert got[4].tolist() == [128] and got[3].tolist() == [256] and stats["tracks"] == [640]
    assert got[0][4].cpu().tolist() == list(range(512, 640)) and (got[1][4] == 1).all()       # tracks 512.. link nothing


@pytest.mark.parametrize("F,N", [(6, 65), (12, 128)], ids=["6x65", "12x128"])
def test_hostile_tables(F, N):
    case = MC.hostile(F, N)
    want, stats, _ = _check(case, sigma_iou=0.05)
    assert stats["tracks"][0] > 1 and (want[1] >= 2).any()
    _check(case, max_gap=1, sigma_iou=0.0)
    half = F // 2
    _check(case, clip_start=[0, half, F], sigma_iou=0.0)                                      # an id is an id inside its clip only


def test_the_widest_cases():
    want, stats, _ = _check(TC.sparse_wide())
    assert stats["tracks"] == [256] and want[3].tolist() == [128] and (want[1][want[0] >= 0] == 4).all()
    want, stats, _ = _check(TC.crowded_wide(), sigma_iou=0.05)
    assert stats["pairs"] == [32 * 32] and want[3].tolist() == [32]


def test_three_clips_in_one_launch_equal_three_launches_and_a_workspace_is_reused():
    from viddet_amd import lib as L
    from viddet_amd import ops
    ids, scores, bboxes, track, cs = TC.three_clips()
    F, N = track.shape
    ws = torch.full((L.TRACK_STITCH_WS_PER_ROW * F * N,), 0xA5, dtype=torch.uint8, device="cuda")   # whatever a last call left behind
    kw = dict(num_class=2, max_gap=12)
    want, stats, fresh = _check((ids, scores, bboxes, track), clip_start=cs, **kw)
    assert all(n > 0 for n in want[3]) and want[4].tolist() == [0, 0, 128]
    again = _check((ids, scores, bboxes, track), clip_start=cs, ws=ws, **kw)[2]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(fresh, again))
    for v, (a, b) in enumerate(zip(cs[:-1], cs[1:])):
        alone = _check((ids[a:b], scores[a:b], bboxes[a:b], track[a:b]), ws=ws, **kw)[2]
        assert all(torch.equal(_bits(fresh[k][a:b]), _bits(alone[k])) for k in range(3))
        assert int(fresh[3][v]) == int(alone[3][0]) and int(fresh[4][v]) == int(alone[4][0])
    # offsets on the device are taken as they are: an empty clip in the middle, and the last frame in no clip
    dv = [torch.from_numpy(a).cuda() for a in (ids, scores, bboxes, track)]
    offs = [0, cs[1], cs[1], cs[2], F - 1]
    dcs = torch.tensor(offs, dtype=torch.int32, device="cuda")
    want = stitch_host(ids[:F - 1], scores[:F - 1], bboxes[:F - 1], track[:F - 1], clip_start=offs, **kw)
    got = ops.stitch(*dv, clip_start=dcs, ws=ws, **kw)
    assert TC.same_five([g[:F - 1].cpu().numpy() for g in got[:3]] + [g.cpu().numpy() for g in got[3:]], want)
    assert (got[0][F - 1] == -1).all() and not got[1][F - 1].any() and (got[2][F - 1] == -1).all() and got[3].tolist()[1] == 0
    with pytest.raises(ValueError, match="ws must be"):
        ops.stitch(*dv, ws=ws[:-1])
    with pytest.raises(ValueError, match="clip_start"):
        ops.stitch(*dv, clip_start=[0, 6, 12])
    with pytest.raises(ValueError, match="max_gap"):
        ops.stitch(*dv, max_gap=33)
    with pytest.raises(ValueError, match="sigma_iou"):
        ops.stitch(*dv, sigma_iou=float("nan"))
    with pytest.raises(ValueError, match="track must be"):
        ops.stitch(dv[0], dv[1], dv[2], dv[3].float())
    with pytest.raises(ValueError, match="scores must be"):
        ops.stitch(dv[0], dv[1].cpu(), dv[2], dv[3])
    with pytest.raises(ValueError, match="num_class"):
        ops.stitch(*dv, num_class=0)
    z = torch.zeros(2, 129, 1, device="cuda")
    with pytest.raises(ValueError, match="at most 128"):
        ops.stitch(z, z, torch.zeros(2, 129, 4, device="cuda"), torch.zeros(2, 129, dtype=torch.int32, device="cuda"))


def _mk():
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(SO.C)], k=SO.K, k_join_type="max", k_join_pos="early")
    P = SO.params("max", "early")
    for name, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[name].astype(np.float32)))
    return net


def test_detect_video_with_stitch():
    from viddet_amd import ops
    net = _mk()
    x = torch.from_numpy(SO.clip_frames()).cuda()
    trk = dict(method="sort", sigma_iou=0.1, sigma_h=0.0, t_min=1, max_age=0)
    plain = [t.clone() for t in net.detect_video(x, chunk=3, track=trk)] + [net.last_rows.clone()]
    links = [t.clone() for t in net.last_tracks]
    tbox = net.last_track_boxes.clone()
    assert net.last_stitch is None and net.last_pre_stitch is None
    assert (plain[0] >= 0).sum() > 10, "fixture produced (almost) no detections"
    for arg, kw in ((True, {}), (dict(max_gap=3, sigma_iou=0.05), dict(max_gap=3, sigma_iou=0.05))):
        got = [t.clone() for t in net.detect_video(x, chunk=3, track=trk, stitch=arg)]
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, plain[:3])) and torch.equal(net.last_rows, plain[3])
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(net.last_pre_stitch, links))
        assert torch.equal(_bits(net.last_track_boxes), _bits(tbox))
        out = ops.stitch(plain[0], plain[1], plain[2], links[0], num_class=SO.C, **kw)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(net.last_tracks, out[:3]))
        assert torch.equal(net.last_stitch[0], out[3]) and torch.equal(net.last_stitch[1], out[4])
        want = stitch_host(plain[0].cpu().numpy(), plain[1].cpu().numpy(), plain[2].cpu().numpy(), links[0].cpu().numpy(),
                           num_class=SO.C, **kw)
        assert TC.same_five([o.cpu().numpy() for o in out], want)
        assert net.last_tubelet is None and net.last_smooth is None
        print("%r: %d rows, %d tracks, %d links" % (kw, (plain[0] >= 0).sum(), len(np.unique(links[0].cpu().numpy())) - 1, int(out[3][0])))
    # smooth and tubelet behind it take the stitched table
    sti = ops.stitch(plain[0], plain[1], plain[2], links[0], num_class=SO.C, max_gap=3, sigma_iou=0.05)
    got = [t.clone() for t in net.detect_video(x, chunk=3, track=trk, stitch=dict(max_gap=3, sigma_iou=0.05), smooth=True, tubelet=True)]
    sbox, slen = ops.smooth(plain[0], plain[1], plain[2], sti[0], num_class=SO.C)
    assert torch.equal(net.last_smooth, slen) and torch.equal(_bits(net.last_pre_tubelet[2]), _bits(sbox))
    tub = ops.tubelet(plain[0], plain[1], sbox, sti[0], num_class=SO.C)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, tub[:3]))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(net.last_tracks, sti[:3]))
    # track's clip: the pass runs on the clipped boxes the tracker saw
    net.detect_video(x, chunk=3, track=dict(trk, clip=SO.SIZE), stitch=True)
    out = ops.stitch(plain[0], plain[1], plain[2].clamp(0, SO.SIZE), net.last_pre_stitch[0], num_class=SO.C)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(net.last_tracks, out[:3]))
    with pytest.raises(ValueError, match="stitch needs track"):
        net.detect_video(x, chunk=3, stitch=True)
    with pytest.raises(ValueError, match="max_gap"):
        net.detect_video(x, chunk=3, track=trk, stitch=dict(max_gap=33))
    # a call without it afterwards: as it was
    after = list(net.detect_video(x, chunk=3, track=trk)) + [net.last_rows]
    torch.cuda.synchronize()
    assert net.last_stitch is None and net.last_pre_stitch is None and all(torch.equal(a, b) for a, b in zip(plain, after))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(net.last_tracks, links))


@pytest.mark.parametrize("path", [["--stream"], []], ids=["stream", "windowed"])
def test_detect_script_track_stitch(tmp_path, path):
    """--stream --track --track_method sort --track_stitch --metrics voc,mot,hota (and the windowed path on --synthetic_videos
    alone) writes byte for byte every file the run without --track_stitch writes, plus the _sti files; pred_sti_trk's lines are
    pred_trk's with other ids - those of stitch_host on the rows `pred_trk` holds."""
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticTracks
    T, W = 5, 64
    common = ["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
              "--synthetic_samples", str(T), "--synthetic_videos", "2", "--data_shape", str(W), "--batch_size", "2",
              "--metrics", "voc,mot,hota", "--save_dir", str(tmp_path), "--track", "--track_method", "sort", "--track_high", "0",
              "--track_min_len", "1", "--track_max_age", "0"] + path
    kw = dict(max_gap=4, sigma_iou=0.05)
    D.main(common + ["--save_prefix", "p"])
    D.main(common + ["--save_prefix", "q", "--track_stitch", "--track_stitch_gap", "4", "--track_stitch_iou", "0.05"])
    p, q = tmp_path / "p", tmp_path / "q"
    made = sorted(os.listdir(p))
    assert sorted(os.listdir(q)) == sorted(made + ["pred_sti_trk", "tracks_sti.txt", "mot_sti.txt", "hota_sti.txt"])
    for name in made:                                                      # everything a run without the flag writes, byte for byte
        if os.path.isdir(p / name):
            assert sorted(os.listdir(p / name)) == sorted(os.listdir(q / name))
            for f in os.listdir(p / name):
                assert open(p / name / f).read() == open(q / name / f).read(), (name, f)
        else:
            assert open(p / name).read() == open(q / name).read(), name
    assert "mot.txt" in made and "hota.txt" in made and "pred" in made and "pred_trk" in made
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=T, window=3, step=1)
    order = [os.path.split(ds.sample_path(i))[1].split(".")[0] + ".txt" for i in range(2 * T)]
    assert sorted(os.listdir(q / "pred_sti_trk")) == sorted(order)
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
    strack, tlen, _, stitches, overflow = stitch_host(ids, scores, bboxes, track, clip_start=[0, T, 2 * T], **kw)
    changed = 0
    for t, f in enumerate(order):
        twin = open(q / "pred_sti_trk" / f).read().splitlines()
        assert len(twin) == len(lines[t]), f
        for i, (a, b) in enumerate(zip(lines[t], twin)):
            a, b = a.split(","), b.split(",")
            assert a[:7] == b[:7], (f, i)                                  # the row itself: untouched
            assert int(b[7]) == strack[t, i], (f, i)
            changed += a[7] != b[7]
    rows = [l.split() for l in open(q / "tracks_sti.txt").read().splitlines()]
    assert [int(r[1]) for r in rows] == [len(np.unique(strack[a:a + T][strack[a:a + T] >= 0])) for a in (0, T)]
    print("rows %d, tracks %d, links %s, rows with another id %d" % ((ids >= 0).sum(), len(np.unique(track[track >= 0])),
                                                                      stitches.tolist(), changed))
    assert changed > 0 and stitches.sum() > 0 and not overflow.any()
