"""GPU: the MOT metric's matching on the device (vd_mot_match, ops.mot_match) equals its definition
(viddet_amd.mot_metric.mot_match_host, itself held to a loop form in tests/test_mot_metric_cpu.py) in every bit of all four
outputs - on the random clips of tests/mot_oracle.py, on the closed forms of tests/mot_cases.py, on several clips in one launch,
with a workspace of the caller's; then DeviceMOTMetric against MOTMetric and detect_yolo3.py --track --metrics mot."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import mot_cases as MC
from tests import mot_oracle as MO
from viddet_amd import mot_metric as M

pytestmark = pytest.mark.gpu
NAMES = ("match", "miou", "flags", "adm")
DTYPES = (np.float32, np.int32, np.int32, np.float32, np.float32, np.float32, np.int32)


@functools.lru_cache(maxsize=None)
def _cases():
    """the random clips with the host's records, computed once"""
    return [(name, arrays, kw, M.mot_match_host(*arrays, **kw)) for name, arrays, kw in MO.random_cases()]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(arrays, want=None, ws=None, **kw):
    from viddet_amd import ops
    host = [np.ascontiguousarray(a, dtype=dt) for a, dt in zip(arrays, DTYPES)]
    if want is None:
        want = M.mot_match_host(*host, **kw)
    ins = [torch.from_numpy(a).cuda() for a in host]
    keep = [t.clone() for t in ins]
    got = ops.mot_match(*ins, ws=ws, **kw)
    torch.cuda.synchronize()
    got = [g.cpu().numpy() for g in got]
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype.itemsize == 4, name
        assert np.array_equal(_bits(g), _bits(w)), (name, kw, np.argwhere(_bits(g) != _bits(w))[:5].tolist())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ins, keep)), "an input was written"
    return want, got


@pytest.mark.parametrize("k", range(len(MO.random_cases())), ids=[c[0] for c in MO.random_cases()])
def test_device_equals_host_on_random_clips(k):
    name, arrays, kw, want = _cases()[k]
    _check(arrays, want, **kw)


@pytest.mark.parametrize("k", range(len(MO.tie_cases())), ids=[c[0] for c in MO.tie_cases()])
def test_device_equals_host_where_equal_costs_abound(k):
    """the lowest column of equal least slack, across the wavefronts of the workgroup"""
    name, arrays, kw = MO.tie_cases()[k]
    _check(arrays, **kw)


@pytest.mark.parametrize("name,arrays,kw,expect", MC.closed_forms(), ids=[c[0] for c in MC.closed_forms()])
def test_closed_forms(name, arrays, kw, expect):
    want, got = _check(arrays, **kw)
    trk = M.masked_track(arrays[3], arrays[4], arrays[6], kw.get("num_class"))
    MC.check_expected(got, M.mot_summary(got, arrays[2], trk, kw.get("clip_start")), expect)


def test_three_clips_in_one_launch_equal_three_launches_and_a_workspace_is_reused():
    from viddet_amd import lib as L
    from viddet_amd import ops
    name, arrays, kw, want = [c for c in _cases() if c[0] == "clips_age7_cls"][0]
    cs = kw["clip_start"]
    assert cs == MO.THREE_CLIPS and cs[1] == cs[2]                         # an empty clip in the middle
    F, G, N = arrays[0].shape[0], arrays[0].shape[1], arrays[5].shape[1]
    ws = torch.full((L.MOT_WS_PER_ROW * F * (G + N),), 0xA5, dtype=torch.uint8, device="cuda")   # whatever a last call left behind
    _, got = _check(arrays, want, **kw)
    _, again = _check(arrays, want, ws=ws, **kw)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))
    one = dict(kw)
    del one["clip_start"]
    for a, b in zip(cs[:-1], cs[1:]):
        if b > a:
            _, alone = _check([x[a:b] for x in arrays], ws=ws, **one)
            assert all(np.array_equal(_bits(g[a:b]), _bits(o)) for g, o in zip(got, alone))
    # offsets on the device are taken as they are: the frames that no clip covers come out as -2 / 0 / 0 / 0
    dv = [torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda() for x, dt in zip(arrays, DTYPES)]
    dcs = torch.tensor([0, 5, 5, 19], dtype=torch.int32, device="cuda")
    part = [g.cpu().numpy() for g in ops.mot_match(*dv, clip_start=dcs, ws=ws, **one)]
    head = M.mot_match_host(*[x[:19] for x in arrays], clip_start=[0, 5, 5, 19], **one)
    for g, w, fill in zip(part, head, (-2, 0, 0, 0)):
        assert np.array_equal(_bits(g[:19]), _bits(w)) and (g[19:] == fill).all()
    with pytest.raises(ValueError, match="ws must be"):
        ops.mot_match(*dv, ws=ws[:-1])
    with pytest.raises(ValueError, match="clip_start"):
        ops.mot_match(*dv, clip_start=[0, 6, 12])
    with pytest.raises(ValueError, match="iou_thresh"):
        ops.mot_match(*dv, iou_thresh=0.0)
    with pytest.raises(ValueError, match="agnostic"):
        ops.mot_match(*dv, agnostic=1)
    with pytest.raises(ValueError, match="num_class"):
        ops.mot_match(*dv, num_class=0)
    with pytest.raises(ValueError, match="track must be"):
        ops.mot_match(*dv[:6], dv[6].float())
    with pytest.raises(ValueError, match="gt_id must be"):
        ops.mot_match(dv[0], dv[1], dv[2].cpu(), *dv[3:])
    with pytest.raises(ValueError, match="gt_cls must be"):
        ops.mot_match(dv[0], dv[1].reshape(-1), *dv[2:])
    z = torch.zeros(F, 129, 4, device="cuda")
    with pytest.raises(ValueError, match="1 to 128"):
        ops.mot_match(z, *dv[1:])
    with pytest.raises(ValueError, match="1 to 128"):
        ops.mot_match(*dv[:5], z, dv[6])


def _tracked_rows(ds, seed=3):
    """per sample id the ground truth jittered, thinned and with clutter, linked by track_host: rows a tracker could have made"""
    from viddet_amd.track import track_host
    rng = np.random.default_rng(seed)
    sids = ds.get_sample_ids()
    T = ds.frames_per_video
    w, h = ds.frame_size
    rows = []
    for sid in sids:
        r = []
        for lab in ds.get_label(sid):
            if rng.random() < 0.85:
                s = np.array([lab[2] - lab[0], lab[3] - lab[1]] * 2)
                r.append([lab[4] if rng.random() < 0.9 else (lab[4] + 1) % len(ds.classes), rng.uniform(0.3, 1.0)]
                         + (lab[:4] + rng.normal(0, 0.04, 4) * s).tolist())
        xy = rng.uniform(0, (w - 60, h - 60))
        r.append([int(rng.integers(0, len(ds.classes))), rng.uniform(0.05, 0.5)] + xy.tolist() + (xy + rng.uniform(10, 60, 2)).tolist())
        rows.append(r)
    N = max(len(r) for r in rows)
    F = len(sids)
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    for t, r in enumerate(rows):
        for j, row in enumerate(r):
            ids[t, j, 0], scores[t, j, 0], bboxes[t, j] = row[0], row[1], row[2:]
    track = track_host(ids, scores, bboxes, clip_start=list(range(0, F + 1, T)), num_class=len(ds.classes), sigma_h=0.0, t_min=1,
                       max_age=2)[0]
    return {sid: [r + [int(track[t, j])] for j, r in enumerate(rows[t])] for t, sid in enumerate(sids)}


@pytest.mark.parametrize("agnostic", [False, True])
def test_device_metric_equals_host_metric_on_synthetic_tracks(agnostic):
    from viddet_amd.data import SyntheticTracks
    from viddet_amd.device_mot_metric import DeviceMOTMetric
    ds = SyntheticTracks("synthetic", num_videos=3, frames_per_video=12, num_class=4)
    results = _tracked_rows(ds)
    host = M.MOTMetric(ds, agnostic=agnostic)
    host._results = {k: list(v) for k, v in results.items()}
    want = host.get()
    for chunk_bytes in (32 << 20, 1):                                      # one chunk, a chunk per clip
        dev = DeviceMOTMetric(ds, agnostic=agnostic, chunk_bytes=chunk_bytes)
        dev._results = {k: list(v) for k, v in results.items()}
        assert dev.get() == want and dev.summary == host.summary
        assert set(dev.timings) == {"pack", "upload", "launch", "enqueue", "download", "summary"}
    got = dict(zip(*want))
    assert 0 < int(got["TP"]) < int(got["GT"]) and int(got["FP"]) > 0 and 0.0 < float(got["IDF1"]) < 1.0
    print(got)


# ---- the script ----------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p).read()
    return out


@pytest.mark.parametrize("tubelet", [[], ["--tubelet"]], ids=["track", "tubelet"])
def test_detect_script_mot(tmp_path, tubelet):
    """--stream --track --track_max_age 2 --metrics vid,mot (and the same with --tubelet) writes byte for byte every file the run
    with --metrics vid writes, plus mot.txt (with --tubelet: mot_tub.txt too), whose contents are MOTMetric's on the saved twin;
    --device_metric writes equal files"""
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticTracks
    common = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--stream", "--track", "--track_max_age", "2", "--track_high", "0",
              "--synthetic_videos", "2", "--synthetic_samples", "8", "--batch_size", "4", "--save_dir", str(tmp_path)] + tubelet
    trees = {}
    for tag, extra in (("plain", ["--metrics", "vid"]), ("mot", ["--metrics", "vid,mot"]), ("dev", ["--metrics", "vid,mot", "--device_metric"])):
        D.main(common + ["--save_prefix", tag] + extra)
        trees[tag] = _tree(tmp_path / tag)
    added = {"mot.txt", "mot_tub.txt"} if tubelet else {"mot.txt"}
    assert set(trees["mot"]) == set(trees["plain"]) | added
    assert all(trees["mot"][k] == v for k, v in trees["plain"].items())      # everything a run without mot writes, byte for byte
    assert trees["dev"] == trees["mot"]                                      # the two --device_metric settings write equal files
    assert "vid.txt" in trees["plain"] and "tracks.txt" in trees["plain"] and ("vid_tub.txt" in trees["plain"]) == bool(tubelet)
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=8)
    rows = sum(len(v.splitlines()) for k, v in trees["mot"].items() if k.startswith("pred_trk" + os.sep))
    assert rows > 10, "fixture produced (almost) no detections"
    for twin, name in (("pred_trk", "mot.txt"), ("pred_tub_trk", "mot_tub.txt"))[:len(added)]:
        names, values = D.evaluate_tracks(M.MOTMetric(ds), ds, D.load_tracked_predictions(str(tmp_path / "mot" / twin), ds))
        assert trees["mot"][name] == "".join("%s %s\n" % kv for kv in zip(names, values)), name
        assert int(dict(zip(names, values))["PRED"]) > 0
        print(name, trees["mot"][name].replace("\n", "; "))
