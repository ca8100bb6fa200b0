"""GPU: the HOTA metric's matching on the device (vd_hota_match, ops.hota_match) equals its definition
(viddet_amd.hota_metric.hota_match_host, itself held to a loop form in tests/test_hota_metric_cpu.py) in every bit of all three
outputs - on crowded frames of every width at which the kernels take another path, on the seeded clips and the closed forms of
the CPU tests, on several clips in one launch, with a workspace of the caller's; then DeviceHOTAMetric against HOTAMetric and
detect_yolo3.py --track --metrics hota."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import hota_cases as HC
from tests import hota_oracle as HO
from viddet_amd import hota_metric as H
from viddet_amd.mot_metric import masked_track

pytestmark = pytest.mark.gpu
NAMES = ("match", "msim", "mscore")
DTYPES = (np.float32, np.int32, np.int32, np.float32, np.float32, np.float32, np.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _host(arrays, A, P, **kw):
    """the definition on the same dense ids: an id outside [0, A) or [0, P) is no id"""
    host = [np.ascontiguousarray(a, dtype=dt) for a, dt in zip(arrays, DTYPES)]
    host[2] = np.where((host[2] >= 0) & (host[2] < A), host[2], -1).astype(np.int32)
    host[6] = np.where((host[6] >= 0) & (host[6] < P), host[6], -1).astype(np.int32)
    return H.hota_match_host(*host, **kw)


def _check(arrays, A, P, want=None, ws=None, **kw):
    from viddet_amd import ops
    host = [np.ascontiguousarray(a, dtype=dt) for a, dt in zip(arrays, DTYPES)]
    if want is None:
        want = _host(arrays, A, P, **kw)
    ins = [torch.from_numpy(a).cuda() for a in host]
    keep = [t.clone() for t in ins]
    got = ops.hota_match(*ins, num_gt_id=A, num_track=P, ws=ws, **kw)
    torch.cuda.synchronize()
    for name, g, w in zip(NAMES, got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert torch.equal(g.cpu().view(torch.int32), w.view(torch.int32)), (name, kw, np.argwhere(_bits(g.cpu().numpy()) != _bits(w.numpy()))[:5].tolist())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ins, keep)), "an input was written"
    return want, [g.cpu().numpy() for g in got]


# (F, G, N, A, P, clip_start, agnostic): one row, a wavefront less one, a wavefront, a wavefront and one, the widest frame
SHAPES = [(1, 1, 1, 1, 1, None, False), (3, 2, 63, 4, 40, None, True), (3, 64, 64, 64, 64, None, False), (2, 65, 65, 1024, 130, None, False),
          (2, 128, 128, 128, 128, None, True), (12, 5, 12, 6, 20, None, False), (12, 5, 12, 6, 20, [0, 5, 5, 12], False)]


@functools.lru_cache(maxsize=None)
def _crowd(k):
    F, G, N, A, P, cs, agnostic = SHAPES[k]
    arrays = HO.crowd(124 if k == 0 else 100 + k, F, G, N, A, P, spread=120.0 if G == 128 else 200.0)   # 124: the one pair meets
    kw = dict(num_class=2, agnostic=agnostic)
    if cs is not None:
        kw["clip_start"] = cs
    return arrays, kw, _host(arrays, A, P, **kw)


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["%dx%dx%d%s" % (s[0], s[1], s[2], "_clips" if s[5] else "") for s in SHAPES])
def test_device_equals_host_on_crowded_frames(k):
    F, G, N, A, P, cs, agnostic = SHAPES[k]
    arrays, kw, want = _crowd(k)
    _check(arrays, A, P, want, **kw)
    matched = int((want[0] >= 0).sum())
    print("matched %d of %d candidates, scores up to %d" % (matched, int((want[0] != -2).sum()), int(want[2].max())))
    if G == 128:
        # every column in play: (almost) every candidate of the narrower side finds a partner
        cand = min(int((want[0][0] != -2).sum()), N)
        assert int((want[0][0] >= 0).sum()) > 0.7 * cand
    assert matched > 0


@pytest.mark.parametrize("seed", (1, 3, 4, 6))
def test_device_equals_host_on_the_seeded_clips_of_the_oracle(seed):
    from tests.test_hota_metric_cpu import _seeded
    arrays, kw, _, _ = _seeded(seed)
    _check(arrays, 1024, 128, **kw)


@pytest.mark.parametrize("name,arrays,kw,expect", HC.closed_forms(), ids=[c[0] for c in HC.closed_forms()])
def test_closed_forms(name, arrays, kw, expect):
    want, got = _check(arrays, 1024, 16, **kw)
    trk = masked_track(arrays[3], arrays[4], arrays[6], kw.get("num_class"))
    HC.check_expected(got, H.hota_summary(got, arrays[2], trk, kw.get("clip_start")), expect)


def test_the_id_ranges_at_both_ends():
    """A = 1024 with the ids 0 and 1023 in play and 1024 outside; P = 1: only track 0 takes part; P = F * N: every row a track
    of its own"""
    F, G, N = 4, 6, 9
    arrays = list(HO.crowd(7, F, G, N, 1024, F * N))
    arrays[2][:, 0], arrays[2][:, 1], arrays[2][:, 2] = 0, 1023, 1024
    arrays[6] = np.arange(F * N, dtype=np.int32).reshape(F, N)[::-1].copy()
    want, _ = _check(arrays, 1024, F * N, num_class=2)
    assert (want[0][:, 2] == -2).all() and (want[0][:, :2] != -2).any()
    arrays[6] = (np.arange(F * N, dtype=np.int32).reshape(F, N) % 3)
    want1, _ = _check(arrays, 1024, 1, num_class=2, agnostic=True)
    assert ((want1[0] >= 0).sum(axis=1) <= 1).all() and (want1[0] >= 0).any()         # one candidate prediction a frame


def test_clips_a_frame_outside_them_a_reused_workspace_and_tensors_at_an_offset():
    from viddet_amd import ops
    k = len(SHAPES) - 1
    F, G, N, A, P, cs, _ = SHAPES[k]
    arrays, kw, want = _crowd(k)
    assert cs[1] == cs[2]                                                  # an empty clip in the middle
    need = ops.hota_ws_bytes(3, A, P)
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")   # NaN bytes, whatever a last call left behind
    _, got = _check(arrays, A, P, want, **kw)
    _, again = _check(arrays, A, P, want, ws=ws, **kw)
    _, third = _check(arrays, A, P, want, ws=ws, **kw)                     # two runs on one workspace are equal
    assert all(np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c)) for a, b, c in zip(got, again, third))
    # the clips of one launch equal a launch each
    one = {x: v for x, v in kw.items() if x != "clip_start"}
    for a, b in zip(cs[:-1], cs[1:]):
        if b > a:
            _, alone = _check([x[a:b] for x in arrays], A, P, ws=ws, **one)
            assert all(np.array_equal(_bits(g[a:b]), _bits(o)) for g, o in zip(got, alone))
    # and differ from the frames taken as one clip: the ids of a clip are its own
    whole = _host(arrays, A, P, **one)
    assert not np.array_equal(whole[2], want[2])
    # offsets on the device are taken as they are: the frames that no clip covers come out as -2 / 0 / 0
    host = [np.ascontiguousarray(x, dtype=dt) for x, dt in zip(arrays, DTYPES)]
    dcs = torch.tensor([0, 5, 5, 10], dtype=torch.int32, device="cuda")
    # every tensor a view at an offset into one buffer (16-byte steps keep the boxes aligned)
    flat = torch.zeros(sum(x.size for x in host) + 4 * 8 * len(host), dtype=torch.int32, device="cuda")
    at, dv = 4, []
    for x in host:
        t = flat[at:at + x.size].view(torch.float32 if x.dtype == np.float32 else torch.int32)
        t.copy_(torch.from_numpy(x.reshape(-1)))
        dv.append(t.view(*x.shape))
        at += (x.size + 7) // 4 * 4 + 4
    assert all(t.data_ptr() != flat.data_ptr() and t.data_ptr() % 16 == 0 for t in dv)
    part = [g.cpu().numpy() for g in ops.hota_match(*dv, num_gt_id=A, num_track=P, clip_start=dcs, ws=ws[8:], **one)]
    head = _host([x[:10] for x in arrays], A, P, clip_start=[0, 5, 5, 10], **one)
    for g, w, fill in zip(part, head, (-2, 0, 0)):
        assert np.array_equal(_bits(g[:10]), _bits(w)) and (g[10:] == fill).all()
    for t, x in zip(dv, host):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(x))
    with pytest.raises(ValueError, match="ws must be"):
        ops.hota_match(*dv, num_gt_id=A, num_track=P, clip_start=dcs, ws=ws[:need - 1])
    with pytest.raises(ValueError, match="ws must be"):
        ops.hota_match(*dv, num_gt_id=A, num_track=P, clip_start=dcs, ws=ws[4:])     # not 8-byte aligned
    with pytest.raises(ValueError, match="clip_start"):
        ops.hota_match(*dv, num_gt_id=A, num_track=P, clip_start=[0, 6, 11])
    with pytest.raises(ValueError, match="num_gt_id"):
        ops.hota_match(*dv, num_gt_id=1025, num_track=P)
    with pytest.raises(ValueError, match="num_track"):
        ops.hota_match(*dv, num_gt_id=A, num_track=0)
    with pytest.raises(ValueError, match="track must be"):
        ops.hota_match(*dv[:6], dv[6].float(), num_gt_id=A, num_track=P)
    z = torch.zeros(F, 129, 4, device="cuda")
    with pytest.raises(ValueError, match="G=129"):
        ops.hota_match(z, *dv[1:], num_gt_id=A, num_track=P)
    with pytest.raises(ValueError, match="N=129"):
        ops.hota_match(*dv[:5], z, dv[6], num_gt_id=A, num_track=P)


# ---- the metric class ------------------------------------------------------------------------------------------------------
def _detections(ds, seed=3):
    """the ground truth jittered, thinned and with clutter: (ids, scores, bboxes) as a detector could have made them"""
    rng = np.random.default_rng(seed)
    w, h = ds.frame_size
    rows = []
    for sid in ds.get_sample_ids():
        r = []
        for lab in ds.get_label(sid):
            if rng.random() < 0.85:
                s = np.array([lab[2] - lab[0], lab[3] - lab[1]] * 2)
                r.append([lab[4] if rng.random() < 0.9 else (lab[4] + 1) % len(ds.classes), rng.uniform(0.3, 1.0)]
                         + (lab[:4] + rng.normal(0, 0.04, 4) * s).tolist())
        xy = rng.uniform(0, (w - 60, h - 60))
        r.append([int(rng.integers(0, len(ds.classes))), rng.uniform(0.05, 0.5)] + xy.tolist() + (xy + rng.uniform(10, 60, 2)).tolist())
        rows.append(r)
    N, F = max(len(r) for r in rows), len(rows)
    ids, scores, bboxes = -np.ones((F, N, 1), np.float32), -np.ones((F, N, 1), np.float32), -np.ones((F, N, 4), np.float32)
    for t, r in enumerate(rows):
        for j, row in enumerate(r):
            ids[t, j, 0], scores[t, j, 0], bboxes[t, j] = row[0], row[1], row[2:]
    return ids, scores, bboxes


@pytest.mark.parametrize("method", ["iou", "sort"])
def test_device_metric_equals_host_metric_on_synthetic_tracks(method):
    from viddet_amd import ops
    from viddet_amd.data import SyntheticTracks
    from viddet_amd.device_hota_metric import DeviceHOTAMetric, clip_chunks
    ds = SyntheticTracks("synthetic", num_videos=4, frames_per_video=8, num_class=4)
    ids, scores, bboxes = _detections(ds)
    F, N = bboxes.shape[:2]
    link = ops.track if method == "iou" else ops.track_sort
    track = link(*[torch.from_numpy(x).cuda() for x in (ids, scores, bboxes)], clip_start=list(range(0, F + 1, 8)),
                 num_class=len(ds.classes), sigma_h=0.0, t_min=1, max_age=2)[0].cpu().numpy()
    results = {}
    for t, sid in enumerate(ds.get_sample_ids()):
        on = np.nonzero(ids[t, :, 0] >= 0)[0]
        results[sid] = [[float(ids[t, i, 0]), float(scores[t, i, 0])] + [float(c) for c in bboxes[t, i]] + [int(track[t, i])] for i in on]
    # four equal clips are cut by their rows into 1, 2 or 4 chunks; three take the workspace cap: the least cap under which
    # the clips' own numbers of ids give three
    from viddet_amd.device_hota_metric import WS_BYTES, dense_ids
    from viddet_amd.mot_metric import pack_clips
    arrays, cs = pack_clips(ds, results)
    G = arrays[0].shape[1]
    num_gt = dense_ids(arrays[2], cs)[1]
    num_pred = dense_ids(masked_track(arrays[3], arrays[4], arrays[6], len(ds.classes)), cs)[1]
    worst = max(8 * a * p + 4 * a + 4 * p for a, p in zip(num_gt, num_pred))
    three = [cap for cap in range(worst, 4 * worst, 4) if len(clip_chunks(cs, G, N, num_gt, num_pred, ws_bytes=cap)) == 3]
    assert three, (num_gt, num_pred)
    for agnostic in (False, True):
        host = H.HOTAMetric(ds, agnostic=agnostic)
        host._results = {k: list(v) for k, v in results.items()}
        want = host.get()
        for chunk_bytes, ws_bytes, chunks in ((32 << 20, WS_BYTES, 1), (32 << 20, three[0], 3), (1, WS_BYTES, 4)):
            dev = DeviceHOTAMetric(ds, agnostic=agnostic, chunk_bytes=chunk_bytes, ws_bytes=ws_bytes)
            dev._results = {k: list(v) for k, v in results.items()}
            assert dev.get() == want and dev.summary == host.summary
            assert set(dev.timings) == {"pack", "upload", "launch", "enqueue", "download", "summary"}
            assert len(clip_chunks(cs, G, N, num_gt, num_pred, chunk_bytes, ws_bytes)) == chunks
    with pytest.raises(ValueError, match="DeviceHOTAMetric: clip \\d holds"):
        dev = DeviceHOTAMetric(ds, ws_bytes=worst - 1)
        dev._results = results
        dev.get()
    got = dict(zip(*want))
    assert 0.0 < float(got["HOTA"]) < 1.0 and 0.0 < float(got["AssA"]) < 1.0 and 0.0 < float(got["DetA"]) < 1.0
    print(method, got)


# ---- the script ----------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p).read()
    return out


def test_detect_script_hota(tmp_path):
    """--stream --track --metrics hota,mot --device_metric writes the hota.txt the host path writes, byte for byte, whose
    contents are HOTAMetric's on the saved twin; a run without hota writes what the run with it writes beside hota.txt"""
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticTracks
    common = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--stream", "--track", "--track_max_age", "2", "--track_high", "0",
              "--synthetic_videos", "2", "--synthetic_samples", "8", "--batch_size", "4", "--save_dir", str(tmp_path)]
    trees, returned = {}, {}
    for tag, extra in (("plain", ["--metrics", "mot"]), ("hota", ["--metrics", "hota,mot"]), ("dev", ["--metrics", "hota,mot", "--device_metric"])):
        returned[tag] = D.main(common + ["--save_prefix", tag] + extra)
        trees[tag] = _tree(tmp_path / tag)
    assert set(trees["hota"]) == set(trees["plain"]) | {"hota.txt"}
    assert all(trees["hota"][k] == v for k, v in trees["plain"].items())      # everything a run without hota writes, byte for byte
    assert trees["dev"] == trees["hota"]                                      # the two --device_metric settings write equal files
    assert returned["plain"] == returned["hota"] == returned["dev"] and returned["plain"][0][0] == "MOTA"
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=8)
    rows = sum(len(v.splitlines()) for k, v in trees["hota"].items() if k.startswith("pred_trk" + os.sep))
    assert rows > 10, "fixture produced (almost) no detections"
    names, values = D.evaluate_tracks(H.HOTAMetric(ds), ds, D.load_tracked_predictions(str(tmp_path / "hota" / "pred_trk"), ds))
    assert trees["hota"]["hota.txt"] == "".join("%s %s\n" % kv for kv in zip(names, values))
    assert int(dict(zip(names, values))["PRED"]) > 0
    print(trees["hota"]["hota.txt"].replace("\n", "; "))
