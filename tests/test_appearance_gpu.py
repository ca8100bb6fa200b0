"""GPU: appearance association on the device equals its definitions bit for bit.  vd_roi_embed (ops.roi_embed)
against viddet_amd.appearance.embed_host with array_equal over the map sizes, pitches, storage types, row counts and the edge
boxes; vd_track_sort_app (ops.track_sort_app) against app_sort_host - track, tlen and tscore with torch.equal, tbox on its
bytes wherever the definition's value is no NaN and a NaN wherever it is, tests/test_sort_gpu.py's rule - and with zero
descriptors against ops.track_sort itself; then through net.detect_video(track={'method': 'sort', 'appearance': ...}) and
detect_yolo3.py --track_app."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import appearance_cases as AC
from tests import sort_cases as SC
from viddet_amd.appearance import app_sort_host, embed_host
from viddet_amd.sort import sort_host

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the descriptor
def _bf16_exact(f):
    """a float32 array whose values bf16 holds exactly"""
    return torch.from_numpy(f).to(torch.bfloat16).to(torch.float32).numpy()


def _embed(f, ids, bx, stride, pad=0, bf16=False, map_index=None):
    from viddet_amd import ops
    S, Hf, Wf, Cn = f.shape
    store = torch.full((S, Hf, Wf, Cn + pad), float("nan"), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    store[..., :Cn] = torch.from_numpy(f).cuda()
    keep = store.clone()
    mi = None if map_index is None else torch.tensor(map_index, dtype=torch.int32, device="cuda")
    dids, dbx = torch.from_numpy(ids).cuda(), torch.from_numpy(bx).cuda()
    runs = [ops.roi_embed(store[..., :Cn], dids, dbx, stride, map_index=mi) for _ in range(2)]
    torch.cuda.synchronize()
    assert runs[0].dtype == torch.int8 and torch.equal(runs[0], runs[1]), "two runs differ"
    assert torch.equal(store.view(torch.int16 if bf16 else torch.int32), keep.view(torch.int16 if bf16 else torch.int32)), "the map was written"
    return runs[0].cpu().numpy()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Cn,pad", [(8, 0), (8, 8), (256, 0), (256, 8)], ids=["c8", "c8_ld16", "c256", "c256_ld264"])
@pytest.mark.parametrize("Hf,Wf", [(5, 7), (1, 1)], ids=["5x7", "1x1"])
def test_roi_embed_equals_the_definition(Hf, Wf, Cn, pad, bf16):
    S = 3
    f = AC.feature_map(S, Hf, Wf, Cn, seed=Cn + Hf)
    if bf16:
        f = _bf16_exact(f)
    for B, N, mi in ((1, 1, None), (3, 100, None), (3, 128, [2, 0, 2]), (1, 100, [1]), (3, 13, [-4, 3, 1])):
        ids, bx = AC.boxes_for(Hf, Wf, 8, N, B, seed=N + B)
        want = embed_host(f, ids, bx, 8, map_index=mi)                     # the definition cuts the index to [0, S) too
        got = _embed(f, ids, bx, 8, pad=pad, bf16=bf16, map_index=mi)
        assert np.array_equal(got, want), (B, N, mi)
        if N >= 13:
            assert want[0, :8].any(axis=1).all() and not want[0, 8:10].any(), "the named rows"
            if mi == [-4, 3, 1]:
                assert np.array_equal(want, embed_host(f, ids, bx, 8, map_index=[0, 2, 1]))


def test_roi_embed_wide_channels_and_the_other_strides():
    f = AC.feature_map(2, 2, 2, 1024, seed=9)
    ids, bx = AC.boxes_for(2, 2, 32, 20, 2, seed=1)
    assert np.array_equal(_embed(f, ids, bx, 32), embed_host(f, ids, bx, 32))
    g = AC.feature_map(1, 6, 4, 64, seed=10)
    ids, bx = AC.boxes_for(6, 4, 16, 30, 1, seed=2)
    assert np.array_equal(_embed(g, ids, bx, 16), embed_host(g, ids, bx, 16))
    h = g.copy()
    h[0, 2, 1, 7] = np.nan                                                 # a NaN of the map: the rows that sample it have none
    want = embed_host(h, ids, bx, 16)
    assert (want.any(axis=2) != embed_host(g, ids, bx, 16).any(axis=2)).any()
    assert np.array_equal(_embed(h, ids, bx, 16), want)
    assert not _embed(np.full((1, 3, 3, 8), 1.5, np.float32), *AC.boxes_for(3, 3, 8, 5, 1, seed=0), 8).any()      # a constant map


def test_roi_embed_argument_checks_return_minus_one():
    from viddet_amd import lib as L
    from viddet_amd import ops
    lib = L.load()
    f = torch.zeros(1, 2, 2, 16, device="cuda")
    ids, bx = torch.zeros(1, 4, device="cuda"), torch.zeros(1, 4, 4, device="cuda")
    emb = torch.zeros(1, 4, 16, dtype=torch.int8, device="cuda")
    p = L.ptr

    def call(fmap=p(f), is_bf16=0, S=1, Hf=2, Wf=2, Cn=16, ld=16, ids_=p(ids), bx_=p(bx), mi=None, B=1, N=4, stride=8, out=p(emb)):
        return lib.vd_roi_embed(fmap, is_bf16, S, Hf, Wf, Cn, ld, ids_, bx_, mi, B, N, stride, out, L.stream_ptr())

    assert call() == 0
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    for kw in (dict(fmap=None), dict(ids_=None), dict(bx_=None), dict(out=None), dict(Cn=12, ld=12), dict(Cn=4, ld=4), dict(Cn=2048, ld=2048),
               dict(ld=8), dict(ld=18), dict(N=129), dict(N=0), dict(B=0), dict(stride=4), dict(stride=64), dict(S=0), dict(Hf=0),
               dict(is_bf16=2), dict(fmap=off(f, 4)), dict(bx_=off(bx, 4)), dict(out=off(emb, 1)), dict(ids_=off(ids, 2))):
        assert call(**kw) == -1, kw
        assert lib.vd_last_error().decode().startswith("vd_roi_embed: "), kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="roi_embed: fmap must be"):
        ops.roi_embed(f.cpu(), ids, bx, 8)
    with pytest.raises(ValueError, match="roi_embed: fmap must be NHWC"):
        ops.roi_embed(f[..., ::2], ids, bx, 8)
    with pytest.raises(ValueError, match="roi_embed: stride must be"):
        ops.roi_embed(f, ids, bx, 7)
    with pytest.raises(ValueError, match="roi_embed: 2 images and 1 maps"):
        ops.roi_embed(f, torch.zeros(2, 4, device="cuda"), torch.zeros(2, 4, 4, device="cuda"), 8)
    with pytest.raises(ValueError, match="at most 128"):
        ops.roi_embed(f, torch.zeros(1, 129, device="cuda"), torch.zeros(1, 129, 4, device="cuda"), 8)


# ------------------------------------------------------------------ the association
def _same(got, want, what=""):
    for name, g, w in zip(("track", "tlen", "tscore"), got, want):
        assert g.dtype == torch.from_numpy(w).dtype and tuple(g.shape) == w.shape, what + name
        assert torch.equal(g.cpu(), torch.from_numpy(w)), what + name
    assert got[3].dtype == torch.float32 and SC.same_tbox(got[3].cpu().numpy(), want[3]), what + "tbox"


def _check(case, emb, num_class, clip_start=None, **kw):
    from viddet_amd import ops
    host = [np.ascontiguousarray(a, dtype=np.float32) for a in case]
    emb = np.ascontiguousarray(emb, dtype=np.int8)
    stats = {}
    want = app_sort_host(*host, emb, clip_start=clip_start, num_class=num_class, stats=stats, **kw)
    ins = [torch.from_numpy(a).cuda() for a in host] + [torch.from_numpy(emb).cuda()]
    keep = [t.clone() for t in ins]
    runs = [ops.track_sort_app(*ins, clip_start=clip_start, num_class=num_class, **kw) for _ in range(2)]
    torch.cuda.synchronize()
    _same(runs[0], want)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(runs[0], runs[1])), "two runs differ"
    assert all(torch.equal(a, b) or bool((a != a).any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))
               for a, b in zip(ins, keep)), "an input was written"
    return want, stats


def test_the_closed_forms():
    emb = AC.two_descriptors(10)
    assert _check(AC.swap_clip(), emb, 1)[0][0].tolist() == AC.KEPT
    assert _check(AC.turn_clip(), emb, 1)[0][0].tolist() == AC.KEPT
    assert _check(AC.far_turn_clip(), emb, 1)[0][0].tolist() == AC.FRAGMENTED
    assert _check(AC.turn_clip(), emb, 1, sigma_prox=0.26)[0][0].tolist() == AC.FRAGMENTED
    from viddet_amd.appearance import cos_q
    c = cos_q(AC.E_A, AC.E_A2)
    moved = emb.copy()
    moved[5:, 0] = AC.E_A2
    assert _check(AC.turn_clip(), moved, 1, sigma_app=np.float32(c) / np.float32(1 << 20))[0][0].tolist() == AC.KEPT
    assert _check(AC.turn_clip(), moved, 1, sigma_app=np.float32(c + 1) / np.float32(1 << 20))[0][0].tolist() == [[0, 1]] * 5 + [[2, 1]] * 5
    gone = emb.copy()
    gone[3:5] = 0
    assert _check(AC.turn_clip(), gone, 1)[0][0].tolist() == AC.KEPT
    both = [np.concatenate([a, b]) for a, b in zip(AC.swap_clip(), AC.turn_clip())]
    assert _check(both, AC.two_descriptors(20), 1, clip_start=[0, 10, 20])[0][0].tolist() == AC.KEPT + AC.KEPT


@pytest.mark.parametrize("name,case,kw,track,tlen", SC.closed_form(), ids=[c[0] for c in SC.closed_form()])
def test_zero_descriptors_give_track_sort_itself(name, case, kw, track, tlen):
    from viddet_amd import ops
    kw = dict(kw)
    num_class = kw.pop("num_class", 1)
    emb = np.zeros(np.asarray(case[2]).shape[:2] + (8,), np.int8)
    _check(case, emb, num_class, **kw)
    ins = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in case]
    a = ops.track_sort_app(*ins, torch.from_numpy(emb).cuda(), num_class=num_class, **kw)
    b = ops.track_sort(*ins, num_class=num_class, **kw)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("T,N,Cn", [(1, 1, 8), (6, 65, 8), (6, 64, 256), (8, 128, 1024)], ids=["1x1", "6x65", "6x64c256", "8x128c1024"])
@pytest.mark.parametrize("max_age", [1, 7])
def test_device_equals_host_over_the_sizes(T, N, Cn, max_age):
    from viddet_amd import ops
    case = SC.random_clip(T, N, seed=7 * T + N, spread=40.0 + N, fill=1.0 if N < 4 else 0.8)
    emb = AC.random_emb(T, N, Cn, seed=N + Cn)
    kw = dict(max_age=max_age, t_min=1 if T == 1 else 2, sigma_h=0.05 if N < 4 else 0.5, sigma_prox=0.05, sigma_app=0.6)
    want, _ = _check(case, emb, 1, **kw)
    assert (want[0] >= 0).any()
    if T > 1:                                                              # appearance decides something here
        plain = sort_host(*case, num_class=1, **{k: v for k, v in kw.items() if not k.startswith("sigma_a") and k != "sigma_prox"})
        assert not np.array_equal(plain[0], want[0]), "the descriptors changed no id"
        ins = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in case]
        zero = ops.track_sort_app(*ins, torch.zeros(T, N, Cn, dtype=torch.int8, device="cuda"), num_class=1, **kw)
        assert torch.equal(zero[0].cpu(), torch.from_numpy(plain[0]))


@pytest.mark.parametrize("extend", [False, True], ids=["grow", "extend"])
def test_the_table_of_active_tracks_and_the_cells_at_their_capacity(extend):
    """F = 10, N = 128, max_age = 7 (tests/track_cases.py's capacity).  grow: boxes disjoint from frame to frame and the default
    sigma_prox, so nothing is near: the table reaches 1024 active tracks in the 8th frame and the two frames after it fill all
    128 x 1024 cells.  extend: sigma_prox = 0 makes every cell of the 128 x 128 near, so every cell forms its dot product."""
    case = SC.capacity(extend)
    emb = AC.random_emb(10, 128, 8, seed=21, none=0.0)
    if extend:
        want, stats = _check(case, emb, 1, max_age=7, t_min=1, sigma_prox=0.0, sigma_app=0.9)
        assert stats["active"].tolist() == [128] * 10
    else:
        want, stats = _check(case, emb, 1, max_age=7, t_min=1)
        assert stats["active"].max() == 1024 and stats["closed"][8] == 128 and (want[1] == 1).all()


def test_three_clips_on_the_device_one_of_them_empty_and_a_reused_workspace():
    from viddet_amd import lib as L
    from viddet_amd import ops
    one = SC.random_clip(6, 24, classes=2, seed=13, fill=1.0)
    case = [np.concatenate([a, a[:4]]) for a in one]
    emb = AC.random_emb(10, 24, 256, seed=5)
    want, _ = _check(case, emb, 2, clip_start=[0, 6, 6, 10], sigma_prox=0.05, sigma_app=0.6)
    dv = [torch.from_numpy(a).cuda() for a in case] + [torch.from_numpy(emb).cuda()]
    cs = torch.tensor([0, 6, 6, 10], dtype=torch.int32, device="cuda")
    kw = dict(num_class=2, sigma_prox=0.05, sigma_app=0.6)
    _same(ops.track_sort_app(*dv, clip_start=cs, **kw), want, "device offsets: ")
    need = L.TRACK_SORT_WS_PER_ROW * 10 * 24 + L.TRACK_SORT_APP_WS_PER_CLIP * 3
    assert L.load().vd_track_sort_app_ws_bytes(3, 10, 24) == need and L.load().vd_track_sort_app_ws_bytes(1, 1, 129) == -1
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    _same(ops.track_sort_app(*dv, clip_start=cs, ws=ws, **kw), want, "ws: ")
    _same(ops.track_sort_app(*dv, clip_start=cs, ws=ws, **kw), want, "ws again: ")
    short = torch.tensor([0, 6, 9], dtype=torch.int32, device="cuda")      # the last frame outside every clip
    got = ops.track_sort_app(*dv, clip_start=short, **kw)
    head = app_sort_host(*[a[:9] for a in case], emb[:9], clip_start=[0, 6, 9], **kw)
    tail = (np.full((1, 24), -1, np.int32), np.zeros((1, 24), np.int32), np.full((1, 24), -1, np.float32), np.full((1, 24, 4), -1, np.float32))
    _same(got, [np.concatenate([h, t]) for h, t in zip(head, tail)], "a frame outside: ")
    with pytest.raises(ValueError, match="track_sort_app: ws must be"):
        ops.track_sort_app(*dv, clip_start=cs, ws=ws[:-1])
    with pytest.raises(ValueError, match="track_sort_app: sigma_app"):
        ops.track_sort_app(*dv, sigma_app=1.5)
    with pytest.raises(ValueError, match="track_sort_app: emb must be"):
        ops.track_sort_app(*dv[:3], dv[3][:9])
    with pytest.raises(ValueError, match="track_sort_app: emb must be a contiguous int8"):
        ops.track_sort_app(*dv[:3], dv[3].to(torch.int32))
    with pytest.raises(ValueError, match="track_sort_app: C must be a power of two"):
        ops.track_sort_app(*dv[:3], torch.zeros(10, 24, 12, dtype=torch.int8, device="cuda"))
    lib, p = L.load(), L.ptr
    outs = [torch.empty(10, 24, dtype=torch.int32, device="cuda"), torch.empty(10, 24, dtype=torch.int32, device="cuda"),
            torch.empty(10, 24, device="cuda"), torch.empty(10, 24, 4, device="cuda")]

    def call(e=p(dv[3]), Cn=256, sa=0.8, sp=0.1, nbytes=need):
        return lib.vd_track_sort_app(p(dv[0]), p(dv[1]), p(dv[2]), e, Cn, p(cs), 3, 10, 24, 2, 0.0, 0.5, 0.3, 2, 1, sa, sp, p(outs[0]),
                                     p(outs[1]), p(outs[2]), p(outs[3]), p(ws), nbytes, L.stream_ptr())

    assert call() == 0
    for kw2 in (dict(e=None), dict(Cn=12), dict(Cn=4), dict(sa=1.5), dict(sp=-0.5), dict(sa=float("nan")), dict(nbytes=need - 1),
                dict(e=C.c_void_p(dv[3].data_ptr() + 1))):
        assert call(**kw2) == -1 and lib.vd_last_error().decode().startswith("vd_track_sort_app: "), kw2
    torch.cuda.synchronize()


# ------------------------------------------------------------------ through the stack
@pytest.mark.parametrize("k,precision", [(1, "fp32"), (1, "bf16"), (3, "fp32")], ids=["k1_fp32", "k1_bf16", "k3_early_max"])
def test_detect_video_with_appearance(k, precision):
    """7 frames of 64 x 64 at chunk 3, so the last chunk is padded.  The descriptors equal the definition on the maps the launches
    read and the returned rows; the tracks equal the definition on the returned rows with those descriptors."""
    from viddet_amd.model import yolo3_darknet53
    kw_net = dict(k=3, k_join_type="max", k_join_pos="early") if k == 3 else {}
    net = yolo3_darknet53(["c%d" % i for i in range(3)], **kw_net)
    net.initialize(init="he", obj_bias=1.0)                                # objectness up: rows exist
    if precision == "bf16":
        net.set_precision("bf16")
    x = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (7, 3, 64, 64)).astype(np.float32)).cuda()
    kw = dict(sigma_h=0.0, max_age=2)
    plain = [t.clone() for t in net.detect_video(x, chunk=3, track=dict(kw, method="sort"))]
    sort_tracks = [t.clone() for t in net.last_tracks]
    assert net.last_embeddings is None and net.last_app_maps is None
    assert (plain[0] >= 0).sum() > 10, "fixture produced (almost) no detections"
    for level, Cn in ((8, 256), (32, 1024)):
        app = dict(level=level, sigma_app=0.5, sigma_prox=0.05, keep_maps=True)
        got = [t.clone() for t in net.detect_video(x, chunk=3, track=dict(kw, method="sort", appearance=app))]
        emb, maps, tracks, tbox = net.last_embeddings, net.last_app_maps, net.last_tracks, net.last_track_boxes
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(plain, got)), "appearance changed what the call returns"
        assert emb.dtype == torch.int8 and tuple(emb.shape) == (7, net.post_nms, Cn)
        assert tuple(maps.shape) == (7, 64 // level, 64 // level, Cn) and maps.dtype == (torch.bfloat16 if precision == "bf16" else torch.float32)
        rows = [t.cpu().numpy() for t in got]
        want_emb = embed_host(maps.float().cpu().numpy(), rows[0], rows[2], level)
        assert np.array_equal(emb.cpu().numpy(), want_emb)
        if level == 8:
            assert want_emb.any(axis=2).sum() == (rows[0] >= 0).sum() > 10, "every detected row has a descriptor"
        want = app_sort_host(*rows, want_emb, num_class=3, sigma_app=0.5, sigma_prox=0.05, **kw)
        _same(tuple(tracks) + (tbox,), want)
        assert (want[0] >= 0).any()
    # the defaults: level 8, sigma_app 0.8, sigma_prox 0.1, no maps kept
    net.detect_video(x, chunk=3, track=dict(kw, method="sort", appearance=True))
    assert net.last_app_maps is None and tuple(net.last_embeddings.shape) == (7, net.post_nms, 256)
    rows = [t.cpu().numpy() for t in plain]
    _same(tuple(net.last_tracks) + (net.last_track_boxes,),
          app_sort_host(*rows, net.last_embeddings.cpu().numpy(), num_class=3, **kw))
    # the later passes see the track table alone
    net.detect_video(x, chunk=3, track=dict(kw, method="sort", appearance=True), tubelet=True, stitch=True, smooth=True)
    assert net.last_tubelet is not None and net.last_stitch is not None and net.last_smooth is not None
    # a following call without it: None again, and the first call's results
    after = net.detect_video(x, chunk=3, track=dict(kw, method="sort"))
    torch.cuda.synchronize()
    assert net.last_embeddings is None and net.last_app_maps is None
    assert all(torch.equal(a, b) for a, b in zip(plain, after)) and all(torch.equal(a, b) for a, b in zip(sort_tracks, net.last_tracks))
    if k == 1 and precision == "fp32":
        with pytest.raises(ValueError, match="detect_video: appearance needs track method 'sort'"):
            net.detect_video(x, chunk=3, track=dict(appearance=True))
        with pytest.raises(ValueError, match="detect_video: appearance beside seq_nms"):
            net.detect_video(x, chunk=3, track=dict(method="sort", appearance=True), seq_nms=True)
        with pytest.raises(NotImplementedError, match="open_video with track's appearance"):
            net.open_video(track=dict(method="sort", online=True, appearance=True))


def test_detect_video_refuses_appearance_with_a_late_join():
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["a", "b"], k=3, k_join_type="max", k_join_pos="late")
    x = torch.zeros(4, 3, 64, 64, device="cuda")
    with pytest.raises(NotImplementedError, match="detect_video with track's appearance and k_join_pos 'late'"):
        net.detect_video(x, track=dict(method="sort", appearance=True))


def test_detect_script_track_app(tmp_path):
    """--stream --track --track_method sort --track_app on two synthetic clips: every line of `pred_trk` is the line of `pred` plus
    the id app_sort_host gives on the rows `pred` holds, with the descriptors the run made (--data_shape 64: a power of two, so
    the saved box / 64 gives the box back exactly, and a float32 prints round-trip: tests/test_sort_gpu.py's reason)."""
    import os
    import detect_yolo3 as D
    from viddet_amd import live
    T, W = 5, 64
    kept = []
    real = live.detect_video

    def spy(net, *a, **kw):                                                # the descriptors of every clip, as the run made them
        out = real(net, *a, **kw)
        kept.append((net.last_embeddings.cpu().numpy(), [t.cpu().numpy() for t in out]))
        return out

    live.detect_video = spy
    try:
        D.main(["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
                "--synthetic_samples", str(T), "--synthetic_videos", "2", "--data_shape", str(W), "--batch_size", "2", "--save_dir",
                str(tmp_path), "--save_prefix", "q", "--stream", "--track", "--track_method", "sort", "--track_high", "0",
                "--track_max_age", "2", "--track_app", "--track_app_cos", "0.5", "--track_app_prox", "0.05"])
    finally:
        live.detect_video = real
    assert len(kept) == 2 and all(e.shape[0] == T and e.shape[2] == 256 for e, _ in kept)
    q = tmp_path / "q"
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("vid", num_videos=2, frames_per_video=T, window=3, step=1)
    order = [os.path.split(ds.sample_path(i))[1].split(".")[0] + ".txt" for i in range(2 * T)]
    assert sorted(os.listdir(q / "pred_trk")) == sorted(order)
    lines = [open(q / "pred" / f).read().splitlines() for f in order]
    assert sum(len(r) for r in lines) > 10, "fixture produced (almost) no detections"
    for v, (emb, out) in enumerate(kept):
        want = app_sort_host(out[0], out[1], np.clip(out[2], 0, W), emb, sigma_h=0.0, max_age=2, sigma_app=0.5, sigma_prox=0.05)
        for t in range(T):
            f = order[v * T + t]
            valid = np.where(out[0][t].reshape(-1) >= 0)[0]
            assert len(valid) == len(lines[v * T + t]), f
            assert open(q / "pred_trk" / f).read().splitlines() == ["%s,%d" % (l, want[0][t, i]) for l, i in zip(lines[v * T + t], valid)], f
