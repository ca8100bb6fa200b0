"""GPU: streaming video detection (net.detect_video).

Kernels: the ring joins of vd_stream.hip bit-equal to vd_temporal_pool / vd_temporal_pool_bf16 / vd_temporal_cat on the copy
gathered by torch, on slot tables that wrap, repeat and stand still.  No launch here carries a slot outside [0, S): the clamp
is read from the code, the host-side validation is tested in tests/test_stream_cpu.py.
Network: detect_video on a clip of seven frames in chunks of three (two full chunks, a short one, the ring wraps) against the
fp64 oracle network on the seven windows gathered on the host (tests/stream_oracle.py) - held to the bounds
tests/test_temporal_gpu.py holds net(windows) to (heads < 1e-3, post-NMS rows through assert_rows_match, scores < 1e-3,
boxes_close) and, under set_precision('bf16'), to the network bound of tests/test_bf16_gpu.py (heads within 3e-2 of the largest
logit).  Every call must have sent each frame through the per-frame prefix exactly once.
"""
import math
import os

import numpy as np
import pytest
import torch

from tests import stream_oracle as SO
from tests.util import dev, maxdiff, boxes_close, assert_rows_match, take_ranks

pytestmark = pytest.mark.gpu

B, S = 3, 7
STRIDE_UNITS = 4096 * 256                      # 16-byte units one sweep of the capped grid covers (gblocks, vd_stream.hip)
BIG_UNITS = STRIDE_UNITS // B + 37             # B * BIG_UNITS > STRIDE_UNITS: some lanes take a second trip of the loop


def _slots(K):
    """[B][K]: a run that wraps and is not ordered (5, 6, 0, ...), a row that stands still, a clip-end row with repeats at
    the front (and from K = 5 at the back too)"""
    from viddet_amd.stream import stream_window_slots
    rows = [[(5 + j) % S for j in range(K)], [3] * K, (stream_window_slots(2, K, 1)[0] + 5).tolist()]
    t = torch.tensor(rows, dtype=torch.int32, device="cuda")
    assert int(t.min()) >= 0 and int(t.max()) < S
    return t


def _ring(inner, bf16, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.round(torch.randn(S, inner, device="cuda", generator=g) * 2) / 2       # a few levels: the max meets ties
    r[6, ::2] = r[5, ::2]              # and ties by construction at every size: slots 5 and 6 open the first row of _slots
    return r.bfloat16() if bf16 else r


def _cases(unit):
    return [(K, n) for K in (1, 2, 3, 5) for n in (unit, 24, 13 * 13 * 256)] + [(3, unit * BIG_UNITS)]


def _check_pool(K, inner, type_, bf16):
    from viddet_amd import lib as L
    lib, s = L.load(), L.stream_ptr
    ring, slots = _ring(inner, bf16, 100 * K + type_), _slots(K)
    keep = ring.clone()
    gathered = ring[slots.long()].contiguous()                                        # [B][K][inner]
    want = torch.full((B, inner), float("nan"), dtype=ring.dtype, device="cuda")
    if bf16:
        L.check(lib.vd_temporal_pool_bf16(gathered.data_ptr(), want.data_ptr(), B, K, inner, type_, s()), "vd_temporal_pool_bf16")
    else:
        L.check(lib.vd_temporal_pool(gathered.data_ptr(), want.data_ptr(), None, B, K, inner, type_, s()), "vd_temporal_pool")
    fn = lib.vd_temporal_pool_idx_bf16 if bf16 else lib.vd_temporal_pool_idx
    got = [torch.full((B, inner), float("nan"), dtype=ring.dtype, device="cuda") for _ in range(2)]
    for y in got:
        L.check(fn(ring.data_ptr(), slots.data_ptr(), y.data_ptr(), S, B, K, inner, type_, s()), "vd_temporal_pool_idx")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(want.float()).any())
    assert torch.equal(got[0], want), "not bit-equal to the windowed kernel on the gathered copy"
    assert torch.equal(got[0], got[1]), "two runs differ"
    assert torch.equal(ring, keep), "the ring was written"
    if type_ == 0 and K > 1:
        assert bool((gathered[0, 0] == gathered[0, 1]).any()), "the fixture has no ties"


@pytest.mark.parametrize("type_", [0, 1], ids=["max", "mean"])
@pytest.mark.parametrize("K,inner", _cases(4))
def test_pool_off_the_ring_fp32(K, inner, type_):
    _check_pool(K, inner, type_, False)


@pytest.mark.parametrize("type_", [0, 1], ids=["max", "mean"])
@pytest.mark.parametrize("K,inner", _cases(8))
def test_pool_off_the_ring_bf16(K, inner, type_):
    _check_pool(K, inner, type_, True)


# (hw, C) in fp32 channels: the smallest legal, 24 = 3 x 8, a 13 x 13 x 256 map, and more units than one sweep of the grid
CAT = [(K, hw, C) for K in (1, 2, 3, 5) for hw, C in ((1, 4), (3, 8), (169, 256))] + [(3, BIG_UNITS // 2, 8)]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,hw,C", CAT)
def test_cat_off_the_ring(K, hw, C, bf16):
    from viddet_amd import lib as L
    lib, s = L.load(), L.stream_ptr
    Ct = 2 * C if bf16 else C                                   # bf16 tensors go through the copy with the channel count halved
    ring, slots = _ring(hw * Ct, bf16, 7 * K + hw), _slots(K)
    keep = ring.clone()
    gathered = ring[slots.long()].contiguous()                  # [B][K][hw][Ct] = the folded [B*K][hw][Ct]
    want = torch.full((B, hw, K * Ct), float("nan"), dtype=ring.dtype, device="cuda")
    L.check(lib.vd_temporal_cat(gathered.data_ptr(), want.data_ptr(), B, K, hw, C, 0, s()), "vd_temporal_cat")
    got = [torch.full((B, hw, K * Ct), float("nan"), dtype=ring.dtype, device="cuda") for _ in range(2)]
    for y in got:
        L.check(lib.vd_temporal_cat_idx(ring.data_ptr(), slots.data_ptr(), y.data_ptr(), S, B, K, hw, C, s()), "vd_temporal_cat_idx")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(want.float()).any())
    assert torch.equal(got[0], want) and torch.equal(got[0], got[1]) and torch.equal(ring, keep)
    # and it is the stacking it claims to be: channel k * C + c of window b = frame slots[b][k]
    assert torch.equal(got[0].view(B, hw, K, Ct), ring.view(S, hw, Ct)[slots.long()].permute(0, 2, 1, 3))


# ------------------------------------------------------------------------------------------------ network
CHUNK = 3


def _mk(jt, jp, **kw):
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(SO.C)], k=SO.K, k_join_type=jt, k_join_pos=jp, **kw)
    P = SO.params(jt, jp)
    assert set(P) == set(net.collect_params().keys())
    for k, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[k].astype(np.float32)))
    return net


def _check_work_done_once(net, T=SO.T, chunk=CHUNK):
    st = net.stream_stats
    print("stream_stats", st)
    assert st['prefix_frames'] == T, "every frame goes through the per-frame prefix exactly once"
    assert st['suffix_frames'] == T and st['chunks'] == math.ceil(T / chunk)
    keys = [k for k in net._programs if k[0] in ('stream', 'stream_bf16')]
    assert keys
    for k in keys:
        sp = net._programs[k]
        names = [r[0] for prog in (sp['pre'], sp['suf']) for r in prog.recs if r[0]]
        windowed = [n for n in names if (n.startswith('vd_temporal_pool') or n.startswith('vd_temporal_cat')) and '_idx' not in n]
        assert not windowed, windowed
        assert sum('_idx' in n for n in names) == 3 and not any('_idx' in r[0] for r in sp['pre'].recs if r[0])


def _stream(net, step, **kw):
    net.stream_keep_heads = True
    out = net.detect_video(dev(SO.clip_frames()), step=step, chunk=CHUNK, **kw)
    torch.cuda.synchronize()
    assert tuple(out[0].shape) == (SO.T, 100, 1) and tuple(out[1].shape) == (SO.T, 100, 1) and tuple(out[2].shape) == (SO.T, 100, 4)
    assert tuple(net.last_rows.shape) == (SO.T, 100) and int(net.last_overflow.max()) == 0
    return out


def _heads_err(net, heads_r):
    A = 3 * (5 + SO.C)
    errs = []
    for s_, h in enumerate(net.stream_heads):
        ref = np.moveaxis(heads_r[s_], 1, -1)
        got = h.cpu().numpy()[..., :A]
        assert got.shape == ref.shape
        errs.append((maxdiff(got, ref), float(np.abs(ref).max())))
    return errs


FP32 = [("max", "early", 1), ("mean", "late", 1), ("cat", "early", 1), ("max", "late", 1), ("max", "early", 2)]


@pytest.mark.parametrize("jt,jp,step", FP32, ids=["%s-%s-step%d" % c for c in FP32])
def test_detect_video_against_the_oracle_on_the_gathered_windows(jt, jp, step):
    ids_r, sc_r, bx_r, rows_r, heads_r = SO.clip_reference(jt, jp, step)
    net = _mk(jt, jp)
    ids, sc, bx = _stream(net, step)
    for s_, (err, mag) in enumerate(_heads_err(net, heads_r)):
        print("head %d: max err %.3e (max |logit| %.2f)" % (s_, err, mag))
        assert err < 1e-3, "head %d" % s_
    perm = assert_rows_match(net.last_rows.cpu().numpy(), rows_r, sc_r)
    assert np.array_equal(take_ranks(ids, perm)[..., 0], ids_r[..., 0])
    assert maxdiff(take_ranks(sc, perm), sc_r) < 1e-3 and boxes_close(take_ranks(bx, perm), bx_r)
    assert (rows_r >= 0).sum() > 20, "fixture keeps (almost) nothing"
    _check_work_done_once(net)
    # a second call reuses the programs and gives the same bits; so does a clip handed over as host memory
    first = [t.clone() for t in (ids, sc, bx, net.last_rows)]
    nprog = len(net._programs)
    again = net.detect_video(torch.from_numpy(SO.clip_frames()), step=step, chunk=CHUNK)
    assert len(net._programs) == nprog
    assert all(torch.equal(a, b_) for a, b_ in zip(first, list(again) + [net.last_rows]))
    _check_work_done_once(net)


@pytest.mark.parametrize("jt,jp", [("max", "early"), ("mean", "late"), ("cat", "early"), ("max", "late")])
def test_detect_video_bf16_against_the_oracle(jt, jp):
    heads_r = SO.clip_reference(jt, jp, 1)[4]
    net = _mk(jt, jp)
    net.set_precision('bf16')
    ids, sc, bx = _stream(net, 1)
    for s_, (err, mag) in enumerate(_heads_err(net, heads_r)):
        print("head %d: max err / max |logit| = %.4f" % (s_, err / mag))
        assert err / mag < 3e-2, "head %d" % s_
    assert bool((ids >= 0).any())
    _check_work_done_once(net)
    assert [k[0] for k in net._programs if k[0].startswith('stream')] == ['stream_bf16']


def test_detect_video_agnostic_against_the_agnostic_oracle():
    ids_r, sc_r, bx_r, rows_r, heads_r = SO.clip_reference("max", "late", 1, agnostic=True)
    net = _mk("max", "late", agnostic=True)
    ids, sc, bx = _stream(net, 1)
    for s_, (err, mag) in enumerate(_heads_err(net, heads_r)):
        assert err < 1e-3, "head %d" % s_
    perm = assert_rows_match(net.last_rows.cpu().numpy(), rows_r, sc_r)
    assert np.array_equal(take_ranks(ids, perm)[..., 0], ids_r[..., 0])
    assert maxdiff(take_ranks(sc, perm), sc_r) < 1e-3 and boxes_close(take_ranks(bx, perm), bx_r)
    kept = rows_r >= 0
    assert kept.sum() > 20 and np.all(ids.cpu().numpy()[..., 0][kept] == 0)
    _check_work_done_once(net)


def test_uint8_clip_and_set_nms_are_honoured():
    """uint8 frames (T,H,W,3) are normalised on the device as net(x) normalises them (the same fp32 operations in the same
    order as the host transform, tests/test_model_gpu.py): bit-identical detections to the host-normalised float clip; set_nms
    reaches the streaming programs."""
    from viddet_amd.data import _to_tensor_normalize
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, (5, SO.SIZE, SO.SIZE, 3), dtype=np.uint8)
    f32 = np.stack([_to_tensor_normalize(f) for f in u8])
    net = _mk("max", "early")
    net.set_nms(nms_thresh=0.3, nms_topk=50, post_nms=20)
    a = [t.clone() for t in net.detect_video(torch.from_numpy(u8), chunk=2)] + [net.last_rows.clone()]
    _check_work_done_once(net, 5, 2)
    b_ = list(net.detect_video(torch.from_numpy(f32), chunk=2)) + [net.last_rows]
    torch.cuda.synchronize()
    assert tuple(a[0].shape) == (5, 20, 1) and bool((a[0] >= 0).any())
    assert all(torch.equal(u, v) for u, v in zip(a, b_))
    with pytest.raises(ValueError):
        net.detect_video(torch.from_numpy(u8[..., :2].copy()))


def test_k1_is_plain_batched_detection():
    """K = 1: detect_video(frames) is net(frames) chunk by chunk, bit for bit.  The short last chunk does NOT take another plan:
    it runs the batch-`chunk` plan on rows padded with repeats of its last frame, so it is compared - bit for bit as well - with
    net() on that padded batch (the fp32 operand scales are per tensor: a batch of one would round differently)."""
    from oracle import net as ON
    from viddet_amd.model import yolo3_darknet53
    P = ON.init_params(SO.C, seed=11, obj_bias=-1.0)
    net = yolo3_darknet53(["c%d" % i for i in range(SO.C)])
    for k, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[k].astype(np.float32)))
    x = dev(SO.clip_frames())
    ids, sc, bx = [t.clone() for t in net.detect_video(x, chunk=CHUNK)]
    rows = net.last_rows.clone()
    assert net.stream_stats == dict(prefix_frames=0, suffix_frames=SO.T, chunks=3)      # no join: there is no prefix
    for t0 in (0, 3, 6):
        n = min(CHUNK, SO.T - t0)
        xb = x[t0:t0 + n] if n == CHUNK else torch.cat([x[t0:t0 + n], x[t0 + n - 1:t0 + n].expand(CHUNK - n, -1, -1, -1)])
        r = net(xb)
        torch.cuda.synchronize()
        assert torch.equal(r[0][:n], ids[t0:t0 + n]) and torch.equal(r[1][:n], sc[t0:t0 + n]) and torch.equal(r[2][:n], bx[t0:t0 + n])
        assert torch.equal(net.last_rows[:n], rows[t0:t0 + n])
    assert bool((ids >= 0).any())


def test_existing_paths_are_unchanged_by_a_streaming_call():
    net = _mk("mean", "late")
    w = dev(SO.clip_windows(1)[:2].astype(np.float32))
    before = [t.clone() for t in net(w)] + [net.last_rows.clone()]
    held = dict(net._programs)
    recs = list(net._programs[('infer', 2, SO.SIZE, SO.SIZE)][0].recs)
    net.detect_video(dev(SO.clip_frames()), chunk=CHUNK)
    for k, v in held.items():
        assert net._programs[k] is v, k
    assert net._programs[('infer', 2, SO.SIZE, SO.SIZE)][0].recs == recs
    assert set(net._programs) - set(held) == {('stream', CHUNK, SO.SIZE, SO.SIZE, 5)}
    after = list(net(w)) + [net.last_rows]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b_) for a, b_ in zip(before, after))


# ------------------------------------------------------------------------------------------------ script
def test_detect_script_stream_writes_what_the_windowed_run_writes(tmp_path, capsys):
    """`--synthetic_videos` selects the clip dataset with or without --stream: the windowed run reads its windows, the
    streamed run its clips.  The same prediction files, mAP within the project's 1e-3."""
    import detect_yolo3 as D
    common = ["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
              "--synthetic_samples", "5", "--synthetic_videos", "2", "--data_shape", "64", "--batch_size", "2", "--metrics", "voc",
              "--save_dir", str(tmp_path)]
    out_s = D.main(common + ["--stream", "--save_prefix", "s"])
    out_w = D.main(common + ["--save_prefix", "w"])
    fs, fw = sorted(os.listdir(tmp_path / "s" / "pred")), sorted(os.listdir(tmp_path / "w" / "pred"))
    assert fs == fw and len(fs) == 10
    for run in ("s", "w"):
        nrows = sum(len(open(tmp_path / run / "pred" / f).read().splitlines()) for f in fs)
        assert nrows > 10, "fixture produced (almost) no detections"
    (names_s, vals_s), (names_w, vals_w) = out_s, out_w
    assert names_s == names_w
    print("mAP streamed %.6f windowed %.6f" % (vals_s[-1], vals_w[-1]))
    assert not np.isnan(vals_w[-1]) and abs(vals_s[-1] - vals_w[-1]) <= 1e-3
    assert capsys.readouterr().out.count("mAP=") == 2
