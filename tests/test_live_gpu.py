"""GPU: live video sessions (net.open_video).

Tracker: vd_track_push (ops.TrackState) equals its definition (viddet_amd.track.track_online_host, itself held to track_host
in tests/test_live_cpu.py) bit for bit - all three outputs with torch.equal - however the frames are cut into pushes: on clips
that tie, break, cross the 64-lane boundary of the rows and fill the table of active tracks, which is then written back full
and read again by the next launch.
Session: a clip cut into pushes and flushed gives torch.equal tensors to net.detect_video on the whole clip - ids, scores,
boxes, last_rows - and the same stream_stats, in fp32 and bf16, plain and agnostic, K = 3 and K = 1; with `track`, the online
rows decided by finalize_tracks are detect_video(track=...)'s last_tracks.  Then the guards and detect_yolo3.py --live."""
import os

import numpy as np
import pytest
import torch

from tests import stream_oracle as SO
from tests import track_cases as TC
from viddet_amd.track import finalize_tracks, track_online_host

pytestmark = pytest.mark.gpu

NAMES = ("track", "tlen", "tscore")


# ------------------------------------------------------------------------------------------------ vd_track_push
def _parts(F):
    """all at once, one frame per push, (1, 3, rest)"""
    out = [(F,), (1,) * F]
    if F > 4:
        out.append((1, 3, F - 4))
    return out


def _push_all(state, ins, parts):
    outs, t = [], 0
    for n in parts:
        outs.append(state.push(*[a[t:t + n].contiguous() for a in ins]))
        t += n
    assert t == ins[2].shape[0]
    return [torch.cat(x) for x in zip(*outs)]


def _check_push(case, num_class, kw, parts_list=None):
    from viddet_amd import ops
    okw = {k: v for k, v in kw.items() if k in ("sigma_l", "sigma_iou", "max_age")}
    host = [np.ascontiguousarray(a, dtype=np.float32) for a in case]
    F, N = host[2].shape[:2]
    _, *want = track_online_host(None, *host, num_class=num_class, **okw)
    ins = [torch.from_numpy(a).cuda() for a in host]
    keep = [t.clone() for t in ins]
    state = ops.TrackState(1, N, num_class, **okw)
    first = None
    for parts in parts_list or _parts(F):
        got = _push_all(state, ins, parts)
        torch.cuda.synchronize()
        for name, g, w in zip(NAMES, got, want):
            assert g.dtype == torch.from_numpy(w).dtype and tuple(g.shape) == w.shape, name
            assert torch.equal(g.cpu(), torch.from_numpy(w)), (name, parts)
        assert state.frames == F
        if first is None:
            first = got
        else:                                                              # the same bits again
            assert all(torch.equal(a, b) for a, b in zip(got, first)), parts
        state.reset()                                                      # the next partition starts afresh
        assert state.frames == 0 and int(state.state.max()) == 0
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ins, keep)), "an input was written"
    return want


PUSH_SIZES = [(1, 1), (5, 64), (5, 65), (6, 128)]
PARAMS = [("defaults", {}), ("off_default", TC.OFF_DEFAULT)]


@pytest.mark.parametrize("pname,kw", PARAMS, ids=[p[0] for p in PARAMS])
@pytest.mark.parametrize("F,N", PUSH_SIZES, ids=["%dx%d" % s for s in PUSH_SIZES])
def test_push_equals_host_over_the_sizes(F, N, pname, kw):
    case = TC.random_clip(F, N, seed=7 * F + N, spread=40.0 + N, fill=1.0 if N < 4 else 0.8)
    want = _check_push(case, 1, kw)
    assert (want[0] >= 0).any()
    if N > 64 and not kw:
        assert (want[1][:, 64:] > 1).any(), "no matched row above the lane boundary"


@pytest.mark.parametrize("pname,kw", PARAMS, ids=[p[0] for p in PARAMS])
@pytest.mark.parametrize("name,case,ckw", [c[:3] for c in TC.closed_form()], ids=[c[0] for c in TC.closed_form()])
def test_push_equals_host_on_the_closed_forms(name, case, ckw, pname, kw):
    _check_push(case, ckw.get("num_class", 1), kw)
    if not kw:                                                             # and at the parameters the case was written for
        own = {k: v for k, v in ckw.items() if k in ("sigma_l", "sigma_iou", "max_age")}
        if own:
            _check_push(case, ckw.get("num_class", 1), own)


@pytest.mark.parametrize("pname,kw", PARAMS, ids=[p[0] for p in PARAMS])
@pytest.mark.parametrize("extend", [False, True], ids=["grow", "extend"])
def test_push_with_the_table_at_its_capacity(extend, pname, kw):
    """F = 10, N = 128, max_age = 7, one frame per push: with boxes disjoint from frame to frame the table holds 1024 tracks
    after the 8th push, is written back full and read back full by the 9th and 10th, which close 128 tracks each."""
    from viddet_amd import lib as L
    want = _check_push(TC.capacity(extend), 1, dict(kw, max_age=7), [(1,) * 10])
    if not extend:
        assert (want[0] == np.arange(1280).reshape(10, 128)).all() and (want[1] == 1).all()
        assert L.TRACK_MAX_ACTIVE == 8 * 128


def test_three_streams_in_one_launch_are_three_launches():
    from viddet_amd import ops
    F, N = 5, 65
    clips = [TC.random_clip(F, N, classes=2, seed=s, fill=0.8) for s in (1, 2, 3)]
    assert not np.array_equal(clips[0][2], clips[1][2])
    kw = dict(sigma_iou=0.35, max_age=2)
    ins = [torch.from_numpy(np.stack([np.ascontiguousarray(c[i], dtype=np.float32) for c in clips])).cuda() for i in range(3)]
    three = ops.TrackState(3, N, 2, **kw)
    got = [three.push(*[a[:, t0:t1].contiguous() for a in ins]) for t0, t1 in ((0, 2), (2, 5))]
    got = [torch.cat(x, dim=1) for x in zip(*got)]
    assert tuple(got[0].shape) == (3, F, N)
    for v in range(3):
        one = ops.TrackState(1, N, 2, **kw)
        alone = [one.push(*[a[v, t0:t1].contiguous() for a in ins]) for t0, t1 in ((0, 2), (2, 5))]
        alone = [torch.cat(x) for x in zip(*alone)]
        _, *want = track_online_host(None, *clips[v], num_class=2, **kw)
        for name, g, a, w in zip(NAMES, got, alone, want):
            assert torch.equal(g[v], a), (name, v)
            assert torch.equal(a.cpu(), torch.from_numpy(w)), (name, v)
        assert torch.equal(three.state[v], one.state[0]), "the state of stream %d" % v
    assert (got[0] >= 0).any()


def test_track_state_checks_its_arguments_on_the_host():
    from viddet_amd import ops
    st = ops.TrackState(1, 20, 3)
    z = lambda *s: torch.zeros(*s, device="cuda")
    out = st.push(z(0, 20, 1), z(0, 20, 1), z(0, 20, 4))                    # no frame: nothing is launched
    assert [tuple(o.shape) for o in out] == [(0, 20)] * 3 and st.frames == 0
    with pytest.raises(ValueError, match="bboxes must be"):
        st.push(z(2, 21, 1), z(2, 21, 1), z(2, 21, 4))
    with pytest.raises(ValueError, match="bboxes must be"):
        st.push(z(2, 2, 20, 1), z(2, 2, 20, 1), z(2, 2, 20, 4))
    with pytest.raises(ValueError, match="scores must be a contiguous float32"):
        st.push(z(2, 20, 1), z(2, 20, 2)[:, :, :1], z(2, 20, 4))
    with pytest.raises(ValueError, match="ids must be a contiguous float32"):
        st.push(z(2, 20, 1).cpu(), z(2, 20, 1), z(2, 20, 4))
    # the ids a stream can hand out: frames * N stays below 2**31, counted on the host
    st.frames = (2 ** 31 - 1) // 20 - 1
    st.push(z(1, 20, 1), z(1, 20, 1), z(1, 20, 4))
    with pytest.raises(ValueError, match=r"2\*\*31 - 1"):
        st.push(z(1, 20, 1), z(1, 20, 1), z(1, 20, 4))
    st.reset()
    st.push(z(1, 20, 1), z(1, 20, 1), z(1, 20, 4))
    for bad in (dict(N=129), dict(N=0), dict(V=0), dict(num_class=0), dict(max_age=8), dict(sigma_iou=float("nan"))):
        with pytest.raises(ValueError):
            ops.TrackState(**dict(dict(V=1, N=20, num_class=1), **bad))


# ------------------------------------------------------------------------------------------------ session
CHUNK = 3
PARTS = [(7,), (1,) * 7, (2, 4, 1)]


def _mk(jt, jp, **kw):
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(SO.C)], k=SO.K, k_join_type=jt, k_join_pos=jp, **kw)
    P = SO.params(jt, jp)
    for k, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[k].astype(np.float32)))
    return net


def _mk_k1():
    from oracle import net as ON
    from viddet_amd.model import yolo3_darknet53
    P = ON.init_params(SO.C, seed=11, obj_bias=-1.0)
    net = yolo3_darknet53(["c%d" % i for i in range(SO.C)])
    for k, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[k].astype(np.float32)))
    return net


def _session_clip(session, frames, parts):
    """the clip through the session in pushes of `parts` frames and a flush -> (ids, scores, bboxes, rows, overflow, tracks)"""
    net = session.net
    held = set(t.untyped_storage().data_ptr() for v in net._programs.values() for t in _tensors(v) if t.is_cuda)
    outs, t, expect = [], 0, 0
    for n in list(parts) + [None]:
        t0, ids, sc, bx = session.flush() if n is None else session.push(frames[t:t + n])
        m = ids.shape[0]
        assert t0 == expect, "the emitted frames are contiguous from 0"
        assert tuple(ids.shape) == (m, net.post_nms, 1) and tuple(sc.shape) == (m, net.post_nms, 1) and tuple(bx.shape) == (m, net.post_nms, 4)
        assert tuple(session.last_rows.shape) == (m, net.post_nms) and tuple(session.last_overflow.shape) == (m,)
        for x in (ids, sc, bx, session.last_rows, session.last_overflow):  # new tensors, never views of a program's buffers
            assert m == 0 or x.untyped_storage().data_ptr() not in held
        if n is not None:
            t += n
            assert session.frames_in == t and session.frames_out == expect + m
            assert net._live is session
        expect += m
        trk = session.last_tracks
        if trk is not None:
            assert all(tuple(a.shape) == (m, net.post_nms) for a in trk)
        outs.append((ids, sc, bx, session.last_rows, session.last_overflow) + (tuple(trk) if trk is not None else ()))
    assert expect == frames.shape[0] and session.frames_in == 0 and session.frames_out == 0 and net._live is None
    return [torch.cat(x) for x in zip(*outs)]


def _tensors(v):
    if torch.is_tensor(v):
        yield v
    elif isinstance(v, dict):
        for x in v.values():
            yield from _tensors(x)
    elif isinstance(v, (list, tuple)):
        for x in v:
            yield from _tensors(x)


def _against_detect_video(net, frames, step, chunk, parts_list):
    T = frames.shape[0]
    want = [t.clone() for t in net.detect_video(frames, step=step, chunk=chunk)] + [net.last_rows.clone(), net.last_overflow.clone()]
    stats = dict(net.stream_stats)
    assert stats['prefix_frames'] == (T if net._k > 1 else 0) and stats['suffix_frames'] == T
    assert bool((want[0] >= 0).any()), "fixture produced no detections"
    progs = dict(net._programs)
    session = net.open_video(step=step, chunk=chunk)
    assert session.last_tracks is None
    for parts in parts_list:                                               # one session, clip after clip: flush() starts a new one
        got = _session_clip(session, frames, parts)
        torch.cuda.synchronize()
        for name, g, w in zip(("ids", "scores", "bboxes", "rows", "overflow"), got, want):
            assert g.dtype == w.dtype and torch.equal(g, w), (name, parts)
        assert session.stream_stats == stats, parts
        if net._k > 1:
            assert session.stream_stats['prefix_frames'] == T
    for k, v in progs.items():                                             # no program entry was replaced, none was added
        assert net._programs[k] is v, k
    assert set(net._programs) == set(progs)
    after = list(net.detect_video(frames, step=step, chunk=chunk)) + [net.last_rows, net.last_overflow]
    assert all(torch.equal(a, b) for a, b in zip(after, want)), "detect_video after a whole session"
    return session


CONFIGS = [("max", "early", 1, {}), ("mean", "late", 1, {}), ("cat", "early", 2, {}),
           ("max", "early", 1, dict(bf16=True)), ("max", "late", 1, dict(agnostic=True))]


@pytest.mark.parametrize("jt,jp,step,kw", CONFIGS, ids=["%s-%s-step%d%s" % (c[0], c[1], c[2], "".join("-" + k for k in c[3])) for c in CONFIGS])
def test_session_equals_detect_video(jt, jp, step, kw):
    kw = dict(kw)
    bf16 = kw.pop("bf16", False)
    net = _mk(jt, jp, **kw)
    if bf16:
        net.set_precision('bf16')
    _against_detect_video(net, torch.from_numpy(SO.clip_frames()).cuda(), step, CHUNK, PARTS)
    assert [k[0] for k in net._programs if k[0].startswith('stream')] == ['stream_bf16' if bf16 else 'stream']


def test_session_equals_detect_video_k1():
    _against_detect_video(_mk_k1(), torch.from_numpy(SO.clip_frames()).cuda(), 1, CHUNK, PARTS)


def test_session_on_a_uint8_clip_from_the_host_with_set_nms():
    """the 5-frame uint8 clip of test_uint8_clip_and_set_nms_are_honoured at chunk 2, handed over as host memory"""
    u8 = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (5, SO.SIZE, SO.SIZE, 3), dtype=np.uint8))
    net = _mk("max", "early")
    net.set_nms(nms_thresh=0.3, nms_topk=50, post_nms=20)
    session = _against_detect_video(net, u8, 1, 2, [(5,), (1,) * 5, (2, 3)])
    # the first push fixes the frame size
    session.push(u8[:1])
    with pytest.raises(ValueError, match="its first push fixed that"):
        session.push(u8[:1, :32])
    with pytest.raises(ValueError, match="its first push fixed that"):
        session.push(torch.zeros(1, 3, SO.SIZE, SO.SIZE))
    with pytest.raises(ValueError, match="expected frames"):
        session.push(u8[0])
    session.flush()
    session.push(torch.zeros(1, 3, SO.SIZE, SO.SIZE))                      # a new clip may have another
    session.flush()


@pytest.mark.parametrize("k1", [False, True], ids=["k3-max-early", "k1"])
def test_detect_video_on_a_float_clip_in_host_memory(k1):
    """the engine slices every group out of the clip where it lives: a float clip on the host gives the device clip's bits"""
    net = _mk_k1() if k1 else _mk("max", "early")
    frames = torch.from_numpy(SO.clip_frames())
    assert frames.dtype == torch.float32 and not frames.is_cuda
    want = [t.clone() for t in net.detect_video(frames.cuda(), chunk=CHUNK)] + [net.last_rows.clone(), net.last_overflow.clone()]
    got = list(net.detect_video(frames.cpu(), chunk=CHUNK)) + [net.last_rows, net.last_overflow]
    torch.cuda.synchronize()
    assert bool((want[0] >= 0).any()), "fixture produced no detections"
    for name, g, w in zip(("ids", "scores", "bboxes", "rows", "overflow"), got, want):
        assert g.is_cuda and g.dtype == w.dtype and torch.equal(g, w), name


def test_session_with_track():
    net = _mk("max", "early")
    frames = torch.from_numpy(SO.clip_frames()).cuda()
    trk = dict(TC.OFF_DEFAULT, clip=SO.SIZE)
    plain = [t.clone() for t in net.detect_video(frames, chunk=CHUNK, track=trk)]
    want = [t.clone() for t in net.last_tracks]
    session = net.open_video(chunk=CHUNK, track=trk)
    assert session.track_decide == dict(sigma_h=TC.OFF_DEFAULT["sigma_h"], t_min=TC.OFF_DEFAULT["t_min"])
    okw = {k: TC.OFF_DEFAULT[k] for k in ("sigma_l", "sigma_iou", "max_age")}
    _, *host = track_online_host(None, plain[0].cpu().numpy(), plain[1].cpu().numpy(), plain[2].clamp(0, SO.SIZE).cpu().numpy(),
                                 num_class=SO.C, **okw)
    for parts in PARTS:
        got = _session_clip(session, frames, parts)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], plain))
        online = [t.cpu().numpy() for t in got[5:]]
        assert len(online) == 3
        for name, o, h in zip(NAMES, online, host):                        # ids from 0 in every clip: flush() reset the state
            assert np.array_equal(o, h), (name, parts)
        final = finalize_tracks(*online, **session.track_decide)
        for name, f, w in zip(NAMES, final, want):
            assert torch.equal(torch.from_numpy(f), w.cpu()), (name, parts)
    print("candidate rows %d, rows of kept tracks %d" % ((host[0] >= 0).sum(), int((want[0] >= 0).sum())))
    # track=True: the defaults; and parameters that keep tracks of this fixture's low scores
    for trk, kept in ((True, False), (dict(sigma_h=0.0, max_age=1), True)):
        net.detect_video(frames, chunk=CHUNK, track=trk)
        want = [t.cpu() for t in net.last_tracks]
        session = net.open_video(chunk=CHUNK, track=trk)
        got = _session_clip(session, frames, (3, 4))
        final = finalize_tracks(*[t.cpu().numpy() for t in got[5:]], **session.track_decide)
        assert all(torch.equal(torch.from_numpy(f), w) for f, w in zip(final, want))
        assert not kept or bool((want[0] >= 0).any()), "no track is kept: the decision is not exercised"


def test_one_session_in_flight_per_net():
    net = _mk("mean", "late")
    frames = torch.from_numpy(SO.clip_frames()).cuda()
    before = [t.clone() for t in net.detect_video(frames, chunk=CHUNK)]
    a = net.open_video(chunk=CHUNK)
    b = net.open_video(chunk=CHUNK)                                        # nothing in flight yet: both may exist
    w = frames[:2, None].expand(-1, SO.K, -1, -1, -1).contiguous()
    plain = [t.clone() for t in net(w)]
    a.push(frames[:2])
    with pytest.raises(RuntimeError, match="VideoSession.*2 frames in"):
        net.detect_video(frames, chunk=CHUNK)
    with pytest.raises(RuntimeError, match="VideoSession.*2 frames in"):
        net.open_video()
    with pytest.raises(RuntimeError, match="another video session"):
        b.push(frames[:1])
    assert all(torch.equal(x, y) for x, y in zip(plain, net(w))), "net(x) is not affected"
    a.push(frames[2:])
    t0, ids, sc, bx = a.flush()
    # free again
    after = net.detect_video(frames, chunk=CHUNK)
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    got = _session_clip(b, frames, (7,))
    assert all(torch.equal(x, y) for x, y in zip(before, got[:3]))
    net.open_video().flush()                                               # an empty clip: nothing in, nothing out
    assert net._live is None


# ------------------------------------------------------------------------------------------------ script
def test_detect_script_live_writes_what_the_stream_run_writes(tmp_path):
    import detect_yolo3 as D
    common = ["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
              "--synthetic_samples", "5", "--synthetic_videos", "2", "--data_shape", "64", "--batch_size", "2", "--metrics", "voc",
              "--save_dir", str(tmp_path), "--stream", "--track"]
    out_s = D.main(common + ["--save_prefix", "s"])
    out_l = D.main(common + ["--save_prefix", "l", "--live", "--live_push", "2"])
    s, l = tmp_path / "s", tmp_path / "l"
    made = sorted(os.listdir(s))
    assert made == sorted(os.listdir(l)) and {"pred", "pred_trk", "tracks.txt"} <= set(made)
    for name in made:                                                      # everything the --stream run writes, byte for byte
        if os.path.isdir(s / name):
            assert sorted(os.listdir(s / name)) == sorted(os.listdir(l / name)) and len(os.listdir(s / name)) == 10
            for f in os.listdir(s / name):
                assert open(s / name / f, "rb").read() == open(l / name / f, "rb").read(), (name, f)
        else:
            assert open(s / name, "rb").read() == open(l / name, "rb").read(), name
    assert sum(len(open(s / "pred" / f).read().splitlines()) for f in os.listdir(s / "pred")) > 10, "(almost) no detections"
    # the voc result (a per-class model writes no voc.txt: main() hands the names and values back): the same numbers exactly
    assert out_s[0] == out_l[0] and np.array_equal(np.asarray(out_s[1]), np.asarray(out_l[1]), equal_nan=True)
