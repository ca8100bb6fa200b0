"""GPU: SORT and BYTE carried through live sessions on the device (vd_track_kf_push, ops.KalmanTrackState).

Kernel: KalmanTrackState.push equals its definition (sort.sort_online_host, byte.byte_online_host, themselves held to sort_host
and byte_host in tests/test_kf_live_cpu.py) bit for bit - track, tlen and tscore with torch.equal, tbox on its bytes wherever
the definition's value is no NaN and a NaN wherever it is - however the frames are cut into pushes: on the closed forms, on
clips that cross the 64-row boundary and run both associations, with the table of active tracks written back full and read back
full, with a 128-row assignment against tracks that crossed a launch boundary, on three streams in one launch; and
finalize_tracks of its rows is what the offline kernels give.
Session: net.open_video(track={'method': 'sort' | 'byte', 'online': True}) gives detect_video's detections, and its online
rows decided by finalize_tracks are detect_video(track=...)'s last_tracks and last_track_boxes.  Then detect_yolo3.py
--track_online."""
import os

import numpy as np
import pytest
import torch

from tests import byte_cases as BC
from tests import sort_cases as SC
from tests import stream_oracle as SO
from viddet_amd import byte as B
from viddet_amd import sort as S
from viddet_amd.byte import byte_host, byte_online_host
from viddet_amd.sort import sort_host, sort_online_host
from viddet_amd.track import finalize_tracks

pytestmark = pytest.mark.gpu

NAMES = ("track", "tlen", "tscore")
ONLINE = dict(sort=sort_online_host, byte=byte_online_host)
OFFLINE = dict(sort=sort_host, byte=byte_host)
DEFAULTS = dict(sort=S.DEFAULTS, byte=B.DEFAULTS)
DECIDE = ("sigma_h", "t_min")


def _okw(method, kw):
    """a case's keyword arguments -> those the method's online form takes"""
    return {k: v for k, v in kw.items() if k in DEFAULTS[method] and k not in DECIDE}


def _same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == torch.from_numpy(w).dtype and tuple(g.shape) == w.shape, (what, name)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (what, name)
    assert got[3].dtype == torch.float32 and SC.same_tbox(got[3].cpu().numpy(), want[3]), (what, "tbox")


def _bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


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


def _check_push(method, case, num_class, okw, parts_list=None):
    """every partition of the clip through one KalmanTrackState, reset() between -> (the definition's four arrays, its stats)"""
    from viddet_amd import ops
    host = [np.ascontiguousarray(a, dtype=np.float32) for a in case]
    F, N = host[2].shape[:2]
    stats = {}
    _, *want = ONLINE[method](None, *host, num_class=num_class, stats=stats, **okw)
    ins = [torch.from_numpy(a).cuda() for a in host]
    keep = [t.clone() for t in ins]
    state = ops.KalmanTrackState(1, N, num_class, method=method, **okw)
    first = None
    for parts in parts_list or _parts(F):
        got = _push_all(state, ins, parts)
        torch.cuda.synchronize()
        _same(got, want, parts)
        assert state.frames == F
        if first is None:
            first = got
        else:                                                              # the same bits again
            assert _bits(got, first), parts
        state.reset()                                                      # the next partition starts afresh
        assert state.frames == 0 and int(state.state.max()) == 0
    assert _bits(ins, keep), "an input was written"
    return want, stats


# ------------------------------------------------------------------------------------------------ vd_track_kf_push
def _dipped_clip(T, N):
    """BC.dipped on more objects than rows, cut to N rows: walkers with score dips (a share of the rows below sigma_d), objects
    that miss frames, and - where the frame holds at least N of them - every row of the frame filled"""
    seed = 3 if (T, N) == (3, 2) else 1
    clip = BC.dipped(seed, dip=0.5, T=T, objects=int(N * 1.25) + 1, classes=1, extent=200.0 + 12.0 * N)
    return [np.ascontiguousarray(a[:, :N]) for a in clip]


@pytest.mark.parametrize("T,N", SC.GPU_SIZES, ids=["%dx%d" % s for s in SC.GPU_SIZES])
@pytest.mark.parametrize("max_age", [0, 1, 7])
@pytest.mark.parametrize("method", ["sort", "byte"])
def test_push_equals_host_over_the_sizes(method, max_age, T, N):
    want, stats = _check_push(method, _dipped_clip(T, N), 1, dict(max_age=max_age))
    assert (want[0] >= 0).any()
    if method == "byte" and T > 1:                                         # both associations ran
        assert stats["first"].sum() > 0 and stats["second"].sum() > 0
    if N > 64:
        assert (want[1][:, 64:] > 1).any(), "no matched row above the lane boundary"
    if N >= 63 and max_age < 7:
        assert stats["closed"].sum() > 0


SORT_FORMS = [("sort",) + c for c in SC.closed_form()]
BYTE_FORMS = [("byte",) + c for c in BC.closed_form()]


@pytest.mark.parametrize("method,name,case,kw,track,tlen", SORT_FORMS + BYTE_FORMS, ids=["%s-%s" % c[:2] for c in SORT_FORMS + BYTE_FORMS])
def test_push_equals_host_on_the_closed_forms(method, name, case, kw, track, tlen):
    F = case[2].shape[0]
    want, _ = _check_push(method, case, kw.get("num_class", 1), _okw(method, kw), [(F,), (1,) * F])
    final = finalize_tracks(*want[:3], tbox=want[3], **{k: v for k, v in kw.items() if k in DECIDE})
    assert final[0].tolist() == np.asarray(track).tolist()                 # the ids written out by hand
    if tlen is not None:
        assert final[1].tolist() == np.asarray(tlen).tolist()


@pytest.mark.parametrize("which", ["sort_grow", "byte_extend", "byte_full"])
def test_push_with_the_state_at_its_capacity(which):
    """F = 10, N = 128, max_age = 7, one frame per push.  sort_grow: with boxes disjoint from frame to frame the state holds
    1024 tracks after the 8th push, is written back full and read back full by the 9th and 10th, which close 128 tracks each.
    byte_extend: every odd push brings 128 low rows, all matched by the second association.  byte_full: the 9th push's 128 low
    rows meet 1024 columns, in a launch that only read its tracks from the state."""
    from viddet_amd import lib as L
    method, case = dict(sort_grow=("sort", lambda: SC.capacity(False)), byte_extend=("byte", lambda: BC.capacity_low(True)),
                        byte_full=("byte", BC.capacity_full))[which]
    want, stats = _check_push(method, case(), 1, dict(max_age=7), [(1,) * 10])
    assert L.TRACK_MAX_ACTIVE == 8 * 128
    if which == "sort_grow":
        assert (want[0] == np.arange(1280).reshape(10, 128)).all() and (want[1] == 1).all()
        assert stats["active"].tolist() == [128 * n for n in range(1, 9)] + [1024, 1024] and stats["closed"].tolist() == [0] * 8 + [128, 128]
    elif which == "byte_extend":
        assert stats["active"].tolist() == [128] * 10 and (want[1] == np.arange(1, 11)[:, None]).all()
        assert stats["second"].tolist() == [0, 128] * 5
    else:
        assert stats["active"].max() == 1024 and stats["second"].tolist() == [0] * 8 + [128, 0] and stats["closed"][8] == 128


def test_a_crowded_frame_pair_across_a_launch_boundary():
    """byte_cases' crowded pair as two pushes of one frame: 64 high and 64 low rows against 128 tracks that the second launch
    reads from the state, most rows with a dozen admissible cells, both associations displacing earlier rows"""
    okw = _okw("byte", BC.CROWDED_KW)
    want, stats = _check_push("byte", BC.crowded_pair(), 1, okw, [(1, 1), (2,)])
    assert stats["first"][1] >= 32 and stats["second"][1] >= 32
    assert want[0][1].tolist() != sorted(want[0][1].tolist())
    final = finalize_tracks(*want[:3], tbox=want[3], t_min=BC.CROWDED_KW["t_min"])
    assert all(np.array_equal(a, b) for a, b in zip(final, byte_host(*BC.crowded_pair(), num_class=1, **BC.CROWDED_KW)))


def _live_part(state, v):
    """stream v's state block as (header (n_active, next_id, cur), the five word tables' live entries, the current filter
    table's live entries)"""
    from viddet_amd import lib as L
    blk = state.state[v].cpu().numpy()
    n, next_id, cur, unused = blk[:16].view(np.int32).tolist()
    assert 0 <= n <= L.TRACK_MAX_ACTIVE and cur in (0, 1) and unused == 0
    words = blk[16:16 + 20 * L.TRACK_MAX_ACTIVE].view(np.int32).reshape(5, L.TRACK_MAX_ACTIVE)[:, :n]
    tables = blk[16 + 20 * L.TRACK_MAX_ACTIVE:].view(np.int32).reshape(2, S.STATE_FLOATS, L.TRACK_MAX_ACTIVE)
    return (n, next_id, cur), words.copy(), tables[cur, :, :n].copy()


def test_three_streams_in_one_launch_are_three_launches():
    from viddet_amd import ops
    F, N = 5, 65
    clips = [_dipped_clip(F, N)] + [[np.ascontiguousarray(a[:, :N]) for a in BC.dipped(s, dip=0.5, T=F, objects=80, classes=2)] for s in (2, 3)]
    assert not np.array_equal(clips[1][2], clips[2][2])
    kw = dict(sigma_iou=0.25, max_age=2)
    ins = [torch.from_numpy(np.stack([c[i] for c in clips])).cuda() for i in range(3)]
    three = ops.KalmanTrackState(3, N, 2, method="byte", **kw)
    got = [three.push(*[a[:, t0:t1].contiguous() for a in ins]) for t0, t1 in ((0, 2), (2, 5))]
    got = [torch.cat(x, dim=1) for x in zip(*got)]
    assert tuple(got[0].shape) == (3, F, N) and tuple(got[3].shape) == (3, F, N, 4)
    for v in range(3):
        one = ops.KalmanTrackState(1, N, 2, method="byte", **kw)
        alone = [one.push(*[a[v, t0:t1].contiguous() for a in ins]) for t0, t1 in ((0, 2), (2, 5))]
        alone = [torch.cat(x) for x in zip(*alone)]
        stats = {}
        s, *want = byte_online_host(None, *clips[v], num_class=2, stats=stats, **kw)
        assert _bits([g[v] for g in got], alone), v
        _same(alone, want, v)
        assert stats["second"].sum() > 0
        a, b = _live_part(three, v), _live_part(one, 0)
        assert a[0] == b[0] == (len(s["id"]), s["next_id"], F % 2), "the header of stream %d" % v
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), "the live entries of stream %d" % v
        assert a[1][1].tolist() == s["id"].tolist() and a[1][3].tolist() == s["len"].tolist()
    assert (got[0] >= 0).any()


@pytest.mark.parametrize("method", ["sort", "byte"])
def test_finalized_device_rows_are_the_offline_kernels(method):
    from viddet_amd import ops
    case = [np.ascontiguousarray(a, dtype=np.float32) for a in BC.random_clip(7, 40, classes=2, seed=3)]
    ins = [torch.from_numpy(a).cuda() for a in case]
    link = dict(sort=ops.track_sort, byte=ops.track_byte)[method]
    sets = [dict(), dict(sigma_l=0.2, sigma_iou=0.35, sigma_h=0.8, t_min=3, max_age=2)]
    if method == "byte":
        sets[1].update(sigma_d=0.45, sigma_new=0.7, sigma_iou2=0.3)
    kept = []
    for kw in sets:
        want = link(*ins, num_class=2, **kw)
        state = ops.KalmanTrackState(1, 40, 2, method=method, **_okw(method, kw))
        rows = _push_all(state, ins, (2, 1, 4))
        torch.cuda.synchronize()
        final = finalize_tracks(*[r.cpu().numpy() for r in rows[:3]], tbox=rows[3].cpu().numpy(), **{k: v for k, v in kw.items() if k in DECIDE})
        for name, f, w in zip(NAMES + ("tbox",), final, want):
            f = torch.from_numpy(f)
            assert f.dtype == w.dtype and torch.equal(f.view(torch.int32), w.cpu().view(torch.int32)), (name, kw)
        kept.append(int((want[0] >= 0).sum()))
        assert kept[-1] > 0 and bool(((rows[0] >= 0) & (want[0] < 0)).any()), "no track is dropped: the decision is not exercised"
    assert kept[0] != kept[1]


def test_kalman_track_state_checks_its_arguments_on_the_host():
    from viddet_amd import ops
    st = ops.KalmanTrackState(1, 20, 3, method="byte")
    z = lambda *s: torch.zeros(*s, device="cuda")
    out = st.push(z(0, 20, 1), z(0, 20, 1), z(0, 20, 4))                    # no frame: nothing is launched
    assert [tuple(o.shape) for o in out] == [(0, 20)] * 3 + [(0, 20, 4)] and st.frames == 0
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
    out = st.push(z(1, 20, 1) - 1, z(1, 20, 1), z(1, 20, 4))
    assert st.frames == 1 and int(out[0].max()) == -1


# ------------------------------------------------------------------------------------------------ session
CHUNK = 3
PARTS = [(1,) * 7, (3, 4), (7,)]


def _mk(jt, jp, **kw):
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(SO.C)], k=SO.K, k_join_type=jt, k_join_pos=jp, **kw)
    P = SO.params(jt, jp)
    for k, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[k].astype(np.float32)))
    return net


def _session_clip(session, frames, parts):
    """the clip through the session in pushes of `parts` frames and a flush -> (ids, scores, bboxes, track, tlen, tscore, tbox)"""
    net = session.net
    outs, t, expect = [], 0, 0
    for n in list(parts) + [None]:
        t0, ids, sc, bx = session.flush() if n is None else session.push(frames[t:t + n])
        m = ids.shape[0]
        assert t0 == expect, "the emitted frames are contiguous from 0"
        if n is not None:
            t += n
            assert session.frames_in == t and session.frames_out == expect + m
        expect += m
        trk, tbox = session.last_tracks, session.last_track_boxes
        assert isinstance(trk, tuple) and len(trk) == 3 and all(tuple(a.shape) == (m, net.post_nms) for a in trk)
        assert tuple(tbox.shape) == (m, net.post_nms, 4) and tbox.dtype == torch.float32
        outs.append((ids, sc, bx) + trk + (tbox,))
    assert expect == frames.shape[0] and session.frames_in == 0 and session.frames_out == 0 and net._live is None
    return [torch.cat(x) for x in zip(*outs)]


@pytest.mark.parametrize("method", ["sort", "byte"])
def test_session_carries_the_tracker(method):
    net = _mk("max", "early")
    frames = torch.from_numpy(SO.clip_frames()).cuda()
    plain = [t.clone() for t in net.detect_video(frames, chunk=CHUNK)]
    sc = plain[1][plain[0] >= 0]
    assert sc.numel() > 10, "fixture produced (almost) no detections"
    # parameters that keep tracks of this fixture's low scores; the split at the rows' median score: half of them are low rows
    kw = dict(sigma_l=0.0, sigma_h=0.0, sigma_iou=0.2, max_age=2)
    if method == "byte":
        kw.update(sigma_d=float(sc.median()), sigma_new=float(sc.median()), sigma_iou2=0.2)
    trk = dict(kw, method=method, clip=SO.SIZE)
    again = net.detect_video(frames, chunk=CHUNK, track=trk)
    want = [t.clone() for t in net.last_tracks] + [net.last_track_boxes.clone()]
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    assert bool((want[0] >= 0).any()), "no track is kept: the decision is not exercised"
    stats = {}
    _, *host = ONLINE[method](None, plain[0].cpu().numpy(), plain[1].cpu().numpy(), plain[2].clamp(0, SO.SIZE).cpu().numpy(),
                              num_class=SO.C, stats=stats, **_okw(method, kw))
    print("candidate rows %d, rows of kept tracks %d, stats %r" % ((host[0] >= 0).sum(), int((want[0] >= 0).sum()), {k: v.tolist() for k, v in stats.items()}))
    if method == "byte":
        assert stats["second"].sum() > 0, "no second-pass match: BYTE's own step is not exercised"
    with pytest.raises(NotImplementedError, match="open_video with track method '%s'" % method):
        net.open_video(chunk=CHUNK, track=trk)
    session = net.open_video(chunk=CHUNK, track=dict(trk, online=True))
    assert session.track_decide == dict(sigma_h=0.0, t_min=2) and session.last_track_boxes is None
    for parts in PARTS:                                                    # one session, clip after clip
        got = _session_clip(session, frames, parts)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got[:3], plain)), parts
        _same(got[3:], host, parts)                                        # ids from 0 in every clip: flush() reset the state
        assert int(got[3][got[3] >= 0].min()) == 0
        final = finalize_tracks(*[t.cpu().numpy() for t in got[3:6]], tbox=got[6].cpu().numpy(), **session.track_decide)
        for name, f, w in zip(NAMES + ("tbox",), final, want):
            f = torch.from_numpy(f)
            assert f.dtype == w.dtype and torch.equal(f.view(torch.int32), w.cpu().view(torch.int32)), (name, parts)
    # the IOU tracker with the word is the session as ever
    iou = net.open_video(chunk=CHUNK, track=dict(method="iou", online=True, sigma_h=0.0))
    iou.push(frames)
    iou.flush()
    assert len(iou.last_tracks) == 3 and iou.last_track_boxes is None


# ------------------------------------------------------------------------------------------------ script
@pytest.mark.parametrize("method", ["sort", "byte"])
def test_detect_script_track_online_writes_what_the_stream_run_writes(tmp_path, method):
    import detect_yolo3 as D
    common = ["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
              "--synthetic_samples", "5", "--synthetic_videos", "2", "--data_shape", "64", "--batch_size", "2", "--metrics", "voc",
              "--save_dir", str(tmp_path), "--stream", "--track", "--track_method", method, "--track_high", "0", "--track_low", "0"]
    if method == "byte":                                                   # every row a candidate, those from 0.05 up high rows
        common += ["--track_det", "0.05", "--track_new", "0.05"]
    out_s = D.main(common + ["--save_prefix", "s"])
    out_l = D.main(common + ["--save_prefix", "l", "--live", "--live_push", "2", "--track_online"])
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
    lines = [line for f in os.listdir(s / "pred_trk") for line in open(s / "pred_trk" / f).read().splitlines()]
    assert len(lines) > 10, "(almost) no detections"
    assert any(int(line.rsplit(",", 1)[1]) >= 0 for line in lines), "no row is tracked: the ids are not exercised"
    assert out_s[0] == out_l[0] and np.array_equal(np.asarray(out_s[1]), np.asarray(out_l[1]), equal_nan=True)
