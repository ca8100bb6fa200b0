"""GPU: fixed-lag smoothing of track boxes in live sessions on the device (vd_track_smooth_push, ops.SmoothLagState).

Kernel: SmoothLagState.push / flush equal the definition (smooth_lag.smooth_lag_host, itself held to smooth_host frame by frame
in tests/test_smooth_lag_cpu.py) bit for bit on sbox and slen, however the frames are cut into pushes: at sizes on either side
of the 64-row boundary and where the 16-slot ring wraps, on hostile tables, on the closed forms, on three streams in one launch.
Session: net.open_video(track=..., smooth={'lag': L}) for the three trackers - with a lag longer than the clip and nothing
dropped it is detect_video(track=..., smooth=...), with lag 2 it is the definition on the session's own online rows, two frames
late.  Then detect_yolo3.py --track_smooth_lag."""
import os

import numpy as np
import pytest
import torch

from tests import smooth_cases as MC
from tests import smooth_lag_cases as LC
from tests import stream_oracle as SO
from viddet_amd.smooth_lag import smooth_lag_host
from viddet_amd.track import finalize_tracks

pytestmark = pytest.mark.gpu

SIZES = MC.GPU_SIZES + [(40, 5)]                      # (40, 5): the ring wraps more than twice


def _bits(got, want):
    return got.dtype == torch.float32 and tuple(got.shape) == want.shape and \
        torch.equal(got.cpu().view(torch.int32), torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32))


def _ins(case):
    host = [np.ascontiguousarray(a, dtype=np.float32) for a in case[:3]] + [np.ascontiguousarray(case[3], dtype=np.int32)]
    return host, [torch.from_numpy(a).cuda() for a in host]


def _push_all(state, ins, parts):
    """the clip in pushes of `parts` frames and a flush -> (sbox, slen) of all its frames"""
    T, lag = ins[2].shape[0], state.lag
    outs, t, expect = [], 0, 0
    for n in list(parts) + [None]:
        t0, sbox, slen = state.flush() if n is None else state.push(*[a[t:t + n].contiguous() for a in ins])
        assert t0 == expect and sbox.shape[0] == slen.shape[0]
        if n is not None:
            t += n
            assert state.frames == t and expect + sbox.shape[0] == max(0, t - lag)         # a frame comes out `lag` late
        expect += sbox.shape[0]
        outs.append((sbox, slen))
    assert t == T == expect and state.frames == 0
    return [torch.cat(x) for x in zip(*outs)]


def _check(case, num_class, lags, gaps, parts_list=None):
    from viddet_amd import ops
    host, ins = _ins(case)
    keep = [t.clone() for t in ins]
    F, N = host[2].shape[:2]
    moved = 0
    for lag in lags:
        for max_gap in gaps:
            want = LC.run_host(tuple(host), num_class, lag, max_gap)
            state = ops.SmoothLagState(1, N, num_class, lag=lag, max_gap=max_gap)
            for parts in parts_list or LC.parts_of(F):
                sbox, slen = _push_all(state, ins, parts)
                assert _bits(sbox, want[0]), (lag, max_gap, parts)
                assert slen.dtype == torch.int32 and torch.equal(slen.cpu(), torch.from_numpy(want[1])), (lag, max_gap, parts)
                assert int(state.state.count_nonzero()) == 0, "flush() leaves the state all zero"
                state.push(*[a[:1].contiguous() for a in ins])
                assert int(state.state.count_nonzero()) > 0
                state.reset()
                assert int(state.state.count_nonzero()) == 0 and state.frames == 0
            moved += int((want[0].view(np.uint32) != host[2].view(np.uint32)).any(axis=2).sum())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ins, keep)), "an input was written"
    return moved


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("F,N", SIZES)
def test_push_equals_the_definition(F, N):
    case = LC.tracked("sort", 3 * F + N, T=F, objects=N) if (F, N) == (40, 5) else MC.sort_table(F, N, 7)
    assert LC.within_bound(case[3])
    moved = _check(case, 2, (0, 1, 7, 15), (0, 7))
    assert moved > 0 or F * N < 8


@pytest.mark.parametrize("F,N", [(6, 65), (12, 128)])
def test_push_equals_the_definition_on_hostile_tables(F, N):
    """ids anywhere, repeated within a frame and outside the causal bound, rows that are not present, boxes with zero heights,
    infinities and NaNs: any table is safe, and the definition says what comes out"""
    case = MC.hostile(F, N)
    assert not LC.within_bound(case[3])
    _check(case, 1, (0, 3, 15), (1, 7), [(F,), (1,) * F])


def test_three_streams_in_one_launch_equal_three_states():
    from viddet_amd import ops
    F, N, lag = 20, 9, 3
    cases = [LC.tracked(k, 11 + i, T=F, objects=N) for i, k in enumerate(("sort", "byte", "iou"))]
    ins = [torch.from_numpy(np.stack([np.ascontiguousarray(c[j], np.int32 if j == 3 else np.float32) for c in cases])).cuda() for j in range(4)]
    many = ops.SmoothLagState(3, N, 2, lag=lag)
    outs, t = [], 0
    for n in (1, 7, 12, None):
        t0, sbox, slen = many.flush() if n is None else many.push(*[a[:, t:t + n].contiguous() for a in ins])
        assert tuple(sbox.shape[:1]) == (3,) and sbox.shape[1] == slen.shape[1]
        t += n or 0
        outs.append((sbox, slen))
    sbox, slen = (torch.cat(x, dim=1) for x in zip(*outs))
    assert tuple(sbox.shape) == (3, F, N, 4) and int(many.state.count_nonzero()) == 0
    for v, case in enumerate(cases):
        one = ops.SmoothLagState(1, N, 2, lag=lag)
        a, b = _push_all(one, [x[v].contiguous() for x in ins], (F,))
        want = LC.run_host(case, 2, lag, 7)
        assert _bits(a, want[0]) and torch.equal(b.cpu(), torch.from_numpy(want[1]))
        assert torch.equal(sbox[v].view(torch.int32), a.view(torch.int32)) and torch.equal(slen[v], b), v


@pytest.mark.parametrize("name", sorted(LC.closed_forms()))
def test_closed_forms(name):
    case = LC.closed_forms()[name]
    F = case[2].shape[0]
    _check(case, 1, (0, 2, 15), (2, 7), [(F,), (1,) * F])


def test_smooth_lag_state_checks_its_arguments_on_the_host():
    from viddet_amd import ops
    with pytest.raises(ValueError, match="lag must be given"):
        ops.SmoothLagState(1, 20, 3)
    with pytest.raises(ValueError, match="SmoothLagState: lag must be an integer in \\[0, 15\\]"):
        ops.SmoothLagState(1, 20, 3, lag=16)
    with pytest.raises(ValueError, match="SmoothLagState: max_gap"):
        ops.SmoothLagState(1, 20, 3, lag=1, max_gap=8)
    with pytest.raises(ValueError, match="N must be an integer in \\[1, 128\\]"):
        ops.SmoothLagState(1, 129, 3, lag=1)
    st = ops.SmoothLagState(1, 20, 3, lag=2)
    z = lambda *s: torch.zeros(*s, device="cuda")
    zi = lambda *s: torch.zeros(*s, device="cuda", dtype=torch.int32)
    t0, sbox, slen = st.push(z(0, 20, 1), z(0, 20, 1), z(0, 20, 4), zi(0, 20))     # no frame: nothing is launched
    assert t0 == 0 and tuple(sbox.shape) == (0, 20, 4) and tuple(slen.shape) == (0, 20) and st.frames == 0
    t0, sbox, slen = st.flush()                                                    # the flush of an empty stream
    assert t0 == 0 and tuple(sbox.shape) == (0, 20, 4) and slen.dtype == torch.int32
    with pytest.raises(ValueError, match="bboxes must be"):
        st.push(z(2, 21, 1), z(2, 21, 1), z(2, 21, 4), zi(2, 21))
    with pytest.raises(ValueError, match="scores must be a contiguous float32"):
        st.push(z(2, 20, 1), z(2, 20, 2)[:, :, :1], z(2, 20, 4), zi(2, 20))
    with pytest.raises(ValueError, match="track must be a contiguous int32"):
        st.push(z(2, 20, 1), z(2, 20, 1), z(2, 20, 4), z(2, 20))
    with pytest.raises(ValueError, match="track must be a contiguous int32"):
        st.push(z(2, 20, 1), z(2, 20, 1), z(2, 20, 4), zi(2, 19))
    t0, sbox, _ = st.push(z(1, 20, 1), z(1, 20, 1), z(1, 20, 4), zi(1, 20))
    assert (t0, sbox.shape[0], st.frames, st.emitted) == (0, 0, 1, 0)
    t0, sbox, _ = st.push(z(3, 20, 1), z(3, 20, 1), z(3, 20, 4), zi(3, 20))
    assert (t0, sbox.shape[0], st.frames, st.emitted) == (0, 2, 4, 2)
    st.frames = (2 ** 31 - 1) // 20                                                # counted on the host
    with pytest.raises(ValueError, match=r"2\*\*31 - 1"):
        st.push(z(1, 20, 1), z(1, 20, 1), z(1, 20, 4), zi(1, 20))
    st.reset()
    assert st.frames == 0 and int(st.state.count_nonzero()) == 0


# ------------------------------------------------------------------------------------------------ session
CHUNK = 3
PARTS = [(1,) * 7, (3, 4), (7,)]
TRACKERS = dict(iou=dict(sigma_iou=0.2, max_age=2), sort=dict(method="sort", online=True, sigma_iou=0.2, max_age=2),
                byte=dict(method="byte", online=True, sigma_iou=0.2, sigma_iou2=0.2, max_age=2))


def _mk(jt, jp, **kw):
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(SO.C)], k=SO.K, k_join_type=jt, k_join_pos=jp, **kw)
    P = SO.params(jt, jp)
    for k, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[k].astype(np.float32)))
    return net


def _session_clip(session, frames, parts, late):
    """the clip through the session -> ([ids, scores, bboxes, track, tlen, tscore, rows, overflow, pre, slen(, tbox)], the
    frames returned after every push).  late: frames_out of a session without the option after the same pushes."""
    net, P = session.net, session.net.post_nms
    outs, counts, t, expect = [], [], 0, 0
    for i, n in enumerate(list(parts) + [None]):
        t0, ids, sc, bx = session.flush() if n is None else session.push(frames[t:t + n])
        m = ids.shape[0]
        assert t0 == expect, "the returned frames are contiguous from 0"
        if n is not None:
            t += n
            assert session.frames_in == t and session.frames_out == expect + m
            if late is not None:
                assert expect + m == max(0, late[i] - session._smo_kw["lag"]), "a frame comes out `lag` frames late"
        expect += m
        counts.append(expect)
        trk = session.last_tracks
        assert tuple(ids.shape) == (m, P, 1) and tuple(sc.shape) == (m, P, 1) and tuple(bx.shape) == (m, P, 4)
        assert isinstance(trk, tuple) and len(trk) == 3 and all(tuple(a.shape) == (m, P) for a in trk)
        assert tuple(session.last_rows.shape) == (m, P) and tuple(session.last_overflow.shape) == (m,)
        assert tuple(session.last_pre_smooth.shape) == (m, P, 4) and tuple(session.last_smooth.shape) == (m, P)
        one = (ids, sc, bx) + trk + (session.last_rows, session.last_overflow, session.last_pre_smooth, session.last_smooth)
        if session.last_track_boxes is not None:
            assert tuple(session.last_track_boxes.shape) == (m, P, 4)
            one += (session.last_track_boxes,)
        outs.append(one)
    assert expect == frames.shape[0] and session.frames_in == 0 and session.frames_out == 0 and net._live is None
    assert session._held is None
    return [torch.cat(x) for x in zip(*outs)], counts


@pytest.mark.parametrize("method", ["iou", "sort", "byte"])
def test_session_smooths_with_a_fixed_lag(method):
    net = _mk("max", "early")
    frames = torch.from_numpy(SO.clip_frames()).cuda()
    plain = [t.clone() for t in net.detect_video(frames, chunk=CHUNK)]
    rows_plain, over_plain = net.last_rows.clone(), net.last_overflow.clone()
    sc = plain[1][plain[0] >= 0]
    assert sc.numel() > 10, "fixture produced (almost) no detections"
    kw = dict(TRACKERS[method], sigma_l=0.0, sigma_h=0.0, t_min=1, clip=SO.SIZE)       # nothing is dropped at the clip's end
    if method == "byte":
        kw.update(sigma_d=float(sc.median()), sigma_new=float(sc.median()))
    off = {k: v for k, v in kw.items() if k != "online"}
    want = [t.clone() for t in net.detect_video(frames, chunk=CHUNK, track=off, smooth={"max_gap": 3})]
    want_trk = [t.clone() for t in net.last_tracks]
    want_tbox = None if net.last_track_boxes is None else net.last_track_boxes.clone()
    want_pre, want_len = net.last_pre_smooth.clone(), net.last_smooth.clone()
    assert bool((want_len >= 2).any()) and not torch.equal(want[2], want_pre), "nothing is smoothed: the pass is not exercised"
    # the frames a session without the option has returned after every push
    late = {}
    for parts in PARTS:
        s, t, late[parts] = net.open_video(chunk=CHUNK, track=kw), 0, []
        for n in parts:
            s.push(frames[t:t + n])
            t += n
            late[parts].append(s.frames_out)
        s.flush()
        assert s.last_pre_smooth is None and s.last_smooth is None
    # a lag longer than the clip: detect_video(track=..., smooth=...)
    session = net.open_video(chunk=CHUNK, track=kw, smooth={"lag": 15, "max_gap": 3})
    for parts in PARTS:                                                    # one session, clip after clip
        got, _ = _session_clip(session, frames, parts, late[parts])
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), parts
        assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)), parts
        assert torch.equal(got[6], rows_plain) and torch.equal(got[7], over_plain)
        assert torch.equal(got[8].view(torch.int32), want_pre.view(torch.int32)) and torch.equal(got[9], want_len)
        tbox = got[10].cpu().numpy() if len(got) > 10 else None
        final = finalize_tracks(*[t.cpu().numpy() for t in got[3:6]], tbox=tbox, **session.track_decide)
        for f, w in zip(final, want_trk + ([want_tbox] if tbox is not None else [])):
            f = torch.from_numpy(f)
            assert f.dtype == w.dtype and torch.equal(f.view(torch.int32), w.cpu().view(torch.int32)), parts
        assert int(got[3][got[3] >= 0].min()) == 0                         # ids from 0 in every clip: flush() reset both states
    # lag 2: the definition on the session's own online rows, two frames late
    session = net.open_video(chunk=CHUNK, track=kw, smooth={"lag": 2})
    first = None
    for parts in PARTS:
        got, counts = _session_clip(session, frames, parts, late[parts])
        torch.cuda.synchronize()
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
        assert torch.equal(got[8], plain[2].clamp(0, SO.SIZE))
        _, t0, sbox, slen = smooth_lag_host(None, got[0].cpu().numpy(), got[1].cpu().numpy(), got[8].cpu().numpy(),
                                            got[3].cpu().numpy(), SO.C, 2, 7, flush=True)
        assert _bits(got[2], sbox) and torch.equal(got[9].cpu(), torch.from_numpy(slen)), parts
        assert int(got[3][got[3] >= 0].min()) == 0
        if first is None:
            first = got
            assert not torch.equal(got[2], want[2]), "lag 2 is the full smoother on this clip: the lag is not exercised"
        else:                                                              # every cutting gives the same bits
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, first)), parts


# ------------------------------------------------------------------------------------------------ script
@pytest.mark.parametrize("method", ["iou", "sort"])
def test_detect_script_live_smooth_writes_what_the_stream_run_writes(tmp_path, method):
    import detect_yolo3 as D
    common = ["--random_init", "--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early",
              "--synthetic_samples", "5", "--synthetic_videos", "2", "--data_shape", "64", "--batch_size", "2", "--metrics", "voc,mot,hota",
              "--save_dir", str(tmp_path), "--stream", "--track", "--track_method", method, "--track_high", "0", "--track_min_len", "1",
              "--track_low", "0", "--track_smooth"]
    live = ["--live", "--live_push", "2", "--track_smooth_lag", "15"] + (["--track_online"] if method != "iou" else [])
    out_s = D.main(common + ["--save_prefix", "s"])
    out_l = D.main(common + ["--save_prefix", "l"] + live)
    s, l = tmp_path / "s", tmp_path / "l"
    made = sorted(os.listdir(s))
    assert made == sorted(os.listdir(l)) and {"pred", "pred_trk", "tracks.txt", "pred_smo", "pred_smo_trk", "tracks_smo.txt"} <= set(made)
    assert {"mot.txt", "hota.txt", "mot_smo.txt", "hota_smo.txt"} <= set(made), made
    for name in made:                                                      # everything the --stream run writes, byte for byte
        if os.path.isdir(s / name):
            assert sorted(os.listdir(s / name)) == sorted(os.listdir(l / name)) and len(os.listdir(s / name)) == 10
            for f in os.listdir(s / name):
                assert open(s / name / f, "rb").read() == open(l / name / f, "rb").read(), (name, f)
        else:
            assert open(s / name, "rb").read() == open(l / name, "rb").read(), name
    plain = [line for f in sorted(os.listdir(s / "pred")) for line in open(s / "pred" / f).read().splitlines()]
    smo = [line for f in sorted(os.listdir(s / "pred_smo")) for line in open(s / "pred_smo" / f).read().splitlines()]
    assert len(plain) > 10 and len(smo) == len(plain) and smo != plain, "no box is smoothed: the pass is not exercised"
    assert out_s[0] == out_l[0] and np.array_equal(np.asarray(out_s[1]), np.asarray(out_l[1]), equal_nan=True)
