"""CPU: the definitions of appearance association (viddet_amd/appearance.py).  The descriptor `embed_host`
against a loop-form oracle in float32 scalars and on closed forms; `cos_q` against the exact integer form; the association
`app_sort_host` on closed forms with the ids written out by hand, with zero descriptors against sort_host, and against the
paper-form oracle (float64 filter, brute-force enumeration) on seeded clips that it decides with a margin; the refusals of the
option and of the script's flags by their messages."""
import math

import numpy as np
import pytest

from tests import appearance_cases as AC
from tests import sort_cases as SC
from tests.appearance_oracle import app_sort_oracle, cos_exact, embed_oracle
from viddet_amd import appearance as A
from viddet_amd.sort import sort_host

_F = np.float32


# ------------------------------------------------------------------ the descriptor
@pytest.mark.parametrize("S,Hf,Wf,C,stride,N,B", [(2, 5, 7, 8, 8, 13, 2), (1, 1, 1, 16, 32, 13, 1), (3, 1, 4, 8, 16, 13, 3),
                                                  (1, 3, 1, 32, 8, 13, 1)], ids=["5x7", "1x1", "1x4", "3x1"])
def test_the_descriptor_equals_the_loop_form(S, Hf, Wf, C, stride, N, B):
    f = AC.feature_map(S, Hf, Wf, C, seed=S + Hf + C)
    ids, bx = AC.boxes_for(Hf, Wf, stride, N, B, seed=3)
    mi = None if B <= S else [S - 1] * B
    got = A.embed_host(f, ids, bx, stride, map_index=mi)
    assert got.dtype == np.int8 and got.shape == (B, N, C)
    assert np.array_equal(got, embed_oracle(f, ids, bx, stride, map_index=mi))
    if Hf * Wf > 1:
        assert (np.abs(got.astype(int)).max(axis=2) == 127).sum() >= B * 8        # a row with a descriptor reaches 127


def test_the_descriptor_on_closed_forms():
    ids = np.zeros((1, 1))
    box = np.array([[[8.0, 8.0, 40.0, 24.0]]], np.float32)
    # a constant map: a = 0, no descriptor
    assert not A.embed_host(np.full((1, 4, 6, 8), 2.5, np.float32), ids, box, 8).any()
    # linear along the channels, the same in every cell: every sample is the cell's vector, p = c, m = 3.5, a = 3.5
    f = np.broadcast_to(np.arange(8, dtype=np.float32), (1, 4, 6, 8)).copy()
    hand = [int(np.rint(_F(_F(_F(c) - _F(3.5)) / _F(3.5)) * _F(127))) for c in range(8)]
    assert hand == [-127, -91, -54, -18, 18, 54, 91, 127]
    assert A.embed_host(f, ids, box, 8)[0, 0].tolist() == hand
    # a box wholly outside the map reads the clamped border cell: the corner's vector alone
    g = AC.feature_map(1, 4, 6, 8, seed=1)
    out = np.array([[[900.0, 700.0, 950.0, 800.0]]], np.float32)
    corner = g[0, 3, 5]
    d = corner - A.hsum(corner) / _F(8)
    assert A.embed_host(g, ids, out, 8)[0, 0].tolist() == np.rint(d / np.abs(d).max() * _F(127)).astype(int).tolist()
    # one cell: every sample is that cell
    one = g[:, 1:2, 2:3]
    d = one[0, 0, 0] - A.hsum(one[0, 0, 0]) / _F(8)
    assert A.embed_host(one, ids, box, 32)[0, 0].tolist() == np.rint(d / np.abs(d).max() * _F(127)).astype(int).tolist()
    # no descriptor: id -1, a NaN id, a NaN or infinite coordinate; a NaN of the map under the box
    for bad_id, bad_box in ((-1.0, box), (np.nan, box), (0.0, [[[np.nan, 8, 40, 24]]]), (0.0, [[[8, 8, np.inf, 24]]]),
                            (0.0, [[[8, -np.inf, 40, 24]]])):
        assert not A.embed_host(g, np.full((1, 1), bad_id), np.asarray(bad_box, np.float32), 8).any()
    h = g.copy()
    h[0, 1, 2, 5] = np.nan
    assert not A.embed_host(h, ids, box, 8).any() and A.embed_host(g, ids, box, 8).any()
    h[0, 1, 2, 5] = np.inf
    assert not A.embed_host(h, ids, box, 8).any()


def test_map_index_repeats_reorders_and_is_cut():
    f = AC.feature_map(3, 4, 6, 8, seed=2)
    ids, bx = AC.boxes_for(4, 6, 8, 5, 4, seed=4)
    got = A.embed_host(f, ids, bx, 8, map_index=[2, 0, 2, 1])
    for b, m in enumerate([2, 0, 2, 1]):
        assert np.array_equal(got[b], A.embed_host(f[m:m + 1], ids[b:b + 1], bx[b:b + 1], 8)[0])
    cut = A.embed_host(f, ids, bx, 8, map_index=[-5, 7, 3, 1])
    assert np.array_equal(cut, A.embed_host(f, ids, bx, 8, map_index=[0, 2, 2, 1]))
    assert np.array_equal(A.embed_host(f[:, :, :, :], ids[:3], bx[:3], 8), A.embed_host(f, ids[:3], bx[:3], 8, map_index=[0, 1, 2]))
    bf = f.astype(np.float32)
    assert np.array_equal(A.embed_host(bf.astype(np.float64), ids, bx, 8, map_index=[0, 1, 2, 0]),
                          A.embed_host(bf, ids, bx, 8, map_index=[0, 1, 2, 0]))
    for C, stride, text in ((12, 8, "power of two"), (4, 8, "power of two"), (2048, 8, "power of two"), (8, 4, "stride must be")):
        with pytest.raises(ValueError, match=text):
            A.embed_host(np.zeros((1, 2, 2, C), np.float32), np.zeros((1, 1)), np.zeros((1, 1, 4), np.float32), stride)


# ------------------------------------------------------------------ the cosine
@pytest.mark.parametrize("C", [8, 256, 1024])
def test_cos_q_equals_the_exact_integer_form(C):
    rng = np.random.RandomState(C)
    pairs = 0
    for spread in (3, 40, 127, 300):
        for _ in range(60):
            e = rng.randint(-127, 128, C)
            g = np.clip(e + rng.randint(-spread, spread + 1, C), -127, 127)
            assert A.cos_q(e.astype(np.int8), g.astype(np.int8)) == cos_exact(e, g)
            pairs += 1
    e = rng.randint(-127, 128, (40, C)).astype(np.int8)
    m, has = A.cos_q_matrix(e[:25], e[20:])
    assert has.all() and m.tolist() == [[cos_exact(a, b) for b in e[20:]] for a in e[:25]]
    assert all(A.cos_q(v, v) == 1 << 20 for v in e) and A.cos_q(e[0], -e[0].astype(np.int64)) == 0
    z = np.zeros(C, np.int8)
    assert A.cos_q(z, e[0]) == 0 and A.cos_q(e[0], z) == 0 and not A.cos_q_matrix(z[None], e[:1])[1].any()
    assert A.cos_q(np.full(C, 127, np.int8), np.full(C, 127, np.int8)) == 1 << 20    # the largest norms


# ------------------------------------------------------------------ the association, closed forms
def _tracks(case, emb, **kw):
    kw.setdefault("num_class", 1)
    return A.app_sort_host(*case, emb, **kw)[0].tolist()


def test_swap_and_turn_geometry_alone_and_with_descriptors():
    assert A.cos_q(AC.E_A, AC.E_B) == 0
    swap, turn = AC.swap_clip(), AC.turn_clip()
    assert sort_host(*swap, num_class=1)[0].tolist() == AC.SWAPPED
    assert sort_host(*turn, num_class=1)[0].tolist() == AC.FRAGMENTED
    emb = AC.two_descriptors(10)
    assert _tracks(swap, emb) == AC.KEPT
    assert _tracks(turn, emb) == AC.KEPT
    got = A.app_sort_host(*turn, emb, num_class=1)
    assert (got[1] == 10).all() and (got[2] == _F(0.9)).all()
    for case in (swap, turn):                                              # zero descriptors: sort_host, bit for bit
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in
                   zip(A.app_sort_host(*case, np.zeros_like(emb), num_class=1), sort_host(*case, num_class=1)))


def test_the_threshold_is_met_exactly_and_missed_by_one_quantum():
    """From the turn on, row 0 shows E_A2: its cosine with the track's E_A is c.  sigma_app = c / 2**20 (exact in float32)
    admits the pair; (c + 1) / 2**20 does not, and row 0 starts track 2 while row 1, whose descriptor never changes, is kept."""
    c = A.cos_q(AC.E_A, AC.E_A2)
    assert 0 < c < (1 << 20) and c == cos_exact(AC.E_A, AC.E_A2)
    emb = AC.two_descriptors(10)
    emb[5:, 0] = AC.E_A2
    at, above = _F(c) / _F(1 << 20), _F(c + 1) / _F(1 << 20)
    assert A.app_threshold(at) == c and A.app_threshold(above) == c + 1
    assert _tracks(AC.turn_clip(), emb, sigma_app=at) == AC.KEPT
    assert _tracks(AC.turn_clip(), emb, sigma_app=above) == [[0, 1]] * 5 + [[2, 1]] * 5


def test_no_rescue_without_proximity_or_across_classes():
    emb = AC.two_descriptors(10)
    far = AC.far_turn_clip()
    assert _tracks(far, emb) == AC.FRAGMENTED == sort_host(*far, num_class=1)[0].tolist()
    assert _tracks(AC.turn_clip(), emb, sigma_prox=0.26) == AC.FRAGMENTED      # 16/64 = 0.25 is the turned box's IoU
    assert _tracks(AC.turn_clip(), emb, sigma_prox=0.25)[:6] == AC.KEPT[:6]     # the plain >=: the turn frame itself is rescued
    # the same boxes and descriptors, but both rows change their class at the turn: never admitted
    ids, sc, bx = AC.turn_clip()
    ids[5:] = 1.0
    assert _tracks((ids, sc, bx), emb, num_class=2) == AC.FRAGMENTED
    # a box that stands still and changes its class: geometry and appearance agree, the class decides
    still = SC.rows([[([0, 0, 10, 10], .9, 0)], [([0, 0, 10, 10], .9, 0)], [([0, 0, 10, 10], .9, 1)], [([0, 0, 10, 10], .9, 1)]])
    one = np.tile(AC.E_A, (4, 1, 1))
    assert _tracks(still, one, num_class=2) == [[0], [0], [1], [1]]


def test_a_row_without_a_descriptor_keeps_the_tracks_previous_one():
    emb = AC.two_descriptors(10)
    emb[3:5] = 0                                                           # the two frames ahead of the turn show none
    assert _tracks(AC.turn_clip(), emb) == AC.KEPT                         # the tracks still hold frame 2's
    emb[:5] = 0                                                            # no frame ahead of the turn shows one
    assert _tracks(AC.turn_clip(), emb) == AC.FRAGMENTED                   # a track without a descriptor: adm alone
    emb = AC.two_descriptors(10)
    emb[5] = 0                                                             # the turned rows show none: adm alone, in that frame
    assert _tracks(AC.turn_clip(), emb) == AC.FRAGMENTED


def test_two_clips_through_clip_start():
    swap, turn = AC.swap_clip(), AC.turn_clip()
    case = [np.concatenate([a, b]) for a, b in zip(swap, turn)]
    emb = AC.two_descriptors(20)
    got = A.app_sort_host(*case, emb, clip_start=[0, 10, 20], num_class=1)
    assert got[0].tolist() == AC.KEPT + AC.KEPT
    for part, rows in ((swap, slice(0, 10)), (turn, slice(10, 20))):
        alone = A.app_sort_host(*part, emb[rows], num_class=1)
        assert all(np.array_equal(a[rows], b, equal_nan=True) for a, b in zip(got, alone))
    one = A.app_sort_host(*case, emb, num_class=1)                         # one clip of 20 frames is another thing
    assert one[0].tolist() != got[0].tolist() or (one[1] != got[1]).any()


@pytest.mark.parametrize("name,case,kw,track,tlen", SC.closed_form(), ids=[c[0] for c in SC.closed_form()])
def test_zero_descriptors_give_sort_host_on_its_own_cases(name, case, kw, track, tlen):
    kw = dict(kw)
    kw.setdefault("num_class", 1)
    emb = np.zeros(case[2].shape[:2] + (8,), np.int8)
    want = sort_host(*case, **kw)
    assert want[0].tolist() == np.asarray(track).tolist()
    got = A.app_sort_host(*case, emb, **kw)
    assert all(a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want))
    stats, ref = {}, {}
    A.app_sort_host(*case, emb, stats=stats, **kw), sort_host(*case, stats=ref, **kw)
    assert stats["tracks"] == ref["tracks"] and np.array_equal(stats["active"], ref["active"])


def test_parameter_checks_name_the_argument():
    case, emb = AC.turn_clip(), AC.two_descriptors(10)
    for kw, text in ((dict(sigma_app=1.5), "app_sort_host: sigma_app must be a number in"), (dict(sigma_app=-0.1), "sigma_app"),
                     (dict(sigma_prox=float("nan")), "app_sort_host: sigma_prox must be a number in"), (dict(sigma_prox="x"), "sigma_prox must be a number"),
                     (dict(sigma_app=True), "sigma_app"), (dict(max_age=9), "app_sort_host: max_age"), (dict(t_min=0), "app_sort_host: t_min")):
        with pytest.raises(ValueError, match=text):
            A.app_sort_host(*case, emb, **kw)
    with pytest.raises(ValueError, match="emb must be"):
        A.app_sort_host(*case, emb[:9])
    with pytest.raises(ValueError, match="emb must be"):
        A.app_sort_host(*case, emb.astype(np.int32))
    A.app_sort_host(*case, emb, sigma_prox=0.9, sigma_iou=0.3)              # sigma_prox <= sigma_iou is not required


# ------------------------------------------------------------------ the association against the paper-form oracle
# the seeds are chosen so that the margins asserted below hold (tests/test_sort_cpu.py does the same)
ORACLE_CASES = [("plain%d" % s, dict(), dict()) for s in (2, 11, 13, 17)] + \
               [("turn%d" % s, dict(turn=5, miss=0.0), dict()) for s in (6, 16, 27, 29)] + \
               [("aged%d" % s, dict(turn=5), dict(max_age=3, sigma_prox=0.05)) for s in (2, 4, 23, 37)]


@pytest.mark.parametrize("name,gen,kw", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_the_definition_equals_the_paper_form(name, gen, kw):
    seed = int("".join(ch for ch in name if ch.isdigit()))
    case = AC.walkers_app(seed, **gen)
    assert case[2].shape[1] <= 6
    margins = {}
    track, tlen = app_sort_oracle(*case, margins=margins, **kw)
    assert margins["iou"] >= 0.01, "an admissibility decision within 0.01 of sigma_iou or sigma_prox"
    assert margins["assign"] >= 2 ** 10, "the best matching beats the runner-up by less than 2**10 quanta"
    got = A.app_sort_host(*case, **kw)
    assert np.array_equal(got[0], track) and np.array_equal(got[1], tlen)
    assert (track >= 0).sum() >= 30


def test_the_oracle_cases_hold_pairs_that_geometry_refuses():
    rescued = 0
    for name, gen, kw in ORACLE_CASES:
        margins = {}
        app_sort_oracle(*AC.walkers_app(int("".join(ch for ch in name if ch.isdigit())), **gen), margins=margins, **kw)
        rescued += margins["rescued"]
    assert rescued >= 5


# ------------------------------------------------------------------ the plumbing: the option, the ABI, the script's flags
def test_parse_option_fills_the_defaults_and_refuses_by_name():
    P = A.parse_option
    assert P(None, "sort", False, "detect_video") is None and P(False, "iou", True, "detect_video") is None
    assert P(True, "sort", False, "detect_video") == dict(level=8, sigma_app=0.8, sigma_prox=0.1, keep_maps=False)
    assert P(dict(level=32, sigma_app=0.5), "sort", False, "detect_video") == dict(level=32, sigma_app=0.5, sigma_prox=0.1, keep_maps=False)
    for method in ("iou", "byte"):
        with pytest.raises(ValueError, match="detect_video: appearance needs track method 'sort', got '%s'" % method):
            P(True, method, False, "detect_video")
    with pytest.raises(ValueError, match="detect_video: appearance beside seq_nms is not taken"):
        P(True, "sort", True, "detect_video")
    with pytest.raises(ValueError, match="detect_video: appearance level must be 8, 16 or 32, got 4"):
        P(dict(level=4), "sort", False, "detect_video")
    with pytest.raises(ValueError, match="detect_video: appearance takes level, sigma_app, sigma_prox and keep_maps, got gallery"):
        P(dict(gallery=3), "sort", False, "detect_video")
    with pytest.raises(ValueError, match="detect_video with appearance: sigma_app must be a number in"):
        P(dict(sigma_app=2), "sort", False, "detect_video")
    with pytest.raises(ValueError, match="detect_video with appearance: sigma_prox must be a number in"):
        P(dict(sigma_prox=-1), "sort", False, "detect_video")
    assert A.split_appearance(None) == (None, None) and A.split_appearance(True) == (True, None)
    assert A.split_appearance(dict(method="sort", appearance=True, max_age=2)) == (dict(method="sort", max_age=2), True)


def test_detect_video_and_open_video_refuse_before_any_gpu_work():
    """on a stand-in for the net that holds only what the refusals read: nothing below reaches a device"""
    import types
    from viddet_amd import live

    def stub(**kw):
        return types.SimpleNamespace(**dict(dict(_stream_refusal=lambda: None, _live=None, post_nms=100, _k=1, _k_join_pos=None), **kw))

    x = np.zeros((2, 3, 64, 64), np.float32)
    with pytest.raises(ValueError, match="detect_video: appearance needs track method 'sort', got 'iou'"):
        live.detect_video(stub(), x, track=dict(appearance=True))
    with pytest.raises(ValueError, match="detect_video: appearance needs track method 'sort', got 'byte'"):
        live.detect_video(stub(), x, track=dict(method="byte", appearance=True))
    with pytest.raises(ValueError, match="detect_video: appearance beside seq_nms"):
        live.detect_video(stub(), x, track=dict(method="sort", appearance=True), seq_nms=True)
    with pytest.raises(ValueError, match="appearance level must be"):
        live.detect_video(stub(), x, track=dict(method="sort", appearance=dict(level=64)))
    with pytest.raises(NotImplementedError, match="detect_video with track's appearance and k_join_pos 'late'"):
        live.detect_video(stub(_k=3, _k_join_pos="late"), x, track=dict(method="sort", appearance=True))
    with pytest.raises(NotImplementedError, match="detect_video with rnn_pos"):      # everything _stream_refusal refuses, first
        live.detect_video(stub(_stream_refusal=lambda: "rnn_pos 'late': ..."), x, track=dict(method="sort", appearance=True))
    with pytest.raises(NotImplementedError, match="open_video with track's appearance"):
        live.VideoSession(stub(), track=dict(method="sort", online=True, appearance=True))
    with pytest.raises(ValueError, match="detect_video: track takes"):     # a call that does not ask is parsed as ever
        live.detect_video(stub(), x, track=dict(method="sort", appearence=True))


def test_library_exports_the_entry_points_and_checks_arguments_before_any_launch():
    import os
    import re
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # entry points were added, nothing changed
    assert len(L.SIGNATURES["vd_roi_embed"][1]) == 15 and len(L.SIGNATURES["vd_track_sort_app"][1]) == 24
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "viddet_hip.h")).read()
    assert "int vd_roi_embed(" in hdr and "int vd_track_sort_app(" in hdr and "int64_t vd_track_sort_app_ws_bytes(int V, int F, int N);" in hdr
    mk = open(os.path.join(root, "viddet_amd", "csrc", "Makefile")).read()
    assert "vd_appearance.hip" in mk and "vd_track_sort_app.hip" in mk
    per_clip = int(re.search(r"#define VD_TRACK_SORT_APP_WS_PER_CLIP\s+(\d+)", hdr).group(1))
    assert per_clip == L.TRACK_SORT_APP_WS_PER_CLIP == L.TRACK_SORT_WS_PER_CLIP + 128 * 1024 * 4
    assert lib.vd_track_sort_app_ws_bytes(3, 10, 24) == 8 * 240 + 3 * per_clip
    for V, F, N in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 129)):
        assert lib.vd_track_sort_app_ws_bytes(V, F, N) == -1
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    good = dict(fmap=P, is_bf16=0, S=1, Hf=2, Wf=2, C=16, ld=16, ids=P, bboxes=P, map_index=None, B=1, N=4, stride=8, emb=P)

    def embed(**kw):
        a = dict(good, **kw)
        return lib.vd_roi_embed(*[a[k] for k in good], None), lib.vd_last_error()

    for kw in (dict(fmap=None), dict(ids=None), dict(bboxes=None), dict(emb=None), dict(C=12, ld=12), dict(C=4, ld=4), dict(C=2048, ld=2048),
               dict(ld=8), dict(ld=18), dict(N=129), dict(N=0), dict(B=0), dict(stride=4), dict(stride=0), dict(S=0), dict(Wf=0),
               dict(is_bf16=3), dict(fmap=P + 4), dict(fmap=P + 4, is_bf16=1), dict(bboxes=P + 8), dict(emb=P + 2), dict(ids=P + 1),
               dict(map_index=P + 2)):
        rc, err = embed(**kw)
        assert rc == -1 and err.startswith(b"vd_roi_embed:"), (kw, err)
    link = dict(ids=P, scores=P, bboxes=P, emb=P, C=256, clip_start=P, V=2, F=6, N=20, num_class=3, sigma_l=0.0, sigma_h=0.5,
                sigma_iou=0.3, t_min=2, max_age=1, sigma_app=0.8, sigma_prox=0.1, out_track=P, out_len=P, out_score=P, out_tbox=P, ws=P,
                ws_bytes=8 * 120 + 2 * per_clip)

    def sort_app(**kw):
        a = dict(link, **kw)
        return lib.vd_track_sort_app(*[a[k] for k in link], None), lib.vd_last_error()

    for kw in (dict(ids=None), dict(emb=None), dict(emb=P + 2), dict(C=12), dict(C=4), dict(C=2048), dict(N=129), dict(F=0), dict(V=0),
               dict(clip_start=None), dict(num_class=0), dict(t_min=0), dict(max_age=8), dict(sigma_iou=float("nan")), dict(sigma_app=1.5),
               dict(sigma_app=float("nan")), dict(sigma_prox=-0.1), dict(ws=None), dict(ws_bytes=8 * 120 + 2 * per_clip - 1),
               dict(ws_bytes=8 * 120 + 2 * L.TRACK_SORT_WS_PER_CLIP), dict(bboxes=P + 4), dict(out_tbox=P + 8), dict(out_track=P + 2)):
        rc, err = sort_app(**kw)
        assert rc == -1 and err.startswith(b"vd_track_sort_app:"), (kw, err)


APP = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--stream", "--track", "--track_method", "sort", "--track_app"]


def test_detect_script_refuses_track_app_by_name_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    flags = D.parse_flags([])
    assert flags.track_app is False and flags.track_app_cos is None and flags.track_app_prox is None and flags.track_app_level is None
    assert D.app_args(flags) is None and "appearance" not in D.track_args(D.parse_flags(["--track", "--track_method", "sort"]))
    assert D.app_args(D.parse_flags(["--track_app"])) == dict(sigma_app=0.8, sigma_prox=0.1, level=8)
    given = D.parse_flags(["--track", "--track_method", "sort", "--track_app", "--track_app_cos", "0.6", "--track_app_prox", "0.2",
                           "--track_app_level", "16"])
    assert D.track_args(given)["appearance"] == dict(sigma_app=0.6, sigma_prox=0.2, level=16) and D.track_args(given)["method"] == "sort"
    base = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--stream"]
    with pytest.raises(NotImplementedError, match="--track_app needs --track --track_method sort"):
        D.main(base + ["--track_app"])
    with pytest.raises(NotImplementedError, match="--track_app needs --track --track_method sort"):
        D.main(base + ["--track", "--track_app"])
    with pytest.raises(NotImplementedError, match="--track_app needs --track --track_method sort"):
        D.main(base + ["--track", "--track_method", "byte", "--track_app"])
    with pytest.raises(NotImplementedError, match="--track_app needs --stream"):
        D.main([a for a in APP if a != "--stream"] + ["--synthetic_videos", "2"])
    with pytest.raises(NotImplementedError, match="--track_app does not combine with --live"):
        D.main(APP + ["--live", "--track_online"])
    with pytest.raises(NotImplementedError, match="--track_app does not combine with --seq_nms"):
        D.main(APP + ["--seq_nms"])
    with pytest.raises(NotImplementedError, match="--track_app does not combine with --k_join_pos late"):
        D.main(APP + ["--window", "3,1", "--k_join_type", "max", "--k_join_pos", "late"])
    with pytest.raises(NotImplementedError, match="--track_app_level must be 8, 16 or 32, got 4"):
        D.main(APP + ["--track_app_level", "4"])
    for v in ("1.5", "-0.1", "nan"):
        with pytest.raises(NotImplementedError, match="--track_app_cos must be a number in \\[0, 1\\]"):
            D.main(APP + ["--track_app_cos", v])
        with pytest.raises(NotImplementedError, match="--track_app_prox must be a number in \\[0, 1\\]"):
            D.main(APP + ["--track_app_prox", v])
    for sub in (["--track_app_cos", "0.8"], ["--track_app_prox", "0.1"], ["--track_app_level", "8"]):
        with pytest.raises(NotImplementedError, match="%s needs --track_app" % sub[0]):
            D.main(APP[:-1] + sub)
    for more in ([], ["--window", "3,1", "--k_join_type", "max", "--k_join_pos", "early"], ["--tubelet"], ["--track_smooth"],
                 ["--track_stitch"], ["--track_app_cos", "1", "--track_app_prox", "0", "--track_app_level", "32"]):
        with pytest.raises(SystemExit, match="needs an MI355X"):           # and what is not refused gets as far as the GPU check
            D.main(APP + more)
