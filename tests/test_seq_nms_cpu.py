"""CPU: the definition of Seq-NMS (viddet_amd/seq_nms.py) against a literal loop form written from the paper
(tests/seqnms_oracle.py), its closed forms, the argument checks of vd_seq_nms and the refusals of detect_yolo3.py --seq_nms,
all before any GPU work."""
import numpy as np
import pytest

from tests import seqnms_cases as SC
from tests.seqnms_oracle import seq_nms_loops
from viddet_amd.seq_nms import seq_nms_host


def assert_equals_loops(case, **kw):
    stats = {}
    got = seq_nms_host(*case, stats=stats, **kw)
    ref = seq_nms_loops(*case, **kw)
    for name, g, r in zip(("ids", "scores", "bboxes", "perm"), got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, name
        assert np.array_equal(g, r), name
    assert stats["rounds"] == ref[4]
    return got, stats["rounds"]


@pytest.mark.parametrize("T", [1, 2, 7, 40])
@pytest.mark.parametrize("N", [1, 3, 20])
def test_host_equals_the_loop_form_on_random_clips(T, N):
    got, rounds = assert_equals_loops(SC.random_clip(T, N, seed=100 * T + N))
    assert rounds >= 1 or not (got[0] >= 0).any()
    if T == 40 and N == 20:                                                # ties everywhere, and still many rounds
        sc = SC.random_clip(T, N, seed=100 * T + N)[1]
        assert len(np.unique(sc[sc >= 0])) <= 12 and rounds > 10


@pytest.mark.parametrize("classes", [2, 3])
@pytest.mark.parametrize("rescore", ["avg", "max"])
def test_host_equals_the_loop_form_with_several_classes(classes, rescore):
    case = SC.random_clip(7, 20, classes=classes, seed=classes)
    got, _ = assert_equals_loops(case, rescore=rescore)
    # a class is untouched by the others: the same rows decided alone give the same new scores
    ids, scores, bboxes = case
    for c in range(classes):
        only = np.where(ids == c, ids, -1).astype(np.float32)
        alone = seq_nms_host(only, scores, bboxes, rescore=rescore)
        for t in range(7):
            mine = got[3][t][(got[0][t, :, 0] == c)]
            assert np.array_equal(mine, alone[3][t][alone[3][t] >= 0])
            assert np.array_equal(got[1][t, got[0][t, :, 0] == c, 0], alone[1][t, alone[3][t] >= 0, 0])


def test_host_equals_the_loop_form_with_empty_frames_and_a_gap():
    assert_equals_loops(SC.random_clip(9, 12, seed=3, empty=(0, 8)))
    case = SC.random_clip(9, 12, seed=4, gap=4, fill=1.0)
    got, _ = assert_equals_loops(case)
    whole, _ = assert_equals_loops(SC.random_clip(9, 12, seed=4, fill=1.0))
    assert (got[0][4] == -1).all() and (got[3][4] == -1).all()
    # the gap cuts every track: what lies ahead of it is decided as a clip of its own
    head = seq_nms_host(*[a[:4] for a in case])
    for a, b in zip(got, head):
        assert np.array_equal(a[:4], b)
    assert not np.array_equal(got[1][:4], whole[1][:4])


def test_clips_do_not_link_across_their_boundary():
    one = SC.random_clip(5, 6, seed=9, fill=1.0)
    both = [np.concatenate([a, a]) for a in one]                           # the same boxes on both sides of the boundary
    got, _ = assert_equals_loops(both, clip_start=[0, 5, 10])
    alone = seq_nms_host(*one)
    for a, b in zip(got, alone):
        assert np.array_equal(a[:5], b) and np.array_equal(a[5:], b)
    joined, _ = assert_equals_loops(both)
    assert not np.array_equal(joined[1], got[1])                           # without the boundary they do link
    three = [np.concatenate([a, a[:1], a[:3]]) for a in one]               # unequal lengths, a clip of one frame, an empty clip
    got3, _ = assert_equals_loops(three, clip_start=[0, 5, 6, 6, 9])
    assert np.array_equal(got3[1][5], seq_nms_host(*[a[:1] for a in one])[1][0])
    with pytest.raises(ValueError, match="clip_start"):
        seq_nms_host(*both, clip_start=[0, 5])
    with pytest.raises(ValueError, match="clip_start"):
        seq_nms_host(*both, clip_start=[0, 6, 5, 10])


def test_the_four_frame_case():
    case = SC.four_frames()
    (ids, scores, bboxes, perm), rounds = assert_equals_loops(case)
    assert rounds == 1
    assert perm.tolist() == [[0, -1, -1], [1, -1, -1], [0, -1, -1], [0, -1, -1]]
    assert np.abs(scores[:, 0, 0] - 0.725).max() < 1e-6 and (scores[:, 1:] == -1).all()
    assert (ids >= 0).sum() == 4                                           # four final rows; the .2 row is dead
    assert np.array_equal(bboxes[1, 0], case[2][1, 1]) and (bboxes[1, 1:] == -1).all()
    mx, _ = assert_equals_loops(case, rescore="max")
    assert np.array_equal(mx[1][:, 0, 0], np.full(4, 0.9, np.float32)) and np.array_equal(mx[3], perm)


def test_an_iou_of_exactly_one_half_is_not_above_one_half():
    from viddet_amd.seq_nms import iou_matrix
    case = SC.exact_half()
    assert iou_matrix(case[2][0, :1], case[2][0, 1:])[0, 0] == np.float32(0.5)
    (ids, scores, _, perm), rounds = assert_equals_loops(case, link_thresh=0.5, nms_thresh=0.5)
    # the tall boxes link (IoU 1): (.6 + .7) / 2; the square one neither links to the tall one nor is suppressed by it
    assert rounds == 2 and perm.tolist() == [[0, 1], [0, -1]]
    assert scores[:, :, 0].tolist() == [[np.float32(0.9), np.float32(np.float32(0.6) + np.float32(0.7)) / np.float32(2)],
                                        [np.float32(np.float32(0.6) + np.float32(0.7)) / np.float32(2), -1.0]]
    below = np.nextafter(np.float32(0.5), np.float32(0))
    (ids, scores, _, perm), rounds = assert_equals_loops(case, link_thresh=below, nms_thresh=below)
    # just below: the square box links to the tall one of frame 1 (.9 + .7), and the tall one of frame 0 dies
    assert rounds == 1 and perm.tolist() == [[0, -1], [0, -1]]
    assert scores[0, 0, 0] == (np.float32(0.9) + np.float32(0.7)) / np.float32(2)


def test_a_lone_box_keeps_its_score_and_agnostic_ids_merge_classes():
    ids = np.array([[[3.0], [-1.0]]], np.float32)
    scores = np.array([[[0.37], [0.9]]], np.float32)
    bboxes = np.array([[[1, 2, 30, 40], [0, 0, 5, 5]]], np.float32)
    got, rounds = assert_equals_loops((ids, scores, bboxes))
    assert rounds == 1 and got[1][0, :, 0].tolist() == [np.float32(0.37), -1.0] and got[0][0, 0, 0] == 3
    # two tracks of two classes on the same boxes: apart they are two sequences, with agnostic ids (all 0) one
    ids = np.array([[[0.0]], [[1.0]], [[0.0]], [[1.0]]], np.float32)
    scores = np.array([[[0.8]], [[0.4]], [[0.6]], [[0.2]]], np.float32)
    bboxes = np.tile(np.array([0, 0, 10, 10], np.float32), (4, 1, 1))
    apart, rounds = assert_equals_loops((ids, scores, bboxes))
    assert rounds == 4 and np.array_equal(apart[1], scores)                # frames of one class are never adjacent
    merged, rounds = assert_equals_loops((np.zeros_like(ids), scores, bboxes))
    assert rounds == 1 and np.all(merged[1] == (((np.float32(0.8) + np.float32(0.4)) + np.float32(0.6)) + np.float32(0.2)) / np.float32(4))


def test_a_nan_score_is_no_candidate_and_num_class_bounds_the_classes():
    ids, scores, bboxes = SC.random_clip(4, 8, classes=3, seed=2, fill=1.0)
    scores[1, 2, 0] = np.nan
    scores[2, 5, 0] = np.inf
    got, _ = assert_equals_loops((ids, scores, bboxes))                    # and the call ends
    assert 2 not in got[3][1] and 5 not in got[3][2] and np.isfinite(got[1]).all()
    assert (got[3][1] >= 0).sum() <= 7
    clean = np.where(np.isfinite(scores), ids, -1).astype(np.float32)
    for a, b in zip(got, seq_nms_host(clean, np.nan_to_num(scores, nan=0.0, posinf=0.0), bboxes)):
        assert np.array_equal(a, b)
    bounded = seq_nms_host(ids, scores, bboxes, num_class=2)
    for a, b in zip(bounded, seq_nms_host(np.where(ids >= 2, -1, ids).astype(np.float32), scores, bboxes)):
        assert np.array_equal(a, b)


def test_output_rows_are_sorted_stably_and_perm_is_the_gather():
    ids, scores, bboxes = SC.random_clip(7, 20, classes=2, seed=8)
    (oi, os_, ob, perm), _ = assert_equals_loops((ids, scores, bboxes), rescore="max")    # maxima come from the ladder: they tie
    assert oi.dtype == os_.dtype == ob.dtype == np.float32 and perm.dtype == np.int32 and perm.shape == (7, 20)
    ties = 0
    for t in range(7):
        n = int((perm[t] >= 0).sum())
        assert (perm[t, :n] >= 0).all() and (perm[t, n:] == -1).all() and len(set(perm[t, :n])) == n
        assert (oi[t, n:] == -1).all() and (os_[t, n:] == -1).all() and (ob[t, n:] == -1).all()
        assert np.array_equal(oi[t, :n], ids[t, perm[t, :n]]) and np.array_equal(ob[t, :n], bboxes[t, perm[t, :n]])
        s = os_[t, :n, 0]
        assert np.all(s[:-1] >= s[1:])
        same = s[:-1] == s[1:]
        assert np.all(perm[t, :n][:-1][same] < perm[t, :n][1:][same])      # stable: equal scores keep the row order
        ties += int(same.sum())
    assert ties > 0
    with pytest.raises(ValueError, match="rescore"):
        seq_nms_host(ids, scores, bboxes, rescore="mean")


def test_library_exports_seq_nms_and_checks_its_arguments_before_any_launch():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # an entry point was added, nothing changed
    assert "vd_seq_nms" in L.SIGNATURES and len(L.SIGNATURES["vd_seq_nms"][1]) == 18
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    good = dict(ids=P, scores=P, bboxes=P, clip_start=P, V=2, F=6, N=20, num_class=3, link=0.5, nms=0.3, rescore=0,
                out_ids=P, out_scores=P, out_bboxes=P, out_perm=P, ws=P, ws_bytes=48 * 6 * 20)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vd_seq_nms(a["ids"], a["scores"], a["bboxes"], a["clip_start"], a["V"], a["F"], a["N"], a["num_class"], a["link"],
                            a["nms"], a["rescore"], a["out_ids"], a["out_scores"], a["out_bboxes"], a["out_perm"], a["ws"],
                            a["ws_bytes"], None)
        return rc, lib.vd_last_error()

    bad = [dict(ids=None), dict(scores=None), dict(bboxes=None), dict(out_ids=None), dict(out_scores=None), dict(out_bboxes=None),
           dict(out_perm=None), dict(ws=None), dict(N=0), dict(N=129), dict(N=-1), dict(F=0), dict(V=0), dict(clip_start=None),
           dict(rescore=2), dict(rescore=-1), dict(num_class=0), dict(ws_bytes=48 * 6 * 20 - 1), dict(ws_bytes=0),
           dict(bboxes=P + 4), dict(out_bboxes=P + 8), dict(ws=P + 4), dict(ids=P + 2), dict(scores=P + 1), dict(clip_start=P + 2),
           dict(out_ids=P + 2), dict(out_scores=P + 3), dict(out_perm=P + 2)]
    for kw in bad:
        rc, err = call(**kw)
        assert rc == -1, kw
        assert err.startswith(b"vd_seq_nms:"), (kw, err)


SEQ = ["--random_init", "--dataset", "vid", "--data_shape", "64", "--seq_nms"]


def test_detect_script_refuses_seq_nms_without_clips_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    with pytest.raises(NotImplementedError, match="--seq_nms needs clips"):
        D.main(SEQ)
    with pytest.raises(NotImplementedError, match="--seq_nms needs clips"):
        D.main(SEQ + ["--metrics", "vid"])
    with pytest.raises(NotImplementedError, match="--seq_nms does not combine with several --dataset names"):
        D.main(["--random_init", "--dataset", "voc,coco", "--seq_nms", "--synthetic_videos", "2"])
    with pytest.raises(NotImplementedError, match="--seq_nms does not combine with --mult_out"):
        D.main(SEQ + ["--stream", "--mult_out"])
    with pytest.raises(NotImplementedError, match="--seq_nms_input_nms"):
        D.main(SEQ + ["--stream", "--seq_nms_input_nms", "1.5"])
    # with clips it gets as far as asking for the GPU
    for extra in (["--stream"], ["--synthetic_videos", "2"], ["--stream", "--model_agnostic", "--seq_nms_rescore", "max"]):
        with pytest.raises(SystemExit):
            D.main(SEQ + extra)
    F = D.parse_flags(["--seq_nms"])
    assert F.seq_nms is True and (F.seq_nms_link, F.seq_nms_thresh, F.seq_nms_rescore, F.seq_nms_input_nms) == (0.5, 0.3, "avg", 0.45)
    assert D.parse_flags([]).seq_nms is False and D.seq_nms_args(D.parse_flags([])) is None
    assert D.seq_nms_args(F) == dict(link_thresh=0.5, nms_thresh=0.3, rescore="avg")


def test_result_names_gain_a_suffix_only_when_asked():
    import os
    import detect_yolo3 as D
    assert D.result_name("vid") == "vid" and D.result_name("vid", seq=True) == "vid_seq"
    assert D.result_name("coco", True, True, seq=True) == "coco_ag_seq" and D.result_name("vid", False, True, True) == "vid_ag_met_seq"
    assert D.pred_dir("r", "p") == os.path.join("r", "p", "pred") and D.pred_dir("r", "p", seq=True) == os.path.join("r", "p", "pred_seq")
    assert D.pred_dir("r", "p", True, seq=True) == os.path.join("r", "p", "pred_ag_seq")
    assert D.clip_offsets([0, 1, 2, 4, 5, 8, 9], 4) == [0, 3, 5, 7] and D.clip_offsets([3], 4) == [0, 1]
    assert D.clip_offsets([2, 3, 4, 5], 4) == [0, 2, 4]


def test_detect_video_refuses_seq_nms_on_more_than_128_rows():
    import torch
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["a", "b"], device="cpu")
    net.set_nms(post_nms=129)
    with pytest.raises(ValueError, match="post_nms=129"):
        net.detect_video(torch.zeros(4, 3, 64, 64), seq_nms=True)
    net.set_nms(post_nms=100)
    with pytest.raises(ValueError, match="seq_nms takes link_thresh"):
        net.detect_video(torch.zeros(4, 3, 64, 64), seq_nms=dict(link=0.4))
