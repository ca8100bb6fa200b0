"""CPU: the host side of streaming video detection - the window rule, the clip dataset, the library surface
and argument checks of the ring joins (vd_stream.hip), the slot-table validation, and every refusal, all before any GPU work."""
import numpy as np
import pytest

from tests import stream_oracle as SO
from viddet_amd.stream import stream_window_slots, ring_size, chunk_slots

CLASSES = ["a", "b"]
NEW = ("vd_temporal_pool_idx", "vd_temporal_pool_idx_bf16", "vd_temporal_cat_idx")


@pytest.mark.parametrize("case", sorted(SO.WINDOWS))
def test_window_rule_against_the_hand_written_table(case):
    got = stream_window_slots(*case)
    assert got.dtype == np.int64 and got.tolist() == SO.WINDOWS[case]


@pytest.mark.parametrize("T,K,step", [(1, 1, 1), (9, 3, 1), (9, 3, 4), (4, 5, 2), (11, 6, 3), (3, 7, 1), (20, 2, 5)])
def test_window_rule_properties(T, K, step):
    w = stream_window_slots(T, K, step)
    assert w.shape == (T, K)
    assert np.array_equal(w[:, K // 2], np.arange(T))                     # the frame itself sits at column K // 2
    assert w.min() >= 0 and w.max() < T
    assert np.all(np.diff(w, axis=1) >= 0)                                # rows never go back in time
    inside = (np.arange(T) - (K // 2) * step >= 0) & (np.arange(T) + (K // 2) * step < T)
    if K > 1 and inside.any():                                            # away from the ends: exactly `step` apart
        assert np.all(np.diff(w[inside], axis=1) == step)
    with pytest.raises(ValueError):
        stream_window_slots(0, K, step)


def test_chunk_slot_tables_are_validated_before_upload():
    w = stream_window_slots(7, 3, 1)
    S = ring_size(3, 1, 3)
    assert S == 5 and ring_size(5, 2, 8) == 16 and ring_size(1, 1, 4) == 4 and ring_size(4, 1, 3) == 7
    tab = chunk_slots(w, 3, 3, 3, S, 2, 7)                                # frames 3..5 read frames 2..6: slots wrap
    assert tab.dtype == np.int32 and tab.tolist() == [[2, 3, 4], [3, 4, 0], [4, 0, 1]]
    tab = chunk_slots(w, 6, 1, 3, S, 2, 7)                                # the short last chunk: padded rows repeat the real one
    assert tab.tolist() == [[0, 1, 1]] * 3
    with pytest.raises(ValueError, match="the ring of 5 slots holds"):
        chunk_slots(w, 3, 3, 3, S, 3, 7)                                  # frame 2 has left the ring
    with pytest.raises(ValueError, match="the ring of 5 slots holds"):
        chunk_slots(w, 3, 3, 3, S, 2, 6)                                  # frame 6 has not been through the prefix yet
    with pytest.raises(ValueError, match="the ring of 5 slots holds"):
        chunk_slots(w, 3, 3, 3, S, 0, 7)                                  # more frames than slots: two would share one
    with pytest.raises(ValueError):
        chunk_slots(w, 6, 2, 3, S, 2, 7)                                  # beyond the clip
    with pytest.raises(ValueError):
        chunk_slots(w, 0, 4, 3, S, 0, 5)                                  # more rows than the table has


def test_synthetic_video_windows_stay_inside_their_clip():
    from viddet_amd.data import SyntheticVideo
    ds = SyntheticVideo("vid", num_videos=3, frames_per_video=5, window=3, step=2, size=(48, 40))
    assert len(ds) == 15 and ds.num_class == 30
    clips = [ds.video_frames(v) for v in range(3)]
    assert clips[0].shape == (5, 40, 48, 3) and clips[0].dtype == np.uint8
    flat = np.concatenate(clips).reshape(15, -1)
    assert len({f.tobytes() for f in flat}) == 15, "frames must be distinct"
    assert np.array_equal(ds.video_frames(1), clips[1]), "deterministic"
    slots = stream_window_slots(5, 3, 2)
    paths = set()
    for v in range(3):
        for t in range(5):
            idx = ds.sample_index(v, t)
            assert idx == v * 5 + t
            img, label = ds[idx]
            assert np.array_equal(img, clips[v][slots[t]])                # the window by the rule, from clip v alone
            assert np.array_equal(label, ds[idx][1]) and label.shape[1] == 6
            paths.add(ds.sample_path(idx))
    assert len(paths) == 15
    one = SyntheticVideo("vid", num_videos=3, frames_per_video=5, window=1, size=(48, 40))
    assert np.array_equal(one[7][0], clips[1][2]) and np.array_equal(one[7][1], ds[7][1])     # the centre frame's label
    with pytest.raises(IndexError):
        ds.sample_index(3, 0)
    with pytest.raises(IndexError):
        ds.video_frames(3)


def test_library_exports_the_ring_joins():
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION                      # entry points were only added
    for name in NEW:
        assert name in L.SIGNATURES and callable(getattr(lib, name))
    assert L.SIGNATURES["vd_temporal_pool_idx"] == L.SIGNATURES["vd_temporal_pool_idx_bf16"] == L.SIGNATURES["vd_temporal_cat_idx"]
    assert len(L.SIGNATURES["vd_temporal_pool_idx"][1]) == 9


def test_ring_joins_check_their_arguments_before_any_launch():
    from viddet_amd import lib as L
    lib = L.load()
    P = 4096                                                               # a 16-byte aligned, never dereferenced address
    good = dict(ring=P, slots=P, y=P, S=7, B=3, K=3, n=8, last=0)

    def call(name, **kw):
        a = dict(good, **kw)
        rc = getattr(lib, name)(a['ring'], a['slots'], a['y'], a['S'], a['B'], a['K'], a['n'], a['last'], None)
        return rc, lib.vd_last_error()

    for name in NEW:
        cat = name == "vd_temporal_cat_idx"
        bad = [dict(ring=None), dict(slots=None), dict(y=None), dict(K=0), dict(K=128), dict(K=-1), dict(S=0), dict(B=0),
               dict(ring=P + 4), dict(y=P + 8), dict(slots=P + 2), dict(n=0)]
        if cat:
            bad += [dict(last=6), dict(last=0), dict(last=-4)]             # (hw = n, C = last) C % 4, C > 0
        else:
            bad += [dict(n=12 if name.endswith("bf16") else 6), dict(last=2), dict(last=-1)]      # inner % 8 / % 4, type
        for kw in bad:
            if cat and 'last' not in kw:
                kw = dict(kw, last=kw.get('last', 4))
            rc, err = call(name, **kw)
            assert rc == -1, (name, kw)
            assert err.startswith(name.encode() + b":"), (name, kw, err)
    # fp32 takes inner % 4 that bf16 refuses
    assert call("vd_temporal_pool_idx_bf16", n=12)[0] == -1


REFUSED = [
    (dict(k=3, k_join_type="max", k_join_pos="late", block_conv_type="3"), "block_conv_type '3'"),
    (dict(k=3, k_join_type="mean", k_join_pos="late", block_conv_type="21"), "block_conv_type '21'"),
    (dict(k=3, corr_pos="early", corr_d=2), "corr_pos 'early'"),
    (dict(k=3, corr_pos="late", corr_d=2), "corr_pos 'late'"),
    (dict(k=3, k_join_type="max", k_join_pos="late", rnn_pos="late"), "rnn_pos 'late'"),
    (dict(k=3, k_join_type="max", k_join_pos="early", rnn_pos="out"), "rnn_pos 'out'"),
]


@pytest.mark.parametrize("kw,name", REFUSED, ids=[r[1] for r in REFUSED])
def test_detect_video_refuses_what_is_not_per_frame(kw, name):
    import torch
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(CLASSES, device="cpu", **kw)
    with pytest.raises(NotImplementedError, match="detect_video with " + name.replace("'", ".")):
        net.detect_video(torch.zeros(4, 3, 64, 64))


def test_detect_video_refuses_the_other_network_families():
    import torch
    from viddet_amd.model import YOLOV3, yolo3_3ddarknet, yolo3_no_backbone
    x = torch.zeros(5, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="detect_video with conv_types"):
        yolo3_3ddarknet(CLASSES, conv_types=[21, 2, 2, 2, 2, 2], k=3, device="cpu").detect_video(x)
    with pytest.raises(NotImplementedError, match="detect_video with noback"):
        yolo3_no_backbone(CLASSES, device="cpu").detect_video(x)
    with pytest.raises(NotImplementedError, match="detect_video with temporal / t_out"):
        YOLOV3(CLASSES, device="cpu", k=5, temporal_out=True).detect_video(x)
    with pytest.raises(NotImplementedError, match="detect_video with temporal / t_out"):
        YOLOV3(CLASSES, device="cpu", k=5, temporal_side=True).detect_video(x)


@pytest.mark.parametrize("jt,jp", [("max", "early"), ("mean", "late"), ("cat", "early"), ("cat", "late")])
def test_graph_split_is_per_frame_for_the_supported_joins(jt, jp):
    from viddet_amd.model import yolo3_darknet53, PoolNode, ConvNode
    net = yolo3_darknet53(CLASSES, device="cpu", k=3, k_join_type=jt, k_join_pos=jp)
    assert net._stream_refusal() is None
    prefix, suffix = net._stream_split()
    assert len(prefix) + len(suffix) == len(net.nodes)
    assert all(n.fr == 1 and getattr(n, 'kd', 1) == 1 for n in prefix) and not any(isinstance(n, PoolNode) for n in prefix)
    assert sum(isinstance(n, PoolNode) for n in suffix) == 3
    # early: the backbone alone; late (2-D blocks): the backbone and the neck - only the joins and the prediction convs are left
    nconv = sum(isinstance(n, ConvNode) for n in suffix)
    assert nconv == (3 if jp == "late" else 3 + 3 * 6 + 2)
    assert all(n.fr == 3 for n in net.nodes if any(n.name == m.name for m in prefix)), "the net's own nodes are untouched"
    # the graph itself says no where the flags would have: a neck conv across the frames of a window
    bad = yolo3_darknet53(CLASSES, device="cpu", k=3, k_join_type="max", k_join_pos="late", block_conv_type="3")
    with pytest.raises(AssertionError, match="upstream of a join is not per-frame"):
        bad._stream_split()


STREAM = ["--random_init", "--dataset", "vid", "--window", "3,1", "--stream", "--data_shape", "64"]


def test_detect_script_refuses_stream_combinations_before_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # a refusal must come before this is asked
    join = ["--k_join_type", "max", "--k_join_pos", "late"]
    for extra, msg in ((["--corr_pos", "late"], "--stream does not combine with --corr_pos"),
                       (join + ["--rnn_pos", "late"], "--stream does not combine with --rnn_pos"),
                       (join + ["--block_conv_type", "3"], "--stream does not combine with --block_conv_type"),
                       (["--conv_types", "21,2,2,2,2,2"], "--stream does not combine with --conv_types"),
                       ([], "needs --k_join_type"),
                       (["--k_join_type", "max"], "needs --k_join_type")):
        with pytest.raises(NotImplementedError, match=msg):
            D.main(STREAM + extra)
    with pytest.raises(NotImplementedError, match="--temp is outside"):
        D.main(STREAM + join + ["--temp"])


def test_detect_script_accepts_stream_up_to_the_gpu_check(monkeypatch):
    import torch
    import detect_yolo3 as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for extra in (["--k_join_type", "max", "--k_join_pos", "early"], ["--k_join_type", "cat", "--k_join_pos", "late", "--precision", "bf16"],
                  ["--k_join_type", "mean", "--k_join_pos", "late", "--model_agnostic", "--synthetic_videos", "3"]):
        with pytest.raises(SystemExit):
            D.main(STREAM + extra)
    with pytest.raises(SystemExit):
        D.main(["--random_init", "--dataset", "vid", "--stream"])          # --window 1: plain batched detection per clip
    F = D.parse_flags(["--stream"])
    assert F.stream is True and F.synthetic_videos is None and D.parse_flags([]).stream is False
