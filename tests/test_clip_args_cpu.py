"""The helpers of viddet_amd/ops.py that state the clip-row argument contract ("The clip-row contract"), called
directly: no GPU.  CPU tensors stand in where a message does not depend on the device."""
import numpy as np
import pytest
import torch

from viddet_amd import ops

WHO = ("stage", "Other.push")


def _message(call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    return str(e.value)


def test_clip_offsets_taken():
    assert ops._clip_offsets("stage", None, 3, "cpu") == (None, 1)
    assert ops._clip_offsets("stage", None, 0, "cpu") == (None, 1)
    for given in ([0, 2, 3], (0, 2, 3), np.array([0, 2, 3]), np.array([0, 2, 3], dtype=np.int16),
                  torch.tensor([0, 2, 3], dtype=torch.int32), torch.tensor([0, 2, 3])):
        cs, V = ops._clip_offsets("stage", given, 3, "cpu")
        assert V == 2 and cs.dtype == torch.int32 and cs.device.type == "cpu" and cs.tolist() == [0, 2, 3]
    cs, V = ops._clip_offsets("stage", [0, 0, 3, 3], 3, "cpu")           # empty clips are clips
    assert V == 3 and cs.tolist() == [0, 0, 3, 3]
    assert ops._clip_offsets("stage", [0, 0], 0, "cpu")[1] == 1


@pytest.mark.parametrize("who", WHO)
@pytest.mark.parametrize("given,F", [([0], 3), ([1, 3], 3), ([0, 2], 3), ([0, 3, 2, 3], 3), ([0, 0], 1), ([], 0)],
                         ids=["short", "first", "last", "descending", "past_no_frames", "empty"])
def test_clip_offsets_refused(who, given, F):
    want = "%s: clip_start must be V+1 ascending offsets from 0 to F=%d, got %r" % (who, F, given)
    for form in (given, np.array(given, dtype=np.int64), torch.tensor(given, dtype=torch.int32)):
        assert _message(ops._clip_offsets, who, form, F, "cpu") == want


@pytest.mark.parametrize("who", WHO)
def test_row_tensors(who):
    good = torch.zeros(2, 3)
    sentence = who + ": rows must be a contiguous float32 device tensor of 6 elements, got %s"
    f32 = torch.float32
    assert _message(ops._row_tensors, who, [("rows", None, 6, f32)]) == sentence % "<class 'NoneType'> ()"
    assert _message(ops._row_tensors, who, [("rows", [0.0] * 6, 6, f32)]) == sentence % "<class 'list'> ()"
    assert _message(ops._row_tensors, who, [("rows", good.numpy(), 6, f32)]) == sentence % "float32 (2, 3)"
    assert _message(ops._row_tensors, who, [("rows", good.double(), 6, f32)]) == sentence % "torch.float64 (2, 3)"
    assert _message(ops._row_tensors, who, [("rows", good[:, :2].contiguous(), 6, f32)]) == sentence % "torch.float32 (2, 2)"
    assert _message(ops._row_tensors, who, [("rows", torch.zeros(3, 2).t(), 6, f32)]) == sentence % "torch.float32 (2, 3)"
    # a host tensor is no device tensor, whatever else it is
    assert _message(ops._row_tensors, who, [("rows", good, 6, f32)]) == sentence % "torch.float32 (2, 3)"
    # the first of the specs that fails is the one named
    assert _message(ops._row_tensors, who, [("track", good.int(), 6, torch.int32), ("rows", None, 6, f32)]) == \
        who + ": track must be a contiguous int32 device tensor of 6 elements, got torch.int32 (2, 3)"
    ops._row_tensors(who, [])


def test_row_specs():
    ids, scores, bboxes, track = (torch.zeros(2, 3, 1), torch.zeros(2, 3), torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32))
    specs = ops._row_specs(ids, scores, bboxes, 6)
    assert [(s[0], s[2], s[3]) for s in specs] == [("ids", 6, torch.float32), ("scores", 6, torch.float32), ("bboxes", 24, torch.float32)]
    assert specs[0][1] is ids and specs[1][1] is scores and specs[2][1] is bboxes
    with_track = ops._row_specs(ids, scores, bboxes, 6, track)
    assert with_track[:3] == specs and with_track[3] == ("track", track, 6, torch.int32)
    assert ops._row_specs(ids, scores, bboxes, 6, None)[3] == ("track", None, 6, torch.int32)   # a missing track is checked, not skipped


@pytest.mark.parametrize("who", WHO)
def test_workspace(who):
    ws = ops._workspace(who, None, 48, "cpu")
    assert ws.dtype == torch.uint8 and tuple(ws.shape) == (48,) and ws.device.type == "cpu"
    assert ops._workspace(who, None, 0, "cpu").numel() == 0
    assert ops._workspace(who, None, 0, "cpu", at_least=1).numel() == 1
    assert ops._workspace(who, None, 48, "cpu", at_least=1).numel() == 48
    plain = "%s: ws must be a contiguous uint8 device tensor of >= 48 bytes" % who
    for bad in (torch.empty(47, dtype=torch.uint8), torch.empty(48, dtype=torch.int8), torch.empty(96, dtype=torch.uint8)[::2],
                torch.empty(48, dtype=torch.uint8), 48, [0] * 48):
        assert _message(ops._workspace, who, bad, 48, "cpu") == plain
    assert _message(ops._workspace, who, torch.empty(47, dtype=torch.uint8), 48, "cpu", align=8) == \
        "%s: ws must be a contiguous, 8-byte aligned uint8 device tensor of >= 48 bytes" % who


@pytest.mark.parametrize("who", WHO)
def test_int_arg(who):
    assert ops._int_arg(who, "n", 1, 1, 128) == 1 and ops._int_arg(who, "n", 128, 1, 128) == 128
    got = ops._int_arg(who, "n", np.int64(7), 1, 128)
    assert got == 7 and type(got) is int
    assert ops._int_arg(who, "n", 2 ** 40, 1) == 2 ** 40
    for bad in (True, False, 1.0, "1", None, 0, -1, 129):
        assert _message(ops._int_arg, who, "n", bad, 1, 128) == "%s: n must be an integer in [1, 128], got %r" % (who, bad)
    for bad in (True, 2.5, 0):
        assert _message(ops._int_arg, who, "n", bad, 1) == "%s: n must be an integer >= 1, got %r" % (who, bad)


def test_rows_shape():
    assert ops._rows_shape("stage", "vd_stage", torch.zeros(2, 3, 4), 3) == (2, 3)
    assert ops._rows_shape("stage", "vd_stage", torch.zeros(0, 0, 4), 3) == (0, 0)
    for bad, got in ((torch.zeros(2, 12), "(2, 12)"), (torch.zeros(2, 4, 3), "(2, 4, 3)"), (None, "()"), ([[[0.0] * 4]], "()")):
        assert _message(ops._rows_shape, "stage", "vd_stage", bad, 3) == "stage: bboxes must be (F,N,4), got " + got
    assert _message(ops._rows_shape, "stage", "vd_stage", torch.zeros(2, 4, 4), 3) == \
        "stage: N=4 rows per frame, vd_stage takes at most 3"


def test_match_shape():
    gt, det = torch.zeros(2, 5, 4), torch.zeros(2, 3, 4)
    assert ops._match_shape("m", gt, det) == (2, 5, 3) and ops._match_shape("m", gt, det, 2) == (2, 5, 3)
    assert _message(ops._match_shape, "m", None, None) == "m: gt_boxes must be (F,G,4), got ()"
    assert _message(ops._match_shape, "m", gt, det.reshape(2, 12)) == "m: bboxes must be (F,N,4), got (2, 12)"
    assert _message(ops._match_shape, "m", gt, det[:1]) == "m: gt_boxes holds 2 frames, bboxes 1"
    assert _message(ops._match_shape, "m", gt, det, 1) == "m: gt_boxes holds F=2 frames, vd_m takes at most 1"
    wide = torch.zeros(2, 129, 4)
    assert _message(ops._match_shape, "m", wide, wide) == "m: gt_boxes holds G=129 label rows per frame, vd_m takes 1 to 128"
    assert _message(ops._match_shape, "m", gt, wide) == "m: bboxes holds N=129 prediction rows per frame, vd_m takes 1 to 128"
    assert _message(ops._match_shape, "m", gt[:, :0], det) == "m: gt_boxes holds G=0 label rows per frame, vd_m takes 1 to 128"


def test_stream_state_without_a_device():
    """the shared constructor and push checks of the live-state classes, on a state tensor that lives on the host"""
    st = ops.TrackState(V=1, N=3, device="cpu")
    assert tuple(st.state.shape) == (1, ops.L.TRACK_STATE_BYTES) and st.frames == 0 and not st.state.any()
    rows = (torch.zeros(2, 3, 1), torch.zeros(2, 3, 1), torch.zeros(2, 3, 4))
    assert _message(st.push, rows[0], rows[1], torch.zeros(2, 4, 4)) == "TrackState.push: bboxes must be (1,F,3,4) or (F,3,4), got (2, 4, 4)"
    assert _message(st.push, rows[0], rows[1], None) == "TrackState.push: bboxes must be (1,F,3,4) or (F,3,4), got ()"
    assert _message(st.push, *rows) == "TrackState.push: ids must be a contiguous float32 device tensor of 6 elements, got torch.float32 (2, 3, 1)"
    lag = ops.SmoothLagState(V=2, N=3, lag=0, device="cpu")
    assert _message(lag.push, rows[0], rows[1], rows[2], None) == "SmoothLagState.push: bboxes must be (2,F,3,4), got (2, 3, 4)"
    st.frames = 5
    st.state.fill_(1)
    st.reset()
    assert st.frames == 0 and not st.state.any()
