"""The clip-row argument contract at every binding that takes it ("The clip-row contract"): the nine clip bindings
and the three live-state classes raise one sentence per shared check, formatted here from the binding's name and compared
whole, and the order of the checks decides which of two faults is reported.  Host clip offsets and the same offsets as a
device tensor give identical results.

test_non_tensor_rows (seq_nms, track, track_sort, track_byte) and test_state_push_non_tensor (the three states) are the
cases that raised AttributeError before the checks were stated once - a non-tensor where the binding asked the object for
its dtype or shape; they raise the sibling bindings' sentence now.  Every other case passed unchanged on the commit before."""
import pytest
import torch

from viddet_amd import lib as L

pytestmark = pytest.mark.gpu

F, N, G = 2, 3, 2
f32, i32 = torch.float32, torch.int32

UNTRACKED = ("seq_nms", "track", "track_sort", "track_byte")
TRACKED = ("tubelet", "smooth", "stitch")
MATCHERS = ("mot_match", "hota_match")
CLIP = UNTRACKED + TRACKED + MATCHERS + ("overlay",)
TAKES_TRACK = TRACKED + MATCHERS + ("overlay",)
NUM_CLASS_GE_1 = TRACKED + ("mot_match",)
STATES = ("TrackState", "KalmanTrackState", "SmoothLagState")
VD = {"seq_nms": "vd_seq_nms", "track": "vd_track", "track_sort": "vd_track_sort", "track_byte": "vd_track_byte",
      "tubelet": "vd_tubelet", "smooth": "vd_track_smooth", "stitch": "vd_track_stitch", "overlay": "vd_overlay"}


def _ops():
    from viddet_amd import ops
    return ops


def _base(name):
    """the keyword arguments of a good call of ops.<name>"""
    dev = "cuda"
    kw = dict(ids=torch.tensor([[0, 1, 0], [0, 1, -1]], dtype=f32, device=dev).reshape(F, N, 1),
              scores=torch.tensor([[.9, .8, .7], [.85, .75, .6]], dtype=f32, device=dev).reshape(F, N, 1),
              bboxes=torch.tensor([[[1, 1, 4, 4], [3, 3, 7, 7], [0, 2, 3, 6]], [[1, 1, 4, 5], [3, 2, 7, 7], [2, 2, 5, 5]]],
                                  dtype=f32, device=dev))
    if name in TAKES_TRACK:
        kw["track"] = torch.tensor([[0, 1, 2], [0, 1, -1]], dtype=i32, device=dev)
    if name in MATCHERS:
        kw["gt_boxes"] = torch.tensor([[[1, 1, 4, 4], [3, 3, 6, 7]], [[1, 1, 4, 5], [3, 2, 7, 6]]], dtype=f32, device=dev)
        kw["gt_cls"] = torch.tensor([[0, 1], [0, 1]], dtype=i32, device=dev)
        kw["gt_id"] = torch.tensor([[0, 1], [0, 1]], dtype=i32, device=dev)
    if name == "hota_match":
        kw.update(num_gt_id=2, num_track=3)
    if name == "overlay":
        kw["frames"] = (torch.arange(F * 8 * 8 * 3, device=dev) % 251).to(torch.uint8).reshape(F, 8, 8, 3)
    return kw


def _need(name, V=1):
    """the workspace bytes of the good call"""
    if name == "hota_match":
        return _ops().hota_ws_bytes(V, 2, 3)
    return {"seq_nms": L.SEQ_NMS_WS_PER_ROW * F * N, "track": L.TRACK_WS_PER_ROW * F * N,
            "track_sort": L.TRACK_SORT_WS_PER_ROW * F * N + L.TRACK_SORT_WS_PER_CLIP * V,
            "track_byte": L.TRACK_SORT_WS_PER_ROW * F * N + L.TRACK_SORT_WS_PER_CLIP * V,
            "tubelet": L.TUBELET_WS_PER_ROW * F * N, "smooth": L.TRACK_SMOOTH_WS_PER_ROW * F * N,
            "stitch": L.TRACK_STITCH_WS_PER_ROW * F * N, "mot_match": L.MOT_WS_PER_ROW * F * (G + N),
            "overlay": L.OVERLAY_WS_PER_ROW * F * N}[name]


def _raises(name, message, **over):
    with pytest.raises(ValueError) as e:
        getattr(_ops(), name)(**dict(_base(name), **over))
    assert str(e.value) == message


def _ws_sentence(name, need):
    if name == "hota_match":
        return "hota_match: ws must be a contiguous, 8-byte aligned uint8 device tensor of >= %d bytes" % need
    return "%s: ws must be a contiguous uint8 device tensor of >= %d bytes" % (name, need)


def _rows_sentence(name, what, n, dtype, got):
    return "%s: %s must be a contiguous %s device tensor of %d elements, got %s" % (name, what, dtype, n, got)


BAD_OFFSETS = "%s: clip_start must be V+1 ascending offsets from 0 to F=2, got [0, 1, 3]"
BAD_DEVICE_OFFSETS = "%s: a device clip_start must be a contiguous int32 vector of V+1 offsets, got torch.int64 (3,)"


@pytest.mark.parametrize("name", CLIP)
def test_clip_start(name):
    dev_cs = torch.tensor([0, 1, 2], device="cuda")
    _raises(name, BAD_DEVICE_OFFSETS % name, clip_start=dev_cs)
    _raises(name, "%s: a device clip_start must be a contiguous int32 vector of V+1 offsets, got torch.int32 (1,)" % name,
            clip_start=dev_cs[:1].int())
    _raises(name, "%s: a device clip_start must be a contiguous int32 vector of V+1 offsets, got torch.int32 (2,)" % name,
            clip_start=torch.zeros(4, dtype=i32, device="cuda")[::2])
    _raises(name, BAD_OFFSETS % name, clip_start=[0, 1, 3])
    _raises(name, "%s: clip_start must be V+1 ascending offsets from 0 to F=2, got [0]" % name, clip_start=torch.tensor([0]))
    _raises(name, "%s: clip_start must be V+1 ascending offsets from 0 to F=2, got [1, 2]" % name, clip_start=(1, 2))
    _raises(name, "%s: clip_start must be V+1 ascending offsets from 0 to F=2, got [0, 2, 1, 2]" % name, clip_start=[0, 2, 1, 2])


@pytest.mark.parametrize("name", CLIP)
def test_workspace(name):
    need = _need(name)
    ws = torch.empty(need + 8, dtype=torch.uint8, device="cuda")
    _raises(name, _ws_sentence(name, need), ws=ws[:need - 1])
    _raises(name, _ws_sentence(name, need), ws=ws[:need].cpu())
    _raises(name, _ws_sentence(name, need), ws=torch.empty(need, dtype=torch.int8, device="cuda"))
    _raises(name, _ws_sentence(name, need), ws=torch.empty(2 * need, dtype=torch.uint8, device="cuda")[::2])
    # two clips: the bytes of a workspace that counts clips grow with V
    need2 = _need(name, V=2)
    _raises(name, _ws_sentence(name, need2), ws=torch.empty(need2 - 1, dtype=torch.uint8, device="cuda"), clip_start=[0, 1, 2])
    if name == "hota_match":
        _raises(name, _ws_sentence(name, need), ws=ws[4:need + 4])
    getattr(_ops(), name)(**dict(_base(name), ws=ws[:need]))


@pytest.mark.parametrize("name", CLIP)
def test_row_tensors(name):
    b = _base(name)
    _raises(name, _rows_sentence(name, "scores", F * N, "float32", "torch.float64 (2, 3, 1)"), scores=b["scores"].double())
    _raises(name, _rows_sentence(name, "ids", F * N, "float32", "torch.float32 (2, 3, 1)"), ids=b["ids"].cpu())
    _raises(name, _rows_sentence(name, "ids", F * N, "float32", "torch.float32 (2, 3)"), ids=b["ids"].reshape(N, F).t())
    _raises(name, _rows_sentence(name, "scores", F * N, "float32", "torch.float32 (2, 2, 1)"), scores=b["scores"][:, :2].contiguous())
    _raises(name, _rows_sentence(name, "bboxes", F * N * 4, "float32", "torch.float16 (2, 3, 4)"), bboxes=b["bboxes"].half())
    if name in TAKES_TRACK:
        _raises(name, _rows_sentence(name, "track", F * N, "int32", "torch.int64 (2, 3)"), track=b["track"].long())
        _raises(name, _rows_sentence(name, "track", F * N, "int32", "<class 'list'> ()"), track=[[0, 1, 2], [0, 1, -1]])
    if name in TRACKED:
        _raises(name, "%s: track must be (F,N) = (2,3), got (3, 2)" % name, track=b["track"].reshape(N, F))
    if name in MATCHERS:
        _raises(name, _rows_sentence(name, "gt_id", F * G, "int32", "torch.float32 (2, 2)"), gt_id=b["gt_id"].float())
        _raises(name, "%s: track must be (2, 3), got (3, 2)" % name, track=b["track"].reshape(N, F))


@pytest.mark.parametrize("name", TAKES_TRACK)
def test_non_tensor_rows_tracked(name):
    _raises(name, _rows_sentence(name, "ids", F * N, "float32", "<class 'NoneType'> ()"), ids=None)
    _raises(name, _rows_sentence(name, "scores", F * N, "float32", "<class 'list'> ()"), scores=[0.5] * (F * N))


@pytest.mark.parametrize("name", UNTRACKED)
def test_non_tensor_rows(name):
    _raises(name, _rows_sentence(name, "ids", F * N, "float32", "<class 'NoneType'> ()"), ids=None)
    _raises(name, _rows_sentence(name, "scores", F * N, "float32", "<class 'list'> ()"), scores=[0.5] * (F * N))


@pytest.mark.parametrize("name", CLIP)
def test_rows_shape(name):
    b = _base(name)
    _raises(name, "%s: bboxes must be (F,N,4), got (2, 12)" % name, bboxes=b["bboxes"].reshape(F, N * 4))
    _raises(name, "%s: bboxes must be (F,N,4), got (2, 4, 3)" % name, bboxes=b["bboxes"].reshape(F, 4, N))
    wide = torch.zeros(F, 129, 4, device="cuda")
    if name in MATCHERS:
        _raises(name, "%s: gt_boxes must be (F,G,4), got (2, 8)" % name, gt_boxes=b["gt_boxes"].reshape(F, G * 4))
        _raises(name, "%s: gt_boxes must be (F,G,4), got ()" % name, gt_boxes=None, bboxes=None)
        _raises(name, "%s: bboxes holds N=129 prediction rows per frame, vd_%s takes 1 to 128" % (name, name), bboxes=wide)
        _raises(name, "%s: gt_boxes holds G=129 label rows per frame, vd_%s takes 1 to 128" % (name, name), gt_boxes=wide,
                bboxes=wide)
        _raises(name, "%s: gt_boxes holds 2 frames, bboxes 1" % name, bboxes=b["bboxes"][:1])
    else:
        # the row limit is checked before the tensors: ids of the narrow shape do not get a word in
        _raises(name, "%s: N=129 rows per frame, %s takes at most 128" % (name, VD[name]), bboxes=wide)


@pytest.mark.parametrize("name", NUM_CLASS_GE_1)
def test_num_class(name):
    for bad in (0, True, 1.0, "1"):
        _raises(name, "%s: num_class must be an integer >= 1, got %r" % (name, bad), num_class=bad)
    # ... and before the tensors
    _raises(name, "%s: num_class must be an integer >= 1, got -1" % name, num_class=-1, ids=None)


def test_num_class_hota():
    for what, hi in (("num_gt_id", 1024), ("num_track", 2 ** 31 - 1), ("num_class", 2 ** 31 - 1)):
        for bad in (0, False, 2.0, hi + 1):
            _raises("hota_match", "hota_match: %s must be an integer in [1, %d], got %r" % (what, hi, bad), **{what: bad})
    _raises("hota_match", "hota_match: num_gt_id must be an integer in [1, 1024], got 0", num_gt_id=0, num_track=0)


@pytest.mark.parametrize("name", CLIP)
def test_order_of_checks(name):
    """two faults at once: the one checked first is the one reported"""
    b = _base(name)
    bad_scores = _rows_sentence(name, "scores", F * N, "float32", "torch.float64 (2, 3, 1)")
    short = torch.empty(_need(name) - 1, dtype=torch.uint8, device="cuda")
    _raises(name, _rows_sentence(name, "ids", F * N, "float32", "torch.float32 (2, 3, 1)"), ids=b["ids"].cpu(),
            scores=b["scores"].double())
    _raises(name, bad_scores, scores=b["scores"].double(), clip_start=[0, 1, 3])
    _raises(name, bad_scores, scores=b["scores"].double(), ws=short)
    _raises(name, BAD_OFFSETS % name, clip_start=[0, 1, 3], ws=short)
    _raises(name, BAD_DEVICE_OFFSETS % name, clip_start=torch.tensor([0, 1, 2], device="cuda"), ws=short)
    if name in TAKES_TRACK:
        _raises(name, _rows_sentence(name, "track", F * N, "int32", "torch.int64 (2, 3)"), track=b["track"].long(),
                clip_start=[0, 1, 3])
        _raises(name, bad_scores, scores=b["scores"].double(), track=b["track"].long())
    if name in TRACKED:
        _raises(name, "%s: track must be (F,N) = (2,3), got (3, 2)" % name, track=b["track"].reshape(N, F), clip_start=[0, 1, 3])
    if name in MATCHERS:
        _raises(name, _rows_sentence(name, "gt_cls", F * G, "int32", "torch.int64 (2, 2)"), gt_cls=b["gt_cls"].long(),
                ids=b["ids"].cpu())
        _raises(name, "%s: gt_cls must be (2, 2), got (4,)" % name, gt_cls=b["gt_cls"].reshape(-1), clip_start=[0, 1, 3])
        _raises(name, "%s: agnostic must be a bool, got 1" % name, agnostic=1, bboxes=None)
    if name == "overlay":
        wrong_out = torch.empty(F, 8, 8, 3, dtype=torch.int8, device="cuda")
        out_sentence = "overlay: out must be a uint8 tensor of the frames' shape and strides on their device (or `frames` itself)"
        _raises(name, out_sentence, out=wrong_out, ws=short)
        _raises(name, BAD_OFFSETS % name, clip_start=[0, 1, 3], out=wrong_out)
        _raises(name, "overlay: 1 frames but rows of 2", frames=b["frames"][:1], ids=None)
        _raises(name, "overlay: frames must be a uint8 tensor, got torch.float32", frames=b["frames"].float(), bboxes=None)


def _same(a, b):
    if torch.is_tensor(a):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    return a == b


@pytest.mark.parametrize("name", CLIP)
def test_host_and_device_offsets_agree(name):
    call = getattr(_ops(), name)
    host = call(**dict(_base(name), clip_start=[0, 1, 2]))
    device = call(**dict(_base(name), clip_start=torch.tensor([0, 1, 2], dtype=i32, device="cuda")))
    torch.cuda.synchronize()
    assert len(host) == len(device) and all(_same(a, b) for a, b in zip(host, device))
    one = call(**_base(name))
    assert len(one) == len(host)


# ---------------------------------------------------------------------------------------------------------------------------
# the live-state classes
# ---------------------------------------------------------------------------------------------------------------------------
def _state(name, V=1, **kw):
    if name == "SmoothLagState":
        kw.setdefault("lag", 1)
    return getattr(_ops(), name)(V=V, N=N, **kw)


def _push_args(name, V=1, lead=True):
    shape = ((V,) if lead else ()) + (F, N)
    args = dict(ids=torch.zeros(shape + (1,), device="cuda"), scores=torch.full(shape + (1,), 0.5, device="cuda"),
                bboxes=torch.tensor([0., 0., 4., 4.], device="cuda").expand(shape + (4,)).contiguous())
    if name == "SmoothLagState":
        args["track"] = torch.zeros(shape, dtype=i32, device="cuda")
    return args


def _push_raises(st, message, args):
    with pytest.raises(ValueError) as e:
        st.push(**args)
    assert str(e.value) == message


@pytest.mark.parametrize("name", STATES)
def test_state_constructor(name):
    lag = {"lag": 1} if name == "SmoothLagState" else {}
    for what, hi in (("V", 2 ** 31 - 1), ("N", 128), ("num_class", 2 ** 31 - 1)):
        for bad in (0, True, 1.5, hi + 1):
            with pytest.raises(ValueError) as e:
                getattr(_ops(), name)(**dict(dict(lag, V=1, N=N), **{what: bad}))
            assert str(e.value) == "%s: %s must be an integer in [1, %d], got %r" % (name, what, hi, bad)
    with pytest.raises(ValueError) as e:
        getattr(_ops(), name)(V=0, N=0, num_class=0, **lag)
    assert str(e.value) == "%s: V must be an integer in [1, 2147483647], got 0" % name


@pytest.mark.parametrize("name,V", [(n, 1) for n in STATES] + [("KalmanTrackState", 2)])
def test_state_push(name, V):
    st = _state(name, V=V)
    who = name + ".push"
    good = _push_args(name, V)
    shape_sentence = "%s: bboxes must be (%d,F,3,4)%s, got %%r" % (who, V, " or (F,3,4)" if V == 1 else "")
    n = V * F * N
    ids_sentence = "%s: ids must be a contiguous float32 device tensor of %d elements, got torch.float64 %r" % (
        who, n, tuple(good["ids"].shape))
    _push_raises(st, shape_sentence % ((V, F, 4, 4),), dict(good, bboxes=torch.zeros(V, F, 4, 4, device="cuda")))
    _push_raises(st, shape_sentence % ((V + 1, F, N, 4),), dict(good, bboxes=torch.zeros(V + 1, F, N, 4, device="cuda")))
    _push_raises(st, shape_sentence % ((N, 4),), dict(good, bboxes=torch.zeros(N, 4, device="cuda")))
    if V > 1:
        _push_raises(st, shape_sentence % ((F, N, 4),), dict(good, bboxes=torch.zeros(F, N, 4, device="cuda")))
    _push_raises(st, ids_sentence, dict(good, ids=good["ids"].double()))
    _push_raises(st, "%s: scores must be a contiguous float32 device tensor of %d elements, got torch.float32 %r"
                 % (who, n, tuple(good["scores"].shape)), dict(good, scores=good["scores"].cpu()))
    # the shape before the tensors, the tensors before the id budget
    _push_raises(st, shape_sentence % ((V, F, 4, 4),), dict(good, bboxes=torch.zeros(V, F, 4, 4, device="cuda"), ids=good["ids"].double()))
    if name == "SmoothLagState":
        track_sentence = "%s: track must be a contiguous int32 device tensor %r, got torch.int64 %r" % (
            who, tuple(good["track"].shape), tuple(good["track"].shape))
        _push_raises(st, track_sentence, dict(good, track=good["track"].long()))
        _push_raises(st, ids_sentence, dict(good, ids=good["ids"].double(), track=good["track"].long()))
    st.frames = (2 ** 31 - 1) // N - 1
    budget = "%s: %d + %d frames of %d rows could %s more than 2**31 - 1 track ids; reset() the state (a new clip) first" % (
        who, st.frames, F, N, "meet" if name == "SmoothLagState" else "hand out")
    _push_raises(st, budget, good)
    _push_raises(st, ids_sentence, dict(good, ids=good["ids"].double()))
    if name == "SmoothLagState":
        _push_raises(st, track_sentence, dict(good, track=good["track"].long()))
    assert st.frames == (2 ** 31 - 1) // N - 1             # a refused push counts no frame
    st.reset()
    assert st.frames == 0 and not st.state.any()
    out = st.push(**good)
    assert st.frames == F and len(out) == {"TrackState": 3, "KalmanTrackState": 4, "SmoothLagState": 3}[name]
    if V == 1:                                             # one stream: the leading axis may be left out
        st2 = _state(name)
        out2 = st2.push(**_push_args(name, lead=False))
        torch.cuda.synchronize()
        assert all(_same(a.reshape(b.shape) if torch.is_tensor(a) else a, b) for a, b in zip(out, out2))
        assert torch.equal(st.state, st2.state)


@pytest.mark.parametrize("name", STATES)
def test_state_push_non_tensor(name):
    st = _state(name)
    good = _push_args(name)
    _push_raises(st, "%s.push: ids must be a contiguous float32 device tensor of %d elements, got <class 'NoneType'> ()"
                 % (name, F * N), dict(good, ids=None))
    _push_raises(st, "%s.push: bboxes must be (1,F,3,4) or (F,3,4), got ()" % name, dict(good, bboxes=None))
    assert st.frames == 0
