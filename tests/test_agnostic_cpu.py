"""Class-agnostic detection (--model_agnostic), the parts that need no GPU: the oracle restatement (tests/agnostic_oracle.py)
on hand-made heads, what the factory accepts and refuses, the parameter set, and detect_yolo3.py's flag handling up to its
GPU check."""
import os

import numpy as np
import pytest
import torch

from oracle import yolo as Y
from tests import agnostic_oracle as AO

CLASSES = ["a", "b", "c"]
GRIDS = [2, 4, 8]            # a 64 x 64 image


def _logit(p):
    return float(np.log(p / (1.0 - p)))


def _blank(b=1, c=2, obj=-20.0, grids=GRIDS):
    """heads on which nothing is valid: objectness logit `obj`, class logits -20, centred unit-anchor boxes"""
    heads = []
    for g in grids:
        h = np.zeros((b, 3, 5 + c, g, g))
        h[:, :, 4] = obj
        h[:, :, 5:] = -20.0
        heads.append(h.reshape(b, 3 * (5 + c), g, g))
    return heads


def _set(head, c, a, y, x, obj=None, cls=None, box=None):
    v = head.reshape(head.shape[0], 3, 5 + c, head.shape[2], head.shape[3])
    if obj is not None:
        v[0, a, 4, y, x] = obj
    if cls is not None:
        v[0, a, 5:, y, x] = cls
    if box is not None:
        v[0, a, 0:4, y, x] = box


def test_rows_ids_and_scores_of_the_agnostic_output():
    c, rng = 3, np.random.default_rng(3)
    heads = [rng.standard_normal((2, 3 * (5 + c), g, g)) for g in GRIDS]
    (ids, sc, bx, rows), alldet = AO.agnostic_detect(heads, c)
    P = 3 * sum(g * g for g in GRIDS)
    assert alldet.shape == (2, P, 6) and np.all(alldet[..., 0] == 0)
    # row = [head][pixel][anchor]; score = sigmoid(objectness) alone; boxes = the training-mode boxes (yolo3.py:172-177)
    g, s, y, x, a = 4, 1, 2, 3, 1
    row = 3 * GRIDS[0] ** 2 + (y * g + x) * 3 + a
    v = heads[s].reshape(2, 3, 5 + c, g, g)
    assert alldet[1, row, 1] == pytest.approx(1.0 / (1.0 + np.exp(-v[1, a, 4, y, x])), abs=1e-15)
    box = np.concatenate([Y.yolo_output(h, c, Y.OUT_ANCHORS[i], Y.OUT_STRIDES[i], training=True)[0] for i, h in enumerate(heads)], axis=1)
    assert np.array_equal(alldet[..., 2:6], box)
    assert ids.shape == (2, 100, 1) and sc.shape == (2, 100, 1) and bx.shape == (2, 100, 4) and rows.shape == (2, 100)
    kept = rows >= 0
    assert np.all(ids[..., 0][kept] == 0) and np.all(ids[..., 0][~kept] == -1) and np.all(bx[~kept] == -1) and np.all(sc[..., 0][~kept] == -1)


def test_overlapping_anchors_of_different_classes_suppress_each_other_only_in_agnostic_mode():
    c = 2
    heads = _blank(c=c)
    # two anchors of one stride-16 cell with (almost) the same box: anchor 0 says class 0, anchor 1 says class 1
    aw = np.asarray(Y.OUT_ANCHORS[1], dtype=np.float64).reshape(3, 2)
    _set(heads[1], c, 0, 1, 1, obj=3.0, cls=[6.0, -20.0], box=[0, 0, np.log(40.0 / aw[0, 0]), np.log(40.0 / aw[0, 1])])
    _set(heads[1], c, 1, 1, 1, obj=2.0, cls=[-20.0, 6.0], box=[0, 0, np.log(42.0 / aw[1, 0]), np.log(42.0 / aw[1, 1])])
    (ids_a, sc_a, bx_a, rows_a), _ = AO.agnostic_detect(heads, c)
    (ids_p, sc_p, bx_p, rows_p), _ = AO.per_class_detect(heads, c)
    base = 3 * GRIDS[0] ** 2 + (1 * 4 + 1) * 3
    assert rows_a[0].tolist()[:2] == [base, -1]                       # the weaker anchor is suppressed: one id
    assert ids_a[0, 0, 0] == 0 and sc_a[0, 0, 0] == pytest.approx(1.0 / (1.0 + np.exp(-3.0)))
    assert (ids_p[0, :, 0] >= 0).sum() == 2 and sorted(ids_p[0, :2, 0].tolist()) == [0.0, 1.0]   # two ids: both stay


def test_score_exactly_at_valid_thresh_is_dropped():
    c = 1
    heads = _blank(c=c)
    _set(heads[0], c, 0, 0, 0, obj=_logit(0.5))
    (_, sc, _, rows), alldet = AO.agnostic_detect(heads, c)
    assert (rows[0] >= 0).sum() == 1
    # a score that IS valid_thresh: box_nms keeps score > valid_thresh
    alldet = alldet.copy()
    alldet[0, 5, 1] = 0.01
    out, kept = Y.box_nms(alldet, 0.45, 0.01, 400)
    assert kept[0].tolist() == [0]
    alldet[0, 5, 1] = np.nextafter(0.01, 1.0)
    out, kept = Y.box_nms(alldet, 0.45, 0.01, 400)
    assert 5 in np.concatenate([kept[0], np.nonzero(alldet[0, :, 1] > 0.01)[0]])   # one ulp above it: valid


def test_more_than_topk_valid_anchors():
    c, topk = 2, 20
    heads = _blank(c=c)
    P = 3 * sum(g * g for g in GRIDS)
    rng = np.random.default_rng(5)
    # every anchor valid, distinct scores, boxes shrunk to 2 px so that nothing overlaps within a head's cells
    lg = rng.permutation(np.linspace(-3.0, 3.0, P))
    off = 0
    for s, g in enumerate(GRIDS):
        v = heads[s].reshape(1, 3, 5 + c, g, g)
        n = g * g * 3
        v[0, :, 4] = lg[off:off + n].reshape(g, g, 3).transpose(2, 0, 1)
        aw = np.asarray(Y.OUT_ANCHORS[s], dtype=np.float64).reshape(3, 2)
        for a in range(3):
            v[0, a, 0] = rng.uniform(-3, 3, (g, g))
            v[0, a, 1] = rng.uniform(-3, 3, (g, g))
            v[0, a, 2] = np.log(1.0 / aw[a, 0])
            v[0, a, 3] = np.log(1.0 / aw[a, 1])
        off += n
    (ids, sc, bx, rows), alldet = AO.agnostic_detect(heads, c, nms_topk=topk, post_nms=100)
    assert (alldet[0, :, 1] > 0.01).all()
    kept = rows[0][rows[0] >= 0]
    assert len(kept) <= topk
    top = np.argsort(-alldet[0, :, 1], kind='stable')[:topk]
    assert set(kept.tolist()) <= set(top.tolist())                       # nothing below the top-k is ever kept
    assert kept[0] == top[0] and np.all(np.diff(sc[0, :len(kept), 0]) < 0)
    assert np.all(rows[0, len(kept):] == -1)


def test_zero_valid_anchors_gives_all_minus_one_rows():
    (ids, sc, bx, rows), alldet = AO.agnostic_detect(_blank(b=2, c=3), 3)
    assert not (alldet[..., 1] > 0.01).any()
    assert np.all(ids == -1) and np.all(sc == -1) and np.all(bx == -1) and np.all(rows == -1)


# ---------------------------------------------------------------------------------------------- factory
def test_factory_accepts_and_refuses():
    from viddet_amd.model import yolo3_darknet53, yolo3_3ddarknet, yolo3_no_backbone, YOLOV3
    mk = lambda **kw: yolo3_darknet53(CLASSES, device="cpu", agnostic=True, **kw)
    for kw in (dict(), dict(k=3, k_join_type='max', k_join_pos='late'), dict(k=3, k_join_type='cat', k_join_pos='early'),
               dict(k=3, k_join_type='mean', k_join_pos='late', block_conv_type='21'),
               dict(k=3, corr_pos='late', corr_d=2), dict(k=3, k_join_type='max', k_join_pos='late', rnn_pos='late')):
        net = mk(**kw)
        assert net.agnostic is True
    assert yolo3_darknet53(CLASSES, device="cpu").agnostic is False
    # bf16 precision is accepted where the per-class network accepts it
    net = mk()
    net.set_precision('bf16')
    assert net.precision == 'bf16'
    # an all-2-D conv_types list is the plain network, flag included
    assert yolo3_3ddarknet(CLASSES, conv_types=[2] * 6, device="cpu", agnostic=True).agnostic is True
    with pytest.raises(NotImplementedError, match="yolo3_3ddarknet without the flag"):
        yolo3_3ddarknet(CLASSES, conv_types=[21, 2, 2, 2, 2, 2], k=3, device="cpu", agnostic=True)
    with pytest.raises(NotImplementedError, match="yolo3_3ddarknet without the flag"):
        YOLOV3(CLASSES, device="cpu", k=3, conv_types=[21, 2, 2, 2, 2, 2], agnostic=True)
    with pytest.raises(NotImplementedError, match="rnn_pos 'out'"):
        mk(k=3, k_join_type='max', k_join_pos='late', rnn_pos='out')
    with pytest.raises(NotImplementedError, match="rnn_pos 'out'"):
        YOLOV3(CLASSES, device="cpu", k=3, k_join_type='max', k_join_pos='late', rnn_pos='out', agnostic=True)
    for kw in (dict(k=5, temporal=True), dict(k=5, t_out=True)):
        with pytest.raises(NotImplementedError, match="YOLOV3Temporal is not passed the flag"):
            mk(**kw)
    for kw in (dict(temporal_out=True), dict(temporal_side=True)):
        with pytest.raises(NotImplementedError, match="YOLOV3Temporal is not passed the flag"):
            YOLOV3(CLASSES, device="cpu", k=5, agnostic=True, **kw)
    with pytest.raises(NotImplementedError, match="YOLOV3_noback has no agnostic argument"):
        yolo3_no_backbone(CLASSES, device="cpu", agnostic=True)


@pytest.mark.parametrize("kw", [dict(), dict(k=3, k_join_type='max', k_join_pos='late'),
                                dict(k=3, k_join_type='max', k_join_pos='late', rnn_pos='late')])
def test_parameters_and_graph_are_those_of_the_per_class_network(kw):
    from viddet_amd.model import yolo3_darknet53
    a = yolo3_darknet53(CLASSES, device="cpu", agnostic=True, **kw)
    p = yolo3_darknet53(CLASSES, device="cpu", **kw)
    sig = lambda net: [(key, tuple(q.shape), q.kind, q.span) for key, q in net.collect_params().items()]
    assert sig(a) == sig(p)
    assert a.n_params == p.n_params and a.head_names == p.head_names
    assert [type(n).__name__ for n in a.nodes] == [type(n).__name__ for n in p.nodes]
    # the class channels stay: 3 * (5 + C) outputs per head
    for name, q in a.collect_params('yolo_outputs.*weight').items():
        assert q.shape[0] == 3 * (5 + len(CLASSES)), name


# ---------------------------------------------------------------------------------------------- detect_yolo3.py
def test_detect_script_flags(monkeypatch):
    import detect_yolo3 as Dt
    assert Dt.pred_dir("results", "0001", True) == os.path.join("results", "0001", "pred_ag")
    assert Dt.pred_dir("results", "0001", False) == os.path.join("results", "0001", "pred")
    assert Dt.result_name("voc", True) == "voc_ag" and Dt.result_name("voc", False) == "voc"

    def flags(argv):
        F = Dt.parse_flags(argv)
        F.window = [int(s) for s in F.window]
        return F

    F = flags(["--model_agnostic"])
    assert Dt.check_flags(F) is None and F.metric_agnostic is True            # detect_yolo3.py:797-798
    for extra in (["--precision", "bf16"], ["--window", "3,1", "--k_join_type", "max", "--k_join_pos", "late"],
                  ["--window", "3,1", "--corr_pos", "late", "--corr_d", "2"],
                  ["--window", "3,1", "--k_join_type", "mean", "--k_join_pos", "late", "--rnn_pos", "late"]):
        assert Dt.check_flags(flags(["--model_agnostic"] + extra)) is None
    with pytest.raises(NotImplementedError, match="--metric_agnostic without --model_agnostic only acts inside VIDDetectionMetric"):
        Dt.check_flags(flags(["--metric_agnostic"]))
    with pytest.raises(NotImplementedError, match="--model_agnostic does not combine with --conv_types 21"):
        Dt.check_flags(flags(["--model_agnostic", "--conv_types", "21,2,2,2,2,2", "--window", "3,1"]))
    with pytest.raises(NotImplementedError, match="--model_agnostic with --rnn_pos out"):
        Dt.check_flags(flags(["--model_agnostic", "--window", "3,1", "--k_join_type", "max", "--rnn_pos", "out"]))
    # main(): refusals come before the GPU check, an accepted combination gets as far as that check
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit):
        Dt.main(["--model_agnostic", "--random_init"])
    with pytest.raises(SystemExit):
        Dt.main(["--model_agnostic", "--random_init", "--precision", "bf16"])
    with pytest.raises(NotImplementedError, match="VIDDetectionMetric"):
        Dt.main(["--metric_agnostic", "--random_init"])
    with pytest.raises(NotImplementedError, match="--conv_types"):
        Dt.main(["--model_agnostic", "--random_init", "--conv_types", "21,2,2,2,2,2", "--window", "3,1"])
