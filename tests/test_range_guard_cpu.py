"""The closure of `YOLOV3._range_exact` over derived tensors, on the graphs alone: no device needed.
The launch records behind it are checked in tests/test_range_guard_derived_gpu.py."""
from viddet_amd.model import YOLOV3, ConvNode, CorrNode, UpcatNode

CLASSES = ["a", "b"]
HEADS = {'dz:yolo_outputs.%d.prediction' % i for i in range(3)}


def _closed(net, names):
    net._range_exact |= set(names)
    return [n.dst for n in net._close_range_exact()]


def test_plain_network_starts_with_the_head_gradients_only():
    net = YOLOV3(CLASSES, device="cpu")
    assert net._range_exact == HEADS
    assert net._close_range_exact() == []


def test_concat_sources_bring_the_concat_in_and_nothing_else():
    net = YOLOV3(CLASSES, device="cpu")
    assert _closed(net, ["n0.tr"]) == ["n0.cat"]
    assert _closed(net, ["n0.tr"]) == []                        # closed already
    net = YOLOV3(CLASSES, device="cpu")
    assert _closed(net, ["f14"]) == ["n1.cat"]                  # the route side
    assert net._range_exact == HEADS | {"f14", "n1.cat"}


def test_a_fused_residual_is_not_followed():
    """f22 is the residual of the cell that writes f23: that cell has a BatchNorm of its own, which the guard examines"""
    net = YOLOV3(CLASSES, device="cpu")
    assert any(isinstance(n, ConvNode) and n.residual == "f22" and n.dst == "f23" for n in net.nodes)
    assert _closed(net, ["f22"]) == []
    assert "f23" not in net._range_exact and "n0.cat" not in net._range_exact


def test_correlation_join_is_one_case_of_the_walk():
    net = YOLOV3(CLASSES, device="cpu", k=3, corr_pos='early', corr_d=2)
    corr = {n.dst for n in net.nodes if isinstance(n, CorrNode)}
    cats = {n.dst for n in net.nodes if isinstance(n, UpcatNode) and n.route in corr}
    assert corr and cats == {"n0.cat", "n1.cat"}
    assert net._range_exact == HEADS | corr | cats


def test_pools_selections_and_adds():
    net = YOLOV3(CLASSES, device="cpu", k=3, k_join_type='max', k_join_pos='early')
    assert _closed(net, ["f28", "f23"]) == ["route1.pool", "route2.pool", "n0.cat"]
    net = YOLOV3(CLASSES, device="cpu", k=3, k_join_type='cat', k_join_pos='late')
    assert _closed(net, ["n0.tip"]) == ["n0.tip.pool"]
    net = YOLOV3(CLASSES, device="cpu", k=5, temporal_side=True)
    assert _closed(net, ["f14", "f23"]) == ["r0", "f14.s", "f23.a", "r1", "n0.cat", "n1.cat"]
