"""What the one inference builder (viddet_amd/infer_plan.py) guarantees, checked on plans built without a device: with
device="cpu" and VD_AUTOTUNE=0 the builders only allocate and append launch records.  Batch 2, 64 x 64, 4 classes."""
import pytest

from viddet_amd.infer_plan import InferPlan
from viddet_amd.model import (AddNode, ConvNode, CorrNode, GruNode, PoolNode, Program, SelNode, TdwNode, UpcatNode,
                              build_graph, yolo3_3ddarknet, yolo3_darknet53)
from viddet_amd.stream import ring_size

CLASSES = ["c%d" % i for i in range(4)]
B, SIZE, CHUNK = 2, 64, 4
NETS = {"default": {}, "k3_max_late": dict(k=3, k_join_type="max", k_join_pos="late"),
        "k3_cat_early": dict(k=3, k_join_type="cat", k_join_pos="early"), "corr": dict(k=3, corr_pos="early", corr_d=2)}
JOINED = ["k3_max_late", "k3_cat_early"]
CONV_FNS = ("vd_conv_igemm", "vd_conv_igemm_bf16", "vd_stem_conv", "vd_stem_conv_c32_bf16")
GEOMETRY = ("N", "Hi", "Wi", "Hg", "Wg", "in_stride", "T", "Kfr")
_built = {}


@pytest.fixture(autouse=True)
def no_tuner(monkeypatch):
    monkeypatch.setenv("VD_AUTOTUNE", "0")
    monkeypatch.setenv("VD_TUNE_CACHE", "off")


def built(name):
    """(net, fp32 program, bf16 program) of one network, built once"""
    if name not in _built:
        net = yolo3_darknet53(CLASSES, device="cpu", **NETS[name])
        _built[name] = (net, net._build_infer(B, SIZE, SIZE)[0], net._build_infer_bf16(B, SIZE, SIZE)[0])
    return _built[name]


def conv_records(net, prog):
    """[(node name, its ConvDesc or None)] of the conv records of a program; the bf16 plan's fused stem record stands for
    two nodes, the stem (no descriptor: it is computed inside the launch) and the stride-2 conv behind it"""
    stem = next(n for n in net.nodes if isinstance(n, ConvNode) and n.stem)
    out = []
    for (fname, _, args), meta in zip(prog.recs, prog.meta):
        if fname not in CONV_FNS:
            continue
        descs = [a._obj for a in args if hasattr(a, "_obj")]
        assert len(descs) == (0 if fname == "vd_stem_conv" else 1)
        if meta.get("fused_stem"):
            out.append((stem.name, None))
        out.append((meta["node"], descs[0] if descs else None))
    return out


def flops(prog):
    return sum(m["flops"] for m in prog.meta if m and "flops" in m)


@pytest.mark.parametrize("name", list(NETS))
def test_fp32_and_bf16_plans_walk_the_same_convs(name):
    net, p32, p16 = built(name)
    c32, c16 = conv_records(net, p32), conv_records(net, p16)
    assert [n for n, _ in c32] == [n for n, _ in c16]                                           # (a)
    assert [n for n, _ in c32] == [n.name for n in net.nodes if isinstance(n, ConvNode)]
    assert any(m and m.get("fused_stem") for m in p16.meta)                                      # the look-ahead did fuse
    compared = 0
    for (node, a), (_, b) in zip(c32, c16):                                                      # (b)
        if a is not None and b is not None:
            assert [getattr(a, f) for f in GEOMETRY] == [getattr(b, f) for f in GEOMETRY], node
            compared += 1
    assert compared == len(c32) - 1                                    # every conv but the stem, which has no descriptor
    assert flops(p32) == flops(p16) > 0                                                          # (c)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", JOINED)
def test_stream_programs_hold_the_plain_plans_convs(name, precision):
    net, p32, p16 = built(name)
    plain = conv_records(net, p32 if precision == "fp32" else p16)
    net.set_precision(precision)
    try:
        sp = net._build_stream(CHUNK, SIZE, SIZE, ring_size(3, 1, CHUNK))
    finally:
        net.set_precision("fp32")
    pre, suf = conv_records(net, sp["pre"]), conv_records(net, sp["suf"])
    # (d) the two programs partition the plain plan's convs, each in the plain plan's order (behind a late join the
    # per-frame nodes of all three scales come first, in the prefix)
    names = [n for n, _ in plain]
    pn, sn = [n for n, _ in pre], [n for n, _ in suf]
    assert pn and sn and not set(pn) & set(sn) and len(set(names)) == len(names)
    assert pn == [n for n in names if n in set(pn)] and sn == [n for n in names if n in set(sn)]
    assert sorted(pn + sn) == sorted(names)
    plain_desc = dict(plain)
    for part, windows in ((pre, B * 3), (suf, B)):
        for node, d in part:
            dp = plain_desc[node]
            assert (d is None) == (dp is None), node
            if d is not None:
                assert d.N == CHUNK and dp.N == windows, node
                assert [getattr(d, f) for f in GEOMETRY[1:]] == [getattr(dp, f) for f in GEOMETRY[1:]], node


def test_dispatch_table_covers_every_node_class():
    graphs = [{}, dict(noback=True), dict(k=5, temporal_out=True), dict(k=5, temporal_side=True),
              dict(k=3, corr_pos="early", corr_d=2), dict(k=3, corr_pos="late", corr_d=2),
              dict(k=3, conv_types=[21, 21, 2, 2, 2, 2], frames=3)]
    graphs += [dict(k=3, k_join_type=jt, k_join_pos=jp, block_conv_type=bt)
               for jt, jp, bt in (("max", "late", "2"), ("mean", "early", "2"), ("cat", "early", "2"), ("cat", "late", "2"),
                                  ("max", "late", "3"), ("max", "late", "21"))]
    graphs += [dict(k=3, k_join_type="max", k_join_pos="late", rnn_pos=rp) for rp in ("late", "out")]
    seen = set()
    for kw in graphs:
        if "conv_types" in kw:
            kw = dict(kw, k=1)                              # (as YOLOV3._build calls it: the window is `frames`)
        seen |= {type(n) for n in build_graph(4, **kw)[0]}
    assert seen == {ConvNode, UpcatNode, PoolNode, CorrNode, GruNode, SelNode, AddNode, TdwNode}  # (e)
    assert seen == set(InferPlan.NODE)
    assert all(callable(getattr(InferPlan, m)) for m in InferPlan.NODE.values())


@pytest.mark.parametrize("kind", ["gru", "tdw"])
def test_bf16_builder_refuses_fp32_only_nodes_by_name(kind):
    if kind == "gru":
        net = yolo3_darknet53(CLASSES, device="cpu", k=3, k_join_type="max", k_join_pos="late", rnn_pos="late")
        node = net.gru_nodes[0]
    else:
        net = yolo3_3ddarknet(CLASSES, device="cpu", k=3, conv_types=[21, 21, 2, 2, 2, 2])
        node = net.tdw_nodes[0]
    assert isinstance(node, GruNode if kind == "gru" else TdwNode)
    prog = Program()
    with pytest.raises(AssertionError, match=node.name.replace(".", r"\.")):                    # (f)
        InferPlan(net, SIZE, SIZE, True).add_nodes(prog, [node], {}, B)
    assert not prog.recs
