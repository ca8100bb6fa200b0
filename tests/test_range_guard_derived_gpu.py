"""The range rule of the fp16-split arithmetic (tests/test_range_guard_gpu.py) behind DERIVED tensors.

A concatenation (UpcatNode), a temporal pool (PoolNode), a frame selection (SelNode) and an add (AddNode) write a tensor
with a new name whose max-abs slot is merged from the sources'.  The rule is enforced by tensor name
(`YOLOV3._amax_or_none`), so a flag on `n0.tr` (transitions.0, read by upcat.0 only) has to reach `n0.cat`, the operand of
the one conv that consumes those channels (yolo_blocks.1.body.0, forward and weight gradient) - and a concatenation whose
two sides differ in scale with flat BatchNorm vectors has to be seen at all.  The tests:
  (a) the launch records behind n0.cat / n1.cat after a flag on the transition or on the route, by pointer;
  (b) the conv the plan really launches on n0.cat against the fp64 conv of the device's own operands, inside the bound of
      the range-exact arithmetic, where the fp16 split on the same operands is demonstrably outside the fp32-grade one;
  (c) a concatenation of a uniformly small transition with an O(1) route: no BatchNorm vector spreads, the ratio of the two
      sides' max-abs slots flags it;
  (d) the temporal nodes: max pool, channel stacking, frame selection, add;
  (e) an untouched network keeps every launch record, and a flag moves exactly the records that read a flagged tensor.
The networks are the 64-pixel, batch-2 ones of the existing guard test: the fault is in which arithmetic a launch record
carries, not in a tile."""
import numpy as np
import pytest
import torch

from oracle import ops as R
from tests.util import dev, dev_nhwc_to_nchw
from tests.test_split_math_gpu import _packed, U

pytestmark = pytest.mark.gpu

C_, SIZE, B_ = 4, 64, 2
THRESH = 2.0 ** -16                    # check_operand_ranges' own default


def _net2d(seed):
    from tests.test_model_gpu import _mk_net, _targets
    net, _ = _mk_net(C_, seed, obj_bias=-1.0)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B_, 3, SIZE, SIZE)).astype(np.float32)
    gt, tg = _targets(rng, B_, C_, SIZE, 3)
    return net, [dev(x), dev(gt)] + [dev(t) for t in tg]


def _temporal_args(rng, K, c):
    from oracle import yolo as Y
    x = rng.standard_normal((B_, K, 3, SIZE, SIZE)).astype(np.float32)
    gt = np.array([[[5., 8., 40., 50.], [-1, -1, -1, -1]], [[10., 12., 30., 28.], [20., 5., 60., 62.]]])
    gid = np.array([[[1.], [-1.]], [[0.], [2.]]])
    tg = Y.prefetch_targets(SIZE, SIZE, [SIZE // 32, SIZE // 16, SIZE // 8], gt, gid, c)
    return [dev(x), dev(gt)] + [dev(t) for t in tg]


def _net_k3(jt, seed=41):
    """a k = 3 fixture of tests/test_temporal_gpu.py (early join, 2-D neck)"""
    from tests.test_temporal_gpu import _mk
    net, _ = _mk(dict(jt=jt, jp="early", bct="2"), 3, seed)
    return net, _temporal_args(np.random.default_rng(seed), 3, 3)


def _net_side(seed=61):
    """the fixture of tests/test_temporal_out_gpu.py::test_temporal_side_branches_inference_and_training (k = 5)"""
    from oracle import net_temporal as OT
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(3)], k=5, temporal=True)
    P = OT.side_init_params(3, seed=seed, obj_bias=-1.0)
    for k, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[k].astype(np.float32)))
    return net, _temporal_args(np.random.default_rng(seed), 5, 3)


def _step(net, args):
    out = [t.clone() for t in net(*args)]
    net.backward()
    torch.cuda.synchronize()
    return out


def _cell(net, name=None, dst=None):
    return [n for n in net.conv_nodes if (n.name == name if name else n.dst == dst)][0]


def _set_bn(net, cell, gamma, beta, ch=None):
    """gamma / beta of a cell's BatchNorm: channel `ch` only, or the whole vector"""
    for key, v in ((".1.gamma", gamma), (".1.beta", beta)):
        p = net.collect_params()[cell.name + key]
        t = p.data().cpu()
        if ch is None:
            t[:] = v
        else:
            t[ch] = v
        p.set_data(t)


def _spread(net, cell):
    """the spread of test_guard_flags_a_spread_layer_and_the_plans_fall_back: one channel's scale 2^-30 of the others'"""
    _set_bn(net, cell, 2.0 ** -30, 0.0, ch=3)


def _derived(net, names):
    """the tensors that carry the channels of `names` on, by the graph alone (no look at net._range_exact): outputs of
    concatenations, temporal pools, frame selections and adds with a source among them, transitively"""
    from viddet_amd.model import UpcatNode, PoolNode, SelNode, AddNode, node_inputs
    got = set(names)
    for n in net.nodes:                                     # node order: a source stands before its readers
        if isinstance(n, (UpcatNode, PoolNode, SelNode, AddNode)) and any(t in got for t in node_inputs(n)):
            got.add(n.dst)
    return got - set(names)


def _conv_records(prog_or_segs):
    """(key, record struct, meta) of every vd_conv_igemm / vd_conv_wgrad record; key = (entry, kind, node, ordinal)"""
    segs = prog_or_segs if isinstance(prog_or_segs, (list, tuple)) else [prog_or_segs]
    out, seen = [], {}
    for seg in segs:
        if not hasattr(seg, 'recs'):
            continue
        for (fname, fn, a), meta in zip(seg.recs, seg.meta):
            if fname in ('vd_conv_igemm', 'vd_conv_wgrad'):
                k3 = (fname, (meta or {}).get('kind'), (meta or {}).get('node'))
                seen[k3] = seen.get(k3, 0) + 1
                out.append((k3 + (seen[k3],), a[0]._obj, meta or {}))
    return out


def _f16x2(d):
    from viddet_amd import lib as L
    return bool(d.flags & L.MATH_F16X2)


def _readers(recs, bufs, names):
    """{tensor: [record structs whose operand `in_` is that tensor's buffer]} - forward convs and weight gradients"""
    ptr = {bufs[t].data_ptr(): t for t in names}
    out = {t: [] for t in names}
    for _, d, _ in recs:
        if d.in_ in ptr:
            out[ptr[d.in_]].append(d)
    return out


def _train_records(net):
    tp = net._last_train
    return _conv_records(tp['fwd'] + tp['bwd'])


def _assert_left_split(net, names, at_least=2):
    """every record of the last training plan that reads one of `names` has left the fp16 split; at least `at_least` such
    records per tensor (a forward conv and its weight gradient)"""
    rd = _readers(_train_records(net), net._last_train['bufs'], names)
    for t, ds in rd.items():
        for d in ds:
            assert not _f16x2(d), "a record that reads %s runs the fp16 split" % t
        assert len(ds) >= at_least, (t, len(ds))
    return rd


def _side_amax(bufs, t):
    from viddet_amd import lib as L
    return float(bufs['amax:' + t].view(-1)[::L.AMAX_STRIDE][:L.AMAX_SLOTS].max())


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("case", ["transition0", "route1", "transition1"])
def test_flag_on_a_concat_source_reaches_the_conv_behind_the_concat(case):
    """(a) A BatchNorm with one channel at 2^-30 on transitions.0 (dst n0.tr, read by upcat.0 only), on the cell that
    produces routes[1] (f23: read by the next stage's stride-2 conv and by upcat.0), on transitions.1 (n1.tr / n1.cat).
    check_operand_ranges() names the cell's output and the concatenation; every forward conv and weight gradient whose
    operand is the cell's output or the concatenation has left the fp16 split (>= 2 records per tensor that a conv reads);
    an fp32 inference program built afterwards leaves it too; nothing new on the second call, outputs bit-identical run to
    run and finite."""
    net, args = _net2d(73)
    if case == "route1":
        cat = [n for n in net.nodes if n.name == "upcat.0"][0]
        cell = _cell(net, dst=cat.route)
        assert cell.dst == "f23"
    else:
        cell = _cell(net, name="transitions.%s" % case[-1])
    cat_t = "n%d.cat" % (1 if case == "transition1" else 0)
    assert _derived(net, [cell.dst]) == {cat_t}
    _step(net, args)
    assert net.check_operand_ranges() == {}
    _spread(net, cell)
    _step(net, args)
    flagged = net.check_operand_ranges()
    assert cell.dst in flagged and flagged[cell.dst] < 2.0 ** -20, flagged
    assert ('dz:' + cell.name) in flagged
    assert not net._programs or all(k[0] == 'buf' for k in net._programs), "plans were not dropped"
    out1 = _step(net, args)
    conv_read = [cat_t] + ([cell.dst] if case == "route1" else [])         # (n0.tr / n1.tr: no conv reads them)
    rd = _assert_left_split(net, conv_read)
    print({t: len(v) for t, v in rd.items()})
    assert cat_t in flagged and flagged[cat_t] < 2.0 ** -20, flagged       # the log line names what moved
    assert set(flagged) == {cell.dst, 'dz:' + cell.name, cat_t}, flagged
    assert net.check_operand_ranges() == {}                                # nothing new
    out2 = [t.clone() for t in net(*args)]
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(out1, out2))
    assert all(bool(torch.isfinite(t).all()) for t in out2)
    # the fp32 inference program built after the flag
    net(args[0])
    torch.cuda.synchronize()
    built = net._programs[('infer', B_, SIZE, SIZE)]
    ird = _readers(_conv_records(built[0]), built[1], conv_read)
    for t, ds in ird.items():
        assert len(ds) >= 1 and not any(_f16x2(d) for d in ds), "inference: a conv that reads %s runs the fp16 split" % t


# ---------------------------------------------------------------------------------------------------------------- (b)
def test_conv_behind_the_concat_against_fp64_on_the_plans_own_operands():
    """(b) The spread of (a) on transitions.0, and four output channels of yolo_blocks.1.body.0 that read ONLY input channel
    3 of the `up` part of n0.cat (the channel at 2^-30).  After the guard has run, one training forward; the device's own
    n0.cat and the raw output of the conv the plan launched on it are found through the launch record's pointers and
    compared with the fp64 conv of exactly those fp32 values: |err| <= (8 u + K u / 16) sum|a||b| on every output with
    operand mass, K = Ci (the bound of the range-exact arithmetic, test_channel_scales_spanning_2_to_the_30).  The same
    operands through the fp16 split are outside 64 u on the selected outputs: the inputs do hit the hole."""
    from viddet_amd import ops
    net, args = _net2d(74)
    cell = _cell(net, name="transitions.0")
    cons = _cell(net, name="yolo_blocks.1.body.0")
    assert cons.src == "n0.cat" and cons.k == 1
    p = net.collect_params()[cons.name + ".0.weight"]
    w = p.data().cpu()
    nsel = 4
    for j in range(nsel):                                  # [up | route]: channel 3 of the concatenation is n0.tr's
        w[j] = 0.0
        w[j, 3] = 2.0 ** -4 * (j + 1)
    p.set_data(w)
    _spread(net, cell)
    _step(net, args)
    assert "n0.tr" in net.check_operand_ranges()
    net(*args)                                             # one training forward on the rebuilt plan
    torch.cuda.synchronize()
    tp = net._last_train
    bufs = tp['bufs']
    fwd = [d for _, d, m in _conv_records(tp['fwd']) if d.in_ == bufs['n0.cat'].data_ptr()]
    assert len(fwd) == 1
    d = fwd[0]
    outs = [t for t in bufs.values() if torch.is_tensor(t) and t.data_ptr() == d.out and t.dim() == 4]
    assert len(outs) == 1 and outs[0].shape[-1] == cons.cout and d.wp == cons.wp.data_ptr()
    xd = bufs['n0.cat'].contiguous()
    ci, co = xd.shape[-1], cons.cout
    assert ci == cons.cin == d.Ci
    x32 = xd.permute(0, 3, 1, 2).double().cpu().numpy()
    w32 = p.data().cpu().double().numpy()
    assert float(np.abs(x32[:, 3]).max()) < 2.0 ** -24 * float(np.abs(x32).max())      # the channel does sit in the hole
    ref = R.conv2d(x32, w32, 1, 0)
    S = R.conv2d(np.abs(x32), np.abs(w32), 1, 0)
    m = S > 0
    assert m[:, :nsel].any()
    e = np.abs(dev_nhwc_to_nchw(outs[0]).astype(np.float64) - ref)
    ratio = float((e[m] / S[m]).max())
    rsel = float((e[:, :nsel][m[:, :nsel]] / S[:, :nsel][m[:, :nsel]]).max())
    # the same operands through the fp16 split
    o2 = torch.empty_like(outs[0])
    ops.conv_fwd(xd, _packed(w32, co), o2, k=1, stride=1, pad=0, Co=co, split="f16x2")
    torch.cuda.synchronize()
    e2 = np.abs(dev_nhwc_to_nchw(o2).astype(np.float64) - ref)
    r16 = float((e2[:, :nsel][m[:, :nsel]] / S[:, :nsel][m[:, :nsel]]).max())
    print("conv behind n0.cat, flags %d: max |err| / sum|a||b| %.2f u (selected outputs %.2f u); fp16 split on the same "
          "operands, selected outputs: %.3g u" % (d.flags, ratio / U, rsel / U, r16 / U))
    assert ratio <= 8 * U + ci * U / 16
    assert r16 > 64 * U


# ---------------------------------------------------------------------------------------------------------------- (c)
def test_concat_of_a_uniformly_small_transition_is_flagged_by_its_two_sides():
    """(c) gamma of transitions.0 = 2^-24 on EVERY channel, beta 0: a flat vector, vd_range_guard flags nothing - but the
    concatenation n0.cat = [up(n0.tr) | f23] holds channels 2^-24 of its max-abs.  check_operand_ranges() returns n0.cat
    with min / max of the two sides' max-abs (each reduced over its sub-slots), below its threshold 2^-16, and the convs
    that read n0.cat leave the fp16 split."""
    net, args = _net2d(75)
    cell = _cell(net, name="transitions.0")
    _step(net, args)
    assert net.check_operand_ranges() == {}
    _set_bn(net, cell, 2.0 ** -24, 0.0)
    _step(net, args)
    bufs = net._last_train['bufs']
    up, route = _side_amax(bufs, "n0.tr"), _side_amax(bufs, "f23")
    want = min(up, route) / max(up, route)
    print("max-abs of n0.tr %.3g, of f23 %.3g: ratio 2^%.1f" % (up, route, np.log2(want)))
    assert 0 < want < THRESH
    flagged = net.check_operand_ranges()
    assert set(flagged) == {"n0.cat"}, flagged            # no BatchNorm vector shows it; n1.cat has two O(1) sides
    assert abs(flagged["n0.cat"] - want) <= 1e-6 * want, (flagged, want)
    assert not net._programs or all(k[0] == 'buf' for k in net._programs), "plans were not dropped"
    out1 = _step(net, args)
    _assert_left_split(net, ["n0.cat"])
    assert net.check_operand_ranges() == {}
    out2 = [t.clone() for t in net(*args)]
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(out1, out2))
    assert all(bool(torch.isfinite(t).all()) for t in out2)


# ---------------------------------------------------------------------------------------------------------------- (d)
def _flag_and_check(net, args, cells, conv_read, derived):
    for c in cells:
        _spread(net, c)
    _step(net, args)
    flagged = net.check_operand_ranges()
    for c in cells:
        assert c.dst in flagged, (c.dst, flagged)
    assert _derived(net, [c.dst for c in cells]) == set(derived)
    _step(net, args)
    rd = _assert_left_split(net, conv_read)
    print({t: len(v) for t, v in rd.items()})
    assert set(derived) <= set(flagged), (derived, flagged)
    assert net.check_operand_ranges() == {}


def test_flag_reaches_the_convs_behind_a_temporal_max_pool():
    """(d) k = 3, early max join: f28 -> pool.route2 -> route2.pool, the operand of yolo_blocks.0.body.0; f23 ->
    pool.route1 -> route1.pool -> upcat.0 -> n0.cat (a pool AND a concatenation between the flag and the conv).
    (No fixture of tests/test_temporal_gpu.py or of the ConvGRU tests puts a derived tensor at a GruNode's src - 'late' reads
    the block's last 1x1 cell, 'out' the tip cell, both conv outputs - so the i2h convs have no case here.)"""
    net, args = _net_k3("max")
    _step(net, args)
    assert net.check_operand_ranges() == {}
    _flag_and_check(net, args, [_cell(net, dst="f28"), _cell(net, dst="f23")],
                    conv_read=["route2.pool", "n0.cat", "f23"], derived=["route2.pool", "route1.pool", "n0.cat"])


def test_flag_reaches_the_convs_behind_a_temporal_cat():
    """(d) k = 3, early 'cat' join (channel stacking): f28 -> route2.pool with 3 x 1024 channels, read by yolo_blocks.0.body.0"""
    net, args = _net_k3("cat")
    _flag_and_check(net, args, [_cell(net, dst="f28")], conv_read=["route2.pool"], derived=["route2.pool"])


def test_flag_reaches_the_convs_behind_frame_selections_and_adds():
    """(d) SelNode and AddNode exist only in the side-branch network (k = 5; no k = 3 graph has them).  f14 (5 frames) ->
    sel.s1 -> f14.s, the operand of stages.1.0; -> sel.r0 -> r0 -> upcat.1 -> n1.cat.  f23 (3 frames) -> add.1 -> f23.a,
    the operand of the second side branch's first conv; -> sel.r1 -> r1, the operand of stages.2.0; -> upcat.0 -> n0.cat."""
    from viddet_amd.model import SelNode, AddNode
    net, args = _net_side()
    assert any(isinstance(n, SelNode) for n in net.nodes) and any(isinstance(n, AddNode) for n in net.nodes)
    _flag_and_check(net, args, [_cell(net, dst="f14"), _cell(net, dst="f23")],
                    conv_read=["f14", "f14.s", "n1.cat", "f23.a", "r1", "n0.cat"],
                    derived=["f14.s", "r0", "n1.cat", "f23.a", "r1", "n0.cat"])


# ---------------------------------------------------------------------------------------------------------------- (e)
def _untouched(net, args):
    """He-initialised network: nothing flagged, no plan dropped, the same records in the fp16 split before and after"""
    _step(net, args)
    tp = net._last_train
    keys = set(net._programs)
    before = [k for k, d, _ in _train_records(net) if _f16x2(d)]
    assert len(before) > 0
    assert net.check_operand_ranges() == {}
    assert set(net._programs) == keys and net._last_train is tp, "plans were dropped"
    _step(net, args)
    assert net._last_train is tp
    after = [k for k, d, _ in _train_records(net) if _f16x2(d)]
    assert net.check_operand_ranges() == {}
    assert before == after
    return before


def test_untouched_temporal_network_keeps_its_plans():
    """(e) the k = 3 fixture: pools and concatenations in the graph, nothing flagged, every record as it was"""
    net, args = _net_k3("max")
    n = len(_untouched(net, args))
    print("%d records in the fp16 split" % n)


def test_untouched_network_keeps_its_plans_and_a_flag_moves_only_its_readers():
    """(e) 2-D network: untouched, check_operand_ranges() returns {} and drops nothing.  Then the flag of (a) on n0.tr: the
    rebuilt plan has the same records, none GAINS the fp16 split, and those that lose it are exactly the ones that read a
    flagged tensor: n0.tr or n0.cat as operand `in_` (by pointer), and - the existing rule, flagged with n0.tr because
    gamma * invstd spreads with gamma - the gradient dz of transitions.0 (its data and weight gradient; dz lives in a
    shared scratch buffer, so these two are named by their node).  A fix that turns the split off everywhere fails here."""
    net, args = _net2d(76)
    before = set(_untouched(net, args))
    recs0 = _train_records(net)
    rd0 = _readers(recs0, net._last_train['bufs'], ["n0.tr", "n0.cat"])
    reads = {id(d) for ds in rd0.values() for d in ds}
    may_move = {k for k, d, m in recs0 if id(d) in reads or
                (m.get('node') == "transitions.0" and m.get('kind') in ('dgrad', 'wgrad'))}
    assert len(rd0["n0.cat"]) >= 2 and not rd0["n0.tr"]            # (no conv reads n0.tr itself)
    _spread(net, _cell(net, name="transitions.0"))
    _step(net, args)
    flagged = net.check_operand_ranges()
    assert "n0.tr" in flagged and "dz:transitions.0" in flagged, flagged
    _step(net, args)
    recs1 = _train_records(net)
    assert [k for k, _, _ in recs1] == [k for k, _, _ in recs0]    # the same launch records, one for one
    after = {k for k, d, _ in recs1 if _f16x2(d)}
    print("records in the fp16 split: %d before, %d after; %d read a flagged tensor" % (len(before), len(after), len(may_move)))
    assert after <= before, sorted(after - before)
    assert before - after == before & may_move, (sorted(before - after), sorted(before & may_move))
    rd1 = _readers(recs1, net._last_train['bufs'], ["n0.cat"])
    assert len(rd1["n0.cat"]) >= 2 and not any(_f16x2(d) for d in rd1["n0.cat"])
    assert set(flagged) == {"n0.tr", "dz:transitions.0", "n0.cat"}, flagged
