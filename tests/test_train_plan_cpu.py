"""The graph analysis of the training-plan builder (node_inputs, consumers_of, grad_required and
single_conv_consumer_tensors' rule) as pure functions of a node list: no device."""
import pytest

from viddet_amd.model import (ROUTE_TENSORS, AddNode, ConvNode, CorrNode, GruNode, PoolNode, SelNode, TdwNode, UpcatNode,
                              build_graph, consumers_of, grad_required, node_inputs, single_conv_consumers)

ROUTES = [r[0] for r in ROUTE_TENSORS]


@pytest.fixture(scope="module")
def g1():
    return build_graph(4)[0]


@pytest.fixture(scope="module")
def g3rnn():
    return build_graph(4, k=3, k_join_type='max', k_join_pos='late', rnn_pos='late')[0]


def old_consumers(nodes):
    """the loop of the former _build_train, word for word"""
    consumers = {}
    for m in nodes:
        srcs = [m.src, m.residual] if isinstance(m, (ConvNode, TdwNode)) else ([m.up, m.route] if isinstance(m, UpcatNode) else
                                                                      ([m.a, m.b] if isinstance(m, AddNode) else [m.src]))
        for t in srcs:
            if t:
                consumers.setdefault(t, []).append(m)
    return consumers


def old_scc_reads(n):
    """the (tensor, read as a conv operand) pairs of the former single_conv_consumer_tensors"""
    if isinstance(n, ConvNode):
        return [(n.src, True)] + ([(n.residual, False)] if n.residual else [])
    return [(getattr(n, a), False) for a in ('src', 'up', 'route', 'a', 'b') if getattr(n, a, None)]


def old_users(nodes, t):
    """the stem-fusion search of the former _add_infer_nodes_bf16"""
    return [m for m in nodes if isinstance(m, ConvNode) and (m.src == t or m.residual == t)] + \
           [m for m in nodes if not isinstance(m, ConvNode) and t in [getattr(m, a, None) for a in ('src', 'up', 'route', 'a', 'b')]]


def test_node_inputs_every_type():
    conv = ConvNode('c', 'x', 'y', 8, 8, 3, 1, 1, residual='r')
    plain = ConvNode('c', 'x', 'y', 8, 8, 3, 1, 1)
    one = [PoolNode('p', 'x', 'y', 3, 'max'), CorrNode('k', 'x', 'y', 3, 1, 8), SelNode('s', 'x', 'y', 3, 1, 1),
           GruNode('g', 'g', 'x', 'y', 3, 8, 8, 3, 8, 32)]
    assert node_inputs(conv) == ['x', 'r'] and node_inputs(plain) == ['x']
    assert node_inputs(TdwNode('t', 't', 'x', 'y', 8, 1, 3, residual='r')) == ['x', 'r']
    assert node_inputs(TdwNode('t', 't', 'x', 'y', 8, 1, 3)) == ['x']
    assert node_inputs(UpcatNode('u', 'a', 'b', 'y', 8, 8, 1)) == ['a', 'b']
    assert node_inputs(AddNode('a', 'p', 'q', 'y', 1)) == ['p', 'q']
    for n in one:
        assert node_inputs(n) == ['x'], type(n).__name__
    for n in [conv, plain] + one + [UpcatNode('u', 'a', 'b', 'y', 8, 8, 1), AddNode('a', 'p', 'q', 'y', 1)]:
        assert node_inputs(n) == [t for t, _ in old_scc_reads(n)], type(n).__name__       # the three old loops agree
        assert node_inputs(n) == [t for t in old_consumers([n])]
        for t in ('x', 'r', 'a', 'b', 'p', 'q', 'y'):
            assert (t in node_inputs(n)) == bool(old_users([n], t))


@pytest.mark.parametrize("graph", ["g1", "g3rnn"])
def test_consumers_match_the_old_loop(graph, request):
    nodes = request.getfixturevalue(graph)
    new, old = consumers_of(nodes), old_consumers(nodes)
    assert list(new) == list(old)
    for t in old:
        assert len(new[t]) == len(old[t]) and all(a is b for a, b in zip(new[t], old[t])), t
    if graph == "g3rnn":
        assert any(isinstance(n, GruNode) for n in nodes)


def downstream(nodes, seeds):
    """tensors reachable from the outputs of `seeds`, those outputs included"""
    hit = {n.dst for n in seeds}
    for m in nodes:
        if any(t in hit for t in node_inputs(m)):
            hit.add(m.dst)
    return hit


def is_in(t):
    return t == 'in'


def test_pruning_all_trainable(g1):
    need = grad_required(g1, lambda c: True, is_in)
    assert need.pop('in') is False
    assert need and all(need.values()) and set(need) == {n.dst for n in g1}


def test_pruning_frozen_backbone(g1):
    last = max(i for i, n in enumerate(g1) if n.dst == ROUTES[-1])
    back = g1[:last + 1]
    need = grad_required(g1, lambda c: all(c is not b for b in back), is_in)
    assert not need['in'] and all(not need[n.dst] for n in back) and not any(need[r] for r in ROUTES)
    assert len(g1) > len(back) and all(need[n.dst] for n in g1[last + 1:])


def test_pruning_one_conv_mid_backbone(g1):
    mid = [n for n in g1 if isinstance(n, ConvNode)][20]
    need = grad_required(g1, lambda c: c is mid, is_in)
    want = downstream(g1, [mid])
    assert {t for t, v in need.items() if v} == want and 0 < len(want) < len(g1)
    assert not need[mid.src]


def test_pruning_gru_cells_and_tdw(g3rnn):
    gru = next(n for n in g3rnn if isinstance(n, GruNode))
    cells = [cn for _, i2h, h2h in gru.cells for cn in (i2h, h2h)]
    need = grad_required(g3rnn, lambda c: c is cells[-1], is_in)
    assert {t for t, v in need.items() if v} == downstream(g3rnn, [gru]) and not need[gru.src]
    assert not any(grad_required(g3rnn, lambda c: False, is_in).values())
    # a (2+1)-D cell by hand: conv -> temporal conv (+ skip) -> conv; only the temporal weight trains
    tdw = TdwNode('t', 't.w', 'a', 'b', 8, 1, 3, residual='in')
    nodes = [ConvNode('c0', 'in', 'a', 8, 8, 3, 1, 1, fr=3), tdw, ConvNode('c1', 'b', 'c', 8, 8, 1, 1, 1, fr=3)]
    assert grad_required(nodes, lambda c: c is tdw, is_in) == {'in': False, 'a': False, 'b': True, 'c': True}
    with pytest.raises(AssertionError):
        grad_required(nodes[1:], lambda c: True, is_in)              # 'a' is read, never produced, and no network input


def test_single_conv_consumer_rule(g1):
    use = {}
    for n in g1:
        for t, conv in old_scc_reads(n):
            use.setdefault(t, []).append(conv)
    old = {n.dst for n in g1 if isinstance(n, ConvNode) and n.bn and not n.residual and not n.stem
           and use.get(n.dst) == [True] and n.dst not in ROUTES}
    assert single_conv_consumers(g1) == old and len(old) > 20
