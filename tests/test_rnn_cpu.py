"""The bidirectional ConvGRU of temporal windows without a GPU: the fp64 restatement (tests/rnn_oracle.py) against an
independent statement of the cell's equations in torch.float64 with autograd, the first-step facts, and the
yolo3_darknet53 rnn_pos flag table (names, shapes, refusals, script plumbing)."""
import numpy as np
import pytest
import torch

from tests import rnn_oracle as RO


def _params(rng, cin, ch, s):
    return {key: rng.standard_normal(shp) * (0.3 if key.endswith("weight") else 0.2) for key, shp in RO.rnn_shapes(cin, ch, s).items()}


def _torch_gru(x5, P, s):
    """the specification's equations, one step after the other; autograd supplies every gradient"""
    F = torch.nn.functional
    B, K, _, h, w = x5.shape

    def run(cell, order):
        Wi, Wh, bi, bh = [P["%s.%s" % (cell, a)] for a in RO.ARRAYS]
        ch = Wh.shape[1]
        hprev = torch.zeros(B, ch, h, w, dtype=torch.float64)
        out = {}
        for t in order:
            I = F.conv2d(x5[:, t], Wi, bi, padding=s // 2)
            H = F.conv2d(hprev, Wh, bh, padding=s // 2)
            Ir, Iz, Io = torch.split(I, ch, dim=1)
            Hr, Hz, Ho = torch.split(H, ch, dim=1)
            r, z = torch.sigmoid(Ir + Hr), torch.sigmoid(Iz + Hz)
            n = torch.tanh(Io + r * Ho)
            hprev = (1 - z) * n + z * hprev
            out[t] = hprev
        return out

    hl, hr = run("l_cell", range(K)), run("r_cell", range(K - 1, -1, -1))
    return torch.stack([(hl[t] + hr[t]) / 2 for t in range(K)], dim=1)


@pytest.mark.parametrize("K,s,cin,ch,h,w", [(2, 1, 3, 2, 3, 5), (3, 3, 2, 3, 5, 3), (5, 3, 3, 2, 3, 3), (3, 1, 4, 4, 1, 7), (2, 3, 2, 2, 7, 5),
                                            (5, 1, 2, 3, 3, 3)])
def test_gru_restatement_matches_autograd(K, s, cin, ch, h, w):
    rng = np.random.default_rng(K * 10 + s)
    x = rng.standard_normal((2, K, cin, h, w))
    P = _params(rng, cin, ch, s)
    y, bw = RO.gru(x, P, s)
    assert y.shape == (2, K, ch, h, w)
    xt = torch.tensor(x, requires_grad=True)
    Pt = {key: torch.tensor(v, requires_grad=True) for key, v in P.items()}
    yt = _torch_gru(xt, Pt, s)
    rel = lambda a, b: float(np.abs(a - b).max()) / max(1e-30, float(np.abs(b).max()))
    assert rel(y, yt.detach().numpy()) <= 1e-10
    g = rng.standard_normal(y.shape)
    yt.backward(torch.tensor(g))
    dx, G = bw(g)
    assert rel(dx, xt.grad.numpy()) <= 1e-10
    assert set(G) == set(P) and len(G) == 8
    for key in P:
        assert np.abs(Pt[key].grad.numpy()).max() > 0, key
        assert rel(G[key], Pt[key].grad.numpy()) <= 1e-10, key


def test_gru_first_step_facts():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 3, 4, 3, 3))
    zero = {key: np.zeros(shp) for key, shp in RO.rnn_shapes(4, 3, 3).items()}
    y, _ = RO.gru(x, zero, 3)
    assert np.all(y == 0)                       # r = z = 1/2, n = tanh(0) = 0, h = 0: a zero channel stays exactly zero
    # K = 1: the only step has no state, and yet h2h_bias enters through H (= the bias alone) and gets a gradient
    P = _params(rng, 4, 3, 1)
    x1 = rng.standard_normal((2, 1, 4, 3, 3))
    y1, bw = RO.gru(x1, P, 1)
    _, G = bw(rng.standard_normal(y1.shape))
    for c in RO.CELLS:
        assert np.abs(G[c + ".h2h_bias"]).max() > 0
        assert np.all(G[c + ".h2h_weight"] == 0)


def _mk(**kw):
    from viddet_amd.model import yolo3_darknet53
    return yolo3_darknet53(["c%d" % i for i in range(3)], device="cpu", **kw)


SUPPORTED = [(k, 'late', jt) for k in (2, 3, 5) for jt in ('max', 'mean', 'cat')] + [(k, 'out', jt) for k in (2, 3) for jt in ('max', 'mean')]


@pytest.mark.parametrize("k,pos,jt", SUPPORTED)
def test_rnn_factory_names_and_shapes(k, pos, jt):
    from viddet_amd.model import GruNode, PoolNode, ConvNode
    net = _mk(k=k, k_join_type=jt, k_join_pos='late', rnn_pos=pos)
    got = {key: tuple(p.shape) for key, p in net.collect_params().items()}
    ref = RO.param_shapes(3, k, pos, jt)
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))[:6]
    for key, shp in ref.items():
        assert got[key] == tuple(shp), (key, got[key], shp)
    grus = [n for n in net.nodes if isinstance(n, GruNode)]
    assert len(grus) == 3
    A = 24
    for i, (g, c) in enumerate(zip(grus, (512, 256, 128))):
        assert (g.cin, g.ch, g.k, g.K) == ((c, 2 * c, 3, k) if pos == 'late' else (2 * c, A, 1, k))
        assert g.chp == (2 * c if pos == 'late' else 32)
    assert len([n for n in net.nodes if isinstance(n, PoolNode)]) == 3
    assert len([n for n in net.conv_nodes if n.head]) == (3 if pos == 'late' else 0)
    # weights in the weight range of the arena, biases in the vector range (beside gamma / beta / head bias)
    for key, p in net.collect_params().items():
        if ".rnn." in key:
            assert (p.span[1] <= net.n_weight) == key.endswith("weight"), key
    if pos == 'out':       # 'out' skips every join in front of the heads: k_join_pos is not read
        net2 = _mk(k=k, k_join_type=jt, k_join_pos='early', rnn_pos='out')
        assert {key: tuple(p.shape) for key, p in net2.collect_params().items()} == got


def test_rnn_flag_table():
    ok = dict(k=3, k_join_type='max', k_join_pos='late')
    refusals = [
        (dict(k=1, rnn_pos='late'), "k > 1"),
        (dict(rnn_pos='out', k_join_type='max'), "k > 1"),
        (dict(ok, rnn_pos='late', block_conv_type='3'), "swaps axes"),
        (dict(ok, rnn_pos='out', block_conv_type='21'), "swaps axes"),
        (dict(ok, rnn_pos='late', corr_pos='late', corr_d=4), "corr_pos"),
        (dict(k=5, rnn_pos='late', temporal=True, t_out=True), "temporal"),
        (dict(k=5, rnn_pos='out', temporal=True), "temporal"),
        (dict(k=3, k_join_type='max', k_join_pos='early', rnn_pos='late'), "k_join_pos 'late'"),
        (dict(k=3, rnn_pos='late'), "k_join_pos 'late'"),
        (dict(k=3, k_join_type='cat', k_join_pos='late', rnn_pos='out'), "max or mean"),
        (dict(k=3, rnn_pos='out'), "max or mean"),
    ]
    for kw, msg in refusals:
        with pytest.raises(NotImplementedError, match=msg):
            _mk(**kw)
    with pytest.raises(ValueError):
        _mk(**dict(ok, rnn_pos='early'))
    for pos in ('late', 'out'):
        net = _mk(**dict(ok, rnn_pos=pos))
        with pytest.raises(NotImplementedError, match="rnn_pos networks"):
            net.set_precision('bf16')
        with pytest.raises(NotImplementedError, match="rnn_pos networks"):
            net.set_storage('bf16')
        assert net.precision == 'fp32' and getattr(net, 'storage', 'fp32') == 'fp32'
        net.set_precision('fp32')
        net.set_storage('fp32')
    with pytest.raises(NotImplementedError, match="reset_class"):
        _mk(**dict(ok, rnn_pos='out')).reset_class(["a", "b"])
    # the class itself refuses what the factory refuses: a direct construction drops nothing silently
    from viddet_amd.model import YOLOV3
    for kw in (dict(k=1, rnn_pos='late'), dict(ok, rnn_pos='late', block_conv_type='21'), dict(ok, rnn_pos='out', corr_pos='late'),
               dict(k=3, k_join_type='max', k_join_pos='early', rnn_pos='late'), dict(k=3, k_join_type='cat', rnn_pos='out'),
               dict(ok, rnn_pos='late', noback=True), dict(dict(ok, k=5), rnn_pos='late', temporal_out=True)):
        with pytest.raises(NotImplementedError, match="rnn_pos"):
            YOLOV3(["a", "b"], device="cpu", **kw)
    with pytest.raises(ValueError):
        YOLOV3(["a", "b"], device="cpu", **dict(ok, rnn_pos='early'))
    # without the flag nothing moves
    plain = {key: tuple(p.shape) for key, p in _mk(**ok).collect_params().items()}
    assert {key: tuple(p.shape) for key, p in _mk(**dict(ok, rnn_pos=None)).collect_params().items()} == plain
    assert not any(".rnn." in key for key in plain)


def test_library_exports_the_gru_kernels():
    from viddet_amd import lib as L
    lib = L.load()
    for name in ("vd_gru_gate_fwd", "vd_gru_gate_bwd", "vd_gru_avg"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    # argument checks run before any launch: no GPU is touched
    assert lib.vd_gru_gate_fwd(16, None, None, None, 16, 1, 3, 0, 4, 32, None) == -1          # neither H nor its bias
    assert b"vd_gru_gate_fwd" in lib.vd_last_error()
    assert lib.vd_gru_gate_fwd(16, 16, None, None, 16, 1, 3, 3, 4, 32, None) == -1            # t outside the window
    assert lib.vd_gru_gate_fwd(16, 16, None, None, 16, 1, 3, 0, 4, 30, None) == -1            # Ch % 4
    assert lib.vd_gru_gate_fwd(16, 8, None, None, 16, 1, 3, 0, 4, 32, None) == -1             # alignment
    assert b"aligned" in lib.vd_last_error()
    assert lib.vd_gru_gate_bwd(16, 16, 1, None, 16, 16, 0.5, None, 0, 1, 3, 0, 4, 32, None) == -1   # a state without dh
    assert lib.vd_gru_avg(16, 16, 16, 1, 3, 6, None, None) == -1


def test_scripts_pass_rnn_pos(monkeypatch):
    import train_yolov3 as T
    seen = {}

    class _Net:
        def initialize(self, **kw):
            pass

    def fake(classes, **kw):
        seen.update(kw)
        return _Net()

    monkeypatch.setattr(T, "yolo3_darknet53", fake)
    monkeypatch.setattr(T, "FLAGS", T.parse_flags(["--dataset", "vid", "--window", "3,1", "--k_join_type", "max", "--k_join_pos", "late",
                                                   "--rnn_pos", "late"]))
    T.get_net(["a"], (0, 1))
    assert seen["rnn_pos"] == "late" and seen["k"] == 3 and seen["k_join_pos"] == "late"
    monkeypatch.setattr(T, "FLAGS", T.parse_flags(["--dataset", "vid", "--window", "3,1", "--k_join_type", "mean", "--rnn_pos", "out"]))
    T.get_net(["a"], (0, 1))
    assert seen["rnn_pos"] == "out"
    monkeypatch.setattr(T, "FLAGS", T.parse_flags(["--dataset", "vid"]))
    T.get_net(["a"], (0, 1))
    assert seen["rnn_pos"] is None
    # detect_yolo3.py no longer stops at the flag: it gets as far as its GPU check
    import detect_yolo3 as Dt
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit):
        Dt.main(["--window", "3,1", "--k_join_type", "max", "--k_join_pos", "late", "--rnn_pos", "late"])
