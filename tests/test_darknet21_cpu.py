"""The (2+1)-D Darknet backbone of frame windows (--conv_types 21) without a GPU: the fp64 restatement of Conv3DRepPad
(tests/darknet21_oracle.py) against an independent torch.float64 autograd statement, the tail-pad quirk, the static-window
identity, the graph tables of yolo3_3ddarknet (names, shapes, pools, frames per tensor), the refusals, the library's new
entry points and the scripts' flag plumbing."""
import numpy as np
import pytest
import torch

from tests import darknet21_oracle as DO

CLASSES = ["c%d" % i for i in range(3)]
CTS = [[21, 2, 2, 2, 2, 2], [21, 21, 21, 21, 2, 2], [21, 21, 21, 21, 21, 2], [21] * 6]


def _torch_tdw(x, w):
    xp = torch.cat([x[:, :, :1], x, x[:, :, -2:-1]], 2)
    return torch.nn.functional.conv3d(xp, w, groups=x.shape[1])


@pytest.mark.parametrize("K", [2, 3, 5])
def test_restatement_matches_autograd(K):
    rng = np.random.default_rng(K)
    x, w = rng.standard_normal((2, 4, K, 3, 5)), rng.standard_normal((4, 1, 3, 1, 1))
    g = rng.standard_normal(x.shape)
    xt, wt = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
    yt = _torch_tdw(xt, wt)
    yt.backward(torch.tensor(g))
    y = DO.tdw_forward(x, w)
    dx, dw = DO.tdw_backward(x, w, g)
    rel = lambda a, b: float(np.abs(a - b).max()) / float(np.abs(b).max())
    assert y.shape == x.shape
    assert rel(y, yt.detach().numpy()) <= 1e-10
    assert rel(dx, xt.grad.numpy()) <= 1e-10
    assert rel(dw, wt.grad.numpy()) <= 1e-10


def test_tail_pad_is_frame_k_minus_2():
    """slice_axis(begin=-2, end=-1) (three_darknet.py:62): the frame behind the window is a copy of frame K-2, so the third
    tap of y[K-1] does not see frame K-1"""
    K = 3
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 2, K, 2, 2))
    w = np.zeros((2, 1, 3, 1, 1))
    w[:, 0, 2] = 1.0                                    # the third tap alone
    x2 = x.copy()
    x2[:, :, K - 1] += 5.0                              # only frame K-1 changes
    y, y2 = DO.tdw_forward(x, w), DO.tdw_forward(x2, w)
    assert np.array_equal(y[:, :, K - 1], y2[:, :, K - 1])
    assert np.array_equal(y[:, :, K - 1], x[:, :, K - 2])
    assert not np.array_equal(y[:, :, K - 2], y2[:, :, K - 2])      # (frame K-1 is the ordinary third tap of y[K-2])


@pytest.mark.parametrize("K", [2, 3, 5])
def test_static_window_with_thirds_is_the_identity(K):
    rng = np.random.default_rng(1)
    f = rng.standard_normal((2, 4, 1, 3, 3))
    x = np.repeat(f, K, axis=2)
    y = DO.tdw_forward(x, np.full((4, 1, 3, 1, 1), 1.0 / 3))
    assert np.abs(y - x).max() <= 1e-15


def _mk(ct, k=3, **kw):
    from viddet_amd.model import yolo3_3ddarknet
    return yolo3_3ddarknet(CLASSES, conv_types=ct, k=k, device="cpu", **kw)


@pytest.mark.parametrize("ct", CTS)
def test_graph_tables(ct):
    from viddet_amd.model import PoolNode, TdwNode, ConvNode
    K = 3
    net = _mk(ct, K)
    got = {key: tuple(p.shape) for key, p in net.collect_params().items()}
    ref = DO.param_shapes(3, ct)
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))[:6]
    for key, shp in ref.items():
        assert got[key] == tuple(shp), (key, got[key], shp)
    cs = DO.conv_swap(ct)
    pools = {n.name: n for n in net.nodes if isinstance(n, PoolNode)}
    # one trunk pool, at the features index where the 2-D stages begin; a route pooled on its own where it left with K frames
    want = {'pool.trunk'} | ({'pool.route0'} if cs >= 5 else set()) | ({'pool.route1'} if cs == 6 else set())
    assert set(pools) == want
    plan = DO.feature_plan(ct)
    assert pools['pool.trunk'].feature_index == [i for i, kind, _, _ in plan if kind == 'pool'][0]
    assert all(p.K == K and p.type == 0 for p in pools.values())
    # frames per tensor: K through the 21 prefix (the spatial and the temporal half of every cell), 1 behind the pool
    n21 = sum(1 for c in ct if c == 21)
    tdw = [n for n in net.nodes if isinstance(n, TdwNode)]
    assert len(tdw) == sum(([1] + [1 + l for l in DO.LAYERS])[:n21])
    assert len(tdw) == len(net.tdw_nodes) == sum(1 for key in got if key.endswith(".3.conv.weight"))
    for n in tdw:
        assert net.tensors[n.src][3] == K and net.tensors[n.dst][3] == K and n.K == K
        assert net.n_wconv <= n.w_off < net.n_weight                       # in the weight range of the arena
    for n in net.nodes:
        if isinstance(n, ConvNode):
            in_prefix = n.name.startswith("d_model.") and getattr(n, 'conv3d', False)
            assert n.fr == (K if in_prefix else 1), n.name
            assert net.tensors[n.dst][3] == n.fr
    for h in net.head_names:
        assert net.tensors[h][3] == 1
    routes = [n.route for n in net.nodes if type(n).__name__ == 'UpcatNode']
    assert all(net.tensors[r][3] == 1 for r in routes)
    # the temporal weights take weight decay / lr like any weight: they merge into the weight range of the optimiser
    rs = net._optimizer_ranges()
    assert len(rs) == 2 and rs[0][:2] == (0, net.n_weight)


def test_refusals():
    from viddet_amd.model import yolo3_3ddarknet, YOLOV3
    table = [
        (dict(conv_types=[3, 2, 2, 2, 2, 2], k=3), "conv_types 3"),
        (dict(conv_types=[21, 3, 2, 2, 2, 2], k=3), "conv_types 3"),
        (dict(conv_types=[2, 21, 2, 2, 2, 2], k=3), "21 after a 2"),
        (dict(conv_types=[21, 2, 21, 2, 2, 2], k=3), "21 after a 2"),
        (dict(conv_types=[21, 2, 2, 2, 2], k=3), "6 entries"),
        (dict(conv_types=[21, 2, 2, 2, 2, 2, 2], k=3), "6 entries"),
        (dict(conv_types=[21, 2, 2, 2, 2, 5], k=3), "must be 2 or 21"),
        (dict(conv_types=[21, 2, 2, 2, 2, 2], k=1), "K = 1 is refused"),
        (dict(conv_types=[21, 2, 2, 2, 2, 2]), "K = 1 is refused"),
        (dict(conv_types=[21, 2, 2, 2, 2, 2], k=3, norm_layer='syncbn', norm_kwargs=dict(scope='all')), "scope 'reference' only"),
    ]
    for kw, msg in table:
        with pytest.raises(NotImplementedError, match=msg):
            yolo3_3ddarknet(CLASSES, device="cpu", **kw)
    # the class refuses what does not combine with the single-frame neck: nothing is dropped silently
    ct = [21, 21, 2, 2, 2, 2]
    for kw in (dict(k_join_type='max', k_join_pos='late'), dict(block_conv_type='21'), dict(corr_pos='late', corr_d=2),
               dict(rnn_pos='late'), dict(temporal_out=True), dict(temporal_side=True), dict(noback=True)):
        with pytest.raises(NotImplementedError, match="do not combine"):
            YOLOV3(CLASSES, device="cpu", k=3, conv_types=ct, **kw)
    net = _mk(ct)
    with pytest.raises(NotImplementedError, match="temporal-conv kernels"):
        net.set_precision('bf16')
    with pytest.raises(NotImplementedError, match="temporal-conv kernels"):
        net.set_storage('bf16')
    assert net.precision == 'fp32' and getattr(net, 'storage', 'fp32') == 'fp32'
    with pytest.raises(NotImplementedError, match="extract_features"):
        net.extract_features(torch.zeros(1, 3, 3, 64, 64))
    assert net.syncbn_scope is None
    assert _mk(ct, norm_layer='syncbn').syncbn_scope == 'reference'


def test_all_2d_is_the_plain_network():
    from viddet_amd.model import yolo3_darknet53, yolo3_3ddarknet, YOLOV3
    plain = yolo3_darknet53(CLASSES, device="cpu")
    sig = lambda net: [(key, tuple(p.shape), p.kind, p.span) for key, p in net.collect_params().items()]
    for net in (yolo3_3ddarknet(CLASSES, conv_types=[2] * 6, device="cpu"), YOLOV3(CLASSES, device="cpu", conv_types=[2] * 6),
                YOLOV3(CLASSES, device="cpu")):
        assert sig(net) == sig(plain)
        assert net.n_wconv == net.n_weight == plain.n_weight and net.n_params == plain.n_params and not net.tdw_nodes
        assert [type(n).__name__ for n in net.nodes] == [type(n).__name__ for n in plain.nodes]


def test_freeze_base_and_multipliers_reach_the_temporal_weights():
    net = _mk([21, 21, 2, 2, 2, 2], freeze_base=True)
    P = net.collect_params()
    assert all((p.grad_req == 'null') == key.startswith("d_model.") for key, p in P.items() if p.span is not None)
    assert P["d_model.features.0.3.conv.weight"].grad_req == 'null'
    assert all(lo >= net._params["yolo_blocks.0.body.0.0.weight"].span[0] for lo, _, _, _ in net._optimizer_ranges())
    net = _mk([21, 21, 2, 2, 2, 2])
    net.collect_params()["d_model.features.1.3.conv.weight"].lr_mult = 0.5
    assert any(r[2] == 0.5 for r in net._optimizer_ranges())
def test_library_exports_the_temporal_conv_kernels():
    from viddet_amd import lib as L
    lib = L.load()
    for name in ("vd_tdw_fwd", "vd_tdw_bwd", "vd_tdw_bwd_ws_bytes"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.vd_abi_version() == 8 == L.ABI_VERSION
    # argument checks run before any launch: no GPU is touched
    err = lambda: lib.vd_last_error()
    assert lib.vd_tdw_fwd(None, 16, None, 16, 2, 3, 35, 32, None, None) == -1 and b"vd_tdw_fwd" in err()   # x NULL
    assert lib.vd_tdw_fwd(16, None, None, 16, 2, 3, 35, 32, None, None) == -1                              # w NULL
    assert lib.vd_tdw_fwd(16, 16, None, None, 2, 3, 35, 32, None, None) == -1                              # y NULL
    assert lib.vd_tdw_fwd(16, 16, None, 16, 2, 1, 35, 32, None, None) == -1 and b"K >= 2" in err()
    assert lib.vd_tdw_fwd(16, 16, None, 16, 2, 3, 35, 30, None, None) == -1 and b"multiple of 4" in err()
    assert lib.vd_tdw_fwd(16, 16, None, 16, 0, 3, 35, 32, None, None) == -1
    assert lib.vd_tdw_fwd(16, 16, None, 16, 2, 3, 0, 32, None, None) == -1
    assert lib.vd_tdw_fwd(16, 16, 8, 16, 2, 3, 35, 32, None, None) == -1 and b"aligned" in err()
    need = lib.vd_tdw_bwd_ws_bytes(2, 3, 35, 32)
    assert need > 0 and need % (3 * 32 * 4) == 0
    assert lib.vd_tdw_bwd_ws_bytes(2, 1, 35, 32) == 0 and lib.vd_tdw_bwd_ws_bytes(2, 3, 35, 30) == 0
    assert lib.vd_tdw_bwd(None, 16, 16, 16, 16, 2, 3, 35, 32, 16, need, None) == -1 and b"vd_tdw_bwd" in err()   # dy NULL
    assert lib.vd_tdw_bwd(16, 16, 16, None, None, 2, 3, 35, 32, 16, need, None) == -1                              # nothing to write
    assert lib.vd_tdw_bwd(16, None, 16, 16, 16, 2, 3, 35, 32, 16, need, None) == -1 and b"dw needs x" in err()
    assert lib.vd_tdw_bwd(16, 16, 16, 16, 16, 2, 1, 35, 32, 16, need, None) == -1 and b"K >= 2" in err()
    assert lib.vd_tdw_bwd(16, 16, 16, 16, 16, 2, 3, 35, 34, 16, need, None) == -1
    assert lib.vd_tdw_bwd(16, 16, 16, 16, 16, 2, 3, 35, 32, 16, need - 1, None) == -1 and b"workspace" in err()
    assert lib.vd_tdw_bwd(16, 16, 16, 16, 16, 2, 3, 35, 32, None, 0, None) == -1


def test_scripts_pass_conv_types(monkeypatch):
    import train_yolov3 as T
    seen = {}

    class _Net:
        def initialize(self, **kw):
            pass

    def fake(which):
        def f(classes, **kw):
            seen.clear()
            seen.update(kw, factory=which)
            return _Net()
        return f

    monkeypatch.setattr(T, "yolo3_darknet53", fake("2d"))
    monkeypatch.setattr(T, "yolo3_3ddarknet", fake("3d"))
    base = ["--dataset", "vid"]
    monkeypatch.setattr(T, "FLAGS", T.parse_flags(base + ["--conv_types", "21,21,2,2,2,2", "--window", "3,1"]))
    T.get_net(["a"], (0, 1))
    assert seen["factory"] == "3d" and seen["conv_types"] == [21, 21, 2, 2, 2, 2] and seen["k"] == 3
    monkeypatch.setattr(T, "FLAGS", T.parse_flags(base))
    T.get_net(["a"], (0, 1))
    assert seen["factory"] == "2d" and "conv_types" not in seen
    monkeypatch.setattr(T, "FLAGS", T.parse_flags(base + ["--conv_types", "2,2,2,2,2,2", "--window", "3,1", "--k_join_type", "max",
                                                          "--k_join_pos", "early"]))
    T.get_net(["a"], (0, 1))
    assert seen["factory"] == "2d" and seen["k"] == 3
    ct = ["--conv_types", "21,2,2,2,2,2", "--window", "3,1"]
    refused = [(["--k_join_type", "max"], "k_join_type"), (["--k_join_pos", "late"], "k_join_pos"), (["--rnn_pos", "late"], "rnn_pos"),
               (["--corr_pos", "late"], "corr_pos"), (["--temp"], "temp"), (["--mult_out"], "mult_out"),
               (["--features_dir", "x"], "features_dir"), (["--mixup"], "mixup"), (["--storage", "bf16"], "storage")]
    for extra, word in refused:
        monkeypatch.setattr(T, "FLAGS", T.parse_flags(base + ct + extra))
        with pytest.raises(NotImplementedError, match="--%s" % word):
            T.get_net(["a"], (0, 1))
    for bad, msg in ((["--conv_types", "3,2,2,2,2,2", "--window", "3,1"], "conv_types 3"),
                     (["--conv_types", "21,2,2,2,2,2"], "K = 1 is refused"),
                     (["--conv_types", "2,21,2,2,2,2", "--window", "3,1"], "21 after a 2")):
        monkeypatch.setattr(T, "FLAGS", T.parse_flags(base + bad))
        with pytest.raises(NotImplementedError, match=msg):
            T.get_net(["a"], (0, 1))
    # detect_yolo3.py: refusals come before its GPU check, an accepted combination gets as far as that check
    import detect_yolo3 as Dt
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit):
        Dt.main(ct)
    with pytest.raises(NotImplementedError, match="--precision"):
        Dt.main(ct + ["--precision", "bf16"])
    with pytest.raises(NotImplementedError, match="--rnn_pos"):
        Dt.main(ct + ["--rnn_pos", "late"])
    with pytest.raises(NotImplementedError, match="conv_types 3"):
        Dt.main(["--conv_types", "3,3,2,2,2,2", "--window", "3,1"])
    import extract_base_features as E
    with pytest.raises(NotImplementedError, match="conv_types"):
        E.main(["--conv_types", "21,2,2,2,2,2"])
