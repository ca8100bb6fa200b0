"""The correlation join without a GPU: the fp64 restatement (tests/corr_oracle.py) against an independent torch autograd
form and against explicit loops, and the yolo3_darknet53 corr_pos / corr_d flag table (yolo3.py:959-1180)."""
import numpy as np
import pytest
import torch

from tests import corr_oracle as CO


def _torch_corr(x5, d):
    """explicit shifts of the zero-padded centre frame; autograd supplies the gradients"""
    B, K, C, H, W = x5.shape
    mid, D = K // 2, 2 * d + 1
    xp = torch.nn.functional.pad(x5[:, mid], (d, d, d, d))
    outs = [x5.reshape(B, K * C, H, W)]
    for t in range(K):
        if t == mid:
            continue
        for dy in range(-d, d + 1):
            for dx in range(-d, d + 1):
                sh = xp[:, :, d + dy:d + dy + H, d + dx:d + dx + W]
                outs.append((x5[:, t] * sh).mean(dim=1, keepdim=True))
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("K,C,H,W,d", [(3, 4, 5, 7, 1), (2, 8, 6, 6, 2), (3, 4, 2, 2, 4), (5, 4, 3, 4, 0), (3, 2, 4, 3, 3)])
def test_corr_restatement_matches_autograd(K, C, H, W, d):
    rng = np.random.default_rng(K * 100 + d)
    x = rng.standard_normal((2, K, C, H, W))
    y, bw = CO.corr(x, d)
    assert y.shape == (2, CO.corr_channels(K, C, d), H, W)
    xt = torch.tensor(x, requires_grad=True)
    yt = _torch_corr(xt, d)
    np.testing.assert_allclose(y, yt.detach().numpy(), rtol=0, atol=1e-12)
    g = rng.standard_normal(y.shape)
    yt.backward(torch.tensor(g))
    dx = bw(g)
    np.testing.assert_allclose(dx, xt.grad.numpy(), rtol=0, atol=1e-12)
    mid = K // 2
    assert np.abs(dx[:, mid]).max() > 0 and np.abs(dx[:, [t for t in range(K) if t != mid]]).max() > 0


def test_corr_channel_order_and_zeros_by_loops():
    K, C, H, W, d = 3, 3, 2, 2, 4                   # d larger than the map: most displacements fall outside it
    D = 2 * d + 1
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, K, C, H, W))
    y, _ = CO.corr(x, d)
    assert np.array_equal(y[:, :K * C], x.reshape(1, K * C, H, W))
    for i, t in enumerate([0, 2]):
        for dy in range(-d, d + 1):
            for dx in range(-d, d + 1):
                ch = K * C + i * D * D + (dy + d) * D + (dx + d)     # vertical offset = the slow index
                for yy in range(H):
                    for xx in range(W):
                        v = 0.0
                        if 0 <= yy + dy < H and 0 <= xx + dx < W:
                            v = sum(x[0, t, c, yy, xx] * x[0, 1, c, yy + dy, xx + dx] for c in range(C)) / C
                        assert abs(y[0, ch, yy, xx] - v) < 1e-12, (t, dy, dx, yy, xx)
    # of the 81 maps of a 2x2 map only the 3x3 displacements around 0 can reach another pixel
    far = [K * C + (dy + d) * D + (dx + d) for dy in range(-d, d + 1) for dx in range(-d, d + 1) if max(abs(dy), abs(dx)) > 1]
    assert np.all(y[:, far] == 0)


def _graph_param_shapes(net):
    from viddet_amd.model import ConvNode
    return {k: tuple(p.shape) for k, p in net.collect_params().items()} if net is not None else None


def _mk(**kw):
    from viddet_amd.model import yolo3_darknet53
    return yolo3_darknet53(["c%d" % i for i in range(3)], device="cpu", **kw)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("pos", ["early", "late"])
@pytest.mark.parametrize("d", [0, 4])
def test_corr_factory_names_and_shapes(k, pos, d):
    net = _mk(k=k, corr_pos=pos, corr_d=d)
    got = _graph_param_shapes(net)
    ref = CO.param_shapes(3, k, pos, d)
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))[:6]
    for key, shp in ref.items():
        assert got[key] == tuple(shp), (key, got[key], shp)
    # the consumers read ldy = round_up(Cc, 64) channels on the device; the reference shape is what the parameter shows
    from viddet_amd.model import CorrNode, ConvNode
    corr_nodes = [n for n in net.nodes if isinstance(n, CorrNode)]
    assert len(corr_nodes) == 3
    for n in corr_nodes:
        assert n.ldy % 64 == 0 and n.ldy >= n.Cc == CO.corr_channels(k, n.C, d)
        users = [m for m in net.nodes if isinstance(m, ConvNode) and m.src == n.dst]
        assert all(m.cin == n.ldy and m.ref_cin == n.Cc for m in users)
    # k_join_type is not read when corr_pos builds the join (the reference's `elif`)
    net2 = _mk(k=k, corr_pos=pos, corr_d=d, k_join_type='max')
    assert _graph_param_shapes(net2) == got


def test_corr_channel_counts_of_the_issue():
    assert CO.corr_channels(3, 256, 4) == 930 and CO.corr_channels(3, 256, 0) == 770


def test_corr_flag_table():
    plain = _graph_param_shapes(_mk(k=1))
    assert _graph_param_shapes(_mk(k=1, corr_pos='early', corr_d=4)) == plain       # no Corr at k = 1
    assert _graph_param_shapes(_mk(k=1, corr_pos='late', corr_d=4)) == plain
    # the same position for the join and corr: the join network, Corr never called
    for pos in ('early', 'late'):
        a = _graph_param_shapes(_mk(k=3, k_join_type='cat', k_join_pos=pos))
        assert _graph_param_shapes(_mk(k=3, k_join_type='cat', k_join_pos=pos, corr_pos=pos, corr_d=4)) == a
        from viddet_amd.model import CorrNode
        assert not any(isinstance(n, CorrNode) for n in _mk(k=3, k_join_type='max', k_join_pos=pos, corr_pos=pos).nodes)
    with pytest.raises(NotImplementedError):
        _mk(k=3, k_join_type='cat', k_join_pos='early', corr_pos='late')
    with pytest.raises(NotImplementedError):
        _mk(k=3, k_join_type='max', k_join_pos='late', corr_pos='early')
    with pytest.raises(NotImplementedError):
        _mk(k=3)                                                                    # neither a join nor corr
    with pytest.raises(AssertionError):
        _mk(k=3, corr_pos='late', block_conv_type='3')                              # yolo3.py:980 needs k_join_pos 'late'
    with pytest.raises(NotImplementedError):
        _mk(k=5, temporal=True, t_out=True, corr_d=4)                               # YOLOV3Temporal's branch stays out


def test_scripts_pass_corr_flags(monkeypatch):
    import train_yolov3 as T
    seen = {}

    class _Net:
        def initialize(self, **kw):
            pass

    def fake(classes, **kw):
        seen.update(kw)
        return _Net()

    monkeypatch.setattr(T, "yolo3_darknet53", fake)
    monkeypatch.setattr(T, "FLAGS", T.parse_flags(["--dataset", "vid", "--window", "3,1", "--corr_pos", "late", "--corr_d", "4"]))
    T.get_net(["a"], (0, 1))
    assert seen["corr_pos"] == "late" and seen["corr_d"] == 4 and seen["k"] == 3
    monkeypatch.setattr(T, "FLAGS", T.parse_flags(["--dataset", "vid", "--window", "3,1", "--corr_pos", "early"]))
    T.get_net(["a"], (0, 1))
    assert seen["corr_pos"] == "early" and seen["corr_d"] == 0                      # the reference's training default
    import detect_yolo3 as Dt
    assert Dt.parse_flags(["--corr_pos", "late"]).corr_d == 4                       # the reference's detection default
    # the flag no longer stops the script: it gets as far as its GPU check
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit):
        Dt.main(["--window", "3,1", "--corr_pos", "late", "--corr_d", "4"])
