"""The correlation join on the MI355X: vd_corr_fwd / vd_corr_bwd / vd_corr_fwd_bf16 against the fp64 restatement
(tests/corr_oracle.py), the corr_pos networks against the fp64 oracle (the pattern of tests/test_temporal_gpu.py), their
bf16 inference, HIP-graph capture, and train_yolov3.py / detect_yolo3.py with --corr_pos."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import yolo as Y
from tests import corr_oracle as CO
from tests.util import dev, maxdiff, boxes_close

pytestmark = pytest.mark.gpu


def _ldy(K, C, d):
    return -(-CO.corr_channels(K, C, d) // 64) * 64


def _run_fwd(x5, d, bf16=False):
    """x5 (B, K, C, H, W) numpy -> device y (B, H, W, ldy) via vd_corr_fwd[_bf16]"""
    from viddet_amd import lib as L
    B, K, C, H, W = x5.shape
    ldy = _ldy(K, C, d)
    dt = torch.bfloat16 if bf16 else torch.float32
    x = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x5, 2, -1))).to(dt).cuda().reshape(B * K, H, W, C)
    y = torch.full((B, H, W, ldy), float('nan'), dtype=dt, device='cuda')
    fn = L.load().vd_corr_fwd_bf16 if bf16 else L.load().vd_corr_fwd
    L.check(fn(x.data_ptr(), y.data_ptr(), B, K, H, W, C, d, ldy, L.stream_ptr()), "vd_corr_fwd")
    return x, y


def _run_bwd(x, g, B, K, H, W, C, d):
    from viddet_amd import lib as L
    dx = torch.full((B * K, H, W, C), float('nan'), device='cuda')
    L.check(L.load().vd_corr_bwd(g.data_ptr(), x.data_ptr(), dx.data_ptr(), B, K, H, W, C, d, g.shape[-1], L.stream_ptr()),
            "vd_corr_bwd")
    return dx


KERNEL_CASES = [(2, 32, 2, 2, 4), (3, 256, 13, 13, 4), (5, 32, 7, 11, 1), (3, 1024, 13, 13, 0), (2, 256, 9, 5, 1),
                (3, 256, 52, 52, 4), (5, 256, 2, 2, 0), (3, 32, 13, 13, 1)]


@pytest.mark.parametrize("K,C,H,W,d", KERNEL_CASES)
def test_corr_kernels_against_the_restatement(K, C, H, W, d):
    B = 2
    rng = np.random.default_rng(K * 1000 + C + d)
    x5 = rng.standard_normal((B, K, C, H, W)).astype(np.float32).astype(np.float64)
    yr, bw = CO.corr(x5, d)
    x, y = _run_fwd(x5, d)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    Cc = yr.shape[1]
    ref = np.moveaxis(yr, 1, -1)
    assert np.array_equal(got[..., :K * C], ref[..., :K * C]), "the 'cat' channels are a copy"
    assert np.all(got[..., Cc:] == 0), "pad channels"
    sc = max(1e-6, float(np.abs(ref[..., K * C:]).max()))
    assert maxdiff(got[..., K * C:Cc], ref[..., K * C:]) <= 1e-5 * sc
    # backward
    g = rng.standard_normal(yr.shape).astype(np.float32).astype(np.float64)
    dr = bw(g)                                                 # (B, K, C, H, W)
    gd = torch.zeros((B, H, W, y.shape[-1]), device='cuda')
    gd[..., :Cc] = torch.from_numpy(np.moveaxis(g, 1, -1)).float().cuda()
    dx = _run_bwd(x, gd, B, K, H, W, C, d)
    dx2 = _run_bwd(x, gd, B, K, H, W, C, d)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2), "two backward runs are bit-identical"
    gotd = np.moveaxis(dx.cpu().numpy().reshape(B, K, H, W, C), -1, 2)
    mid = K // 2
    for t in range(K):
        s = max(1e-6, float(np.abs(dr[:, t]).max()))
        assert maxdiff(gotd[:, t], dr[:, t]) <= 1e-5 * s, ("centre" if t == mid else "side", t)


@pytest.mark.parametrize("K,C,H,W,d", [(3, 256, 13, 13, 4), (2, 64, 9, 7, 1)])
def test_corr_bf16_forward(K, C, H, W, d):
    B = 2
    rng = np.random.default_rng(3)
    x5 = torch.from_numpy(rng.standard_normal((B, K, C, H, W))).to(torch.bfloat16).double().numpy()   # bf16-representable
    yr, _ = CO.corr(x5, d)
    _, y = _run_fwd(x5, d, bf16=True)
    torch.cuda.synchronize()
    got = y.float().cpu().numpy()
    ref = np.moveaxis(yr, 1, -1)
    Cc = yr.shape[1]
    assert np.array_equal(got[..., :K * C], ref[..., :K * C]) and np.all(got[..., Cc:] == 0)
    sc = float(np.abs(ref[..., K * C:]).max())
    assert maxdiff(got[..., K * C:Cc], ref[..., K * C:]) <= sc * 2 ** -8 + 1e-6   # one bf16 rounding of the output


def _mk(c, k, pos, d, seed):
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(c)], k=k, corr_pos=pos, corr_d=d)
    P = CO.init_params(c, k, pos, d, seed=seed, obj_bias=-1.0)
    assert set(P) == set(net.collect_params().keys())
    for key, p in net.collect_params().items():
        assert tuple(P[key].shape) == p.shape, (key, P[key].shape, p.shape)
        p.set_data(torch.from_numpy(P[key].astype(np.float32)))
    return net, P


def _padded_columns(net):
    """the packed weight rows' zero tails of every consumer of a correlation join"""
    from viddet_amd.model import ConvNode
    out = []
    for n in net.conv_nodes:
        if n.cin != n.ref_cin:
            w = n.wp.view(-1, n.cin)[:n.cout]
            out.append((n.name, w[:, n.ref_cin:]))
    return out


NET_CFGS = [(3, "early", 0), (3, "early", 4), (3, "late", 0), (3, "late", 4), (2, "late", 1)]


@pytest.mark.parametrize("k,pos,d", NET_CFGS)
def test_corr_network_inference_and_training(k, pos, d):
    c, b, size = 3, 2, 64
    net, P = _mk(c, k, pos, d, 43)
    rng = np.random.default_rng(43)
    x = rng.standard_normal((b, k, 3, size, size)).astype(np.float32)
    onet = CO.CorrNet(P, c, k, pos, d)
    ids_r, sc_r, bx_r, rows_r, heads_r = onet.detect(x.astype(np.float64))
    ids, sc, bx = net(dev(x))
    torch.cuda.synchronize()
    bufs = net._programs[('buf', b, size, size, False)]
    for s, hname in enumerate(net.head_names):
        got = bufs[hname].cpu().numpy()[..., :3 * (5 + c)]
        assert maxdiff(got, np.moveaxis(heads_r[s], 1, -1)) < 1e-3, "head %d" % s
    from tests.util import assert_rows_match, take_ranks
    perm = assert_rows_match(net.last_rows.cpu().numpy(), rows_r, sc_r)
    assert maxdiff(take_ranks(sc, perm), sc_r) < 1e-3 and boxes_close(take_ranks(bx, perm), bx_r)
    # one training step against the oracle
    gt = np.array([[[5., 8., 40., 50.], [-1, -1, -1, -1]], [[10., 12., 30., 28.], [20., 5., 60., 62.]]])
    gid = np.array([[[1.], [-1.]], [[0.], [2.]]])
    tg = Y.prefetch_targets(size, size, [size // 32, size // 16, size // 8], gt, gid, c)
    out = net(dev(x), dev(gt), *[dev(t) for t in tg])
    net.backward()
    torch.cuda.synchronize()
    tb = net._programs[('buf', b, size, size, True)]
    from tests.util import device_leaky_masks
    onet.mask_override = device_leaky_masks(net, tb)
    losses_r, G, heads_t = onet.train_step(x.astype(np.float64), gt, *tg)
    for i in range(4):
        assert np.all(np.abs(out[i].cpu().numpy() - losses_r[i]) <= 2e-3 * np.maximum(1.0, np.abs(losses_r[i])))
    for key, v in onet.new_running.items():
        assert maxdiff(net.collect_params()[key].data().cpu().numpy(), v) < 1e-4, key
    bad = []
    for key, gref in G.items():
        got = net.collect_params()[key].grad().cpu().numpy()
        scale = max(1e-3, float(np.abs(gref).max()))
        if maxdiff(got, gref) / scale >= 5e-4:
            bad.append((key, maxdiff(got, gref) / scale))
    assert not bad, bad[:6]
    # the zero tails stay exactly zero through an SGD step with momentum and weight decay: their inputs are exact zeros
    padded = _padded_columns(net)
    assert len(padded) == 3 and all(bool((w == 0).all()) for _, w in padded)
    net.sgd_step(1e-3, 0.9, 5e-4, b)
    net.sgd_step(1e-3, 0.9, 5e-4, b)
    torch.cuda.synchronize()
    for name, w in _padded_columns(net):
        assert bool((w == 0).all()), name
    for n in net.conv_nodes:
        if n.cin != n.ref_cin:
            g_ = n.gwp.view(-1, n.cin)[:n.cout, n.ref_cin:]
            assert bool((g_ == 0).all()), n.name


def test_corr_network_bf16_inference_and_capture():
    c, b, size, k = 3, 2, 64, 3
    net, P = _mk(c, k, "early", 4, 47)
    rng = np.random.default_rng(47)
    x = rng.standard_normal((b, k, 3, size, size)).astype(np.float32)
    a = [t.clone() for t in net(dev(x))]
    net.use_graphs = True
    g1 = [t.clone() for t in net(dev(x))]
    g2 = [t.clone() for t in net(dev(x))]
    torch.cuda.synchronize()
    for u, v, w in zip(a, g1, g2):
        assert torch.equal(u, v) and torch.equal(u, w)
    net.use_graphs = False
    _, _, _, _, heads_r = CO.CorrNet(P, c, k, "early", 4).detect(x.astype(np.float64))
    net.set_precision('bf16')
    net(dev(x))
    torch.cuda.synchronize()
    b16 = net._programs[('infer_bf16', b, size, size)][1]
    for s, hname in enumerate(net.head_names):
        ref = np.moveaxis(heads_r[s], 1, -1)
        got = b16[hname][..., :3 * (5 + c)].float().cpu().numpy()
        rel = maxdiff(got, ref) / float(np.abs(ref).max())
        assert rel < 3e-2, (hname, rel)               # tests/test_bf16_gpu.py's network bound


@pytest.mark.parametrize("pos,d", [("late", 4), ("early", 0)])
def test_corr_scripts_train_then_detect(tmp_path, monkeypatch, pos, d):
    import train_yolov3 as T
    import detect_yolo3 as D
    monkeypatch.chdir(tmp_path)
    flags = ["--window", "3,1", "--corr_pos", pos, "--corr_d", str(d)]
    net = T.main(["--dataset", "vid", "--batch_size", "2", "--data_shape", "64", "--epochs", "1", "--synthetic_samples", "4",
                  "--save_prefix", "c", "--log_interval", "1", "--no_random_shape"] + flags)
    ref = CO.param_shapes(len(net.classes), 3, pos, d)
    assert {key: p.shape for key, p in net.collect_params().items()} == {key: tuple(s) for key, s in ref.items()}
    cks = sorted(glob.glob(str(tmp_path / "models" / "experiments" / "c" / "*.params")))
    assert cks, os.listdir(str(tmp_path))
    D.main(["--model_path", cks[-1], "--dataset", "vid", "--batch_size", "2", "--data_shape", "64", "--synthetic_samples", "4",
            "--save_dir", str(tmp_path / "results"), "--save_prefix", "c1"] + flags)
    rows = glob.glob(str(tmp_path / "results" / "c1" / "pred" / "*"))
    assert rows
