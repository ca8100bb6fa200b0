"""The bidirectional ConvGRU of temporal windows on the MI355X: the gate kernels (vd_gru.hip) against the fp64 restatement
's equations written out in NumPy, the rnn_pos networks against the fp64 oracle (the pattern of tests/test_corr_gpu.py), their zero pad
channels, frozen parameters, --no_wd, HIP-graph capture, and train_yolov3.py / detect_yolo3.py with --rnn_pos."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import yolo as Y
from tests import rnn_oracle as RO
from tests.util import dev, maxdiff, boxes_close

pytestmark = pytest.mark.gpu


def _sig(a):
    return 1.0 / (1.0 + np.exp(-a))


# (B, HW, Ch): M = B * HW rows from 2 * 2^2 x 32 up to 2 * 52^2 x 256 and 16 * 13^2 x 1024
GATE_CASES = [(2, 4, 32), (2, 49, 96), (3, 35, 64), (2, 2704, 256), (16, 169, 1024)]


@pytest.mark.parametrize("B,HW,Ch", GATE_CASES)
@pytest.mark.parametrize("state", [True, False])
def test_gate_kernels_against_the_restatement(B, HW, Ch, state):
    _gate_case(B, HW, Ch, state, 3, 1)


@pytest.mark.parametrize("K,t", [(1, 0), (2, 0), (2, 1), (5, 0), (5, 4)])
@pytest.mark.parametrize("state", [True, False])
def test_gate_kernels_index_every_frame_of_the_folded_tensors(K, t, state):
    """frame t of I and dy is row block b * K + t: the first and the last frame of a window, and a window of one"""
    _gate_case(3, 35, 64, state, K, t)


def _gate_case(B, HW, Ch, state, K, t):
    """one forward and two backward launches on frame t of K against the cell's equations in fp64 NumPy (written out here,
    independent of tests/rnn_oracle.py); tolerance 1e-5 x the reference array's max-abs"""
    from viddet_amd import lib as L
    lib = L.load()
    rng = np.random.default_rng(B * 1000 + Ch + int(state) + 7 * K + t)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    I = f32(rng.standard_normal((B, K, HW, 3 * Ch)))
    H = f32(rng.standard_normal((B * HW, 3 * Ch)))
    bh = f32(rng.standard_normal(3 * Ch))
    hp = f32(rng.uniform(-1, 1, (B * HW, Ch))) if state else np.zeros((B * HW, Ch))
    It = I[:, t].reshape(B * HW, 3 * Ch)
    Hv = H if state else np.broadcast_to(bh, H.shape)
    r, z = _sig(It[:, :Ch] + Hv[:, :Ch]), _sig(It[:, Ch:2 * Ch] + Hv[:, Ch:2 * Ch])
    Ho = Hv[:, 2 * Ch:]
    n = np.tanh(It[:, 2 * Ch:] + r * Ho)
    h_ref = (1 - z) * n + z * hp
    dI_ = torch.from_numpy(I).float().cuda().contiguous()
    dH_ = torch.from_numpy(H).float().cuda() if state else torch.full((B * HW, 3 * Ch), float('nan'), device='cuda')
    dbh, dhp = torch.from_numpy(bh).float().cuda(), torch.from_numpy(hp).float().cuda()
    h = torch.full((B * HW, Ch), float('nan'), device='cuda')
    L.check(lib.vd_gru_gate_fwd(dI_.data_ptr(), dH_.data_ptr() if state else None, dbh.data_ptr(), dhp.data_ptr() if state else None,
                                h.data_ptr(), B, K, t, HW, Ch, L.stream_ptr()), "vd_gru_gate_fwd")
    torch.cuda.synchronize()
    print("fwd max err / max-abs", maxdiff(h.cpu().numpy(), h_ref) / np.abs(h_ref).max())
    assert maxdiff(h.cpu().numpy(), h_ref) <= 1e-5 * np.abs(h_ref).max()
    # backward: dh = dy / 2 + carry
    dy = f32(rng.standard_normal((B, K, HW, Ch)))
    carry = f32(rng.standard_normal((B * HW, Ch)))
    g = dy[:, t].reshape(B * HW, Ch) / 2 + carry
    da = g * (1 - z) * (1 - n * n)
    drp, dzp = da * Ho * r * (1 - r), g * (hp - n) * z * (1 - z)
    ref = dict(dI=np.concatenate([drp, dzp, da], axis=1), dH=np.concatenate([drp, dzp, da * r], axis=1), dh=g * z)
    ddy = torch.from_numpy(dy).float().cuda().contiguous()
    runs = []
    for _ in range(2):
        Ib = dI_.clone()
        Hb = dH_.clone()
        dh = torch.from_numpy(carry).float().cuda()
        L.check(lib.vd_gru_gate_bwd(Ib.data_ptr(), Hb.data_ptr(), 1 if state else 0, dbh.data_ptr(), dhp.data_ptr() if state else None,
                                    ddy.data_ptr(), 0.5, dh.data_ptr(), 1, B, K, t, HW, Ch, L.stream_ptr()), "vd_gru_gate_bwd")
        runs.append((Ib, Hb, dh))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two backward runs are bit-identical"
    Ib, Hb, dh = runs[0]
    got_dI = Ib.cpu().numpy().reshape(B, K, HW, 3 * Ch)
    other = [u for u in range(K) if u != t]
    assert np.array_equal(got_dI[:, other], I[:, other].astype(np.float32)), "the other frames of I are untouched"
    got = dict(dI=got_dI[:, t].reshape(B * HW, 3 * Ch), dH=Hb.cpu().numpy())
    if state:
        got['dh'] = dh.cpu().numpy()
    else:
        assert np.array_equal(dh.cpu().numpy(), carry.astype(np.float32)), "no state: dh is not written"
    for key, v in got.items():
        print(key, "max err / max-abs", maxdiff(v, ref[key]) / np.abs(ref[key]).max())
        assert maxdiff(v, ref[key]) <= 1e-5 * np.abs(ref[key]).max(), key


def test_gru_avg_folds_the_two_directions():
    from viddet_amd import lib as L
    B, K, inner = 3, 5, 7 * 32
    rng = np.random.default_rng(1)
    hl, hr = rng.standard_normal((K, B, inner)).astype(np.float32), rng.standard_normal((K, B, inner)).astype(np.float32)
    y = torch.full((B * K, inner), float('nan'), device='cuda')
    am = torch.zeros(L.AMAX_FLOATS, device='cuda')
    a, b = torch.from_numpy(hl).cuda(), torch.from_numpy(hr).cuda()
    L.check(L.load().vd_gru_avg(a.data_ptr(), b.data_ptr(), y.data_ptr(), B, K, inner, am.data_ptr(), L.stream_ptr()), "vd_gru_avg")
    torch.cuda.synchronize()
    ref = np.stack([[(hl[t, bb] + hr[K - 1 - t, bb]) * np.float32(0.5) for t in range(K)] for bb in range(B)]).reshape(B * K, inner)
    assert np.array_equal(y.cpu().numpy(), ref)
    from viddet_amd import ops
    assert ops.amax_value(am) == float(np.abs(ref).max())


def _mk(c, k, pos, jt, seed):
    from viddet_amd.model import yolo3_darknet53
    net = yolo3_darknet53(["c%d" % i for i in range(c)], k=k, k_join_type=jt, k_join_pos='late', rnn_pos=pos)
    P = RO.init_params(c, k, pos, jt, seed=seed, obj_bias=-1.0)
    assert set(P) == set(net.collect_params().keys())
    for key, p in net.collect_params().items():
        assert tuple(P[key].shape) == p.shape, (key, P[key].shape, p.shape)
        p.set_data(torch.from_numpy(P[key].astype(np.float32)))
    return net, P


def _pads(net):
    """every device element of the GRU arrays (weights, gradients, momentum) that belongs to a pad channel"""
    out = []
    for g in net.gru_nodes:
        if g.chp == g.ch:
            continue
        for _, i2h, h2h in g.cells:
            for cn in (i2h, h2h):
                for arena in (net.weights, net.grads, net.momentum_buf):
                    w = arena[cn.w_off:cn.w_off + cn.w_numel].view(3, g.chp, cn.T, cn.cin)
                    out.append(w[:, g.ch:])
                    if cn is h2h:
                        out.append(w[:, :, :, g.ch:])
                    out.append(arena[cn.bias_off:cn.bias_off + cn.co_pad].view(3, g.chp)[:, g.ch:])
    return out


NET_CFGS = [(3, "late", "max"), (3, "late", "cat"), (2, "late", "mean"), (5, "late", "max"), (3, "out", "max"), (3, "out", "mean")]


@pytest.mark.parametrize("k,pos,jt", NET_CFGS)
def test_rnn_network_inference_and_training(k, pos, jt):
    c, b, size = 3, 2, 64
    net, P = _mk(c, k, pos, jt, 53)
    rng = np.random.default_rng(53)
    x = rng.standard_normal((b, k, 3, size, size)).astype(np.float32)
    onet = RO.RnnNet(P, c, k, pos, jt)
    ids_r, sc_r, bx_r, rows_r, heads_r = onet.detect(x.astype(np.float64))
    ids, sc, bx = net(dev(x))
    torch.cuda.synchronize()
    bufs = net._programs[('buf', b, size, size, False)]
    for s, hname in enumerate(net.head_names):
        got = bufs[hname].cpu().numpy()
        print("head", s, "max err", maxdiff(got[..., :3 * (5 + c)], np.moveaxis(heads_r[s], 1, -1)))
        assert maxdiff(got[..., :3 * (5 + c)], np.moveaxis(heads_r[s], 1, -1)) < 1e-3, "head %d" % s
        assert np.all(got[..., 3 * (5 + c):] == 0), "pad channels of head %d" % s
    from tests.util import assert_rows_match, take_ranks
    perm = assert_rows_match(net.last_rows.cpu().numpy(), rows_r, sc_r)
    assert maxdiff(take_ranks(sc, perm), sc_r) < 1e-3 and boxes_close(take_ranks(bx, perm), bx_r)
    # fp32 inference under a captured graph is bit-equal to the plain launch loop
    plain = [t.clone() for t in (ids, sc, bx)]
    net.use_graphs = True
    g1 = [t.clone() for t in net(dev(x))]
    g2 = [t.clone() for t in net(dev(x))]
    torch.cuda.synchronize()
    net.use_graphs = False
    for u, v, w in zip(plain, g1, g2):
        assert torch.equal(u, v) and torch.equal(u, w)
    # one training step against the oracle
    gt = np.array([[[5., 8., 40., 50.], [-1, -1, -1, -1]], [[10., 12., 30., 28.], [20., 5., 60., 62.]]])
    gid = np.array([[[1.], [-1.]], [[0.], [2.]]])
    tg = Y.prefetch_targets(size, size, [size // 32, size // 16, size // 8], gt, gid, c)
    out = net(dev(x), dev(gt), *[dev(t) for t in tg])
    net.backward()
    torch.cuda.synchronize()
    tb = net._programs[('buf', b, size, size, True)]
    from tests.util import device_leaky_masks, check_masks_differ_only_at_ties
    from viddet_amd.model import PoolNode
    onet.mask_override = device_leaky_masks(net, tb)
    for n in net.nodes:                                      # the max join's winner among the K frames, borrowed at ties
        if isinstance(n, PoolNode) and n.type == 0:
            am = np.moveaxis(tb['am:' + n.dst].cpu().numpy().astype(np.int64), -1, 1)
            onet.argmax_override[n.name] = am[:, :onet_channels(onet, n, c)]
    losses_r, G, heads_t = onet.train_step(x.astype(np.float64), gt, *tg)
    check_masks_differ_only_at_ties(onet.pre, onet.mask_override)
    for name, (am, v5) in onet.argmax_natural.items():
        if name in onet.argmax_override:
            d = am != onet.argmax_override[name]
            if d.any():      # a different winner is only acceptable between (numerically) equal candidates
                a = np.take_along_axis(v5, am[:, None], axis=1)[:, 0]
                bwin = np.take_along_axis(v5, onet.argmax_override[name][:, None], axis=1)[:, 0]
                assert np.abs(a - bwin)[d].max() < 2e-4, name
    for i in range(4):
        assert np.all(np.abs(out[i].cpu().numpy() - losses_r[i]) <= 2e-3 * np.maximum(1.0, np.abs(losses_r[i])))
    for key, v in onet.new_running.items():
        assert maxdiff(net.collect_params()[key].data().cpu().numpy(), v) < 1e-4, key
    assert set(G) == {key for key, p in net.collect_params().items() if p.span is not None}
    bad, worst = [], 0.0
    for key, gref in G.items():
        got = net.collect_params()[key].grad().cpu().numpy()
        scale = max(1e-3, float(np.abs(gref).max()))
        if ".rnn." in key:
            worst = max(worst, maxdiff(got, gref) / scale)
        if maxdiff(got, gref) / scale >= 5e-4:
            bad.append((key, maxdiff(got, gref) / scale))
    print("worst GRU gradient error / max:", worst)
    assert not bad, bad[:6]
    # the convs that read the state or a gate gradient never run the fp16 split (no max-abs slots: range-exact arithmetic)
    from viddet_amd import lib as L
    gru_w = {cn.wamax.data_ptr() for cn in net.conv_nodes if hasattr(cn, 'pw')}
    nrec = 0
    for prog in [net._programs[('infer', b, size, size)][0]] + net._last_train['fwd'] + net._last_train['bwd']:
        for fname, _, args in prog.recs:
            if fname == 'vd_conv_igemm' and int(args[0]._obj.amax_w or 0) in gru_w and not args[0]._obj.amax_in:
                nrec += 1
                assert not (args[0]._obj.flags & L.MATH_F16X2)
            if fname == 'vd_conv_wgrad' and not args[0]._obj.amax_dout:
                assert not (args[0]._obj.flags & L.MATH_F16X2)
    assert nrec == 3 * 2 * (2 * (k - 1) + (k - 1) + 1)      # per scale and direction: h2h fwd (infer, train), h2h dgrad, i2h dgrad
    # pad channels (out: A = 24 -> 32 per gate block) stay exactly zero through SGD with momentum and weight decay
    pads = _pads(net)
    assert (len(pads) > 0) == (pos == 'out')
    net.sgd_step(1e-3, 0.9, 5e-4, b)
    net(dev(x), dev(gt), *[dev(t) for t in tg])
    net.backward()
    net.sgd_step(1e-3, 0.9, 5e-4, b)
    torch.cuda.synchronize()
    for w in _pads(net):
        assert bool((w == 0).all())
    assert all(bool(torch.isfinite(p.data()).all()) for p in net.collect_params().values())


def onet_channels(onet, n, c):
    """channels of the oracle's tensor at a join (the device's head tensors carry pad channels)"""
    return 3 * (5 + c) if n.name.startswith('pool.head') else 10 ** 9


def test_rnn_frozen_parameters_and_no_wd():
    c, b, size, k = 3, 2, 64, 3
    net, P = _mk(c, k, "late", "max", 59)
    rng = np.random.default_rng(59)
    x = rng.standard_normal((b, k, 3, size, size)).astype(np.float32)
    gt = np.array([[[5., 8., 40., 50.], [-1, -1, -1, -1]], [[10., 12., 30., 28.], [20., 5., 60., 62.]]])
    gid = np.array([[[1.], [-1.]], [[0.], [2.]]])
    tg = Y.prefetch_targets(size, size, [size // 32, size // 16, size // 8], gt, gid, c)
    PR = net.collect_params()
    frozen_w, frozen_b = "yolo_tips.1.tip.rnn.r_cell.h2h_weight", "yolo_tips.2.tip.rnn.l_cell.i2h_bias"
    PR[frozen_w].grad_req = 'null'
    PR[frozen_b].grad_req = 'null'
    net.grads.fill_(7.0)                                    # a launch that still ran would overwrite its range
    net(dev(x), dev(gt), *[dev(t) for t in tg])
    net.backward()
    torch.cuda.synchronize()
    tp = net._last_train
    wgrads = [r for sg in tp['bwd'] for r in sg.recs if r[0] == 'vd_conv_wgrad']
    ptrs = {int(r[2][0]._obj.dwp) for r in wgrads}
    hit = {cn.pw: cn.gwp.data_ptr() in ptrs for cn in net.conv_nodes if hasattr(cn, 'pw')}
    assert not hit[frozen_w] and sum(hit.values()) == 11
    for key in (frozen_w, frozen_b):
        lo, hi = PR[key].span
        assert bool((net.grads[lo:hi] == 7.0).all()), key
    live = "yolo_tips.1.tip.rnn.r_cell.i2h_weight"
    assert not bool((net.grads[PR[live].span[0]:PR[live].span[1]] == 7.0).any())
    before = {key: PR[key].data().clone() for key in (frozen_w, frozen_b, live)}
    # --no_wd: lr = 0 leaves only the weight-decay term ... of momentum 0, so use the gradient-free view: zero gradients
    net.grads.zero_()
    net.sgd_step(0.1, 0.0, 0.5, b, no_wd=True)
    torch.cuda.synchronize()
    for key in (frozen_w, frozen_b):
        assert torch.equal(PR[key].data(), before[key]), key               # no update, no decay
    assert torch.allclose(PR[live].data(), before[live] * (1 - 0.1 * 0.5), rtol=1e-6, atol=0)    # weights decay
    for key, p in PR.items():
        if ".rnn." in key and key.endswith("bias") and key != frozen_b:
            assert torch.equal(p.data(), torch.from_numpy(P[key].astype(np.float32)).cuda()), key   # the eight biases do not


@pytest.mark.parametrize("pos,jt", [("late", "max"), ("out", "max")])
def test_rnn_scripts_train_then_detect(tmp_path, monkeypatch, pos, jt):
    import train_yolov3 as T
    import detect_yolo3 as D
    monkeypatch.chdir(tmp_path)
    flags = ["--window", "3,1", "--k_join_type", jt, "--k_join_pos", "late", "--rnn_pos", pos]
    net = T.main(["--dataset", "vid", "--batch_size", "2", "--data_shape", "64", "--epochs", "1", "--synthetic_samples", "4",
                  "--save_prefix", "r", "--log_interval", "1", "--no_random_shape"] + flags)
    ref = RO.param_shapes(len(net.classes), 3, pos, jt)
    assert {key: p.shape for key, p in net.collect_params().items()} == {key: tuple(s) for key, s in ref.items()}
    cks = sorted(glob.glob(str(tmp_path / "models" / "experiments" / "r" / "*.params")))
    assert cks, os.listdir(str(tmp_path))
    # checkpoint round trip: every array, the GRU's included, comes back bit for bit
    from viddet_amd.model import yolo3_darknet53
    net2 = yolo3_darknet53(net.classes, k=3, k_join_type=jt, k_join_pos='late', rnn_pos=pos)
    net.save_parameters(str(tmp_path / "rt.params"))
    net2.load_parameters(str(tmp_path / "rt.params"))
    for key, p in net.collect_params().items():
        assert torch.equal(p.data(), net2.collect_params()[key].data()), key
    D.main(["--model_path", cks[-1], "--dataset", "vid", "--batch_size", "2", "--data_shape", "64", "--synthetic_samples", "4",
            "--save_dir", str(tmp_path / "results"), "--save_prefix", "r1"] + flags)
    rows = glob.glob(str(tmp_path / "results" / "r1" / "pred" / "*"))
    assert rows
