"""The (2+1)-D Darknet backbone of frame windows (--conv_types 21) on the MI355X: the temporal-conv kernels (vd_tdw.hip)
against the fp64 restatement with bounds derived from fp32 rounding, the yolo3_3ddarknet networks against the fp64 oracle
(the comparison and tolerances of tests/test_rnn_gpu.py), inflation from a 2-D detector, frozen parameters, weight decay,
and train_yolov3.py / detect_yolo3.py with --conv_types."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import net as ON
from oracle import yolo as Y
from tests import darknet21_oracle as DO
from tests.util import dev, maxdiff, boxes_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit round-off of fp32


def _nhwc(a5):
    """(B,C,K,h,w) -> the device's folded rows [B*K, h*w, C]"""
    B, C_, K, h, w = a5.shape
    return np.ascontiguousarray(a5.transpose(0, 2, 3, 4, 1).reshape(B * K, h * w, C_))


def _from_nhwc(t, B, K, h, w):
    a = t.cpu().numpy().astype(np.float64)
    return a.reshape(B, K, h, w, -1).transpose(0, 4, 1, 2, 3)


# B = 2; 7 x 5 pixels (no multiple of any tile); C = 32 / 64: 8 / 16 channel lanes per workgroup; 320: more channel groups than
# lanes (two passes of the channel loop, the second partly filled); 182 x 181 pixels: more work than one grid pass in both
# kernels (grid-stride loops, the cap of the partial table)
KERNEL_CASES = [(K, 7, 5, C_, res) for K in (2, 3, 5) for C_ in (32, 64) for res in (False, True)] + \
               [(3, 7, 5, 320, True), (2, 182, 181, 64, True)]


@pytest.mark.parametrize("K,h,w,C_,res", KERNEL_CASES)
def test_temporal_conv_kernels_against_the_restatement(K, h, w, C_, res):
    from viddet_amd import lib as L
    from viddet_amd import ops
    B = 2
    rng = np.random.default_rng(K * 1000 + C_ + int(res) + h)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    x = f32(rng.standard_normal((B, C_, K, h, w)))                      # every frame random and distinct
    wt = f32(1.0 / 3 + 0.5 * rng.standard_normal((C_, 1, 3, 1, 1)))
    r = f32(rng.standard_normal(x.shape)) if res else None
    dy = f32(rng.standard_normal(x.shape))
    y_ref = DO.tdw_forward(x, wt) + (r if res else 0.0)
    dx_ref, dw_ref = DO.tdw_backward(x, wt, dy)
    aw = np.abs(wt)
    # sum of the magnitudes of the terms of every output element (the restatement applied to magnitudes)
    y_mag = DO.tdw_forward(np.abs(x), aw) + (np.abs(r) if res else 0.0)
    dx_mag, dw_mag = DO.tdw_backward(np.abs(x), aw, np.abs(dy))
    N = B * K * h * w
    xd, wd_, dyd = dev(_nhwc(x)), dev(wt.reshape(-1)), dev(_nhwc(dy))
    rd = dev(_nhwc(r)) if res else None
    ws = torch.empty(ops.tdw_bwd_ws_bytes(B, K, h * w, C_), dtype=torch.uint8, device='cuda')
    runs = []
    for _ in range(2):
        y = torch.full_like(xd, float('nan'))
        am = torch.zeros(L.AMAX_FLOATS, device='cuda')
        dx = torch.full_like(xd, float('nan'))
        dw = torch.full((C_ * 3,), float('nan'), device='cuda')
        ops.tdw_fwd(xd, wd_, rd, y, B, K, h * w, C_, am)
        ops.tdw_bwd(dyd, xd, wd_, dx, dw, B, K, h * w, C_, ws)
        runs.append((y, am, dx, dw))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs are bit-identical"
    y, am, dx, dw = runs[0]
    got_y, got_dx = _from_nhwc(y, B, K, h, w), _from_nhwc(dx, B, K, h, w)
    got_dw = dw.cpu().numpy().astype(np.float64).reshape(C_, 1, 3, 1, 1)
    for name, got, ref, bound in (("y", got_y, y_ref, 4 * U * y_mag), ("dx", got_dx, dx_ref, 4 * U * dx_mag),
                                  ("dw", got_dw, dw_ref, (N + 2) * U * dw_mag)):
        err = np.abs(got - ref)
        print(name, "max err %.3e, max err / bound %.3f" % (err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), name
    assert ops.amax_value(am) == float(y.abs().max()), "the published max-abs is max|y| exactly"
    # the skipped forms leave their buffers untouched
    dx2 = torch.full_like(xd, 7.0)
    dw2 = torch.full((C_ * 3,), 7.0, device='cuda')
    ops.tdw_bwd(dyd, xd, wd_, None, dw2, B, K, h * w, C_, ws)
    torch.cuda.synchronize()
    assert torch.equal(dw2, dw) and bool((dx2 == 7.0).all())
    dw3 = torch.full((C_ * 3,), 7.0, device='cuda')
    ops.tdw_bwd(dyd, xd, wd_, dx2, None, B, K, h * w, C_, None)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx) and bool((dw3 == 7.0).all())


def _mk(c, ct, k, seed, **kw):
    from viddet_amd.model import yolo3_3ddarknet
    net = yolo3_3ddarknet(["c%d" % i for i in range(c)], conv_types=ct, k=k, **kw)
    P = DO.init_params(c, ct, seed=seed, obj_bias=-1.0)
    assert set(P) == set(net.collect_params().keys())
    for key, p in net.collect_params().items():
        assert tuple(P[key].shape) == p.shape, (key, P[key].shape, p.shape)
        p.set_data(torch.from_numpy(P[key].astype(np.float32)))
    return net, P


def _targets(size, c):
    gt = np.array([[[5., 8., 40., 50.], [-1, -1, -1, -1]], [[10., 12., 30., 28.], [20., 5., 60., 62.]]])
    gid = np.array([[[1.], [-1.]], [[0.], [1.]]])
    return gt, Y.prefetch_targets(size, size, [size // 32, size // 16, size // 8], gt, gid, c)


NET_CTS = [[21, 2, 2, 2, 2, 2], [21, 21, 21, 21, 21, 2], [21] * 6]


@pytest.mark.parametrize("ct", NET_CTS, ids=lambda ct: "-".join(map(str, ct)))
def test_network_inference_and_training(ct):
    c, b, size, k = 2, 2, 64, 3
    net, P = _mk(c, ct, k, 61)
    rng = np.random.default_rng(61)
    x = rng.standard_normal((b, k, 3, size, size)).astype(np.float32)
    onet = DO.D21Net(P, c, ct, k)
    ids_r, sc_r, bx_r, rows_r, heads_r = onet.detect(x.astype(np.float64))
    ids, sc, bx = net(dev(x))
    torch.cuda.synchronize()
    bufs = net._programs[('buf', b, size, size, False)]
    for s, hname in enumerate(net.head_names):
        got = bufs[hname].cpu().numpy()
        print("head", s, "max err", maxdiff(got[..., :3 * (5 + c)], np.moveaxis(heads_r[s], 1, -1)))
        assert maxdiff(got[..., :3 * (5 + c)], np.moveaxis(heads_r[s], 1, -1)) < 1e-3, "head %d" % s
    from tests.util import assert_rows_match, take_ranks
    perm = assert_rows_match(net.last_rows.cpu().numpy(), rows_r, sc_r)
    assert maxdiff(take_ranks(sc, perm), sc_r) < 1e-3 and boxes_close(take_ranks(bx, perm), bx_r)
    # one training step against the oracle
    gt, tg = _targets(size, c)
    out = net(dev(x), dev(gt), *[dev(t) for t in tg])
    net.backward()
    torch.cuda.synchronize()
    tb = net._programs[('buf', b, size, size, True)]
    from tests.util import device_leaky_masks, check_masks_differ_only_at_ties
    from viddet_amd.model import PoolNode
    onet.mask_override = device_leaky_masks(net, tb)
    for n in net.nodes:                                      # the max pool's winner among the K frames, borrowed at ties
        if isinstance(n, PoolNode):
            onet.argmax_override[n.name] = np.moveaxis(tb['am:' + n.dst].cpu().numpy().astype(np.int64), -1, 1)
    losses_r, G, heads_t = onet.train_step(x.astype(np.float64), gt, *tg)
    check_masks_differ_only_at_ties(onet.pre, onet.mask_override)
    assert set(onet.argmax_natural) == set(onet.argmax_override)
    for name, (am, v5) in onet.argmax_natural.items():
        d = am != onet.argmax_override[name]
        if d.any():          # a different winner is only acceptable between (numerically) equal candidates
            a = np.take_along_axis(v5, am[:, None], axis=1)[:, 0]
            bwin = np.take_along_axis(v5, onet.argmax_override[name][:, None], axis=1)[:, 0]
            assert np.abs(a - bwin)[d].max() < 2e-4, name
    for i in range(4):
        assert np.all(np.abs(out[i].cpu().numpy() - losses_r[i]) <= 2e-3 * np.maximum(1.0, np.abs(losses_r[i])))
    PR = net.collect_params()
    for key, v in onet.new_running.items():
        assert maxdiff(PR[key].data().cpu().numpy(), v) < 1e-4, key
    assert set(G) == {key for key, p in PR.items() if p.span is not None}
    bad, worst = [], 0.0
    for key, gref in G.items():
        got = PR[key].grad().cpu().numpy()
        assert got.shape == gref.shape, key
        scale = max(1e-3, float(np.abs(gref).max()))
        if key.endswith(".3.conv.weight"):
            worst = max(worst, maxdiff(got, gref) / scale)
            assert np.abs(gref).max() > 0, key
        if maxdiff(got, gref) / scale >= 5e-4:
            bad.append((key, maxdiff(got, gref) / scale))
    print("worst temporal-weight gradient error / max:", worst)
    assert not bad, bad[:6]
    # parameters after one SGD step (momentum buffers start at zero)
    lr, wd = 1e-3, 5e-4
    net.sgd_step(lr, 0.9, wd, b)
    torch.cuda.synchronize()
    for key, gref in G.items():
        want = P[key] - lr * (gref / b + wd * P[key])
        assert maxdiff(PR[key].data().cpu().numpy(), want) < 1e-4, key


def test_inflated_network_reproduces_the_2d_network_on_a_static_window():
    from viddet_amd.model import yolo3_darknet53, yolo3_3ddarknet
    c, b, size, k = 2, 2, 64, 3
    classes = ["c%d" % i for i in range(c)]
    P = ON.init_params(c, seed=67, obj_bias=-1.0)
    net2 = yolo3_darknet53(classes)
    for key, p in net2.collect_params().items():
        p.set_data(torch.from_numpy(P[key].astype(np.float32)))
    net3 = yolo3_3ddarknet(classes, conv_types=[21] * 6, k=k)
    net3.initialize(init='he', seed=1)
    net3.inflate_from_2d(net2)
    PR = net3.collect_params()
    assert torch.equal(PR["d_model.features.0.3.conv.weight"].data(), torch.full((32, 1, 3, 1, 1), 1.0 / 3, device='cuda'))
    assert torch.equal(PR["d_model.features.4.body.1.0.weight"].data()[:, :, 0], net2.collect_params()["stages.0.4.body.1.0.weight"].data())
    assert torch.equal(PR["d_model.features.28.body.0.1.running_var"].data(), net2.collect_params()["stages.2.4.body.0.1.running_var"].data())
    assert torch.equal(PR["yolo_blocks.1.tip.0.weight"].data(), net2.collect_params()["yolo_blocks.1.tip.0.weight"].data())
    # a parameter dict works as well, and a network with the pool in the first slice shifts the names behind it
    net3b = yolo3_3ddarknet(classes, conv_types=[21, 21, 2, 2, 2, 2], k=k)
    net3b.inflate_from_2d({key: p.data() for key, p in net2.collect_params().items()})
    assert torch.equal(net3b.collect_params()["d_model.features.4.0.weight"].data(), net2.collect_params()["stages.0.3.0.weight"].data())
    rng = np.random.default_rng(67)
    f = rng.standard_normal((b, 1, 3, size, size)).astype(np.float32)
    net2(dev(f[:, 0]))
    rows2 = net2.last_rows.clone()
    h2 = [net2._programs[('buf', b, size, size, False)][h].clone() for h in net2.head_names]
    for net in (net3, net3b):
        net(dev(np.repeat(f, k, axis=1)))
        torch.cuda.synchronize()
        for s, h in enumerate(net.head_names):
            d = float((net._programs[('buf', b, size, size, False)][h] - h2[s]).abs().max())
            print("head", s, "max difference to the 2-D network", d)
            assert d < 1e-3
        assert torch.equal(net.last_rows, rows2)


def test_frozen_base_weight_decay_and_reset_class():
    c, b, size, k = 2, 2, 64, 3
    ct = [21, 21, 2, 2, 2, 2]
    net, P = _mk(c, ct, k, 71, freeze_base=True)
    rng = np.random.default_rng(71)
    x = rng.standard_normal((b, k, 3, size, size)).astype(np.float32)
    gt, tg = _targets(size, c)
    PR = net.collect_params()
    before = {key: p.data().clone() for key, p in PR.items()}
    net.grads.fill_(7.0)
    net(dev(x), dev(gt), *[dev(t) for t in tg])
    net.backward()
    net.sgd_step(1e-2, 0.9, 5e-2, b)
    torch.cuda.synchronize()
    assert not any(r[0] == 'vd_tdw_bwd' for sg in net._last_train['bwd'] for r in sg.recs)
    for key, p in PR.items():
        if key.startswith("d_model.") and p.span is not None:
            assert torch.equal(p.data(), before[key]), key                 # no update, no decay, temporal weights included
            assert bool((net.grads[p.span[0]:p.span[1]] == 7.0).all()), key
    assert not torch.equal(PR["yolo_blocks.0.body.0.0.weight"].data(), before["yolo_blocks.0.body.0.0.weight"])
    # unfrozen: weight decay and --no_wd reach the temporal weights as they reach conv weights (zero gradients: decay alone)
    net, P = _mk(c, ct, k, 71)
    PR = net.collect_params()
    tw, cw, ga = "d_model.features.1.3.conv.weight", "d_model.features.1.0.weight", "d_model.features.1.1.gamma"
    before = {key: PR[key].data().clone() for key in (tw, cw, ga)}
    net.grads.zero_()
    net.sgd_step(0.1, 0.0, 0.5, b, no_wd=True)
    torch.cuda.synchronize()
    assert torch.allclose(PR[tw].data(), before[tw] * (1 - 0.1 * 0.5), rtol=1e-6, atol=0)
    assert torch.allclose(PR[cw].data(), before[cw] * (1 - 0.1 * 0.5), rtol=1e-6, atol=1e-9)
    assert torch.equal(PR[ga].data(), before[ga])
    PR[tw].wd_mult = 0.0
    keep = PR[tw].data().clone()
    net.sgd_step(0.1, 0.0, 0.5, b)
    torch.cuda.synchronize()
    assert torch.equal(PR[tw].data(), keep)
    # one trainable temporal weight under a frozen rest of the trunk still gets its gradient; the others' launches skip dw
    for key, p in PR.items():
        if key.startswith("d_model.") and p.span is not None and key != tw:
            p.grad_req = 'null'
    net.grads.fill_(7.0)
    net(dev(x), dev(gt), *[dev(t) for t in tg])
    net.backward()
    torch.cuda.synchronize()
    recs = [r for sg in net._last_train['bwd'] for r in sg.recs if r[0] == 'vd_tdw_bwd']
    # (the block above it passes the gradient down: dx, no dw; the trainable one: dw, and no dx - nothing below needs it)
    assert sorted((r[2][3] is None, r[2][4] is None) for r in recs) == [(False, True), (True, False)]
    lo, hi = PR[tw].span
    assert not bool((net.grads[lo:lo + 3 * 64] == 7.0).any())
    lo, hi = PR["d_model.features.0.3.conv.weight"].span
    assert bool((net.grads[lo:hi] == 7.0).all())
    # initialize(): the rule of every conv weight; reset_class keeps the trunk
    net.initialize(init='uniform', seed=3)
    w = PR["d_model.features.0.3.conv.weight"].data()
    assert tuple(w.shape) == (32, 1, 3, 1, 1) and 0 < float(w.abs().max()) <= 0.07
    trunk = {key: p.data().clone() for key, p in net.collect_params().items() if key.startswith("d_model.")}
    net.reset_class(["a", "b", "c"])
    assert net.num_class == 3 and len(net.tdw_nodes) == 3
    for key, v in trunk.items():
        assert torch.equal(net.collect_params()[key].data(), v), key
    net(dev(x))
    torch.cuda.synchronize()


def test_scripts_train_then_detect(tmp_path, monkeypatch):
    import train_yolov3 as T
    import detect_yolo3 as D
    monkeypatch.chdir(tmp_path)
    ct = [21, 21, 2, 2, 2, 2]
    flags = ["--window", "3,1", "--conv_types", ",".join(map(str, ct))]
    net = T.main(["--dataset", "vid", "--batch_size", "2", "--data_shape", "64", "--epochs", "1", "--synthetic_samples", "4",
                  "--save_prefix", "d", "--log_interval", "1", "--no_random_shape"] + flags)
    ref = DO.param_shapes(len(net.classes), ct)
    assert {key: p.shape for key, p in net.collect_params().items()} == {key: tuple(s) for key, s in ref.items()}
    cks = sorted(glob.glob(str(tmp_path / "models" / "experiments" / "d" / "*.params")))
    assert cks, os.listdir(str(tmp_path))
    from viddet_amd.model import yolo3_3ddarknet
    net2 = yolo3_3ddarknet(net.classes, conv_types=ct, k=3)
    net.save_parameters(str(tmp_path / "rt.params"))
    net2.load_parameters(str(tmp_path / "rt.params"))
    for key, p in net.collect_params().items():
        assert torch.equal(p.data(), net2.collect_params()[key].data()), key
    D.main(["--model_path", cks[-1], "--dataset", "vid", "--batch_size", "2", "--data_shape", "64", "--synthetic_samples", "4",
            "--save_dir", str(tmp_path / "results"), "--save_prefix", "d1"] + flags)
    assert glob.glob(str(tmp_path / "results" / "d1" / "pred" / "*"))
