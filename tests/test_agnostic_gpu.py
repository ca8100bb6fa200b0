"""GPU: class-agnostic detection (--model_agnostic) against the fp64 restatement in tests/agnostic_oracle.py.

Kernel cases: vd_yolo_decode_filter_agnostic + vd_nms_agnostic on made-up heads, fp32 and bf16 tensors (the oracle reads the
same rounded values).  Identical post-NMS rows and ids, scores within 1e-5 and boxes within tests/util.boxes_close - the bounds
tests/test_yolo_gpu.py holds the per-class tail to - the candidate set equal to the oracle's valid set, two runs bit-identical.
No case may lean on a near-tie, so each first checks on the ORACLE's result that every IoU the sweep compares is further
than 1e-4 from nms_thresh, that neighbouring top-k scores (and the first one below them) differ by more than the score
tolerance, and that no score lies within it of valid_thresh.  The objectness logits are therefore DEALT from a grid whose
scores are spaced by construction (a random permutation over the anchors; bf16: distinct bf16 values), everything else is
random; the seeds in SEEDS were searched on the CPU for the IoU condition.
Network cases: agnostic=True networks against the oracle network with the agnostic tail; training untouched.
Script: detect_yolo3.py --model_agnostic end to end."""
import os

import numpy as np
import pytest
import torch

from oracle import net as ON
from oracle import yolo as Y
from tests import agnostic_oracle as AO
from tests.util import dev, maxdiff, boxes_close, assert_rows_match, take_ranks

pytestmark = pytest.mark.gpu

SCORE_TOL, IOU_BAND, VALID, NMS_T, TOPK, POST = 1e-5, 1e-4, 0.01, 0.45, 400, 100
LO, HI = -4.4, 1.0            # logits of valid anchors: sigmoid(-4.4) = 0.0121 > valid_thresh, sigmoid'(1) = 0.197


def _bf16_values(lo, hi):
    """every bf16 value in [lo, hi] with |v| >= 2^-3, ascending (neighbours' sigmoids differ by >= 2.4e-4 there)"""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).double().numpy()
    v = np.unique(bits[np.isfinite(bits)])
    return v[(v >= lo) & (v <= hi) & (np.abs(v) >= 0.125)]


def make_heads(seed, b, c, size, mode, bf16):
    """heads (B, 3*(5+C), g, g) fp64 holding fp32- (bf16-) representable values.  mode: 'none' no valid anchor, 'some' ~50 valid
    per image, 'all' every anchor valid."""
    rng = np.random.default_rng(seed)
    grids = [size // 32, size // 16, size // 8]
    P = 3 * sum(g * g for g in grids)
    nvalid = dict(none=0, some=min(50, P), all=P)[mode]
    obj = np.empty((b, P))
    for bi in range(b):
        o = -7.0 - rng.uniform(0.0, 2.0, P)                      # invalid: sigmoid <= 9.1e-4
        if nvalid:
            ntop = min(nvalid, TOPK + 50)                        # the ranks the top-k (and its boundary) can see: distinct
            if bf16:
                grid = _bf16_values(LO, HI)
            else:
                grid = np.linspace(LO, HI, max(nvalid, ntop))
                grid = grid + rng.uniform(-0.2, 0.2, len(grid)) * (grid[1] - grid[0])
            vals = np.concatenate([grid[len(grid) - ntop:], rng.choice(grid[:len(grid) - ntop], nvalid - ntop)]) \
                if nvalid > ntop else grid[len(grid) - ntop:]
            o[rng.permutation(P)[:nvalid]] = rng.permutation(vals)
        obj[bi] = o
    heads, off = [], 0
    for g in grids:
        p = rng.standard_normal((b, 3, 5 + c, g, g))
        p[:, :, 2:4] *= 0.5
        p[:, :, 5:] = p[:, :, 5:] * 2.0 + 1.0                    # class logits: never read by the agnostic tail
        n = g * g * 3
        p[:, :, 4] = obj[:, off:off + n].reshape(b, g, g, 3).transpose(0, 3, 1, 2)
        off += n
        t = torch.from_numpy(p.reshape(b, 3 * (5 + c), g, g)).float()
        heads.append((t.bfloat16() if bf16 else t).double().numpy())
    return heads, grids, P


def oracle_and_margins(heads, c):
    """the oracle's result and the three tie-proofing checks of the module docstring, asserted on it"""
    (ids_r, sc_r, bx_r, rows_r), alldet = AO.agnostic_detect(heads, c, NMS_T, TOPK, POST)
    s = alldet[..., 1]
    assert np.abs(s - VALID).min() > SCORE_TOL, "a score lies within the tolerance of valid_thresh"
    for bi, (top, nxt, ious) in enumerate(AO.sweep_pairs(alldet, NMS_T, VALID, TOPK)):
        chain = np.concatenate([top, [nxt]]) if nxt is not None else top
        if len(chain) > 1:
            assert (-np.diff(chain)).min() > SCORE_TOL, "image %d: neighbouring top-k scores within the tolerance" % bi
        if len(ious):
            assert np.abs(ious - NMS_T).min() > IOU_BAND, "image %d: a compared IoU within 1e-4 of nms_thresh" % bi
    return (ids_r, sc_r, bx_r, rows_r), alldet


# 64 x 64: 252 anchors per image (the direct sort of vd_nms_agnostic), 160 x 160: 1575 > nms_topk and > the 1024 keys the direct sort
# takes (radix select, scores held in registers), 832 x 832: 42588 > the 40960 scores the registers hold (streaming select).
# C = 1, 2: 5 + C no multiple of 4, channels padded to 32; C = 80: 255 of 256 channels, an anchor straddles 128-byte lines.
CASES = [(size, c, mode, bf16) for size in (64, 160) for c in (1, 2, 80) for mode in ("none", "some", "all") for bf16 in (False, True)]
CASES += [(832, 1, "all", False), (832, 1, "all", True)]
# case -> seed: the first of 100, 101, ... whose fixture passes oracle_and_margins (searched on the CPU; the test asserts it)
SEEDS = {(64, 80, 'some', True): 101, (64, 80, 'all', True): 101, (160, 80, 'all', False): 101, (160, 80, 'all', True): 101}


def _seed(case):
    return SEEDS.get(case, 100)


def _run_tail(ops, h, b, P, bf16):
    cs = torch.empty(b, P, device="cuda")
    cr = torch.empty(b, P, dtype=torch.int32, device="cuda")
    cnt = torch.empty(b, dtype=torch.int32, device="cuda")
    ids = torch.empty(b, POST, device="cuda"); sc = torch.empty(b, POST, device="cuda")
    bx = torch.empty(b, POST, 4, device="cuda"); rows = torch.empty(b, POST, dtype=torch.int32, device="cuda")
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ops.yolo_decode_filter_agnostic(h, VALID, cs, cr, P, cnt, head_bf16=bf16)
    ops.nms_agnostic(h, cs, cr, P, cnt, NMS_T, TOPK, POST, ids, sc, bx, rows, ws, head_bf16=bf16)
    torch.cuda.synchronize()
    return cs, cr, cnt, ids, sc, bx, rows, ws


@pytest.mark.parametrize("case", CASES, ids=lambda k: "%d-C%d-%s-%s" % (k[0], k[1], k[2], "bf16" if k[3] else "fp32"))
def test_agnostic_decode_nms_kernels(case):
    from viddet_amd import ops
    from tests.util import nchw_to_dev_nhwc
    size, c, mode, bf16 = case
    b = 2
    heads, grids, P = make_heads(_seed(case), b, c, size, mode, bf16)
    (ids_r, sc_r, bx_r, rows_r), alldet = oracle_and_margins(heads, c)
    nval = (alldet[..., 1] > VALID).sum(axis=1)
    assert np.all(nval == dict(none=0, some=min(50, P), all=P)[mode])
    ldh = ops.round_up(3 * (5 + c), 32)
    hd = [nchw_to_dev_nhwc(h, ldh) for h in heads]
    if bf16:
        hd = [t.bfloat16() for t in hd]                         # exact: the values are bf16-representable
    h = ops.make_head_desc(hd, grids, ldh, Y.OUT_STRIDES, Y.OUT_ANCHORS, b, c)
    cs, cr, cnt, ids, sc, bx, rows, ws = _run_tail(ops, h, b, P, bf16)
    assert int(ws.view(torch.int32)[:b].max()) == 0
    for bi in range(b):
        n = int(cnt[bi])
        print("image %d: %d candidates (oracle %d)" % (bi, n, nval[bi]))
        assert n == nval[bi], "candidate count differs from the oracle's"
        got_rows = cr[bi, :n].cpu().numpy()
        assert sorted(got_rows.tolist()) == np.nonzero(alldet[bi, :, 1] > VALID)[0].tolist()
        assert n == 0 or maxdiff(cs[bi, :n].cpu().numpy(), alldet[bi, got_rows, 1]) < SCORE_TOL
    assert np.array_equal(rows.cpu().numpy().astype(np.int64), rows_r), "post-NMS row indices differ"
    assert np.array_equal(ids.cpu().numpy(), ids_r[..., 0])
    kept = rows_r >= 0
    if mode != "none":
        assert kept.any() and np.all(ids_r[..., 0][kept] == 0)
    print("scores: max err %.3e; kept %s" % (maxdiff(sc.cpu().numpy(), sc_r[..., 0]), kept.sum(axis=1).tolist()))
    assert maxdiff(sc.cpu().numpy(), sc_r[..., 0]) < SCORE_TOL
    assert boxes_close(bx.cpu().numpy(), bx_r)
    # a second run: the append order of the candidates may differ, nothing that leaves the NMS may
    again = _run_tail(ops, h, b, P, bf16)
    for a0, a1 in zip((cnt, ids, sc, bx, rows), (again[2], again[3], again[4], again[5], again[6])):
        assert torch.equal(a0, a1)


# ------------------------------------------------------------------------------------------------ networks
def _plain(c, seed, **kw):
    from viddet_amd.model import yolo3_darknet53
    P = ON.init_params(c, seed=seed, obj_bias=-1.0)
    net = yolo3_darknet53(["c%d" % i for i in range(c)], **kw)
    for k, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[k].astype(np.float32)))
    return net, P


def _train_outputs(net, x, size, c, key):
    gt = np.array([[[5., 8., 40., 50.], [-1, -1, -1, -1]], [[10., 12., 30., 28.], [20., 5., 60., 62.]]])
    gid = np.array([[[1.], [-1.]], [[0.], [2.]]])
    tg = Y.prefetch_targets(size, size, [size // 32, size // 16, size // 8], gt, gid, c)
    out = [t.clone() for t in net(dev(x), dev(gt), *[dev(t) for t in tg])]
    torch.cuda.synchronize()
    tb = net._programs[key]
    return out + [tb[h].clone() for h in net.head_names]


def _check_against(net, ids, sc, bx, want):
    ids_r, sc_r, bx_r, rows_r = want
    perm = assert_rows_match(net.last_rows.cpu().numpy(), rows_r, sc_r)
    assert np.array_equal(take_ranks(ids, perm)[..., 0], ids_r[..., 0])
    assert maxdiff(take_ranks(sc, perm), sc_r) < 1e-3 and boxes_close(take_ranks(bx, perm), bx_r)
    kept = rows_r >= 0
    assert kept.sum() > 4, "fixture keeps (almost) nothing"
    assert np.all(ids.cpu().numpy()[..., 0][kept] == 0)


def test_agnostic_network_k1_fp32_and_bf16(tmp_path):
    c, b, size = 4, 2, 64
    net, P = _plain(c, 11, agnostic=True)
    ref, _ = _plain(c, 11)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((b, 3, size, size)).astype(np.float32)
    onet = ON.Net(P, c)
    ids_r, sc_r, bx_r, rows_r, heads_r = AO.net_detect(onet, x.astype(np.float64))
    ids, sc, bx = net(dev(x))
    torch.cuda.synchronize()
    assert tuple(ids.shape) == (b, POST, 1) and tuple(sc.shape) == (b, POST, 1) and tuple(bx.shape) == (b, POST, 4)
    _check_against(net, ids, sc, bx, (ids_r, sc_r, bx_r, rows_r))
    # the per-class network on the same weights answers differently (the fixture can tell the two tails apart)
    pid = ref(dev(x))[0]
    assert not torch.equal(pid, ids)
    # the HIP-graph replay of the inference program
    first = [t.clone() for t in (ids, sc, bx, net.last_rows)]
    net.use_graphs = True
    for _ in range(2):
        g = net(dev(x))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b_) for a, b_ in zip(first, list(g) + [net.last_rows]))
    net.use_graphs = False
    # bf16 inference: fp32 heads within the bf16 plan's bound of the oracle's, and the tail EXACT on the heads it was given
    net.set_precision('bf16')
    ids16, sc16, bx16 = net(dev(x))
    torch.cuda.synchronize()
    bufs = net._programs[('infer_bf16', b, size, size)][1]
    dev_heads = []
    for s_, hname in enumerate(net.head_names):
        got = bufs[hname].cpu().numpy()[..., :3 * (5 + c)]
        refh = np.moveaxis(heads_r[s_], 1, -1)
        assert maxdiff(got, refh) / np.abs(refh).max() < 3e-2
        dev_heads.append(np.moveaxis(got.astype(np.float64), -1, 1))
    want16, _ = AO.agnostic_detect(dev_heads, c)
    _check_against(net, ids16, sc16, bx16, want16)
    net.set_precision('fp32')
    again = net(dev(x))
    torch.cuda.synchronize()
    assert torch.equal(again[0], first[0]) and torch.equal(again[2], first[2])
    # training is untouched: losses and training-mode heads bit-equal to the agnostic=False network's
    key = ('buf', b, size, size, True)
    for t_a, t_p in zip(_train_outputs(net, x, size, c, key), _train_outputs(ref, x, size, c, key)):
        assert torch.equal(t_a, t_p)
    # the same .params, both ways; reset_class keeps the mode
    f = str(tmp_path / "ag.params")
    net.save_parameters(f)
    ref.load_parameters(f)
    for k, q in net.collect_params().items():
        assert torch.equal(q.data(), ref.collect_params()[k].data()), k
    net.reset_class(["x", "y"])
    assert net.agnostic and net.num_class == 2
    r = net(dev(x))
    torch.cuda.synchronize()
    assert tuple(r[0].shape) == (b, POST, 1) and bool(((r[0] == 0) | (r[0] == -1)).all())


def test_agnostic_network_k3_max_late():
    from oracle import net_temporal as OT
    from tests.test_temporal_gpu import _mk
    from viddet_amd.model import yolo3_darknet53
    cfg = dict(jt="max", jp="late", bct="2")
    c, b, size, K = 3, 2, 64, 3
    ref, P = _mk(cfg, c, 41)
    net = yolo3_darknet53(["c%d" % i for i in range(c)], k=K, k_join_type="max", k_join_pos="late", agnostic=True)
    for k, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[k].astype(np.float32)))
    rng = np.random.default_rng(41)
    x = rng.standard_normal((b, K, 3, size, size)).astype(np.float32)
    onet = OT.TemporalNet(P, c, K, "max", "late", "2")
    ids_r, sc_r, bx_r, rows_r, _ = AO.net_detect(onet, x.astype(np.float64))
    ids, sc, bx = net(dev(x))
    torch.cuda.synchronize()
    _check_against(net, ids, sc, bx, (ids_r, sc_r, bx_r, rows_r))
    key = ('buf', b, size, size, True)
    for t_a, t_p in zip(_train_outputs(net, x, size, c, key), _train_outputs(ref, x, size, c, key)):
        assert torch.equal(t_a, t_p)


# ------------------------------------------------------------------------------------------------ script
def test_detect_script_model_agnostic(tmp_path, capsys):
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticDetection, YOLO3VideoInferenceTransform
    size, nsamp = 96, 6
    out = D.main(["--model_agnostic", "--random_init", "--dataset", "voc", "--batch_size", "4", "--data_shape", str(size),
                  "--synthetic_samples", str(nsamp), "--save_dir", str(tmp_path / "results"), "--save_prefix", "t1",
                  "--metrics", "voc"])
    printed = capsys.readouterr().out
    ds = SyntheticDetection("voc", num_samples=nsamp)
    tf = YOLO3VideoInferenceTransform(size, size)
    pdir = tmp_path / "results" / "t1" / "pred_ag"
    assert pdir.is_dir() and not (tmp_path / "results" / "t1" / "pred").exists()
    metric = Y.VOCMApMetric(iou_thresh=0.5, class_names=ds.classes)
    nrows = 0
    for idx in range(nsamp):
        img, label = ds[idx]
        _, gt, _ = tf(img, label, idx)
        img_path = ds.sample_path(idx)
        fid = os.path.split(img_path)[1].split(".")[0]
        with open(pdir / (fid + ".txt")) as f:
            lines = [ln.rstrip().split(",") for ln in f if ln.strip()]
        assert all(ln[0] == img_path and ln[1] == "0" for ln in lines), "an agnostic model writes id 0 on every row"
        pred = np.array([[float(v) for v in ln[1:7]] for ln in lines], dtype=np.float64).reshape(-1, 6)
        nrows += len(lines)
        metric.update([pred[:, 2:6]], [pred[:, 0]], [pred[:, 1]], [gt[:, :4] / size], [gt[:, 4]], [gt[:, 5]])
    assert nrows > 10, "fixture produced (almost) no detections"
    names, values = out
    aps_r, map_r = metric.get()
    assert abs(values[-1] - map_r) <= 1e-3 or (np.isnan(values[-1]) and np.isnan(map_r)), (values[-1], map_r)
    assert np.allclose(values[:-1], aps_r, atol=1e-3, equal_nan=True)
    assert "mAP={:.4f}".format(values[-1]) in printed
    with open(tmp_path / "results" / "t1" / "voc_ag.txt") as f:
        res = [ln.split() for ln in f if ln.strip()]
    assert [r[0] for r in res] == list(names) and res[-1][0] == "mAP"
