"""GPU parity: fused decode+filter, top-k + per-class NMS, and the fused IoU-matching loss vs the
fp64 oracle (oracle/yolo.py).  Post-NMS row indices must be identical; boxes/scores within 1e-3
(north_star tolerance), losses within 1e-3 relative."""
import numpy as np
import pytest
import torch

from oracle import yolo as Y
from tests.util import dev, nchw_to_dev_nhwc, maxdiff

pytestmark = pytest.mark.gpu


def _heads(rng, b, c, grids, obj_bias, cls_bias=0.0):
    heads = []
    for g in grids:
        p = rng.standard_normal((b, 3 * (5 + c), g, g))
        p = p.reshape(b, 3, 5 + c, g, g)
        p[:, :, 2:4] *= 0.5
        p[:, :, 4] = p[:, :, 4] * 2.0 + obj_bias
        p[:, :, 5:] = p[:, :, 5:] * 2.0 + cls_bias
        heads.append(p.reshape(b, 3 * (5 + c), g, g).astype(np.float32).astype(np.float64))
    return heads


def _desc(ops, heads_np, c, b):
    grids = [h.shape[2] for h in heads_np]
    ldh = ops.round_up(3 * (5 + c), 32)
    hd = [nchw_to_dev_nhwc(h, ldh) for h in heads_np]
    return ops.make_head_desc(hd, grids, ldh, Y.OUT_STRIDES, Y.OUT_ANCHORS, b, c), hd, grids, ldh


def _oracle_detect(heads, c, topk=400, post=100):
    dets = [Y.yolo_output(h, c, Y.OUT_ANCHORS[s], Y.OUT_STRIDES[s], training=False) for s, h in enumerate(heads)]
    return Y.detect_postprocess(dets, 0.45, topk, post), np.concatenate(dets, axis=1)


@pytest.mark.parametrize("cfg", [
    dict(b=2, c=20, grids=[3, 6, 12], obj_bias=-1.0, seed=21),           # few candidates (<1024): direct sort path
    dict(b=2, c=20, grids=[13, 26, 52], obj_bias=-2.5, seed=22),         # radix-select path
    dict(b=1, c=80, grids=[7, 14, 28], obj_bias=-2.0, seed=23),          # C > 64: two class sweeps per anchor
    dict(b=3, c=4, grids=[2, 4, 8], obj_bias=-9.0, seed=24),             # (almost) nothing passes
    dict(b=1, c=20, grids=[5, 10, 20], obj_bias=3.0, cls_bias=2.0, seed=25),   # everything passes, heavy overlap
    dict(b=2, c=285, grids=[4, 8, 16], obj_bias=-2.0, seed=28),          # combined set (configs[4]): A = 870, 5 class sweeps
    dict(b=1, c=285, grids=[19, 38, 76], obj_bias=-3.0, seed=29),        # ... at the full 608x608 grids (C*P = 6.48 M rows)
])
def test_decode_filter_nms(cfg):
    from viddet_amd import ops
    b, c, grids = cfg["b"], cfg["c"], cfg["grids"]
    # fp32 (device) and fp64 (oracle) sigmoids may disagree only for scores within ~1e-6 of valid_thresh.
    # Such a row sits at the very bottom of the ranking, so it can change the result only when fewer than
    # topk rows are valid: in that case pick the next seed whose fixture has no borderline score.
    for seed in range(cfg["seed"], cfg["seed"] + 1000, 100):
        rng = np.random.default_rng(seed)
        heads = _heads(rng, b, c, grids, cfg["obj_bias"], cfg.get("cls_bias", 0.0))
        (ids_r, sc_r, bx_r, rows_r), alldet = _oracle_detect(heads, c)
        border = np.abs(alldet[..., 1] - 0.01) < 2e-6
        nvalid = (alldet[..., 1] > 0.01).sum(axis=1)
        if not np.any(border.any(axis=1) & (nvalid <= 400)):
            break
    else:
        raise AssertionError("no tie-free fixture found")
    h, hd, _, _ = _desc(ops, heads, c, b)
    P = 3 * sum(g * g for g in grids)
    cap = c * P
    cs = torch.empty(b, cap, device="cuda")
    cr = torch.empty(b, cap, dtype=torch.int32, device="cuda")
    cnt = torch.empty(b, dtype=torch.int32, device="cuda")
    ops.yolo_decode_filter(h, 0.01, cs, cr, cap, cnt)
    ids = torch.empty(b, 100, device="cuda"); sc = torch.empty(b, 100, device="cuda")
    bx = torch.empty(b, 100, 4, device="cuda"); rows = torch.empty(b, 100, dtype=torch.int32, device="cuda")
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ops.nms_topk(h, cs, cr, cap, cnt, 0.45, 400, 100, ids, sc, bx, rows, ws)
    torch.cuda.synchronize()
    # candidate set == oracle's valid set (margin-checked: fp32 vs fp64 sigmoid can only differ at the threshold)
    for bi in range(b):
        s64 = alldet[bi, :, 1]
        n = int(cnt[bi])
        got = set(cr[bi, :n].cpu().numpy().tolist())
        want = set(np.nonzero(s64 > 0.01)[0].tolist())
        assert (got ^ want) <= set(np.nonzero(border[bi])[0].tolist()), "candidate set differs beyond the threshold band"
    assert np.array_equal(rows.cpu().numpy().astype(np.int64), rows_r), "post-NMS row indices differ"
    assert np.array_equal(ids.cpu().numpy(), ids_r[..., 0])
    assert maxdiff(sc.cpu().numpy(), sc_r[..., 0]) < 1e-5
    assert maxdiff(bx.cpu().numpy(), bx_r) < 1e-3


def test_nms_all_pass_with_exact_score_ties_keeps_row_order():
    """Every one of the C*P rows passes valid_thresh and the scores take only ~40 distinct values, so thousands of rows
    tie exactly at the top-400 threshold: the kept set must be the oracle's (stable sort = lowest original rows first,
    SURVEY A.2), whatever order the filter's atomics appended the candidates in.  Objectness logits of +20 make
    sigmoid(obj) == 1.0f on the device and 1 - 2e-9 in the fp64 oracle - a common factor - and class logits on a 0.1
    grid keep distinct scores >= 1e-3 apart, so both sides rank identically and tie exactly where the logits are equal."""
    from viddet_amd import ops
    b, c, grids = 2, 20, [5, 10, 20]
    rng = np.random.default_rng(27)
    heads = _heads(rng, b, c, grids, 0.0)
    for hh in heads:
        v = hh.reshape(b, 3, 5 + c, hh.shape[2], hh.shape[3])
        v[:, :, 4] = 20.0
        v[:, :, 5:] = np.round(rng.uniform(-2.0, 2.0, v[:, :, 5:].shape) * 10.0) / 10.0
    (ids_r, sc_r, bx_r, rows_r), alldet = _oracle_detect(heads, c)
    assert (alldet[..., 1] > 0.01).all()
    kth = np.sort(alldet[0, :, 1])[-400]
    assert (alldet[0, :, 1] == kth).sum() > 50, "fixture has no mass tie at the top-k threshold"
    h, hd, _, _ = _desc(ops, heads, c, b)
    cap = c * 3 * sum(g * g for g in grids)
    cs = torch.empty(b, cap, device="cuda"); cr = torch.empty(b, cap, dtype=torch.int32, device="cuda")
    cnt = torch.empty(b, dtype=torch.int32, device="cuda")
    ids = torch.empty(b, 100, device="cuda"); sc = torch.empty(b, 100, device="cuda")
    bx = torch.empty(b, 100, 4, device="cuda"); rows = torch.empty(b, 100, dtype=torch.int32, device="cuda")
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")
    first = None
    for rep in range(3):                    # the append order differs from launch to launch; the result must not
        ops.yolo_decode_filter(h, 0.01, cs, cr, cap, cnt)
        ops.nms_topk(h, cs, cr, cap, cnt, 0.45, 400, 100, ids, sc, bx, rows, ws)
        torch.cuda.synchronize()
        assert int(cnt.min()) == cap and int(ws.view(torch.int32)[:b].max()) == 0
        got = rows.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, rows_r), "post-NMS row indices differ under exact score ties"
        first = got if first is None else first
        assert np.array_equal(got, first)
    assert np.array_equal(ids.cpu().numpy(), ids_r[..., 0])
    assert maxdiff(bx.cpu().numpy(), bx_r) < 1e-3


def test_decode_filter_cap_overflow_reported():
    from viddet_amd import ops
    b, c, grids = 1, 20, [5, 10, 20]
    rng = np.random.default_rng(26)
    heads = _heads(rng, b, c, grids, 3.0, 2.0)
    h, hd, _, _ = _desc(ops, heads, c, b)
    cap = 2048
    cs = torch.empty(b, cap, device="cuda"); cr = torch.empty(b, cap, dtype=torch.int32, device="cuda")
    cnt = torch.empty(b, dtype=torch.int32, device="cuda")
    ops.yolo_decode_filter(h, 0.01, cs, cr, cap, cnt)
    ids = torch.empty(b, 100, device="cuda"); sc = torch.empty(b, 100, device="cuda")
    bx = torch.empty(b, 100, 4, device="cuda"); rows = torch.empty(b, 100, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4 * b, dtype=torch.uint8, device="cuda")
    ops.nms_topk(h, cs, cr, cap, cnt, 0.45, 400, 100, ids, sc, bx, rows, ws)
    torch.cuda.synchronize()
    assert int(cnt[0]) > cap
    assert int(ws.view(torch.int32)[0]) == int(cnt[0])   # overflow is reported, never silent


def _gt(rng, b, m, size, c, nvalid):
    gt = np.full((b, m, 4), -1.0)
    ids = np.full((b, m, 1), -1.0)
    for bi in range(b):
        for j in range(nvalid[bi]):
            cx, cy = rng.uniform(0.1, 0.9, 2) * size
            w, h = rng.uniform(8, 0.5 * size, 2)
            gt[bi, j] = [max(cx - w / 2, 0), max(cy - h / 2, 0), min(cx + w / 2, size - 1), min(cy + h / 2, size - 1)]
            ids[bi, j, 0] = rng.integers(0, c)
    return gt, ids


@pytest.mark.parametrize("cfg", [
    dict(b=2, c=20, size=96, m=4, nvalid=[3, 1], smooth=False, seed=31),
    dict(b=3, c=80, size=160, m=6, nvalid=[6, 0, 2], smooth=False, seed=32),     # an image with no gt
    dict(b=2, c=20, size=128, m=5, nvalid=[5, 4], smooth=True, seed=33),         # label smoothing
    dict(b=1, c=30, size=416, m=8, nvalid=[8], smooth=False, seed=34),           # full 416 grid
    dict(b=2, c=285, size=96, m=5, nvalid=[4, 2], smooth=False, seed=35),        # combined set: 285 classes
    dict(b=1, c=285, size=608, m=8, nvalid=[8], smooth=True, seed=36),           # ... one full 608x608 frame, smoothed
    dict(b=2, c=20, size=128, m=6, nvalid=[6, 3], smooth=False, seed=37, mix=True),   # --mixup: objectness targets = mix ratios
])
def test_loss_fwd_bwd(cfg):
    from viddet_amd import ops
    b, c, size, m = cfg["b"], cfg["c"], cfg["size"], cfg["m"]
    grids = [size // 32, size // 16, size // 8]
    rng = np.random.default_rng(cfg["seed"])
    heads = _heads(rng, b, c, grids, -1.0)
    gt, ids = _gt(rng, b, m, size, c, cfg["nvalid"])
    # make some predictions overlap a gt strongly so the ignore branch (IoU > 0.7) is exercised
    # --mixup (yolo_target.py:124-125): a positive's objectness target is its box's mix ratio in (0, 1) - it then weights
    # the objectness term, the box terms and the class mask
    mix = rng.uniform(0.05, 0.95, (b, m, 1)) if cfg.get("mix") else None
    targets = Y.prefetch_targets(size, size, grids, gt, ids, c, mix)
    obj_t, ctr_t, scl_t, wgt_t, cls_t = targets
    if mix is not None:
        assert ((obj_t > 0) & (obj_t < 1)).sum() >= sum(cfg["nvalid"]) - 2
    # oracle
    outs = [Y.yolo_output(hh, c, Y.OUT_ANCHORS[s], Y.OUT_STRIDES[s], training=True) for s, hh in enumerate(heads)]
    box = np.concatenate([o[0] for o in outs], axis=1)
    rawc = np.concatenate([o[1].reshape(b, -1, 2) for o in outs], axis=1)
    raws = np.concatenate([o[2].reshape(b, -1, 2) for o in outs], axis=1)
    obj = np.concatenate([o[3].reshape(b, -1, 1) for o in outs], axis=1)
    cls = np.concatenate([o[4].reshape(b, -1, c) for o in outs], axis=1)
    merged = Y.merge_targets(box, gt, obj_t, ctr_t, scl_t, wgt_t, cls_t, c, 0.7, cfg["smooth"])
    losses_r, grads_r = Y.yolo3_loss(obj, rawc, raws, cls, *merged, with_grads=True)
    # device
    h, hd, _, ldh = _desc(ops, heads, c, b)
    dheads = [torch.full_like(t, 5.0) for t in hd]
    P = box.shape[1]
    losses = torch.empty(b, 4, device="cuda")
    box_out = torch.empty(b, P, 4, device="cuda")
    ws = torch.empty(max(16, ops.yolo_loss_ws_bytes(h)), dtype=torch.uint8, device="cuda")
    ops.yolo_loss_fwd_bwd(h, dev(gt), m, dev(obj_t), dev(ctr_t), dev(scl_t), dev(wgt_t), dev(cls_t), 0.7, cfg["smooth"],
                          losses, dheads, box_out, ws)
    torch.cuda.synchronize()
    assert maxdiff(box_out.cpu().numpy(), box) < 1e-3
    lr = np.stack(losses_r, axis=1)
    got = losses.cpu().numpy()
    assert np.all(np.abs(got - lr) <= 1e-3 * np.maximum(1.0, np.abs(lr))), (got, lr)
    # gradients: map the oracle's (B,P,k) gradients back to the head layout [B,g,g,a*(5+C)+j]
    g_obj, g_ctr, g_scl, g_cls = grads_r
    off = 0
    for s, g in enumerate(grids):
        n = g * g * 3
        ref = np.concatenate([g_ctr[:, off:off + n], g_scl[:, off:off + n], g_obj[:, off:off + n],
                              g_cls[:, off:off + n]], axis=-1).reshape(b, g, g, 3 * (5 + c))
        d = dheads[s].cpu().numpy()
        assert maxdiff(d[..., :3 * (5 + c)], ref) < 1e-5
        assert float(np.abs(d[..., 3 * (5 + c):]).max(initial=0.0)) == 0.0
        off += n
    # the ignore branch was really taken somewhere (dynamic IoU > 0.7 on a non-positive anchor): seeds 32..36 have 1, 2, 1, 3
    # and 4 such anchors by the oracle (31 and 37 have none; tests/test_yolo_edges_gpu.py plants them by the dozen)
    if 32 <= cfg["seed"] <= 36:
        assert ((merged[0] < 0) & ~(obj_t > 0)).sum() > 0
