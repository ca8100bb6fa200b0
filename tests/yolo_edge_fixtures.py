"""Fixtures of the detection-head edge tests: built once (cached), checked by tests/test_yolo_edges_cpu.py without a GPU and
run on the device by tests/test_yolo_edges_gpu.py (and tests/yolo_rows_child.py).  The reference is oracle/yolo.py in fp64.

Band rules.  The device computes IoU and sigmoid in fp32, the oracle in fp64, so a comparison against a threshold (0.7 ignore,
the NMS thresholds, 0.01 valid) may differ inside a narrow band: fp32 IoU error is a few 1e-7 relative, the band is 1e-4 (a
100x margin); for the valid threshold it is the 2e-6 of tests/test_yolo_gpu.py.  A fixture has NO value inside a band: a seed
that has one is stepped (at most MAX_SEEDS seeds, then an error) and no anchor is ever masked out of a comparison.
Every head holds fp32-representable values, so the device and the oracle read the same numbers."""
import functools
import math
from types import SimpleNamespace

import numpy as np

from oracle import yolo as Y

IGNORE_T, IOU_BAND = 0.7, 1e-4
VALID_T, VALID_BAND = 0.01, 2e-6
PLANT_HI, PLANT_LO = 0.8, 0.6          # a planted prediction's IoU lies in one of two bands: >= 0.8 or <= 0.6
MAX_SEEDS = 10
LOSS_MAX_GT, DF_LCAP, SORT_N, TOPK_MAX = 256, 2048, 1024, 512      # the kernels' constants the cases are built around


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def grids_of(size):
    return [size // 32, size // 16, size // 8]


def loss_blocks(b, grids):
    """the loss (and row-streaming decode) grid: one workgroup per four head rows, capped at 2048 / B + 1"""
    return max(1, min((sum(g * g for g in grids) + 3) // 4, 2048 // b + 1))


def random_heads(rng, b, c, grids, obj_bias, cls_bias=0.0, live=None):
    """live: instead of one broad objectness distribution, that fraction of the anchors is confident (logit 2 +- 0.5, class
    logits 1.5 +- 1.5: nearly every class passes valid_thresh = 0.01) and the rest is dead (logit -9 +- 0.3).  The density of
    scores around valid_thresh is then low enough for a tensor of 1e5 rows to have none inside the 2e-6 band."""
    heads = []
    for g in grids:
        p = rng.standard_normal((b, 3, 5 + c, g, g))
        p[:, :, 2:4] *= 0.5
        if live is None:
            p[:, :, 4] = p[:, :, 4] * 2.0 + obj_bias
            p[:, :, 5:] = p[:, :, 5:] * 2.0 + cls_bias
        else:
            p[:, :, 4] = np.where(rng.random(p[:, :, 4].shape) < live, p[:, :, 4] * 0.5 + 2.0, p[:, :, 4] * 0.3 - 9.0)
            p[:, :, 5:] = p[:, :, 5:] * 1.5 + 1.5
        heads.append(p.reshape(b, 3 * (5 + c), g, g))
    return heads


def first_clear(build, seed0):
    """build(seed) -> (fixture, number of values inside a band); the first of MAX_SEEDS seeds with none"""
    for seed in range(seed0, seed0 + MAX_SEEDS):
        fx, nband = build(seed)
        if nband == 0:
            fx.seed = seed
            return fx
    raise AssertionError("no band-free fixture among seeds %d..%d" % (seed0, seed0 + MAX_SEEDS - 1))


# ---------------------------------------------------------------------------------------------
# planted predictions
# ---------------------------------------------------------------------------------------------
def plant(heads, c, s, bi, cy, cx, a, box):
    """Raw logits of anchor `a` of cell (cy, cx) of head `s`, image `bi`, whose decode is `box` (x1, y1, x2, y2):
    raw_xy = logit(centre / stride - cell), raw_wh = log(size / anchor)."""
    stride = Y.OUT_STRIDES[s]
    aw, ah = Y.OUT_ANCHORS[s][2 * a], Y.OUT_ANCHORS[s][2 * a + 1]
    g = heads[s].shape[2]
    fx, fy = (box[0] + box[2]) / 2 / stride - cx, (box[1] + box[3]) / 2 / stride - cy
    assert 0.0 < fx < 1.0 and 0.0 < fy < 1.0 and 0 <= cx < g and 0 <= cy < g
    v = heads[s].reshape(heads[s].shape[0], 3, 5 + c, g, g)               # (a view: the heads are contiguous)
    v[bi, a, 0, cy, cx] = math.log(fx / (1.0 - fx))
    v[bi, a, 1, cy, cx] = math.log(fy / (1.0 - fy))
    v[bi, a, 2, cy, cx] = math.log((box[2] - box[0]) / aw)
    v[bi, a, 3, cy, cx] = math.log((box[3] - box[1]) / ah)


def _iou1(box, gts):
    iw = np.maximum(np.minimum(box[2], gts[:, 2]) - np.maximum(box[0], gts[:, 0]), 0.0)
    ih = np.maximum(np.minimum(box[3], gts[:, 3]) - np.maximum(box[1], gts[:, 1]), 0.0)
    i = iw * ih
    return i / ((box[2] - box[0]) * (box[3] - box[1]) + (gts[:, 2] - gts[:, 0]) * (gts[:, 3] - gts[:, 1]) - i + 1e-15)


def plant_copies(rng, heads, c, grids, gt_b, bi, taken, j, n, band, others_max=None, strict=True):
    """Plants n jittered copies of gt j of image bi on anchors not in `taken` (the positives and earlier plants; extended).
    band 'hi': IoU with gt j >= 0.82 (and, with others_max, IoU with every other gt <= others_max: gt j alone decides the
    ignore flag); band 'lo': the maximum IoU over all gts in [0.3, 0.58] - a near miss.  Returns the anchor indices (fewer than
    n only with strict=False: a gt's neighbourhood has nine anchors per cell)."""
    offs = np.concatenate([[0], np.cumsum([3 * g * g for g in grids])])
    x1, y1, x2, y2 = gt_b[j]
    w, h, cx, cy = x2 - x1, y2 - y1, (x1 + x2) / 2, (y1 + y2) / 2
    out = []
    for _ in range(4000):
        if len(out) == n:
            return out
        if band == 'hi':
            sw, sh = rng.uniform(0.96, 1.04, 2)
            dx, dy = rng.uniform(-0.07, 0.07, 2) * (w, h)
        else:
            sw, sh = rng.uniform(0.62, 0.85, 2)
            dx, dy = rng.uniform(-0.12, 0.12, 2) * (w, h)
        nw, nh, ncx, ncy = w * sw, h * sh, cx + dx, cy + dy
        box = np.array([ncx - nw / 2, ncy - nh / 2, ncx + nw / 2, ncy + nh / 2])
        s, a = int(rng.integers(3)), int(rng.integers(3))
        stride, g = Y.OUT_STRIDES[s], grids[s]
        cell_x, cell_y = int(ncx // stride), int(ncy // stride)
        if not (0 <= cell_x < g and 0 <= cell_y < g):
            continue
        if not (0.02 < ncx / stride - cell_x < 0.98 and 0.02 < ncy / stride - cell_y < 0.98):
            continue
        p = int(offs[s]) + (cell_y * g + cell_x) * 3 + a
        if p in taken:
            continue
        iou = _iou1(box, gt_b)
        if band == 'hi':
            if iou[j] < 0.82 or (others_max is not None and np.delete(iou, j).max(initial=0.0) > others_max):
                continue
        elif not (0.3 <= iou.max() <= 0.58):
            continue
        plant(heads, c, s, bi, cell_y, cell_x, a, box)
        taken.add(p)
        out.append(p)
    if len(out) == n or not strict:
        return out
    raise AssertionError("could not plant %d '%s' copies of gt %d of image %d" % (n, band, j, bi))


# ---------------------------------------------------------------------------------------------
# loss fixtures
# ---------------------------------------------------------------------------------------------
def make_gt(rng, b, m, size, c, valid, wh=(8.0, 40.0), mutual=0.4, corner=()):
    """gt (B, M, 4) / ids (B, M, 1), -1 padded; valid[bi] = the slots of image bi that hold a box (holes allowed: the target
    generator stops at the first padding row, the ignore mask looks at every slot).  Boxes of one image overlap each other
    by IoU <= mutual, so a jittered copy of one is not also a near-copy of another.  A slot in `corner` gets a large box centred
    on a cell corner of all three grids, so that slightly shifted copies of it fall into four cells of each (a dozen anchors
    per grid instead of three)."""
    gt = np.full((b, m, 4), -1.0)
    ids = np.full((b, m, 1), -1.0)
    for bi in range(b):
        boxes = np.zeros((0, 4))
        for j in valid[bi]:
            for _ in range(2000):
                cx, cy = rng.uniform(0.1, 0.9, 2) * size
                w, h = rng.uniform(wh[0], wh[1], 2)
                if j in corner:
                    cx, cy = 32.0 * (size // 64) + rng.uniform(-0.3, 0.3, 2)
                    w, h = rng.uniform(0.4 * size, 0.6 * size, 2)
                bx = np.array([max(cx - w / 2, 0), max(cy - h / 2, 0), min(cx + w / 2, size - 1), min(cy + h / 2, size - 1)])
                if len(boxes) == 0 or _iou1(bx, boxes).max() <= mutual:
                    break
            else:
                raise AssertionError("no room for gt %d of image %d" % (j, bi))
            boxes = np.concatenate([boxes, bx[None]])
            gt[bi, j] = bx
            ids[bi, j, 0] = rng.integers(0, c)
    return f32(gt), ids


def loss_reference(b, c, size, gt, ids, heads, smooth=False, mix=None, targets=None):
    """The oracle's whole answer for one loss launch."""
    grids = grids_of(size)
    m = gt.shape[1]
    if targets is None:
        targets = Y.prefetch_targets(size, size, grids, gt, ids, c, mix)
    obj_t, ctr_t, scl_t, wgt_t, cls_t = targets
    outs = [Y.yolo_output(hh, c, Y.OUT_ANCHORS[s], Y.OUT_STRIDES[s], training=True) for s, hh in enumerate(heads)]
    box = np.concatenate([o[0] for o in outs], axis=1)
    rawc = np.concatenate([o[1].reshape(b, -1, 2) for o in outs], axis=1)
    raws = np.concatenate([o[2].reshape(b, -1, 2) for o in outs], axis=1)
    obj = np.concatenate([o[3].reshape(b, -1, 1) for o in outs], axis=1)
    cls = np.concatenate([o[4].reshape(b, -1, c) for o in outs], axis=1)
    merged = Y.merge_targets(box, gt, obj_t, ctr_t, scl_t, wgt_t, cls_t, c, IGNORE_T, smooth)
    losses_r, (g_obj, g_ctr, g_scl, g_cls) = Y.yolo3_loss(obj, rawc, raws, cls, *merged, with_grads=True)
    grads, off = [], 0
    for g in grids:                              # the oracle's (B, P, k) gradients in the head layout [B, g, g, a*(5+C)+j]
        n = g * g * 3
        grads.append(np.concatenate([g_ctr[:, off:off + n], g_scl[:, off:off + n], g_obj[:, off:off + n],
                                     g_cls[:, off:off + n]], axis=-1).reshape(b, g, g, 3 * (5 + c)))
        off += n
    iou = Y.bbox_batch_iou(box, gt) if m else np.zeros(box.shape[:2] + (0,))
    ioumax = iou.max(axis=-1) if m else np.full(box.shape[:2], -1.0)
    positive = obj_t[..., 0] > 0
    fx = SimpleNamespace(b=b, c=c, size=size, m=m, grids=grids, gt=gt, ids=ids, heads=heads, smooth=smooth, mix=mix,
                         targets=targets, box=box, merged=merged, losses=np.stack(losses_r, axis=1), grads=grads, iou=iou,
                         ioumax=ioumax, positive=positive, ignored=(merged[0][..., 0] < 0) & ~positive)
    return fx, int((np.abs(ioumax - IGNORE_T) < IOU_BAND).sum())


@functools.lru_cache(maxsize=None)
def planted_loss(c=20, mix=False, b=2, size=128, m=6, seed0=4100):
    """Case A1: per image >= 30 non-positive anchors planted above the ignore threshold and >= 30 planted near misses."""
    def build(seed):
        rng = np.random.default_rng(seed)
        grids = grids_of(size)
        valid = [list(range(m)), list(range(m - 1))][:b] + [list(range(m))] * max(0, b - 2)
        gt, ids = make_gt(rng, b, m, size, c, valid, wh=(20.0, 60.0))
        mx = rng.uniform(0.05, 0.95, (b, m, 1)) if mix else None
        targets = Y.prefetch_targets(size, size, grids, gt, ids, c, mx)
        heads = random_heads(rng, b, c, grids, -1.0)
        hi, lo = [], []
        for bi in range(b):
            taken = set(np.nonzero(targets[0][bi, :, 0] > 0)[0].tolist())
            nv = len(valid[bi])
            for band, dst in (('hi', hi), ('lo', lo)):
                dst.append(sum((plant_copies(rng, heads, c, grids, gt[bi, :nv], bi, taken, j, 8, band, strict=False)
                                for j in range(nv)), []))
                assert len(dst[-1]) >= 30, "image %d: only %d '%s' plants" % (bi, len(dst[-1]), band)
        fx, nband = loss_reference(b, c, size, gt, ids, [f32(h) for h in heads], False, mx, targets)
        fx.planted_hi, fx.planted_lo = hi, lo
        return fx, nband
    return first_clear(build, seed0)


def msweep_valid(m, bi):
    """valid gt slots of image bi of the M sweep: padding rows BETWEEN valid gts (not only at the tail), the last slot valid"""
    holes = {0: (7, 19, m - 3), 1: (5, 21, m - 4)}[bi] if m >= 16 else ()
    return [j for j in range(m) if j not in holes]


def msweep_deciders(m, valid):
    """the gt slots that each get anchors only THEY push over the ignore threshold: for M >= 17 ten picks among the slots >= 16
    (the second trip of the 16-lane gt loop), the last slot first; slots 8..15 (the 16-lane maximum's last step); slot M - 1"""
    late = [j for j in valid if j >= 16]
    picks = []
    if late:
        picks = [m - 1] + [late[(i * len(late)) // 9] for i in range(9)]
    picks += [j for j in valid if 8 <= j < 16][-3:]
    if m and m - 1 not in picks:
        picks.append(m - 1)
    return picks


@functools.lru_cache(maxsize=None)
def msweep_loss(m, b=2, c=4, size=96, seed0=4200):
    """Case A2: M gt slots at R = 189 head rows."""
    def build(seed):
        rng = np.random.default_rng(seed + 16 * m)
        grids = grids_of(size)
        valid = [msweep_valid(m, bi) for bi in range(b)]
        gt, ids = make_gt(rng, b, m, size, c, valid, wh=(8.0, 40.0), mutual=0.4, corner=(16,) if m == 17 else ())
        targets = Y.prefetch_targets(size, size, grids, gt, ids, c, None)
        heads = random_heads(rng, b, c, grids, -1.0)
        sole = []
        for bi in range(b):
            taken = set(np.nonzero(targets[0][bi, :, 0] > 0)[0].tolist())
            # (padding rows take part as what they are - zero-area boxes - so slot numbers stay the kernel's)
            sole.append([(j, plant_copies(rng, heads, c, grids, gt[bi], bi, taken, j, 1, 'hi', others_max=0.58)[0])
                         for j in msweep_deciders(m, valid[bi])])
        fx, nband = loss_reference(b, c, size, gt, ids, [f32(h) for h in heads], False, None, targets)
        fx.sole, fx.valid = sole, valid
        return fx, nband
    return first_clear(build, seed0)


@functools.lru_cache(maxsize=None)
def plain_loss(b, c, size, m, smooth=False, seed0=4300):
    """random heads, every image with gts of its own (1 + bi % m of them): cases A4 (grid-stride trip) and A6 (shape edges)"""
    def build(seed):
        rng = np.random.default_rng(seed)
        grids = grids_of(size)
        valid = [list(range(1 + bi % m)) for bi in range(b)]
        gt, ids = make_gt(rng, b, m, size, c, valid, wh=(8.0, 0.5 * size))
        heads = [f32(h) for h in random_heads(rng, b, c, grids, -1.0)]
        return loss_reference(b, c, size, gt, ids, heads, smooth)
    return first_clear(build, seed0)


# ---------------------------------------------------------------------------------------------
# decode fixtures (row-streaming form, cap boundary)
# ---------------------------------------------------------------------------------------------
DECODE_GRIDS, DECODE_B = [3, 6, 12], 2
# name -> (C, ldh, objectness bias, class bias, live fraction - see random_heads).  RW = the staged row of k_decode_filter, 3 * (5 + C) rounded up to 4 floats.
DECODE_CASES = {
    "c20": (20, 96, -1.0, 0.0, None),                 # aligned, 16-byte staged path
    "c80": (80, 256, 0.0, 0.0, 0.1),                # two class sweeps per anchor
    "c337": (337, 1056, 0.0, 0.0, 0.1),             # RW = 1028 > 1024: scalar staging
    "c20_ldh75": (20, 75, -1.0, 0.0, None),           # odd pitch, no padding channel: scalar staging
    "allpass_c200": (200, 640, 3.0, 2.0, None),       # 2400 candidates per workgroup > the 2048 LDS slots: direct-to-global appends
}


@functools.lru_cache(maxsize=None)
def decode_fixture(name, seed0=4400):
    c, ldh, ob, cb, live = DECODE_CASES[name]

    def build(seed):
        rng = np.random.default_rng(seed)
        heads = [f32(h) for h in random_heads(rng, DECODE_B, c, DECODE_GRIDS, ob, cb, live)]
        dets = [Y.yolo_output(h, c, Y.OUT_ANCHORS[s], Y.OUT_STRIDES[s], training=False) for s, h in enumerate(heads)]
        score = np.concatenate(dets, axis=1)[..., 1]
        fx = SimpleNamespace(name=name, b=DECODE_B, c=c, ldh=ldh, grids=DECODE_GRIDS, heads=heads, score=score,
                             valid=[np.nonzero(score[bi] > VALID_T)[0] for bi in range(DECODE_B)])
        return fx, int((np.abs(score - VALID_T) < VALID_BAND).sum())
    return first_clear(build, seed0)


def decode_rows_per_block(fx):
    """valid rows per workgroup of the row-streaming form (workgroup k of image bi owns head rows 4 k .. 4 k + 3, one trip)"""
    nb = loss_blocks(fx.b, fx.grids)
    R = sum(g * g for g in fx.grids)
    assert nb * 4 >= R
    out = np.zeros((fx.b, nb), dtype=np.int64)
    off_rows, off_det = 0, 0
    for g in fx.grids:
        sc = fx.score[:, off_det:off_det + fx.c * g * g * 3].reshape(fx.b, fx.c, g * g, 3)
        per_pixel = (sc > VALID_T).sum(axis=(1, 3))                       # (B, g*g)
        for pix in range(g * g):
            out[:, (off_rows + pix) // 4] += per_pixel[:, pix]
        off_rows += g * g
        off_det += fx.c * g * g * 3
    return out


# ---------------------------------------------------------------------------------------------
# NMS fixtures: hand-made candidate lists
# ---------------------------------------------------------------------------------------------
NMS_THRESHOLDS = (0.3, 0.45, 0.7)
NMS_CAP = 5008
NMS_CLASSES = (0, 3, 7, 12, 19)        # per-class candidates come from five of the 20 classes, so that the top-k holds enough
                                       # same-class neighbours for the sweep to suppress some of them


@functools.lru_cache(maxsize=None)
def nms_base(agnostic):
    """the rows candidates are drawn from: per class (B = 3, C = 20, grids [5, 10, 20]: 31500 rows), or the agnostic tensor
    (C = 2, grids [10, 20, 40]: 6300 rows, every id 0)"""
    from tests import agnostic_oracle as AO
    rng = np.random.default_rng(4500 + int(agnostic))
    b, c, grids = (3, 2, [10, 20, 40]) if agnostic else (3, 20, [5, 10, 20])
    heads = [f32(h) for h in random_heads(rng, b, c, grids, -1.0)]
    out = AO.agnostic_output if agnostic else (lambda h, c_, a, s: Y.yolo_output(h, c_, a, s, training=False))
    alldet = np.concatenate([out(h, c, Y.OUT_ANCHORS[s], Y.OUT_STRIDES[s]) for s, h in enumerate(heads)], axis=1)
    return SimpleNamespace(b=b, c=c, grids=grids, heads=heads, alldet=alldet, ldh=32 * ((3 * (5 + c) + 31) // 32))


def _band_rows(d, rows):
    """of the candidate rows `rows` of one image: those among the top TOPK_MAX that sit in a same-class pair whose IoU is
    within IOU_BAND of one of NMS_THRESHOLDS (the later row of each such pair)"""
    top = rows[np.lexsort((rows, -d[rows, 1]))][:TOPK_MAX]
    bx, ids = d[top, 2:6], d[top, 0]
    area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
    iw = np.maximum(0.0, np.minimum(bx[:, None, 2], bx[None, :, 2]) - np.maximum(bx[:, None, 0], bx[None, :, 0]))
    ih = np.maximum(0.0, np.minimum(bx[:, None, 3], bx[None, :, 3]) - np.maximum(bx[:, None, 1], bx[None, :, 1]))
    inter = iw * ih
    union = area[:, None] + area[None, :] - inter
    iou = np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)
    near = np.zeros_like(iou, dtype=bool)
    for t in NMS_THRESHOLDS:
        near |= np.abs(iou - t) < IOU_BAND
    near &= (ids[:, None] == ids[None, :]) & np.triu(np.ones_like(near), 1)
    return top[near.any(axis=0)]


def pick_candidates(d, n, rng, classes=None):
    """n rows of one image's (N, 6) tensor: valid, no two with the same fp32 score, no top-TOPK_MAX pair inside an IoU band"""
    s32 = d[:, 1].astype(np.float32)
    _, first = np.unique(s32, return_index=True)
    pool = first[d[first, 1] > 0.011]
    if classes is not None:
        pool = pool[np.isin(d[pool, 0], classes)]
    pool = pool[rng.permutation(len(pool))]
    rows, spare = pool[:n], list(pool[n:])
    for _ in range(200):
        bad = _band_rows(d, rows) if n > 1 else np.zeros(0, dtype=np.int64)
        if len(bad) == 0:
            return rows[rng.permutation(n)]
        assert len(spare) >= len(bad), "candidate pool exhausted"
        keep = rows[~np.isin(rows, bad)]
        rows = np.concatenate([keep, [spare.pop() for _ in range(len(bad))]]).astype(np.int64)
    raise AssertionError("no band-free candidate list")


@functools.lru_cache(maxsize=None)
def nms_case(agnostic, ns, seed=4600):
    """Candidate lists of ns[bi] rows for image bi (shuffled: the kernels key by (score, row), not by arrival)."""
    base = nms_base(agnostic)
    rng = np.random.default_rng(seed + sum(ns))
    b = len(ns)
    cand_score = np.full((b, NMS_CAP), -7.0, dtype=np.float32)           # (slots beyond the count are never read)
    cand_row = np.full((b, NMS_CAP), -7, dtype=np.int32)
    masked = base.alldet[:b].copy()
    masked[..., 1] = -1.0
    for bi, n in enumerate(ns):
        rows = pick_candidates(base.alldet[bi], n, rng, None if agnostic else NMS_CLASSES)
        if n:                                   # the best candidate sits in the LAST slot: a list cut short by one loses its winner
            top = int(np.argmax(base.alldet[bi, rows, 1]))
            rows[[top, n - 1]] = rows[[n - 1, top]]
        cand_row[bi, :n] = rows
        cand_score[bi, :n] = base.alldet[bi, rows, 1].astype(np.float32)
        masked[bi, rows, 1] = base.alldet[bi, rows, 1]
    return SimpleNamespace(base=base, b=b, ns=tuple(ns), cand_score=cand_score, cand_row=cand_row,
                           counts=np.asarray(ns, dtype=np.int32), masked=masked)


@functools.lru_cache(maxsize=None)
def nms_reference(agnostic, ns, thresh, topk, post):
    """Y.box_nms on the tensor with every non-candidate row's score at -1, then the post_nms slice."""
    cs = nms_case(agnostic, ns)
    out, kept = Y.box_nms(cs.masked, thresh, VALID_T, topk)
    res = np.full((cs.b, post, 6), -1.0)
    rows = np.full((cs.b, post), -1, dtype=np.int64)
    nsel = []
    for bi, k in enumerate(kept):
        k = k[:post]
        res[bi, :len(k)] = cs.masked[bi, k]
        rows[bi, :len(k)] = k
        nsel.append(min(cs.ns[bi], topk))
    return SimpleNamespace(ids=res[..., 0], scores=res[..., 1], boxes=res[..., 2:6], rows=rows,
                           nkept=[len(k) for k in kept], nsel=nsel)


NMS_COUNT_BATCHES = [(0, 1024, 5000), (1, 399, 400), (401, 1023, 1025)]
# (topk, post_nms, nms_thresh): eight of the eighteen, every value at least once (and post_nms = 600 > topk with each topk)
NMS_PARAM_CASES = [(1, 1, 0.3), (1, 600, 0.7), (511, 1, 0.7), (511, 100, 0.3), (511, 600, 0.7), (512, 1, 0.3),
                   (512, 100, 0.7), (512, 600, 0.3)]
NMS_PARAM_NS = (1025, 5000)
