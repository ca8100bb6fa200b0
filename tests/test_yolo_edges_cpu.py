"""Self-checks of the detection-head edge fixtures (tests/yolo_edge_fixtures.py), without a GPU: every fixture that
tests/test_yolo_edges_gpu.py launches keeps the band rules (no IoU within 1e-4 of a threshold it is compared with, no score
within 2e-6 of valid_thresh, no tied candidate scores) and reaches the kernel branch it is meant for - counted on the fp64
oracle's own numbers."""
import numpy as np
import pytest

from oracle import yolo as Y
from tests import yolo_edge_fixtures as F


def _no_ignore_band(fx):
    assert not (np.abs(fx.ioumax - F.IGNORE_T) < F.IOU_BAND).any(), "an anchor's maximum IoU lies inside the ignore band"


@pytest.mark.parametrize("c,mix", [(20, False), (20, True), (4, False)])
def test_planted_ignore_fixture(c, mix):
    fx = F.planted_loss(c=c, mix=mix)
    _no_ignore_band(fx)
    assert fx.m == 6 and fx.b == 2 and fx.size == 128
    assert not np.array_equal(fx.gt[0], fx.gt[1])
    for bi in range(fx.b):
        hi, lo = np.asarray(fx.planted_hi[bi]), np.asarray(fx.planted_lo[bi])
        assert len(hi) >= 30 and len(lo) >= 30 and not fx.positive[bi, hi].any() and not fx.positive[bi, lo].any()
        assert (fx.ioumax[bi, hi] >= F.PLANT_HI).all() and (fx.merged[0][bi, hi, 0] == -1.0).all()
        assert (fx.ioumax[bi, lo] <= F.PLANT_LO).all() and (fx.ioumax[bi, lo] >= 0.25).all() and (fx.merged[0][bi, lo, 0] == 0.0).all()
        nign = int(((fx.ioumax[bi] > F.IGNORE_T) & ~fx.positive[bi]).sum())
        print("image %d: %d non-positive anchors above the ignore threshold, %d planted near misses" % (bi, nign, len(lo)))
        assert nign >= 30 and nign == int(fx.ignored[bi].sum())
    if mix:
        o = fx.targets[0]
        assert ((o > 0) & (o < 1)).sum() >= 9


@pytest.mark.parametrize("m", [0, 1, 16, 17, 40, 256])
def test_m_sweep_fixture(m):
    fx = F.msweep_loss(m)
    _no_ignore_band(fx)
    assert fx.m == m and sum(g * g for g in fx.grids) == 189 and m <= F.LOSS_MAX_GT
    if m == 0:
        assert fx.gt.shape == (2, 0, 4) and not fx.ignored.any() and not fx.positive.any() and (fx.merged[0] == 0).all()
        return
    assert not np.array_equal(fx.gt[0], fx.gt[1])
    for bi in range(fx.b):
        valid = np.all(fx.gt[bi] >= 0, axis=1)
        assert valid[m - 1], "the last slot holds a box"
        if m >= 16:
            holes = np.nonzero(~valid)[0]
            assert len(holes) >= 2 and holes.max() < m - 1 and valid[holes.min() + 1:].any(), "padding rows sit between valid gts"
        above = fx.iou[bi] > F.IGNORE_T                                        # (P, M)
        nonpos = ~fx.positive[bi]
        only_one = above.sum(axis=1) == 1
        decider = above.argmax(axis=1)
        # every planted anchor is decided by its slot alone, every other slot staying below the lower plant band
        for j, p in fx.sole[bi]:
            assert nonpos[p] and only_one[p] and decider[p] == j and fx.iou[bi, p, j] >= F.PLANT_HI
            assert np.delete(fx.iou[bi, p], j).max(initial=0.0) <= F.PLANT_LO
        assert (nonpos & only_one & (decider == m - 1)).any(), "no anchor is ignored through the last slot alone"
        if m >= 16:                # the last step of the 16-lane maximum (lanes 8..15)
            assert (nonpos & only_one & (decider % 16 >= 8)).any()
        if m >= 17:                # the second trip of the gt loop
            late_only = nonpos & above[:, 16:].any(axis=1) & ~above[:, :16].any(axis=1)
            print("M=%d image %d: %d anchors ignored only through a slot >= 16" % (m, bi, int(late_only.sum())))
            assert late_only.sum() >= 10
            assert (fx.iou[bi][late_only][:, :16].max(axis=1) <= F.IGNORE_T - F.IOU_BAND).all()


def test_grid_stride_fixture():
    fx = F.plain_loss(64, 4, 96, 3)
    _no_ignore_band(fx)
    R = sum(g * g for g in fx.grids)
    assert (R + 3) // 4 == 48 and F.loss_blocks(64, fx.grids) == 33 == 2048 // 64 + 1      # a second trip of the row loop
    assert len({fx.gt[bi].tobytes() for bi in range(64)}) == 64, "every image has gts of its own"
    assert fx.positive.any(axis=1).all() and fx.ignored.sum() > 0


@pytest.mark.parametrize("b,c,size,m,smooth", [
    (2, 39, 64, 3, True), (2, 40, 64, 3, True), (2, 41, 64, 3, True),          # the label-smoothing weight switches at C = 40
    (2, 3, 64, 3, False), (2, 7, 64, 3, False),                               # ldh == 3 * (5 + C), a multiple of 4
    (2, 20, 32, 3, False),                                                    # grids 1, 2, 4
    (1, 1008, 32, 2, False),                                                  # the largest C the LDS row stage takes
])
def test_shape_edge_fixtures(b, c, size, m, smooth):
    fx = F.plain_loss(b, c, size, m, smooth)
    _no_ignore_band(fx)
    assert fx.positive.sum() >= b
    if smooth:
        sw = min(1.0 / c, 1.0 / 40)
        t = fx.merged[4][fx.positive]
        assert np.isclose(t, sw).any() and np.isclose(t, 1.0 - sw).any()
    if c in (3, 7):
        assert (3 * (5 + c)) % 4 == 0
    if c == 1008:              # 4 waves x (row + 32) floats: exactly 48 KB; one more class is over
        assert 4 * (((3 * (5 + c) + 3) & ~3) + 32) * 4 == 48 * 1024 and 4 * (((3 * (5 + c + 1) + 3) & ~3) + 32) * 4 > 48 * 1024


def test_existing_loss_fixtures_take_the_ignore_branch():
    """tests/test_yolo_gpu.py::test_loss_fwd_bwd asserts count > 0 for its seeds 32..36: the oracle's counts there"""
    from tests import test_yolo_gpu as T
    cfgs = {cfg["seed"]: cfg for cfg in T.test_loss_fwd_bwd.pytestmark[0].args[1]}
    want = {32: 1, 33: 2, 34: 1, 35: 3, 36: 4}
    for seed, n in want.items():
        cfg = cfgs[seed]
        b, c, size, m = cfg["b"], cfg["c"], cfg["size"], cfg["m"]
        grids = F.grids_of(size)
        rng = np.random.default_rng(seed)
        heads = T._heads(rng, b, c, grids, -1.0)
        gt, ids = T._gt(rng, b, m, size, c, cfg["nvalid"])
        fx, _ = F.loss_reference(b, c, size, gt, ids, heads, cfg["smooth"])
        assert int(fx.ignored.sum()) == n, (seed, int(fx.ignored.sum()))


@pytest.mark.parametrize("name", sorted(F.DECODE_CASES))
def test_decode_fixture(name):
    fx = F.decode_fixture(name)
    assert not (np.abs(fx.score - F.VALID_T) < F.VALID_BAND).any()
    A = 3 * (5 + fx.c)
    RW = (A + 3) & ~3
    per_block = F.decode_rows_per_block(fx)
    assert per_block.sum(axis=1).tolist() == [len(v) for v in fx.valid]
    print("%s: %s candidates, busiest workgroup %d" % (name, [len(v) for v in fx.valid], per_block.max()))
    vec = fx.ldh % 4 == 0 and RW <= 1024
    assert vec == (name in ("c20", "c80", "allpass_c200"))
    assert (name == "c337") == (RW > 1024) and (name == "c20_ldh75") == (fx.ldh == A and A % 4 != 0)
    if name == "allpass_c200":
        assert per_block.max() > F.DF_LCAP and all(len(v) > 0.99 * fx.c * 567 for v in fx.valid)
    else:
        assert all(0 < len(v) < fx.c * 567 for v in fx.valid)


def _check_candidates(agnostic, ns):
    cs = F.nms_case(agnostic, ns)
    for bi, n in enumerate(ns):
        rows, sc = cs.cand_row[bi, :n].astype(np.int64), cs.cand_score[bi, :n]
        assert len(np.unique(rows)) == n and len(np.unique(sc)) == n, "tied scores or repeated rows"
        assert n == 0 or sc.min() > F.VALID_T + F.VALID_BAND
        assert (cs.masked[bi, :, 1] > F.VALID_T).sum() == n
        assert n == 0 or sc[n - 1] == sc.max(), "the best candidate sits in the last slot"
        if n > 1:
            assert len(F._band_rows(cs.base.alldet[bi], rows)) == 0, "a top-k pair's IoU lies inside an NMS band"
    return cs


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("ns", F.NMS_COUNT_BATCHES)
def test_nms_count_fixtures(agnostic, ns):
    _check_candidates(agnostic, ns)
    ref = F.nms_reference(agnostic, ns, 0.45, 400, 100)
    for bi, n in enumerate(ns):
        assert ref.nsel[bi] == min(n, 400) and (n < 399 or ref.nkept[bi] < ref.nsel[bi]), "the sweep suppresses nothing"
        assert (ref.rows[bi] >= 0).sum() == min(ref.nkept[bi], 100)
    assert sorted(n for b in F.NMS_COUNT_BATCHES for n in b) == [0, 1, 399, 400, 401, 1023, 1024, 1025, 5000]
    assert (0, 1024, 5000) in F.NMS_COUNT_BATCHES and F.SORT_N == 1024


@pytest.mark.parametrize("agnostic", [False, True])
def test_nms_param_fixtures(agnostic):
    _check_candidates(agnostic, F.NMS_PARAM_NS)
    assert len(F.NMS_PARAM_CASES) <= 8                                   # two kernels: at most 16 launches
    assert {k for k, _, _ in F.NMS_PARAM_CASES} == {1, 511, 512} and {p for _, p, _ in F.NMS_PARAM_CASES} == {1, 100, 600}
    assert {t for _, _, t in F.NMS_PARAM_CASES} == {0.3, 0.7} and F.TOPK_MAX == 512
    for topk, post, thresh in F.NMS_PARAM_CASES:
        ref = F.nms_reference(agnostic, F.NMS_PARAM_NS, thresh, topk, post)
        assert topk == 1 or min(ref.nkept) < topk, "the sweep suppresses nothing (at 0.7 only a few pairs overlap enough)"
        for bi in range(2):
            assert ref.nsel[bi] == topk and 1 <= ref.nkept[bi] <= topk
            if topk > 1 and thresh < 0.5:
                assert ref.nkept[bi] < topk - 50, "the sweep suppresses next to nothing"
            if post > topk:
                assert (ref.rows[bi, topk:] == -1).all() and (ref.boxes[bi, topk:] == -1).all()
