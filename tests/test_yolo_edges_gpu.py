"""GPU: the detection-head kernels (vd_yolo.hip) on the paths tests/test_yolo_gpu.py never takes, against oracle/yolo.py in
fp64.  The fixtures come from tests/yolo_edge_fixtures.py; tests/test_yolo_edges_cpu.py proves without a GPU that each one
keeps the band rules and reaches its branch.  Tolerances are the project's: decoded boxes 1e-3, losses 1e-3 relative against
max(1, |ref|), head gradients 1e-5, post-NMS rows and ids identical, scores 1e-5, bf16 gradient rows bit-equal to the fp32 rows
rounded once.  Every gradient tensor sits inside a larger buffer with a sentinel band of >= ldh elements on either side.

Mutations, each applied alone to a scratch copy of vd_yolo.hip, and the cases of this file that then fail on an MI355X:
  k_yolo_loss, `m += 16` -> `m += 32`                       test_loss_m_sweep[17], [40], [256]
  k_yolo_loss, the `__shfl_xor(ioumax, 8)` step dropped     test_loss_m_sweep[16], [17], [40], [256]
  k_yolo_loss, scalar staging `e < A` -> `e < A - 1`        test_loss_scalar_form: 7 of its 8 cases (head_off1-bf16 finds the
                                                            unstaged logit still in LDS from the launch before it)
  k_decode_filter, the same loop, `e < A` -> `e < A - 1`    test_decode_rows_form
  k_yolo_loss, `r += gridDim.x * 4` -> leave after one trip test_loss_grid_stride_trip
  k_yolo_loss, the last vd_amax_publish (am2) skipped       test_loss_dhead_amax
  k_nms, `n <= SORT_N` -> `n < SORT_N`                      none, and none can: the radix select is exact for every n, so at
                                                            n = 1024 either path gives the same keys (an equivalent mutant)
  k_nms, `n <= SORT_N` -> `n <= SORT_N + 1` (the nearest    test_nms_count_sweep[n401_1023_1025-*] and all 16 cases of
    wrong one: the direct sort takes 1024 keys)             test_nms_parameter_sweep (n = 1025: the winner sits in the last slot)
Nothing else of the file fails under any of them.
"""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import yolo as Y
from tests import yolo_edge_fixtures as F
from tests.util import dev, maxdiff, nchw_to_dev_nhwc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
SENTINEL = 5.0


# ---------------------------------------------------------------------------------------------
# A. loss
# ---------------------------------------------------------------------------------------------
def _head_tensors(fx, ldh, off=0):
    """the head logits as device tensors [B, g, g, ldh] that start `off` elements into their (aligned) buffers"""
    out = []
    for hh in fx.heads:
        x = np.moveaxis(hh, 1, -1)
        z = np.zeros(x.shape[:-1] + (ldh,))
        z[..., :x.shape[-1]] = x
        buf = torch.zeros(z.size + 8, device="cuda")
        view = buf[off:off + z.size].view(z.shape)
        view.copy_(dev(z))
        out.append(view)
    return out


def _run_loss(fx, ldh, dtype=torch.float32, head_off=0, grad_off=0, amax=None):
    from viddet_amd import ops
    b, c = fx.b, fx.c
    hd = _head_tensors(fx, ldh, head_off)
    h = ops.make_head_desc(hd, fx.grids, ldh, Y.OUT_STRIDES, Y.OUT_ANCHORS, b, c)
    band = ops.round_up(ldh, 8)                       # (16 bytes of either type: the band keeps the rows' alignment)
    bufs, dheads = [], []
    for g in fx.grids:
        n = b * g * g * ldh
        buf = torch.full((band + grad_off + n + band,), SENTINEL, dtype=dtype, device="cuda")
        bufs.append(buf)
        dheads.append(buf[band + grad_off:band + grad_off + n].view(b, g, g, ldh))
    P = fx.box.shape[1]
    losses = torch.full((b, 4), -3.0, device="cuda")
    box_out = torch.full((b, P, 4), -3.0, device="cuda")
    ws = torch.empty(max(16, ops.yolo_loss_ws_bytes(h)), dtype=torch.uint8, device="cuda")
    tg = [dev(t) for t in fx.targets]
    gt = dev(fx.gt)
    ops.yolo_loss_fwd_bwd(h, gt, fx.m, *tg, F.IGNORE_T, fx.smooth, losses, dheads, box_out, ws, dhead_amax=amax)
    torch.cuda.synchronize()
    for buf, d in zip(bufs, dheads):
        lo, hi = band + grad_off, band + grad_off + d.numel()
        assert bool((buf[:lo] == SENTINEL).all()), "the sentinel band in front of the gradient rows was written"
        assert bool((buf[hi:] == SENTINEL).all()), "the sentinel band behind the gradient rows was written"
    return SimpleNamespace(losses=losses, dheads=dheads, box=box_out, h=h, keep=(hd, bufs))


def _check_fp32(fx, res, what=""):
    """boxes, the four losses per image and every gradient row (zero padding channels included) against the oracle"""
    A = 3 * (5 + fx.c)
    eb = maxdiff(res.box.cpu().numpy(), fx.box)
    got = res.losses.cpu().numpy()
    el = float(np.max(np.abs(got - fx.losses) / np.maximum(1.0, np.abs(fx.losses))))
    eg = 0.0
    for d, ref in zip(res.dheads, fx.grads):
        d = d.cpu().numpy()
        eg = max(eg, maxdiff(d[..., :A], ref))
        assert float(np.abs(d[..., A:]).max(initial=0.0)) == 0.0, "padding channels of the gradient are not zero"
    print("%s boxes %.2e px, losses %.2e rel, gradients %.2e" % (what, eb, el, eg))
    assert eb < 1e-3
    assert np.all(np.abs(got - fx.losses) <= 1e-3 * np.maximum(1.0, np.abs(fx.losses))), (got, fx.losses)
    assert eg < 1e-5


def _check_bf16(res16, res32):
    """bf16 gradient rows = the fp32 launch's rows rounded once; losses and boxes are the same arithmetic: bit-equal"""
    assert torch.equal(res16.losses, res32.losses) and torch.equal(res16.box, res32.box)
    for a, d in zip(res32.dheads, res16.dheads):
        assert d.dtype == BF and torch.equal(a.to(BF), d)


def _both_types(fx, ldh, what=""):
    r32 = _run_loss(fx, ldh)
    _check_fp32(fx, r32, what)
    _check_bf16(_run_loss(fx, ldh, BF), r32)
    return r32


@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mixup"])
def test_loss_planted_ignore_branch(mix):
    """A1: >= 30 planted anchors per image above the ignore threshold, >= 30 planted near misses (counted in the CPU file)"""
    fx = F.planted_loss(c=20, mix=mix)
    assert all(len(p) >= 30 for p in fx.planted_hi + fx.planted_lo)
    _both_types(fx, 96)


@pytest.mark.parametrize("m", [0, 1, 16, 17, 40, 256])
def test_loss_m_sweep(m):
    """A2: the 16-lane gt loop - no gt at all, one trip, the second trip, the full LDS table; padding rows between valid gts"""
    _both_types(F.msweep_loss(m), 32, "M=%d" % m)


def test_loss_refuses_m_257():
    from viddet_amd import ops
    from viddet_amd.lib import VidDetHipError
    fx = F.msweep_loss(1)
    hd = _head_tensors(fx, 32)
    h = ops.make_head_desc(hd, fx.grids, 32, Y.OUT_STRIDES, Y.OUT_ANCHORS, fx.b, fx.c)
    dheads = [torch.full_like(t, SENTINEL) for t in hd]
    losses = torch.full((fx.b, 4), -3.0, device="cuda")
    ws = torch.empty(max(16, ops.yolo_loss_ws_bytes(h)), dtype=torch.uint8, device="cuda")
    gt = torch.full((fx.b, 257, 4), -1.0, device="cuda")
    with pytest.raises(VidDetHipError, match=r"M=257 outside \[0,256\]"):
        ops.yolo_loss_fwd_bwd(h, gt, 257, *[dev(t) for t in fx.targets], F.IGNORE_T, False, losses, dheads, None, ws)
    torch.cuda.synchronize()
    assert bool((losses == -3.0).all()) and all(bool((d == SENTINEL).all()) for d in dheads), "refused, yet something ran"


# variant -> (C of the planted fixture, pitch of the aligned launch, pitch, head offset, gradient offset) of the scalar launch
SCALAR_VARIANTS = {
    "ldh75": (20, 96, 75, 0, 0),            # (a) ldh = 3 * (5 + C), no multiple of 4
    "ldh27": (4, 32, 27, 0, 0),
    "head_off1": (20, 96, 96, 1, 0),        # (b) ldh % 4 == 0, the head tensors one element into their buffers
    "grad_off1": (20, 96, 96, 0, 1),        # (c) the same offset on the gradient tensors only
}


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("variant", sorted(SCALAR_VARIANTS))
def test_loss_scalar_form(variant, dtype):
    """A3: k_yolo_loss<false, .> - odd pitches and tensors that are not 16-byte aligned - on the planted fixture"""
    c, ldh_al, ldh, hoff, goff = SCALAR_VARIANTS[variant]
    fx = F.planted_loss(c=c)
    A = 3 * (5 + c)
    al32 = _run_loss(fx, ldh_al)
    _check_fp32(fx, al32, "aligned")
    sc = _run_loss(fx, ldh, dtype, hoff, goff)
    if dtype == BF:
        al = _run_loss(fx, ldh_al, BF)
        _check_bf16(al, al32)
    else:
        al = al32
        _check_fp32(fx, sc, "scalar")
    # the aligned launch of the same logits: both forms do the same arithmetic per element ...
    assert torch.equal(sc.box, al.box)
    for a, d in zip(al.dheads, sc.dheads):
        assert torch.equal(a[..., :A], d[..., :A]) and bool((d[..., A:] == 0).all())
    # ... and the four losses are bit-equal too.  For the objectness, centre and scale terms that is structural: lane 0 of each
    # anchor's 16 adds them in both forms and rows map to waves alike.  The class terms are added by the lane that stores the
    # element - elements 4 l .. 4 l + 3 (+ 256 k) in the 16-byte form, l (+ 64 k) in the scalar one - so a workgroup's fp32
    # partial may differ in its last bit between the forms; on these fixtures the per-image totals (fp64 sum of the partials,
    # rounded to fp32) come out identical, and both forms are deterministic.
    la, ls = al.losses.cpu().numpy(), sc.losses.cpu().numpy()
    print("losses, aligned - scalar:", (la.astype(np.float64) - ls).tolist())
    assert np.array_equal(la, ls)


def test_loss_grid_stride_trip():
    """A4: 48 workgroups wanted, 2048 / 64 + 1 = 33 launched: the row loop's second trip"""
    from viddet_amd import ops
    fx = F.plain_loss(64, 4, 96, 3)
    r32 = _both_types(fx, 32)
    assert ops.yolo_loss_ws_bytes(r32.h) == 64 * 33 * 16 == 64 * F.loss_blocks(64, fx.grids) * 16


def test_loss_dhead_amax():
    """A5: the three max-abs slots of the C ABI"""
    from viddet_amd import ops
    fx = F.planted_loss(c=20)
    slots = [torch.zeros(ops.AMAX_FLOATS, device="cuda") for _ in range(3)]          # zeroed, as the header asks of the caller
    res = _run_loss(fx, 96, amax=slots)
    _check_fp32(fx, res)
    want = [d.abs().max().item() for d in res.dheads]
    first = [s.clone() for s in slots]
    for s, (slot, w) in enumerate(zip(slots, want)):
        assert w > 0 and ops.amax_value(slot) == w, "scale %d: slot %r, max |dhead| %r" % (s, ops.amax_value(slot), w)
        sub = slot.view(ops.L.AMAX_SLOTS, ops.L.AMAX_STRIDE)
        assert bool((sub[:, 1:] == 0).all()), "only the first float of each sub-slot is written"
    res2 = _run_loss(fx, 96, amax=slots)                                           # not cleared: a maximum stays what it is
    for a, d in zip(res.dheads, res2.dheads):
        assert torch.equal(a, d)
    assert all(torch.equal(a, b_) for a, b_ in zip(first, slots))


@pytest.mark.parametrize("b,c,size,m,smooth", [
    (2, 39, 64, 3, True), (2, 40, 64, 3, True), (2, 41, 64, 3, True),          # label smoothing: min(1 / C, 1 / 40) switches at 40
    (2, 3, 64, 3, False), (2, 7, 64, 3, False),                               # ldh == 3 * (5 + C): no padding channel (16-byte form)
    (2, 20, 32, 3, False),                                                    # a grid side of 1
    (1, 1008, 32, 2, False),                                                  # the LDS bound on C
])
def test_loss_shape_edges(b, c, size, m, smooth):
    """A6"""
    from viddet_amd import ops
    fx = F.plain_loss(b, c, size, m, smooth)
    A = 3 * (5 + c)
    ldh = A if c in (3, 7) else ops.round_up(A, 32)
    assert (c in (3, 7)) == (ldh == A) and ldh % 4 == 0
    if size == 32:
        assert fx.grids == [1, 2, 4]
    _both_types(fx, ldh, "C=%d size=%d" % (c, size))


def test_loss_refuses_c_1009():
    from viddet_amd import ops
    from viddet_amd.lib import VidDetHipError
    b, c, grids = 1, 1009, [1, 2, 4]
    ldh = ops.round_up(3 * (5 + c), 32)
    P = 3 * sum(g * g for g in grids)
    hd = [torch.zeros(b, g, g, ldh, device="cuda") for g in grids]
    h = ops.make_head_desc(hd, grids, ldh, Y.OUT_STRIDES, Y.OUT_ANCHORS, b, c)
    dheads = [torch.full_like(t, SENTINEL) for t in hd]
    losses = torch.full((b, 4), -3.0, device="cuda")
    ws = torch.empty(max(16, ops.yolo_loss_ws_bytes(h)), dtype=torch.uint8, device="cuda")
    z = lambda k: torch.zeros(b, P, k, device="cuda")
    with pytest.raises(VidDetHipError, match="too many classes for the LDS row stage"):
        ops.yolo_loss_fwd_bwd(h, torch.full((b, 1, 4), -1.0, device="cuda"), 1, z(1), z(2), z(2), z(2), z(c), F.IGNORE_T, False,
                              losses, dheads, None, ws)
    torch.cuda.synchronize()
    assert bool((losses == -3.0).all()) and all(bool((d == SENTINEL).all()) for d in dheads)


# ---------------------------------------------------------------------------------------------
# B. decode
# ---------------------------------------------------------------------------------------------
def test_decode_rows_form(tmp_path):
    """B1: k_decode_filter (VD_DECODE_ROWS=1, read once per process: a fresh child) - the 16-byte staged path, its scalar
    fallbacks (RW > 1024, an odd pitch) and the direct-to-global appends of a full LDS buffer.  Candidate SETS against the
    oracle's valid set and against the default form's, from this process."""
    from viddet_amd import ops
    from tests.yolo_rows_child import decode_candidates
    assert not os.environ.get("VD_DECODE_ROWS"), "this process must run the default (objectness-first) form"
    out = tmp_path / "rows.npz"
    env = dict(os.environ)
    env["VD_DECODE_ROWS"] = "1"
    r = subprocess.run([sys.executable, "-m", "tests.yolo_rows_child", str(out)], cwd=ROOT, env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "child failed (%d):\n%s" % (r.returncode, r.stdout[-4000:])
    got = np.load(str(out))
    for name in sorted(F.DECODE_CASES):
        fx = F.decode_fixture(name)
        default = decode_candidates(ops, fx)
        for bi in range(fx.b):
            rows, sc = got["%s_rows%d" % (name, bi)], got["%s_score%d" % (name, bi)]
            print("%s image %d: %d candidates (oracle %d, default form %d)" % (name, bi, len(rows), len(fx.valid[bi]), len(default[bi][0])))
            assert np.array_equal(rows.astype(np.int64), fx.valid[bi]), "row-streaming form: candidate set differs from the oracle's"
            assert np.array_equal(default[bi][0].astype(np.int64), fx.valid[bi]), "default form: candidate set differs from the oracle's"
            assert maxdiff(sc, fx.score[bi, fx.valid[bi]]) < 1e-5 and maxdiff(default[bi][1], fx.score[bi, fx.valid[bi]]) < 1e-5


def test_decode_cap_boundary():
    """B2: cap == count reports no overflow, cap == count - 1 reports `count` in the workspace flag (and writes cap slots)"""
    from viddet_amd import ops
    fx = F.decode_fixture("c20")
    hd = [nchw_to_dev_nhwc(hh, fx.ldh) for hh in fx.heads]
    h = ops.make_head_desc(hd, fx.grids, fx.ldh, Y.OUT_STRIDES, Y.OUT_ANCHORS, fx.b, fx.c)
    counts = [len(v) for v in fx.valid]
    image = int(np.argmax(counts))                   # the image with the most candidates: the other one fits either way
    count = counts[image]
    assert count > min(counts)
    for cap, flag in ((count, 0), (count - 1, count)):
        cs = torch.full((fx.b * cap + 64,), -7.0, device="cuda")
        cr = torch.full((fx.b * cap + 64,), -7, dtype=torch.int32, device="cuda")
        cnt = torch.empty(fx.b, dtype=torch.int32, device="cuda")
        ops.yolo_decode_filter(h, F.VALID_T, cs, cr, cap, cnt)
        outs = [torch.empty(fx.b, 100, device="cuda"), torch.empty(fx.b, 100, device="cuda"),
                torch.empty(fx.b, 100, 4, device="cuda"), torch.empty(fx.b, 100, dtype=torch.int32, device="cuda")]
        ws = torch.full((fx.b,), -9, dtype=torch.int32, device="cuda")
        ops.nms_topk(h, cs, cr, cap, cnt, 0.45, 400, 100, *outs, ws)
        torch.cuda.synchronize()
        assert cnt.cpu().tolist() == counts
        assert bool((cs[fx.b * cap:] == -7.0).all()) and bool((cr[fx.b * cap:] == -7).all()), "appends past the cap"
        want = [0] * fx.b
        want[image] = flag
        assert ws.cpu().tolist() == want
        stored = cr[image * cap:(image + 1) * cap].cpu().numpy().astype(np.int64)
        assert len(np.unique(stored)) == cap and np.isin(stored, fx.valid[image]).all()


# ---------------------------------------------------------------------------------------------
# C. NMS on hand-made candidate lists
# ---------------------------------------------------------------------------------------------
def _run_nms(agnostic, ns, thresh, topk, post):
    from viddet_amd import ops
    cs = F.nms_case(agnostic, ns)
    base, b = cs.base, cs.b
    hd = [nchw_to_dev_nhwc(hh[:b], base.ldh) for hh in base.heads]
    h = ops.make_head_desc(hd, base.grids, base.ldh, Y.OUT_STRIDES, Y.OUT_ANCHORS, b, base.c)
    guard = 64
    flat = [torch.full((b * post * k + guard,), 7.0, device="cuda") for k in (1, 1, 4)]
    flat.append(torch.full((b * post + guard,), 7, dtype=torch.int32, device="cuda"))
    ws = torch.full((b,), -9, dtype=torch.int32, device="cuda")
    fn = ops.nms_agnostic if agnostic else ops.nms_topk
    fn(h, dev(cs.cand_score), dev(cs.cand_row, torch.int32), F.NMS_CAP, dev(cs.counts, torch.int32), thresh, topk, post, *flat, ws)
    torch.cuda.synchronize()
    for t, k in zip(flat, (1, 1, 4, 1)):
        assert bool((t[b * post * k:] == 7).all()), "an output was written past post_nms"
    assert ws.cpu().tolist() == [0] * b
    ids, sc, bx, rows = [t[:b * post * k].cpu().numpy() for t, k in zip(flat, (1, 1, 4, 1))]
    return ids.reshape(b, post), sc.reshape(b, post), bx.reshape(b, post, 4), rows.reshape(b, post)


def _check_nms(agnostic, ns, thresh, topk, post):
    ref = F.nms_reference(agnostic, ns, thresh, topk, post)
    ids, sc, bx, rows = _run_nms(agnostic, ns, thresh, topk, post)
    print("n=%s topk=%d post=%d thresh=%.2f: kept %s of %s" % (list(ns), topk, post, thresh, ref.nkept, ref.nsel))
    assert np.array_equal(rows.astype(np.int64), ref.rows), "post-NMS row indices differ"
    assert np.array_equal(ids, ref.ids)
    assert maxdiff(sc, ref.scores) < 1e-5
    assert maxdiff(bx, ref.boxes) < 1e-3
    return ids, sc, bx, rows


@pytest.mark.parametrize("agnostic", [False, True], ids=["per_class", "agnostic"])
@pytest.mark.parametrize("ns", F.NMS_COUNT_BATCHES, ids=lambda ns: "n" + "_".join(map(str, ns)))
def test_nms_count_sweep(agnostic, ns):
    """C1: candidate counts around nms_topk = 400 and the 1024 keys of the direct sort; an empty image beside full ones"""
    _check_nms(agnostic, ns, 0.45, 400, 100)


@pytest.mark.parametrize("agnostic", [False, True], ids=["per_class", "agnostic"])
@pytest.mark.parametrize("topk,post,thresh", F.NMS_PARAM_CASES)
def test_nms_parameter_sweep(agnostic, topk, post, thresh):
    """C2: topk of 1 and TOPK_MAX, post_nms of 1 and beyond topk (the tail is the -1 fill in all four outputs)"""
    ids, sc, bx, rows = _check_nms(agnostic, F.NMS_PARAM_NS, thresh, topk, post)
    if post > topk:
        assert (ids[:, topk:] == -1).all() and (sc[:, topk:] == -1).all() and (bx[:, topk:] == -1).all() and (rows[:, topk:] == -1).all()


@pytest.mark.parametrize("agnostic", [False, True], ids=["per_class", "agnostic"])
def test_nms_refuses_topk_513(agnostic):
    from viddet_amd.lib import VidDetHipError
    with pytest.raises(VidDetHipError, match=r"topk=513 outside \(0,512\]"):
        _run_nms(agnostic, F.NMS_PARAM_NS, 0.45, 513, 100)
