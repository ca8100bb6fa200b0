"""GPU: the BatchNorm kernels between the convolutions (vd_bn.hip) on the paths the one-shape tests never take.

* the fused tails vd_bn_sum_finalize / vd_bn_sum_param_grads (k_bn_sum_fused<0/1>): ragged channel counts, the 16-slice /
  4-in-flight row loop around its boundaries, the hand-over to the unfused pair past 1024 rows, the var < 0 clamp, a count that
  is not the row count, the optional NULL outputs, guard bands round every output;
* the "column never changes" invariant of k_bn_apply_leaky / k_bn_bwd_apply (fixed_col_blocks) at sizes where the grid-stride
  loop takes a second pass and the float4 column count is no power of two, fp32 and bf16;
* both bf16 reduction kernels (8 channels per thread, and the 4-channel fallback by channel count or by alignment).

References are numpy fp64 on the fp32 / bf16 values the device reads.  u = 2^-24 (one fp32 rounding)."""
import numpy as np
import pytest
import torch

from tests.util import dev

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U = 2.0 ** -24
EPS_BF = 2.0 ** -8            # tests/test_bf16_train_gpu.py EPS: one bf16 rounding is 2^-9 relative, its bounds use 2^-8
GUARD = 64                    # sentinel elements on both sides of every output
SENT = -7.0e30                # in the guard bands of a floating-point buffer; -77777 in those of an integer one
BN_EPS = np.float32(1e-5)
MOM = np.float32(0.9)
ROWS = 4                      # rows of the source tensor behind one row of the partial table

NBLKS = [1, 15, 16, 17, 48, 49, 64, 65, 255, 256, 257, 1023, 1024, 1025]
CASES = [(36, n) for n in NBLKS] + [(4, n) for n in (1, 16, 49, 257, 1024)] + [(32, n) for n in (15, 48, 65, 256, 1025)] + \
        [(96, n) for n in (17, 64, 255, 1023, 1025)] + [(1056, n) for n in (1, 49, 257, 1024, 1025)]


def _sentinel(dtype):
    return SENT if dtype.is_floating_point else -77777


def _guarded(n, dtype=torch.float32, init=None):
    """an n-element output carved out of a larger buffer: GUARD sentinels on both sides, the interior 16-byte aligned"""
    buf = torch.full((n + 2 * GUARD,), _sentinel(dtype), dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + n]
    assert view.data_ptr() % 16 == 0
    if init is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype))
    return buf, view


def _intact(buf, n):
    s = _sentinel(buf.dtype)
    return bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + n:] == s).all())


def _negative_variance_constant():
    """an fp32 value v whose fp32-rounded square lies BELOW v * v: a channel that is constant at v has
    sum of squares / count - mean^2 < 0 in exact arithmetic on the table's fp32 entries"""
    for v in (1.1, 1.3, 1.7, 2.3, 0.7, 0.9):
        v = float(np.float32(v))
        if float(np.float32(ROWS * v * v)) < ROWS * v * v:
            return v
    raise AssertionError("no candidate rounds down")


_TABLES = {}


def _table(C, nblk):
    """part[nblk][2C] of a real fp32 tensor x[ROWS * nblk][C] split into nblk row groups: column sums (first half: normal
    values plus a per-channel offset) and column sums of squares (second half), each rounded to fp32 as a conv epilogue
    writes them.  Channel 0 is constant at 3.0 (variance exactly 0), channel 1 at a value whose table gives a variance
    just below 0 (the clamp)."""
    if (C, nblk) not in _TABLES:
        rng = np.random.default_rng(1000 * C + nblk)
        x = (rng.standard_normal((ROWS * nblk, C)) + rng.standard_normal(C) * 2.0).astype(np.float32).astype(np.float64)
        x[:, 0] = 3.0
        x[:, 1] = _negative_variance_constant()
        g = x.reshape(nblk, ROWS, C)
        part = np.concatenate([g.sum(axis=1), (g * g).sum(axis=1)], axis=1).astype(np.float32)
        gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
        beta = (rng.standard_normal(C) * 0.3).astype(np.float32)
        rmean0 = rng.standard_normal(C).astype(np.float32)
        rvar0 = rng.uniform(0.5, 2.0, C).astype(np.float32)
        _TABLES[(C, nblk)] = (part, gamma, beta, rmean0, rvar0)
    return _TABLES[(C, nblk)]


def _ref_finalize(part, count, gamma, beta, rmean0, rvar0):
    """fp64 on the fp32 inputs; eps and momentum are the fp32 arguments widened (1 - momentum is exact in fp32)"""
    p = part.astype(np.float64)
    C = p.shape[1] // 2
    sums = p.sum(axis=0)
    mean = sums[:C] / count
    var_raw = sums[C:] / count - mean * mean
    var = np.maximum(var_raw, 0.0)
    invstd = 1.0 / np.sqrt(var + float(BN_EPS))
    scale = gamma.astype(np.float64) * invstd
    mom = float(MOM)
    return dict(sums=sums, mean=mean, var=var, var_raw=var_raw, invstd=invstd, scale=scale, shift=beta.astype(np.float64) - mean * scale,
                rmean=rmean0.astype(np.float64) * mom + mean * (1.0 - mom), rvar=rvar0.astype(np.float64) * mom + var * (1.0 - mom),
                sums_tol=part.shape[0] * 2.0 ** -52 * np.abs(p).sum(axis=0))


def _ws(nblk, C):
    from viddet_amd import ops
    if nblk <= 1024:
        return None                       # the fused launch takes no workspace
    return torch.empty(ops.bn_sum_partials_ws_bytes(nblk, C), dtype=torch.uint8, device="cuda")


def _run_finalize(C, nblk, count, skip=()):
    """vd_bn_sum_finalize on the table with every output guard-banded; the outputs named in `skip` are passed as NULL"""
    from viddet_amd import ops
    part, gamma, beta, rmean0, rvar0 = _table(C, nblk)
    bufs = {"sums": _guarded(2 * C, torch.float64), "rmean": _guarded(C, init=rmean0), "rvar": _guarded(C, init=rvar0)}
    for k in ("scale", "shift", "smean", "sinv"):
        bufs[k] = _guarded(C)
    a = {k: (None if k in skip else v[1]) for k, v in bufs.items()}
    ops.bn_sum_finalize(dev(part), nblk, C, a["sums"], count, dev(gamma), dev(beta), float(BN_EPS), float(MOM), a["rmean"], a["rvar"],
                        a["scale"], a["shift"], a["smean"], a["sinv"], ws=_ws(nblk, C))
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view.numel()), "guard band of %s" % k
    return {k: v[1].clone() for k, v in bufs.items() if k not in skip}


def _close(name, got, ref, tol):
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    worst = int(np.argmax(err - tol))
    print("%-6s worst |err| %.3e at %d (bound %.3e)" % (name, err[worst], worst, tol[worst]))
    assert np.all(np.isfinite(got)), name
    assert np.all(err <= tol), (name, worst, float(err[worst]), float(tol[worst]))


@pytest.mark.parametrize("C,nblk", CASES)
def test_fused_forward_tail_against_fp64(C, nblk):
    """vd_bn_sum_finalize: sums, scale, shift, save_mean, save_invstd and the running statistics against fp64, with the row
    count and with twice the row count (the SyncBN meaning of `count`) as count.

    Bounds: sums nblk * 2^-52 * sum |part| per column (an fp64 sum in any order); the fp32 outputs 4u of the reference value;
    the running statistics 2u (|old| + |batch|), momentum being the fp32 argument widened.  The error of the fp64 sums that
    the fp32 outputs are computed from is below 1e-12 of them and is not added.

    shift = beta - fl(mean) * scale is held to 4u |shift| + u |beta| + 4u |mean * scale|.  That is 3u |mean * scale| wider than
    "4u of the value plus u (|beta| + |mean * scale|)": the product's operands carry three roundings (mean to fp32, invstd to
    fp32, gamma * invstd) and the product a fourth unless the compiler contracts it into an FMA, which nothing in the build
    pins; where beta cancels most of mean * scale the narrower form does not pay for them.  A correctly rounded fp32
    evaluation of the kernel's formula in numpy, on these tables, reaches 1.14 of the narrower bound uncontracted and 0.87
    with the FMA.

    The constant channel's variance is 0 and the other constant channel's is clamped from below 0: save_invstd is
    1 / sqrt(eps) within 4u, running_var shrinks."""
    part, gamma, beta, rmean0, rvar0 = _table(C, nblk)
    for mult in (1, 2):
        count = float(mult * ROWS * nblk)
        r = _ref_finalize(part, count, gamma, beta, rmean0, rvar0)
        assert np.all(r["var_raw"][2:] > 1e-3), "the table's variance is positive except in the constant channels"
        if mult == 1:
            assert r["var_raw"][0] == 0.0 and r["var_raw"][1] < 0.0, "channel 0: variance 0; channel 1: below 0 (the clamp)"
        o = _run_finalize(C, nblk, count)
        _close("sums", o["sums"], r["sums"], r["sums_tol"])
        _close("mean", o["smean"], r["mean"], 4 * U * np.abs(r["mean"]))
        _close("invstd", o["sinv"], r["invstd"], 4 * U * r["invstd"])
        _close("scale", o["scale"], r["scale"], 4 * U * np.abs(r["scale"]))
        _close("shift", o["shift"], r["shift"], 4 * U * np.abs(r["shift"]) + U * np.abs(beta) + 4 * U * np.abs(r["mean"] * r["scale"]))
        _close("rmean", o["rmean"], r["rmean"], 2 * U * (np.abs(rmean0) + np.abs(r["mean"])))
        _close("rvar", o["rvar"], r["rvar"], 2 * U * (np.abs(rvar0) + np.abs(r["var"])))
        inv0 = 1.0 / np.sqrt(float(BN_EPS))
        for ch in ((0, 1) if mult == 1 else ()):      # with twice the count a constant channel has variance v^2 / 4
            assert abs(float(o["sinv"][ch]) - inv0) <= 4 * U * inv0
            assert 0.0 < float(o["rvar"][ch]) < float(rvar0[ch]), "running_var moves towards 0"


@pytest.mark.parametrize("C,nblk", CASES)
def test_fused_backward_tail_against_fp64(C, nblk):
    """vd_bn_sum_param_grads: sums2 within the fp64 bound, dbeta = its first half and dgamma = its second half rounded to fp32
    (4u of the reference value plus the bound of the sum that is rounded)."""
    from viddet_amd import ops
    part = _table(C, nblk)[0].copy()
    part[:, :C] -= part[:, :C].mean(axis=0, dtype=np.float64).astype(np.float32)      # signed columns that nearly cancel
    p = part.astype(np.float64)
    ref, tol = p.sum(axis=0), nblk * 2.0 ** -52 * np.abs(p).sum(axis=0)
    (bs, sums2), (bg, dgamma), (bb, dbeta) = _guarded(2 * C, torch.float64), _guarded(C), _guarded(C)
    ops.bn_sum_param_grads(dev(part), nblk, C, sums2, dgamma, dbeta, ws=_ws(nblk, C))
    torch.cuda.synchronize()
    assert _intact(bs, 2 * C) and _intact(bg, C) and _intact(bb, C)
    _close("sums2", sums2, ref, tol)
    _close("dbeta", dbeta, ref[:C], 4 * U * np.abs(ref[:C]) + tol[:C])
    _close("dgamma", dgamma, ref[C:], 4 * U * np.abs(ref[C:]) + tol[C:])


@pytest.mark.parametrize("C,nblk", [c for c in CASES if c[1] <= 256])
def test_fused_sums_are_bit_equal_to_the_direct_reduction(C, nblk):
    """Up to 256 rows vd_bn_sum_partials is one launch of the same 16 slices in the same order: the fused tails' fp64 sums
    are its sums bit for bit, forward and backward."""
    from viddet_amd import ops
    part = dev(_table(C, nblk)[0])
    direct = torch.empty(2 * C, dtype=torch.float64, device="cuda")
    ops.bn_sum_partials(part, nblk, C, direct)
    fwd = _run_finalize(C, nblk, float(ROWS * nblk))["sums"]
    bwd = torch.empty(2 * C, dtype=torch.float64, device="cuda")
    ops.bn_sum_param_grads(part, nblk, C, bwd, torch.empty(C, device="cuda"), torch.empty(C, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(fwd.view(torch.int64), direct.view(torch.int64))
    assert torch.equal(bwd.view(torch.int64), direct.view(torch.int64))


@pytest.mark.parametrize("C", [36, 96])
def test_tall_table_without_a_workspace_is_refused_and_writes_nothing(C):
    """1025 rows go through the unfused pair, which needs vd_bn_sum_partials_ws_bytes of workspace: without one both tails
    return VD_EWORKSPACE and leave the running statistics, scale and the parameter gradients as they were."""
    from viddet_amd import lib as L
    nblk = 1025
    lib = L.load()
    part, gamma, beta, rmean0, rvar0 = _table(C, nblk)
    assert lib.vd_bn_sum_partials_ws_bytes(nblk, C) > 0
    pd, gd, bd = dev(part), dev(gamma), dev(beta)
    sums = torch.zeros(2 * C, dtype=torch.float64, device="cuda")
    rmean, rvar, scale, shift, dg, db = dev(rmean0), dev(rvar0), dev(rvar0 * 3), dev(rmean0 * 5), dev(gamma * 7), dev(beta * 9)
    before = [t.clone() for t in (rmean, rvar, scale, shift, dg, db)]
    p = lambda t: t.data_ptr()
    rc = lib.vd_bn_sum_finalize(p(pd), nblk, C, p(sums), float(ROWS * nblk), p(gd), p(bd), float(BN_EPS), float(MOM), p(rmean), p(rvar),
                                p(scale), p(shift), None, None, None, 0, L.stream_ptr())
    rc2 = lib.vd_bn_sum_param_grads(p(pd), nblk, C, p(sums), p(dg), p(db), None, 0, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -3 and rc2 == -3                   # VD_EWORKSPACE
    for t, b in zip((rmean, rvar, scale, shift, dg, db), before):
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))
    # a workspace one byte short is refused as well
    ws = torch.empty(lib.vd_bn_sum_partials_ws_bytes(nblk, C), dtype=torch.uint8, device="cuda")
    assert lib.vd_bn_sum_param_grads(p(pd), nblk, C, p(sums), p(dg), p(db), p(ws), ws.numel() - 1, L.stream_ptr()) == -3


@pytest.mark.parametrize("C,nblk", [(36, 49), (36, 1024), (96, 1025)])
def test_optional_outputs_of_the_forward_tail(C, nblk):
    """save_mean, save_invstd, running_mean, running_var NULL in turn: the call succeeds and every other output is what the
    all-present call wrote, bit for bit."""
    count = float(ROWS * nblk)
    full = _run_finalize(C, nblk, count)
    for name in ("smean", "sinv", "rmean", "rvar"):
        o = _run_finalize(C, nblk, count, skip=(name,))
        assert sorted(o) == sorted(k for k in full if k != name)
        for k, v in o.items():
            assert torch.equal(v.view(torch.int64 if v.dtype == torch.float64 else torch.int32),
                               full[k].view(torch.int64 if v.dtype == torch.float64 else torch.int32)), (name, k)


# ---- the column invariant of the streaming kernels -----------------------------------------------------------------------------
def _channel_vectors(C):
    c = np.arange(C, dtype=np.float64)
    scale = 1.0 + c                                   # a wrong column is off by orders of magnitude
    shift = ((c * 5) % 11 - 5.0) * 0.37 * (1.0 + c / 8)
    mean = ((c * 7) % 13 - 6.0) * 0.21
    invstd = 0.5 + (c % 9) * 0.3
    f = lambda a: a.astype(np.float32).astype(np.float64)
    return f(scale), f(shift), f(mean), f(invstd)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,C", [(44000, 96), (4100, 1056), (1, 4), (1, 1056)])
def test_streaming_kernels_keep_their_channel_column(M, C, bf16):
    """vd_bn_apply_leaky (with / without residual, with / without amax_out) and vd_bn_bwd_apply where the grid-stride loop
    takes a second pass (n4 = M C / 4 > 4096 * 256) and the float4 column count (24, 264) does not divide 256, and at one
    row.  scale = 1 + c, and shift / mean / invstd / the two sums differ from channel to channel as strongly.

    fp32: tests/test_bn_pointwise_gpu.py::test_bn_train_forward_backward's 1e-4 (y) / 2e-4 (dx) absolute at unit scale, times
    max |scale|.  bf16: tests/test_bf16_train_gpu.py::test_batchnorm_passes_on_bf16_tensors' 1e-5 + max |ref| * 2^-8.  The
    published max-abs equals max |y| of the device's own output exactly."""
    from viddet_amd import ops, lib as L
    rng = np.random.default_rng(M + C)
    dt = BF if bf16 else torch.float32
    rnd = lambda a: torch.from_numpy(a.astype(np.float32)).to(dt)
    z, res, dy = [rnd(rng.standard_normal((M, C), dtype=np.float32) * s_) for s_ in (1.5, 1.0, 0.7)]
    zr, rr, dr = [t.double().numpy() for t in (z, res, dy)]
    scale, shift, mean, invstd = _channel_vectors(C)
    if M * (C // 4) > 4096 * 256:
        assert (C // 4) & (C // 4 - 1), "a power-of-two column count divides 256: the invariant would hold trivially"
    zd, rd, dyd = z.cuda(), res.cuda(), dy.cuda()
    sc, sh, mu, iv = dev(scale), dev(shift), dev(mean), dev(invstd)
    u = zr * scale + shift
    act = np.where(u > 0, u, 0.1 * u)
    smax = float(np.abs(scale).max())
    tol = lambda ref, f32: (1e-5 + np.abs(ref).max() * EPS_BF) if bf16 else f32 * smax
    for with_res in (False, True):
        ref = act + rr if with_res else act
        for with_amax in ((False,) if bf16 else (False, True)):
            y = torch.full((M, C), float("nan"), dtype=dt, device="cuda")
            slot = torch.zeros(L.AMAX_FLOATS, device="cuda") if with_amax else None
            ops.bn_apply_leaky(zd, sc, sh, rd if with_res else None, y, M, C, amax_out=slot)
            torch.cuda.synchronize()
            err = float(np.abs(y.double().cpu().numpy() - ref).max())
            print("apply res=%d amax=%d: %.3e (bound %.3e)" % (with_res, with_amax, err, tol(ref, 1e-4)))
            assert err <= tol(ref, 1e-4)
            if with_amax:
                assert ops.amax_value(slot) == float(y.abs().max())
    # backward: sums2 = count * (per-channel means of g and of g * xhat), chosen per channel, not reduced from the data
    c = np.arange(C, dtype=np.float64)
    mg, mgx = ((c * 3) % 7 - 3.0) * 0.11, ((c * 5) % 9 - 4.0) * 0.07
    count = float(M)
    sums2 = np.concatenate([mg, mgx]) * count
    g = np.where(u > 0, dr, 0.1 * dr)
    xh = (zr - mean) * invstd
    refd = scale * (g - sums2[:C] / count - xh * sums2[C:] / count)
    for with_amax in ((False,) if bf16 else (False, True)):
        dx = torch.full((M, C), float("nan"), dtype=dt, device="cuda")
        slot = torch.zeros(L.AMAX_FLOATS, device="cuda") if with_amax else None
        ops.bn_bwd_apply(zd, dyd, sc, sh, mu, iv, torch.from_numpy(sums2).cuda(), count, M, C, dx, amax_out=slot)
        torch.cuda.synchronize()
        err = float(np.abs(dx.double().cpu().numpy() - refd).max())
        print("bwd amax=%d: %.3e (bound %.3e)" % (with_amax, err, tol(refd, 2e-4)))
        assert err <= tol(refd, 2e-4)
        if with_amax:
            assert ops.amax_value(slot) == float(dx.abs().max())


# ---- bf16 reductions: the 8-channel kernel and the 4-channel fallback ------------------------------------------------------------
def _bf16_reductions(M, C, misalign):
    """bn_stats of dy and bn_bwd_reduce of (x, dy) on bf16 tensors; misalign: x and the tensor bn_stats reads start 8 bytes into
    their allocation (a slice of a larger tensor), which sends both calls to the 4-channel kernel.  Returns device and fp64
    results.  The values do not depend on `misalign`."""
    from viddet_amd import ops
    rng = np.random.default_rng(7 * M + C)
    rnd = lambda a: torch.from_numpy(a).to(BF)
    z, dy = rnd(rng.standard_normal((M, C), dtype=np.float32) * 2.0), rnd(rng.standard_normal((M, C), dtype=np.float32) * 0.7)
    zr, dr = z.double().numpy(), dy.double().numpy()
    scale, shift = rng.uniform(0.5, 1.5, C), rng.standard_normal(C)
    mean, invstd = rng.standard_normal(C) * 0.1, rng.uniform(0.5, 2.0, C)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    scale, shift, mean, invstd = f(scale), f(shift), f(mean), f(invstd)

    def place(t):
        off = 4 if misalign else 0                    # 4 bf16 = 8 bytes
        buf = torch.empty(M * C + 8, dtype=BF, device="cuda")
        v = buf[off:off + M * C].view(M, C)
        v.copy_(t)
        assert v.data_ptr() % 16 == (8 if misalign else 0)
        return v
    zd, dyd, dys = place(z), dy.cuda(), place(dy)
    ws = torch.empty(max(ops.bn_stats_ws_bytes(M, C), 16), dtype=torch.uint8, device="cuda")
    sums, sums2 = torch.empty(2 * C, dtype=torch.float64, device="cuda"), torch.empty(2 * C, dtype=torch.float64, device="cuda")
    ops.bn_stats(M, C, dys, sums, ws)
    ops.bn_bwd_reduce(zd, dyd, dev(scale), dev(shift), dev(mean), dev(invstd), M, C, sums2, ws)
    torch.cuda.synchronize()
    u = zr * scale + shift
    g = np.where(u > 0, dr, 0.1 * dr)
    xh = (zr - mean) * invstd
    return (sums.cpu().numpy(), sums2.cpu().numpy(), np.concatenate([dr.sum(0), (dr ** 2).sum(0)]),
            np.concatenate([g.sum(0), (g * xh).sum(0)]))


def _check_bf16_reductions(M, got, got2, ref, ref2):
    """tests/test_bf16_train_gpu.py::test_batchnorm_passes_on_bf16_tensors' rtol 1e-5 / 1e-4, its atol (1e-3 / 2e-3 at 969 rows)
    times sqrt(M / 969): fp32 partial sums of runs of M / 1024 rows, then fp64"""
    k = np.sqrt(M / 969.0)
    print("M=%d: sums %.3e, sums2 %.3e (atol %.3e / %.3e)" % (M, np.abs(got - ref).max(), np.abs(got2 - ref2).max(), 1e-3 * k, 2e-3 * k))
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-3 * k)
    assert np.allclose(got2, ref2, rtol=1e-4, atol=2e-3 * k)


@pytest.mark.parametrize("M", [1, 2, 3, 255, 969, 70001])
@pytest.mark.parametrize("C", [96, 36])
def test_bf16_reductions_in_both_kernels(M, C):
    """C = 96 aligned runs k_bn_partial_bf16x8, C = 36 and C = 96 eight bytes off run k_bn_partial<., bf16>.  70001 rows: the
    1024 blocks loop over 69 rows each and the last row of a thread's run has no partner (two == false).  The aligned and the
    misaligned C = 96 runs read the same values and agree within the same tolerance."""
    got, got2, ref, ref2 = _bf16_reductions(M, C, False)
    _check_bf16_reductions(M, got, got2, ref, ref2)
    if C == 96:
        mis, mis2, _, _ = _bf16_reductions(M, C, True)
        _check_bf16_reductions(M, mis, mis2, ref, ref2)
        k = np.sqrt(M / 969.0)
        assert np.allclose(mis, got, rtol=1e-5, atol=1e-3 * k) and np.allclose(mis2, got2, rtol=1e-4, atol=2e-3 * k)


def test_bf16_reductions_with_132_column_groups():
    """C = 1056: the 8-channel kernel with 132 column groups (one row lane, 124 idle threads)"""
    M = 969
    _check_bf16_reductions(M, *_bf16_reductions(M, 1056, False))
