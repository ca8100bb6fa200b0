"""GPU parity of the FRAME taps of every conv kernel against the fp64 conv3d oracle (tests/temporal_conv_oracle.py).

The 3-D (3,3,3) and 2+1-D (3,1,1) neck convs of the frame-window networks (models/definitions/layers.py:73-79) run through the
tap-list kernels of the 2-D convs with a frame offset per tap (dz) and a window length (Kfr); a tap is dropped when
n % Kfr + dz leaves [0, Kfr).  That predicate is written out in k_conv_igemm (fp32 MFMA, split / f16x2 / bf16 products,
one tile per workgroup and stream-K), k_conv_igemm_bf16 (one tile, stream-K, split-K), k_conv_wgrad (fp32, split forms, bf16
storage) and on the host (fwd_taps, dgrad_plans, the weight packers with kd = 3, the unpack into a 5-D weight).  Here each of
them is launched with Kfr > 1 on maps where frames and windows end inside a tile and compared with fp64; outputs are
NaN-filled before every launch, so an element that is not written fails.  Tolerances are those of the 2-D tests of the same
arithmetic (test_conv_gpu.py, test_split_math_gpu.py, test_bf16_gpu.py, test_bf16_train_gpu.py); the measured error / bound
is printed per case and the worst per group at the end of the module.  tests/test_temporal_conv_cpu.py shows on the same
inputs that a wrong predicate (windows leaking, frame taps ignored) would miss these bounds by two orders of magnitude (the
relative-rms bound of the bf16 products: by more than 25 x, which is what a relative rms leaves room for)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import temporal_conv_oracle as T
from tests.temporal_conv_oracle import Case
from tests.util import maxdiff

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
WORST = {}          # group -> (error / bound, label)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for g in sorted(WORST):
        print("temporal conv taps, worst error / bound: %-28s %.3f  (%s)" % (g, WORST[g][0], WORST[g][1]))


def _note(group, label, ratio):
    if not (ratio <= WORST.get(group, (-1.0, ""))[0]):
        WORST[group] = (ratio, label)


def _check(group, label, got, ref, tol):
    """max |got - ref| < tol; a NaN (an element the launch did not write) fails"""
    err = maxdiff(got, ref)
    _note(group, label, err / tol)
    assert err < tol, (group, label, err, tol)
    return err / tol


def _check_rms(group, label, got, ref):
    """the error measure of the bf16-product arithmetic (test_split_math_gpu.py::test_bf16_products_forward_and_gradients):
    rms error relative to the reference's rms, upper bound 1e-2"""
    rel = float(np.sqrt(((got - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean()))
    _note(group, label, rel / T.RMS_BOUND)
    assert rel < T.RMS_BOUND, (group, label, rel)
    return rel / T.RMS_BOUND


def _bf16_tol(ref):
    return T.TOL + float(np.abs(ref).max()) * 2.0 ** -8          # + one bf16 rounding of the output (test_bf16_gpu.py)


# ---------------------------------------------------------------------------------------------------------------------
# device operands, one set per case
# ---------------------------------------------------------------------------------------------------------------------
_DEV = {}
_WS = []


def _f32(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()          # (a copy: the cached operands are read-only)


def _ws():
    if not _WS:
        _WS.append(torch.empty(64 << 20, dtype=torch.uint8, device="cuda"))
    return _WS[0]


def _D(c):
    from viddet_amd import ops
    if c in _DEV:
        return _DEV[c]
    o = T.operands(c)
    Tn = o["kd"] * o["k"] * o["k"]
    D = dict(o)
    D.update(N=o["B"] * o["K"], T=Tn, ci=c.ci, co=c.co)
    for name in ("x", "dy", "res", "prev", "bs_z"):
        D[name] = _f32(T.fold(o[name]))
    for name in ("scale", "shift", "in_scale", "in_shift", "bs_scale", "bs_shift", "bs_mean", "bs_invstd"):
        D[name] = _f32(o[name])
    D["w5"] = _f32(o["w"])                                                    # OIDHW
    D["wp"] = torch.full((c.co, Tn * c.ci), NAN, device="cuda")               # fwd-packed [co][tap][ci]
    ops.pack_weight_fwd(D["w5"], D["wp"], c.co)
    D["ax"], D["aw"], D["ady"] = ops.amax(D["x"]), ops.amax(D["wp"]), ops.amax(D["dy"])
    if c.bf16:
        for name in ("x", "dy", "res", "prev", "bs_z"):
            D[name + "b"] = D[name].to(BF)                                    # exact: the operands are bf16-representable
        D["wb"] = torch.full((c.co, Tn * c.ci), NAN, dtype=BF, device="cuda")
        ops.pack_weight_bf16(D["wp"], D["wb"], Co=c.co, Co_pad=c.co, Ci=c.ci, Ci_pad=c.ci, T=Tn)
    torch.cuda.synchronize()
    _DEV[c] = D
    return D


def _taps(D):
    from viddet_amd import ops
    return ops.fwd_taps(D["k"], D["pad"], D["kd"], D["pad_d"])


def _fwd(c, K=None, *, tile=0, split=False, epi=False, xf=False, ws=None, desc_out=None):
    """k_conv_igemm forward -> oracle layout (B', Co, K, H, W)"""
    from viddet_amd import ops
    D = _D(c)
    K = D["K"] if K is None else K
    out = torch.full((D["N"], D["H"], D["W"], c.co), NAN, device="cuda")
    kw = dict(scale=D["scale"], shift=D["shift"], residual=D["res"], leaky=True) if epi else {}
    if xf:
        kw.update(in_scale=D["in_scale"], in_shift=D["in_shift"], in_slope=0.1)
    if split == "f16x2":
        kw.update(amax_in=D["ax"], amax_w=D["aw"])
    ops.conv_fwd(D["x"], D["wp"], out, k=D["k"], stride=1, pad=D["pad"], Co=c.co, kd=D["kd"], pad_d=D["pad_d"], kfr=K, tile=tile,
                 split=split, streamk_ws=ws, desc_out=desc_out, **kw)
    torch.cuda.synchronize()
    return T.unfold(out, K)


def _fwd_bf16(c, K=None, *, tile=0, out_f32=False, epi=False, part=None, ws=None, splitk=False, desc_out=None):
    """k_conv_igemm_bf16 forward -> oracle layout"""
    from viddet_amd import ops
    D = _D(c)
    K = D["K"] if K is None else K
    out = torch.full((D["N"], D["H"], D["W"], c.co), NAN, dtype=torch.float32 if out_f32 else BF, device="cuda")
    kw = dict(scale=D["scale"], shift=D["shift"], residual=D["resb"], ldr=c.co, leaky=True) if epi else {}
    d = ops.conv_igemm_bf16(D["xb"], D["wb"], out, N=D["N"], Hi=D["H"], Wi=D["W"], Ci=c.ci, Hg=D["H"], Wg=D["W"], in_stride=1,
                            taps=_taps(D), Ho=D["H"], Wo=D["W"], Co=c.co, ldo=c.co, kfr=K, tile=tile, stats_part=part,
                            streamk_ws=ws, splitk=splitk, **kw)
    torch.cuda.synchronize()
    if desc_out is not None:
        desc_out.append(d)
    return T.unfold(out, K)


def _ref(c, K=None, epi=False, xf=False):
    K = T.operands(c)["K"] if K is None else K
    return T.forward_epilogue(c, K, xf, "right") if epi else T.forward(c, K, xf, "right")


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.FP32_TILE0, ids=T.case_id)
def test_forward_fp32_mfma(c):
    """every shape of the table, the 27-tap and the 3-tap kernel, plain and with affine + LeakyReLU + residual; "workload"
    and "ragged" on every explicit tile"""
    for epi in (False, True):
        worst = max(_check("forward fp32", "%s tile %d%s" % (T.case_id(c), tile, " epi" if epi else ""),
                           _fwd(c, tile=tile, epi=epi), _ref(c, epi=epi), T.TOL)
                    for tile in ((0, 1, 2, 3, 4, 5, 6, 7, 8) if c in T.EVERY_TILE else (0,)))
        print("fp32 MFMA %s%s: maxdiff / tol = %.3f" % (T.case_id(c), " + epilogue" if epi else "", worst))


@pytest.mark.parametrize("mode", [True, "f16x2", "bf16"], ids=["bf16x3", "f16x2", "bf16"])
@pytest.mark.parametrize("c", T.EVERY_TILE, ids=T.case_id)
def test_forward_split_arithmetics(c, mode):
    if mode == "bf16":
        worst = max(_check_rms("forward bf16 products", "%s tile %d" % (T.case_id(c), tile), _fwd(c, tile=tile, split=mode), _ref(c))
                    for tile in (1, 4, 5, 9, 11, 16))
        print("bf16 products %s: rms error / bound = %.3f" % (T.case_id(c), worst))
        return
    tiles = range(1, 17) if mode == "f16x2" else (1, 4, 5, 9, 11, 16)
    for epi in (False, True):
        worst = max(_check("forward split", "%s %s tile %d%s" % (T.case_id(c), mode, tile, " epi" if epi else ""),
                           _fwd(c, tile=tile, split=mode, epi=epi), _ref(c, epi=epi), T.TOL) for tile in tiles)
        print("%s %s%s: maxdiff / tol = %.3f" % (mode, T.case_id(c), " + epilogue" if epi else "", worst))


def test_forward_stream_k_against_the_oracle():
    """the persistent stream-K grid of the f16x2 kernel on 27 frame taps: against fp64, not only against the one-tile launch"""
    from viddet_amd import ops, lib as L
    c = T.STREAMK
    ws = ops.streamk_workspace()
    for epi in (False, True):
        ds = []
        got = _fwd(c, tile=4, split="f16x2", epi=epi, ws=ws, desc_out=ds)
        assert L.load().vd_conv_igemm_streamk(C.byref(ds[0])) == 1, "the stream-K form was expected to apply here"
        r = _check("forward stream-K", "%s%s" % (T.case_id(c), " epi" if epi else ""), got, _ref(c, epi=epi), T.TOL)
        print("stream-K f16x2 %s%s: maxdiff / tol = %.3f" % (T.case_id(c), " + epilogue" if epi else "", r))
    assert int(ws.view(torch.int32)[2047]) == 0, "a hand-off poll gave up on an idle GPU"


@pytest.mark.parametrize("mode", [False, True], ids=["fp32-mfma", "bf16x3"])
@pytest.mark.parametrize("c", T.XF_CASES, ids=T.case_id)
def test_forward_in_load_transform_keeps_padded_frames_zero(c, mode):
    """leaky(x * s + b) applied in the gather: an out-of-window frame contributes 0, not leaky(b) (the shifts are O(1))"""
    worst = max(_check("forward in-load transform", "%s %s tile %d" % (T.case_id(c), mode, tile),
                       _fwd(c, tile=tile, split=mode, xf=True), _ref(c, xf=True), T.TOL)
                for tile in ((0, 1, 4) if not mode else (0, 2, 4, 11)))
    print("in-load transform %s %s: maxdiff / tol = %.3f" % (mode, T.case_id(c), worst))


def _conv_desc(c, K, out, flags, tile):
    from viddet_amd import ops, lib as L
    D = _D(c)
    d = L.ConvDesc()
    d.in_, d.wp, d.out = D["x"].data_ptr(), D["wp"].data_ptr(), out.data_ptr()
    d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.in_stride = D["N"], D["H"], D["W"], c.ci, D["H"], D["W"], 1
    ops._set_taps(d, _taps(D))
    d.Kfr, d.Ho, d.Wo, d.Co, d.out_stride, d.ldo, d.ldr = K, D["H"], D["W"], c.co, 1, c.co, c.co
    d.flags, d.tile, d.slope = flags, tile, 0.1
    d.amax_in, d.amax_w = D["ax"].data_ptr(), D["aw"].data_ptr()
    return d


def _check_statistics(group, label, sums, c, atol1, tol2):
    s1, s2 = T.statistics(c, T.operands(c)["K"])
    sv = sums.cpu().numpy()
    r1 = _check(group, label + " sum", sv[:c.co], s1, atol1)
    r2 = _check(group, label + " sum of squares", sv[c.co:], s2, tol2(s2))
    return max(r1, r2)


@pytest.mark.parametrize("c", T.STATS_CASES, ids=T.case_id)
def test_forward_fused_statistics_fp32(c):
    """per-channel sum and sum of squares of the raw output from the conv epilogue (flags 0), finished by vd_bn_sum_partials;
    tolerances of test_conv_gpu.py::test_conv_fused_bn_statistics"""
    from viddet_amd import ops, lib as L
    D = _D(c)
    for flags, name in ((0, "fp32"), (L.MATH_F16X2, "f16x2")):
        for tile in (0, 1, 2, 4, 5):
            out = torch.full((D["N"], D["H"], D["W"], c.co), NAN, device="cuda")
            d = _conv_desc(c, D["K"], out, flags, tile)
            mt = L.load().vd_conv_igemm_mtiles(C.byref(d))
            part = torch.full((mt, 2 * c.co), NAN, device="cuda")
            d.stats_part = part.data_ptr()
            L.check(L.load().vd_conv_igemm(C.byref(d), L.stream_ptr()), "vd_conv_igemm")
            sums = torch.full((2 * c.co,), NAN, dtype=torch.float64, device="cuda")
            ops.bn_sum_partials(part, mt, c.co, sums)
            torch.cuda.synchronize()
            label = "%s %s tile %d" % (T.case_id(c), name, tile)
            _check("forward fp32", label + " (statistics launch)", T.unfold(out, D["K"]), _ref(c), T.TOL)
            r = _check_statistics("fused statistics fp32", label, sums, c, 1e-3, lambda s2: 1e-3 * max(1.0, float(s2.max()) / 100))
            print("fused statistics %s: error / bound = %.3f" % (label, r))


@pytest.mark.parametrize("c,out_f32", T.BF16_STATS, ids=lambda v: T.case_id(v) if isinstance(v, Case) else ("f32out" if v else "bf16out"))
def test_forward_fused_statistics_bf16_kernel(c, out_f32):
    """the bf16 kernel's training form with Kfr > 1; tolerances of test_bf16_train_gpu.py::test_forward_conv_with_fused_statistics
    (sum: atol 2e-3 + rtol 1e-5, sum of squares: rtol 1e-5)"""
    from viddet_amd import ops
    D = _D(c)
    s1, s2 = T.statistics(c, D["K"])
    for tile in (0, 1, 2, 6, 10, 13):
        mt = ops.conv_bf16_mtiles(D["N"], D["H"], D["W"], c.ci, c.co, tile)
        part = torch.full((mt, 2 * c.co), NAN, device="cuda")
        got = _fwd_bf16(c, tile=tile, out_f32=out_f32, part=part)
        sums = torch.full((2 * c.co,), NAN, dtype=torch.float64, device="cuda")
        ops.bn_sum_partials(part, mt, c.co, sums)
        torch.cuda.synchronize()
        label = "%s tile %d" % (T.case_id(c), tile)
        _check("forward bf16 kernel", label + " (statistics launch)", got, _ref(c), T.TOL if out_f32 else _bf16_tol(_ref(c)))
        sv = sums.cpu().numpy()
        b1, b2 = 2e-3 + 1e-5 * np.abs(s1), 1e-8 + 1e-5 * np.abs(s2)               # np.allclose(atol, rtol) spelled out
        r = max(float((np.abs(sv[:c.co] - s1) / b1).max()), float((np.abs(sv[c.co:] - s2) / b2).max()))
        _note("fused statistics bf16 kernel", label, r)
        print("fused statistics bf16 kernel %s: error / bound = %.3f" % (label, r))
        assert np.allclose(sv[:c.co], s1, atol=2e-3) and np.allclose(sv[c.co:], s2, rtol=1e-5), label


@pytest.mark.parametrize("c", T.BF16_EVERY_TILE + T.BF16_CI32, ids=T.case_id)
def test_forward_bf16_kernel(c):
    """k_conv_igemm_bf16 with Kfr > 1 on bf16-representable operands: bf16 and fp32 outputs, plain and with the epilogue;
    every tile on "workload", the two-taps-per-K-step layout of 32 input channels (T = 27 and T = 3 leave the last step
    half filled) on "ragged" """
    tiles = (0, 11, 13, 14) if c.ci == 32 else tuple(range(0, 14))
    for out_f32 in (False, True):
        for epi in (False, True):
            ref = _ref(c, epi=epi)
            tol = T.TOL if out_f32 else _bf16_tol(ref)
            worst = max(_check("forward bf16 kernel", "%s tile %d%s%s" % (T.case_id(c), tile, " f32out" if out_f32 else "", " epi" if epi else ""),
                               _fwd_bf16(c, tile=tile, out_f32=out_f32, epi=epi), ref, tol) for tile in tiles)
            print("bf16 kernel %s %s%s: maxdiff / tol = %.3f" % (T.case_id(c), "fp32 out" if out_f32 else "bf16 out", " + epilogue" if epi else "", worst))


def test_forward_bf16_kernel_stream_k_and_split_k():
    """the two persistent forms of the bf16 kernel on 27 frame taps against fp64: stream-K (a launch with more tiles than
    workgroup slots) and split-K (too few tiles: the K cuts of the 27-tap reduction fall inside taps)"""
    from viddet_amd import ops, lib as L
    ws = ops.streamk_workspace()
    c = T.STREAMK
    ds = []
    got = _fwd_bf16(c, tile=4, ws=ws, desc_out=ds)
    assert L.load().vd_conv_igemm_bf16_streamk(C.byref(ds[0]), 0) == 1, "the stream-K form was expected to apply here"
    r = _check("forward bf16 kernel stream-K", T.case_id(c), got, _ref(c), _bf16_tol(_ref(c)))
    print("bf16 kernel stream-K %s: maxdiff / tol = %.3f" % (T.case_id(c), r))
    assert int(ws.view(torch.int32)[2047]) == 0, "a hand-off poll gave up on an idle GPU"
    c = T.BF16_SPLITK
    for epi in (False, True):
        for tile in (1, 2, 4):
            ds = []
            got = _fwd_bf16(c, tile=tile, epi=epi, ws=ws, splitk=True, desc_out=ds)
            assert L.load().vd_conv_igemm_bf16_streamk(C.byref(ds[0]), 0) == 2, "the split-K form was expected to apply here"
            ref = _ref(c, epi=epi)
            r = _check("forward bf16 kernel split-K", "%s tile %d%s" % (T.case_id(c), tile, " epi" if epi else ""), got, ref, _bf16_tol(ref))
            print("bf16 kernel split-K %s tile %d%s: maxdiff / tol = %.3f" % (T.case_id(c), tile, " + epilogue" if epi else "", r))
    assert int(ws.view(torch.int32)[L.SK_HEADER_BYTES // 8:L.SK_HEADER_BYTES // 4].abs().max()) == 0      # arrival counters back at zero


# ---------------------------------------------------------------------------------------------------------------------
# data gradient
# ---------------------------------------------------------------------------------------------------------------------
def _dgrad_weights(c, src_packed):
    """the data gradient's tap plan and weight image [ci][tap][co], from OIDHW or from the fwd-packed source"""
    from viddet_amd import ops
    D = _D(c)
    plans = ops.dgrad_plans(D["k"], D["pad"], 1, D["H"], D["W"], D["kd"], D["pad_d"])
    assert len(plans) == 1 and len(plans[0]["taps"]) == D["T"]
    pl = plans[0]
    wpk = torch.full((c.ci, D["T"] * c.co), NAN, device="cuda")
    ops.pack_weight_dgrad(D["wp"] if src_packed else D["w5"], wpk, Co=c.co, Co_pad=c.co, Ci=c.ci, kd=D["kd"], kh=D["k"], kw=D["k"],
                          tap_ids=pl["tap_ids"], src_packed=src_packed)
    return pl, wpk


def _dgrad(c, mode, src_packed, K=None, tile=0):
    from viddet_amd import ops
    D = _D(c)
    K = D["K"] if K is None else K
    pl, wpk = _dgrad_weights(c, src_packed)
    geo = dict(N=D["N"], Hi=D["H"], Wi=D["W"], Ci=c.co, Hg=D["H"], Wg=D["W"], in_stride=1, taps=pl["taps"], Ho=D["H"], Wo=D["W"],
               Co=c.ci, ldo=c.ci, kfr=K, tile=tile)
    if mode == "bf16-kernel":           # accumulates onto an existing bf16 gradient, as bf16-storage training does
        wb = torch.full((c.ci, D["T"] * c.co), NAN, dtype=BF, device="cuda")
        ops.pack_weight_bf16(wpk, wb, Co=c.ci, Co_pad=c.ci, Ci=c.co, Ci_pad=c.co, T=D["T"])
        dx = torch.full((D["N"], D["H"], D["W"], c.ci), NAN, dtype=BF, device="cuda")
        ops.conv_igemm_bf16(D["dyb"], wb, dx, residual=D["prevb"], ldr=c.ci, **geo)
    else:
        dx = torch.full((D["N"], D["H"], D["W"], c.ci), NAN, device="cuda")
        kw = dict(amax_in=D["ady"], amax_w=ops.amax(wpk)) if mode == "f16x2" else {}
        ops.conv_igemm(D["dy"], wpk, dx, split=mode, **geo, **kw)
    torch.cuda.synchronize()
    return T.unfold(dx, K)


DGRAD_CASES = [Case("workload", 128, 96, "333"), Case("workload", 128, 96, "311"), Case("ragged", 64, 96, "333"),
               Case("pair", 64, 96, "333"), Case("pair", 64, 96, "311"), Case("tiny", 64, 128, "333")]
DGRAD_BF16_CASES = [Case("workload", 64, 128, "333", True), Case("ragged", 64, 128, "311", True), Case("pair", 128, 64, "333", True),
                    Case("tiny", 64, 128, "333", True)]


@pytest.mark.parametrize("c", DGRAD_CASES, ids=T.case_id)
def test_data_gradient_fp32_and_f16x2(c):
    """dgrad_plans(kd = 3, pad_d = 1) + pack_weight_dgrad(kd = 3) through k_conv_igemm with Kfr > 1: dz = pad_d - kz"""
    dx_ref = T.backward(c, T.operands(c)["K"])[0]
    for mode in (False, "f16x2"):
        for src_packed in (False, True):
            worst = max(_check("data gradient", "%s %s %s tile %d" % (T.case_id(c), mode or "fp32", "packed" if src_packed else "OIDHW", tile),
                               _dgrad(c, mode, src_packed, tile=tile), dx_ref, T.TOL)
                        for tile in ((0, 1, 5) if c.shape in ("workload", "ragged") else (0,)))
            print("data gradient %s %s from %s: maxdiff / tol = %.3f" % (mode or "fp32", T.case_id(c), "fwd-packed" if src_packed else "OIDHW", worst))


@pytest.mark.parametrize("c", DGRAD_BF16_CASES, ids=T.case_id)
def test_data_gradient_bf16_kernel(c):
    K = T.operands(c)["K"]
    ref = T.backward(c, K)[0] + T.rewindow(T.operands(c)["prev"], K)
    for src_packed in (False, True):
        worst = max(_check("data gradient bf16 kernel", "%s %s tile %d" % (T.case_id(c), "packed" if src_packed else "OIDHW", tile),
                           _dgrad(c, "bf16-kernel", src_packed, tile=tile), ref, _bf16_tol(ref)) for tile in (0, 1, 4))
        print("data gradient bf16 kernel %s from %s: maxdiff / tol = %.3f" % (T.case_id(c), "fwd-packed" if src_packed else "OIDHW", worst))


@pytest.mark.parametrize("c", [Case("workload", 128, 96, "333"), Case("ragged", 64, 96, "333")], ids=T.case_id)
def test_data_gradient_accumulating_with_fused_batchnorm_backward_reductions(c):
    """the f16x2 data gradient accumulating into an existing gradient (residual epilogue) and carrying the fused
    BatchNorm-backward reductions (bs_*): sum g and sum g * xhat against the restated sums, atol / rtol of
    test_bf16_train_gpu.py::test_data_gradient_with_fused_batchnorm_backward_reductions"""
    from viddet_amd import ops, lib as L
    D = _D(c)
    K = D["K"]
    g_all, sums_ref = T.backward_bn_sums(c, K)
    pl, wpk = _dgrad_weights(c, True)
    aw = ops.amax(wpk)
    for tile in (0, 1, 5, 12):
        dx = torch.full((D["N"], D["H"], D["W"], c.ci), NAN, device="cuda")
        d = L.ConvDesc()
        d.in_, d.wp, d.out, d.residual = D["dy"].data_ptr(), wpk.data_ptr(), dx.data_ptr(), D["prev"].data_ptr()
        d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.in_stride = D["N"], D["H"], D["W"], c.co, D["H"], D["W"], 1
        ops._set_taps(d, pl["taps"])
        d.Kfr, d.Ho, d.Wo, d.Co, d.out_stride, d.ldo, d.ldr = K, D["H"], D["W"], c.ci, 1, c.ci, c.ci
        d.flags, d.tile, d.slope = L.MATH_F16X2 | L.EPI_RESIDUAL, tile, 0.1
        d.amax_in, d.amax_w = D["ady"].data_ptr(), aw.data_ptr()
        mt = L.load().vd_conv_igemm_mtiles(C.byref(d))
        part = torch.full((mt, 2 * c.ci), NAN, device="cuda")
        d.bs_z, d.bs_scale, d.bs_shift = D["bs_z"].data_ptr(), D["bs_scale"].data_ptr(), D["bs_shift"].data_ptr()
        d.bs_mean, d.bs_invstd, d.bs_part, d.bs_slope = D["bs_mean"].data_ptr(), D["bs_invstd"].data_ptr(), part.data_ptr(), 0.1
        L.check(L.load().vd_conv_igemm(C.byref(d), L.stream_ptr()), "vd_conv_igemm")
        torch.cuda.synchronize()
        label = "%s tile %d" % (T.case_id(c), tile)
        _check("data gradient", label + " accumulate + bs", T.unfold(dx, K), g_all, T.TOL)
        got = part.double().sum(dim=0).cpu().numpy()
        atol = 2e-3 * np.sqrt(D["N"] * D["H"] * D["W"])
        r = float((np.abs(got - sums_ref) / (atol + 1e-4 * np.abs(sums_ref))).max())
        _note("fused BatchNorm-backward sums", label, r)
        print("fused BatchNorm-backward sums %s: error / bound = %.3f" % (label, r))
        assert np.allclose(got, sums_ref, rtol=1e-4, atol=atol), (label, float(np.abs(got - sums_ref).max()))


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
def _wgrad(c, mode, splits, K=None, raw=False, xf=False):
    """mode: False / True / 'f16x2' / 'f16x2h' / 'bf16' on fp32 tensors, 'stored' / 'halo' on bf16-stored operands
    (VD_STORE_BF16, 'halo': with VD_WGRAD_HALO).  Returns the 5-D gradient (numpy), or with raw the packed device tensor."""
    from viddet_amd import ops
    D = _D(c)
    K = D["K"] if K is None else K
    dwp = torch.full((c.co, D["T"] * c.ci), NAN, device="cuda")
    stored = mode in ("stored", "halo")
    x, dy = (D["xb"], D["dyb"]) if stored else (D["x"], D["dy"])
    kw = dict(amax_in=D["ax"], amax_dout=D["ady"]) if mode in ("f16x2", "f16x2h") else {}
    if xf:
        kw.update(in_scale=D["in_scale"], in_shift=D["in_shift"], in_slope=0.1)
    ops.conv_wgrad(x, dy, dwp, _ws(), k=D["k"], stride=1, pad=D["pad"], Co=c.co, kd=D["kd"], pad_d=D["pad_d"], kfr=K, splits=splits,
                   split=("halo" if mode == "halo" else False) if stored else mode, **kw)
    if raw:
        torch.cuda.synchronize()
        return dwp
    dw = torch.full((c.co, c.ci, D["kd"], D["k"], D["k"]), NAN, device="cuda")
    ops.unpack_weight(dwp, dw)
    torch.cuda.synchronize()
    return dw.double().cpu().numpy()


def _wgrad_tol(c):
    o = T.operands(c)
    return T.TOL * np.sqrt(o["B"] * o["K"] * o["H"] * o["W"])


WGRAD_FP32 = [Case("workload", 128, 96, "333"), Case("workload", 128, 96, "311"), Case("ragged", 64, 96, "333"), Case("ragged", 64, 96, "311"),
              Case("tiny", 64, 128, "333"), Case("tiny", 64, 128, "311"), Case("pair", 64, 96, "333"), Case("single", 128, 128, "333"),
              Case("long", 64, 128, "333"), Case("long", 64, 128, "311")]
WGRAD_SPLIT = [Case("workload", 128, 96, "333"), Case("workload", 128, 96, "311"), Case("ragged", 64, 96, "333"), Case("tiny", 64, 128, "333")]
WGRAD_STORED = [Case("workload", 64, 128, "333", True), Case("workload", 128, 96, "311", True), Case("ragged", 32, 96, "333", True),
                Case("tiny", 64, 128, "333", True)]


@pytest.mark.parametrize("c", WGRAD_FP32, ids=T.case_id)
def test_weight_gradient_fp32(c):
    """k_conv_wgrad with kd = 3, Kfr > 1, unpacked into a 5-D weight; split counts 0 (picked), 1 (no slabs) and 7 (pixel
    ranges end inside frames and inside windows)"""
    dw_ref = T.backward(c, T.operands(c)["K"])[1]
    worst = max(_check("weight gradient", "%s fp32 splits %d" % (T.case_id(c), s), _wgrad(c, False, s), dw_ref, _wgrad_tol(c)) for s in (0, 1, 7))
    print("weight gradient fp32 %s: maxdiff / tol = %.3f" % (T.case_id(c), worst))


@pytest.mark.parametrize("mode", [True, "f16x2", "bf16"], ids=["bf16x3", "f16x2", "bf16"])
@pytest.mark.parametrize("c", WGRAD_SPLIT, ids=T.case_id)
def test_weight_gradient_split_arithmetics(c, mode):
    dw_ref = T.backward(c, T.operands(c)["K"])[1]
    if mode == "bf16":
        worst = max(_check_rms("weight gradient bf16 products", "%s splits %d" % (T.case_id(c), s), _wgrad(c, mode, s), dw_ref) for s in (0, 1, 7))
        print("weight gradient bf16 products %s: rms error / bound = %.3f" % (T.case_id(c), worst))
        return
    worst = max(_check("weight gradient", "%s %s splits %d" % (T.case_id(c), mode, s), _wgrad(c, mode, s), dw_ref, _wgrad_tol(c)) for s in (0, 1, 7))
    print("weight gradient %s %s: maxdiff / tol = %.3f" % (mode, T.case_id(c), worst))


@pytest.mark.parametrize("c", WGRAD_STORED, ids=T.case_id)
def test_weight_gradient_from_bf16_stored_operands(c):
    """VD_STORE_BF16: exact products of bf16 operands, fp32 sums - the fp32 bound, no bf16 term (test_bf16_train_gpu.py)"""
    dw_ref = T.backward(c, T.operands(c)["K"])[1]
    worst = max(_check("weight gradient bf16-stored", "%s splits %d" % (T.case_id(c), s), _wgrad(c, "stored", s), dw_ref, _wgrad_tol(c)) for s in (0, 1, 7))
    print("weight gradient bf16-stored %s: maxdiff / tol = %.3f" % (T.case_id(c), worst))


@pytest.mark.parametrize("mode", [False, True], ids=["fp32-mfma", "bf16x3"])
@pytest.mark.parametrize("c", T.XF_CASES, ids=T.case_id)
def test_weight_gradient_in_load_transform_keeps_padded_frames_zero(c, mode):
    """the weight gradient's own in-load transform: an out-of-window frame contributes 0 to the sum, not leaky(b)"""
    dw_ref = T.backward(c, T.operands(c)["K"], True)[1]
    worst = max(_check("weight gradient in-load transform", "%s %s splits %d" % (T.case_id(c), mode, s), _wgrad(c, mode, s, xf=True), dw_ref, _wgrad_tol(c))
                for s in (0, 1, 7))
    print("weight gradient in-load transform %s %s: maxdiff / tol = %.3f" % (mode, T.case_id(c), worst))


def test_weight_gradient_halo_flag_is_ignored_on_frame_taps():
    """VD_WGRAD_HALO on a 27-tap launch: the halo-ring kernel (3x3, no frame taps) does not apply, says so, and the result is
    the generic kernel's bit for bit"""
    from viddet_amd import ops, lib as L
    for c, halo_mode, plain_mode in ((Case("workload", 128, 128, "333"), "f16x2h", "f16x2"), (Case("workload", 64, 128, "333", True), "halo", "stored")):
        D = _D(c)
        d = L.WgradDesc()
        d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.Co, d.ldd = D["N"], D["H"], D["W"], c.ci, D["H"], D["W"], c.co, c.co
        d.in_stride, d.Kfr = 1, D["K"]
        ops._set_taps(d, _taps(D))
        if c.bf16:
            d.flags = L.STORE_BF16 | L.MATH_BF16 | L.WGRAD_HALO
        else:
            d.flags = L.MATH_F16X2 | L.WGRAD_HALO
            d.amax_in = d.amax_dout = 1          # only tested for NULL
        assert L.load().vd_conv_wgrad_uses_halo(C.byref(d)) == 0
        a, b = _wgrad(c, halo_mode, 0, raw=True), _wgrad(c, plain_mode, 0, raw=True)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        dw = torch.full((c.co, c.ci, 3, 3, 3), NAN, device="cuda")
        ops.unpack_weight(a, dw)
        torch.cuda.synchronize()
        _check("weight gradient bf16-stored" if c.bf16 else "weight gradient", "%s with VD_WGRAD_HALO" % T.case_id(c), dw.double().cpu().numpy(),
               T.backward(c, D["K"])[1], _wgrad_tol(c))


# ---------------------------------------------------------------------------------------------------------------------
# the window length is honoured, not assumed
# ---------------------------------------------------------------------------------------------------------------------
def _internal_boundaries(n, k_long, k_short):
    """frames that start or end a window of k_short inside a window of k_long"""
    return [f for f in range(n) if (f % k_short == 0 and f % k_long != 0) or (f % k_short == k_short - 1 and f % k_long != k_long - 1)]


def _frames(a):
    return np.abs(a).max(axis=(1, 3, 4)).reshape(-1)          # (B, C, K, H, W) -> per frame b*K + t


def test_window_length_is_honoured():
    """the SAME buffers of 18 frames as 2 windows of 9 and as 6 windows of 3: each launch matches its own reference, and the
    two differ exactly at the frames where a window of 3 ends inside a window of 9 (by far more than any tolerance).  This
    is the check a kernel with a wrong frame predicate fails - without breaking the predicate in a kernel."""
    c32, cbf = T.WINDOW_CASES
    n = 18
    bnd = _internal_boundaries(n, 9, 3)
    assert bnd == [2, 3, 5, 6, 11, 12, 14, 15]
    rest = [f for f in range(n) if f not in bnd]
    runs = [("forward fp32", c32, lambda K: _fwd(c32, K), lambda K: T.forward(c32, K, False, "right"), T.TOL),
            ("forward split", c32, lambda K: _fwd(c32, K, split="f16x2", tile=5), lambda K: T.forward(c32, K, False, "right"), T.TOL),
            ("forward bf16 kernel", cbf, lambda K: _fwd_bf16(cbf, K), lambda K: T.forward(cbf, K, False, "right"), None),
            ("data gradient", c32, lambda K: _dgrad(c32, False, True, K), lambda K: T.backward(c32, K)[0], T.TOL)]
    for group, c, run, ref, tol in runs:
        got = {}
        for K in T.WINDOW_LENGTHS:
            r = ref(K)
            t = _bf16_tol(r) if tol is None else tol
            got[K] = T.rewindow(run(K), 9)
            print("window length %d, %s %s: maxdiff / tol = %.3f" % (K, group, T.case_id(c), _check(group, "%s Kfr %d" % (T.case_id(c), K), got[K], T.rewindow(r, 9), t)))
        diff = _frames(got[9] - got[3])
        assert diff[bnd].min() > 100 * t and diff[rest].max() < 2 * t, (group, diff)
    # the weight gradient sums over every frame: the two window lengths give different gradients of the frame taps kz != 1
    dw = {K: _wgrad(c32, False, 0, K) for K in T.WINDOW_LENGTHS}
    for K in T.WINDOW_LENGTHS:
        print("window length %d, weight gradient: maxdiff / tol = %.3f" % (K, _check("weight gradient", "%s Kfr %d" % (T.case_id(c32), K), dw[K], T.backward(c32, K)[1], _wgrad_tol(c32))))
    d = np.abs(dw[9] - dw[3]).max(axis=(0, 1, 3, 4))
    assert d[0] > 100 * _wgrad_tol(c32) and d[2] > 100 * _wgrad_tol(c32) and d[1] < 2 * _wgrad_tol(c32), d
