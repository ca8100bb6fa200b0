"""GPU: the streaming kernels of vd_pointwise.hip past one sweep of their capped grid, at their smallest legal shapes, and on
the paths the host takes but no kernel test did (in-place add, scalar tails, NULL outputs, fp32 pool ties, K = 1 and 2, the
misaligned max-abs scan, the planar preprocess against the oracle).

Every kernel here launches at most 4096 blocks of 256 threads and strides: the first size past one sweep is 4096 * 256 =
1,048,576 units (a unit is what one thread moves per step: a float4, a pixel, a scalar).  Each kernel gets one shape just past
that with a remainder that is no multiple of 256, and its smallest legal shape.  Copies, the max pool, its gradient and the fp32
add are bit-equal to numpy; the other bounds are counted in roundings of u = 2^-24 and stated where they are used."""
import numpy as np
import pytest
import torch

from oracle import ops as R
from tests.test_bn_fused_gpu import EPS_BF, _guarded, _intact        # guard-banded outputs; the bf16 bound's 2^-8
from tests.util import dev

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U = 2.0 ** -24
SWEEP = 4096 * 256
EINVAL = -1


def _lib():
    from viddet_amd import lib as L
    return L, L.load()


def _f32(rng, shape, scale=1.0):
    return (rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(t, ref):
    """device fp32 tensor == numpy fp32 array, bit for bit (-0.0 and NaN payloads included)"""
    return np.array_equal(_bits(t.cpu().numpy()).reshape(-1), _bits(ref).reshape(-1))


# 4 * SWEEP + 3 fills one sweep of float4 units exactly (every thread one step, three tail elements); 4 * (SWEEP + 37) + 3 takes the
# float4 body of k_add / k_sgd into a second pass with a ragged end
NS = [1, 2, 3, 4, 5, 7, 1003, 4 * SWEEP + 3, 4 * (SWEEP + 37) + 3]
assert NS[-1] // 4 > SWEEP and (NS[-1] // 4 - SWEEP) % 256


# ---- add, SGD, fill -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_add_out_of_place_and_in_place(n):
    """vd_add is one correctly rounded fp32 add per element: bit-equal to numpy, float4 body and scalar tail, also with
    out == a (how the backward accumulates a second gradient into the first)."""
    from viddet_amd import ops
    rng = np.random.default_rng(n % 1000)
    a, b = _f32(rng, n), _f32(rng, n, 3.0)
    ref = a + b
    buf, out = _guarded(n)
    ops.add(dev(a), dev(b), out)
    buf2, acc = _guarded(n, init=a)
    ops.add(acc, dev(b), acc)
    torch.cuda.synchronize()
    assert _same_bits(out, ref) and _intact(buf, n)
    assert _same_bits(acc, ref) and _intact(buf2, n)


@pytest.mark.parametrize("n", [8, 8 * SWEEP + 8])
def test_add_bf16_in_place(n):
    """vd_add_bf16 with out == a: the fp32 sum of the widened values rounded to bf16 once - within 2^-8 of each sum."""
    from viddet_amd import ops
    rng = np.random.default_rng(n % 1000)
    a, b = torch.from_numpy(_f32(rng, n)).to(BF), torch.from_numpy(_f32(rng, n, 3.0)).to(BF)
    ref = a.double().numpy() + b.double().numpy()
    buf, acc = _guarded(n, BF)
    acc.copy_(a)
    ops.add(acc, b.cuda(), acc)
    torch.cuda.synchronize()
    assert np.all(np.abs(acc.double().cpu().numpy() - ref) <= np.abs(ref) * EPS_BF) and _intact(buf, n)


@pytest.mark.parametrize("n", NS)
def test_sgd_momentum_two_steps(n):
    """m' = momentum m - lr (rescale g + wd w), w' = w + m': four roundings at most on either line (the compiler may contract
    to FMA, so no bit-equality): 4u (|momentum m| + lr (|rescale g| + |wd w|) + |w|) per element, against fp64 on the fp32
    arguments.  The second step starts from the device's own state."""
    from viddet_amd import ops
    rng = np.random.default_rng(n % 1000 + 1)
    lr, mom, wd, rescale = [float(np.float32(v)) for v in (0.01, 0.9, 5e-4, 1.0 / 64)]
    w, m = dev(_f32(rng, n)), dev(_f32(rng, n, 0.1))
    bw, wg = _guarded(n)
    bm, mg = _guarded(n)
    wg.copy_(w)
    mg.copy_(m)
    for step in range(2):
        g = _f32(rng, n, 2.0)
        w0, m0 = wg.double().cpu().numpy(), mg.double().cpu().numpy()
        g0 = g.astype(np.float64)
        m1, w1 = R.sgd_momentum(w0, g0, m0, lr, mom, wd, rescale)[::-1]
        tol = 4 * U * (np.abs(mom * m0) + lr * (np.abs(rescale * g0) + np.abs(wd * w0)) + np.abs(w0))
        ops.sgd_momentum(wg, dev(g), mg, lr, mom, wd, rescale)
        torch.cuda.synchronize()
        assert np.all(np.abs(mg.double().cpu().numpy() - m1) <= tol), step
        assert np.all(np.abs(wg.double().cpu().numpy() - w1) <= tol), step
        assert _intact(bw, n) and _intact(bm, n)


@pytest.mark.parametrize("n", [1, SWEEP + 5])
def test_fill(n):
    from viddet_amd import ops
    buf, out = _guarded(n)
    ops.fill(out, 2.5)
    torch.cuda.synchronize()
    assert _same_bits(out, np.full(n, 2.5, np.float32)) and _intact(buf, n)


# ---- upsample + concat ----------------------------------------------------------------------------------------------------------
# (N, Ho, Wo, Cu, Cr).  (3, 38, 74, 128, 256) is 809,856 float4 units (one sweep); (4, 38, 74, 4, 388) takes the forward
# (1,102,304 units) and the route gradient (1,091,056) into a second pass with Cu != Cr and Wo / 2 odd; (2, 364, 364, 64, 4) the up
# gradient (1,059,968 units: it reads four children per unit, so its smallest two-pass shape has a 72 MB gradient).
UPCAT = [(1, 2, 2, 4, 4), (2, 6, 10, 32, 64), (3, 38, 74, 128, 256), (4, 38, 74, 4, 388), (2, 6, 14, 24, 8)]
UPCAT_BWD = UPCAT + [(2, 364, 364, 64, 4)]


def _units_upcat(n, ho, wo, cu, cr):
    return n * ho * wo * (cu + cr) // 4, n * (ho // 2) * (wo // 2) * cu // 4, n * ho * wo * cr // 4


def test_upcat_shapes_reach_a_second_pass():
    fwd, up, route = zip(*[_units_upcat(*s) for s in UPCAT_BWD])
    for units in (fwd[:len(UPCAT)], up, route):
        assert any(u > SWEEP and (u - SWEEP) % 256 for u in units)


@pytest.mark.parametrize("shape", UPCAT)
def test_upsample_concat_forward(shape):
    from viddet_amd import ops
    n, ho, wo, cu, cr = shape
    rng = np.random.default_rng(sum(shape))
    up, route = _f32(rng, (n, ho // 2, wo // 2, cu)), _f32(rng, (n, ho, wo, cr))
    ref = np.concatenate([up.repeat(2, axis=1).repeat(2, axis=2), route], axis=-1)
    buf, out = _guarded(ref.size)
    ops.upsample2x_concat(dev(up), dev(route), out.view(n, ho, wo, cu + cr))
    torch.cuda.synchronize()
    assert _same_bits(out, ref) and _intact(buf, ref.size)


@pytest.mark.parametrize("shape", UPCAT_BWD)
def test_upsample_concat_backward_and_its_null_outputs(shape):
    """droute is a copy (bit-equal); dup sums four children in fp32, three adds: 3u * the sum of their magnitudes.  With dup
    or droute NULL (a frozen backbone) the other output is what the two-output call wrote, bit for bit; both NULL: VD_EINVAL."""
    L, lib = _lib()
    n, ho, wo, cu, cr = shape
    hu, wu = ho // 2, wo // 2
    rng = np.random.default_rng(sum(shape) + 1)
    dout = _f32(rng, (n, ho, wo, cu + cr))
    kids = dout[..., :cu].reshape(n, hu, 2, wu, 2, cu)
    ref_up = kids.sum(axis=(2, 4), dtype=np.float64)
    tol_up = 3 * U * np.abs(kids).sum(axis=(2, 4), dtype=np.float64)
    dd = dev(dout)
    s = L.stream_ptr()
    call = lambda a, b: lib.vd_upsample2x_concat_bwd(dd.data_ptr(), None if a is None else a.data_ptr(),
                                                     None if b is None else b.data_ptr(), n, ho, wo, cu, cr, s)
    (bu, dup), (br, drt) = _guarded(ref_up.size), _guarded(n * ho * wo * cr)
    (bu1, dup1), (br1, drt1) = _guarded(ref_up.size), _guarded(n * ho * wo * cr)
    assert call(dup, drt) == 0 and call(dup1, None) == 0 and call(None, drt1) == 0
    assert call(None, None) == EINVAL
    torch.cuda.synchronize()
    assert all(_intact(b_, v.numel()) for b_, v in ((bu, dup), (br, drt), (bu1, dup1), (br1, drt1)))
    assert _same_bits(drt, dout[..., cu:])
    assert np.all(np.abs(dup.double().cpu().numpy().reshape(ref_up.shape) - ref_up) <= tol_up)
    assert torch.equal(dup1.view(torch.int32), dup.view(torch.int32)) and torch.equal(drt1.view(torch.int32), drt.view(torch.int32))


@pytest.mark.parametrize("shape", [(2, 6, 10, 8, 24), (2, 364, 364, 128, 8), (4, 38, 74, 8, 776)])
def test_upsample_concat_backward_on_bf16_tensors(shape):
    """vd_upsample2x_concat_bwd_bf16: the route half a copy; the up half the fp32 sum of four widened values rounded once:
    2^-8 of the sum plus 3u of the children's magnitudes.  (2, 364, 364, 128, 8) takes the up kernel (1,059,968 units of eight
    channels) and (4, 38, 74, 8, 776) the route kernel (1,091,056 units) into a second pass.  NULL outputs as in fp32."""
    L, lib = _lib()
    n, ho, wo, cu, cr = shape
    hu, wu = ho // 2, wo // 2
    rng = np.random.default_rng(sum(shape) + 2)
    dout = torch.from_numpy(_f32(rng, (n, ho, wo, cu + cr))).to(BF)
    d64 = dout.float().numpy()
    kids = d64[..., :cu].reshape(n, hu, 2, wu, 2, cu)
    ref_up = kids.sum(axis=(2, 4), dtype=np.float64)
    tol_up = EPS_BF * np.abs(ref_up) + 3 * U * np.abs(kids).sum(axis=(2, 4), dtype=np.float64)
    dd = dout.cuda()
    s = L.stream_ptr()
    call = lambda a, b: lib.vd_upsample2x_concat_bwd_bf16(dd.data_ptr(), None if a is None else a.data_ptr(),
                                                          None if b is None else b.data_ptr(), n, ho, wo, cu, cr, s)
    (bu, dup), (br, drt) = _guarded(ref_up.size, BF), _guarded(n * ho * wo * cr, BF)
    (bu1, dup1), (br1, drt1) = _guarded(ref_up.size, BF), _guarded(n * ho * wo * cr, BF)
    assert call(dup, drt) == 0 and call(dup1, None) == 0 and call(None, drt1) == 0
    assert call(None, None) == EINVAL
    torch.cuda.synchronize()
    assert all(_intact(b_, v.numel()) for b_, v in ((bu, dup), (br, drt), (bu1, dup1), (br1, drt1)))
    assert torch.equal(drt.view(torch.int16).cpu(), dout[..., cu:].contiguous().view(torch.int16).reshape(-1))
    assert np.all(np.abs(dup.double().cpu().numpy().reshape(ref_up.shape) - ref_up) <= tol_up)
    assert torch.equal(dup1.view(torch.int16), dup.view(torch.int16)) and torch.equal(drt1.view(torch.int16), drt.view(torch.int16))


# ---- temporal pooling -----------------------------------------------------------------------------------------------------------
# B * inner = 1, 800 and 1,048,576 + 77 (= 3 * 349,551: the batch index of the second pass is not 0)
POOL_SIZES = [(1, 1), (2, 400), (3, 349551)]


@pytest.mark.parametrize("B,inner", POOL_SIZES)
@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_max_pool_ties_go_to_the_lowest_frame(K, B, inner):
    """fp32 max join on inputs quantised to seven levels (tests/test_temporal_bf16_kernels_gpu.py's construction, narrowed so
    that two frames already tie on more than 30 % of the positions): values bit-equal, argmax = numpy's first maximum, the
    backward with the device's argmax bit-equal to the one-hot scatter and written whole; argmax = NULL gives the same y;
    the backward without an argmax is refused."""
    L, lib = _lib()
    from viddet_amd import ops
    rng = np.random.default_rng(K * 7 + inner % 1000)
    x = np.clip(np.round(rng.standard_normal((B, K, inner)) * 0.7), -3, 3).astype(np.float32)
    if B * inner == 1:
        x[:] = 2.0                                        # the one position ties across all K frames
    first = x.argmax(axis=1)                              # numpy: the first of equal maxima (-0.0 == 0.0: np.round makes both)
    ymax = np.take_along_axis(x, first[:, None, :], axis=1)[:, 0]       # that frame's value, so a zero keeps its sign
    if K > 1:
        share = float(np.mean((x == ymax[:, None]).sum(axis=1) > 1))
        assert share > 0.3, "the data must tie (%.3f)" % share
    xd = dev(x)
    by, y = _guarded(B * inner)
    ba, am = _guarded(B * inner, torch.int32)
    by2, y2 = _guarded(B * inner)
    ops.temporal_pool(xd, y, am, B, K, inner, 0)
    ops.temporal_pool(xd, y2, None, B, K, inner, 0)
    torch.cuda.synchronize()
    assert _intact(by, B * inner) and _intact(ba, B * inner) and _intact(by2, B * inner)
    assert _same_bits(y, ymax) and _same_bits(y2, ymax)
    assert np.array_equal(am.cpu().numpy().reshape(B, inner), first.astype(np.int32))
    dy = _f32(rng, (B, inner))
    bx, dx = _guarded(B * K * inner)
    dx.fill_(float("nan"))
    ops.temporal_pool_bwd(dev(dy), am, dx, B, K, inner, 0)
    torch.cuda.synchronize()
    ref = np.where(np.arange(K)[None, :, None] == first[:, None, :], dy[:, None, :], np.float32(0.0))
    assert _same_bits(dx, ref) and _intact(bx, B * K * inner)
    assert lib.vd_temporal_pool_bwd(xd.data_ptr(), None, dx.data_ptr(), B, K, inner, 0, L.stream_ptr()) == EINVAL


@pytest.mark.parametrize("B,inner", POOL_SIZES)
@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_mean_pool(K, B, inner):
    """K - 1 fp32 adds and one division: K u * mean |x| over the frames.  The backward is dy / K, one correctly rounded fp32
    division, with or without an argmax pointer."""
    from viddet_amd import ops
    rng = np.random.default_rng(K * 11 + inner % 1000)
    x = _f32(rng, (B, K, inner), 2.0)
    x64 = x.astype(np.float64)
    by, y = _guarded(B * inner)
    ops.temporal_pool(dev(x), y, None, B, K, inner, 1)
    dy = _f32(rng, (B, inner))
    bx, dx = _guarded(B * K * inner)
    dx.fill_(float("nan"))
    ops.temporal_pool_bwd(dev(dy), None, dx, B, K, inner, 1)
    torch.cuda.synchronize()
    assert _intact(by, B * inner) and _intact(bx, B * K * inner)
    assert np.all(np.abs(y.double().cpu().numpy().reshape(B, inner) - x64.mean(axis=1)) <= K * U * np.abs(x64).mean(axis=1))
    assert _same_bits(dx, np.repeat((dy / np.float32(K))[:, None, :], K, axis=1))


# ---- frame slice, 'cat' join ------------------------------------------------------------------------------------------------------
def _slice_inners(K, kc, B):
    """4 and 1028 floats, and a size past one sweep: of the forward (B kc inner / 4 units) where kc >= 3, else of the backward
    alone (B K inner / 4 units), which keeps the K-frame tensor near 17 MB"""
    return [4, 1028, 4 * (SWEEP // (B * (kc if kc >= 3 else K)) + 37)]


@pytest.mark.parametrize("K,k0,kc", [(3, 1, 1), (5, 1, 3), (4, 0, 4), (4, 3, 1), (2, 0, 1)])
def test_frame_slice_forward_and_backward(K, k0, kc):
    """forward bit-equal to the numpy slice; the backward bit-equal to the zero-padded scatter with every element of the K-frame
    tensor written (NaN before the call).  The backward takes a second pass in all five cases; the forward in (5, 1, 3) and
    (4, 0, 4) only (_slice_inners): with kc = 1 its index arithmetic is the same loop with t % 1 == 0."""
    from viddet_amd import ops
    B = 2
    for inner in _slice_inners(K, kc, B):
        rng = np.random.default_rng(K * 100 + k0 * 10 + kc)
        x = _f32(rng, (B, K, inner))
        by, y = _guarded(B * kc * inner)
        ops.frame_slice(dev(x), y, B, K, k0, kc, inner)
        dy = _f32(rng, (B, kc, inner))
        bx, dx = _guarded(B * K * inner)
        dx.fill_(float("nan"))
        ops.frame_slice(dev(dy), dx, B, K, k0, kc, inner, backward=True)
        torch.cuda.synchronize()
        ref = np.zeros((B, K, inner), np.float32)
        ref[:, k0:k0 + kc] = dy
        assert _same_bits(y, x[:, k0:k0 + kc]) and _intact(by, B * kc * inner), inner
        assert _same_bits(dx, ref) and _intact(bx, B * K * inner), inner
    assert B * K * _slice_inners(K, kc, B)[-1] // 4 > SWEEP


def test_frame_slice_rejects_bad_arguments():
    L, lib = _lib()
    t = torch.zeros(64, device="cuda")
    s = L.stream_ptr()
    assert lib.vd_frame_slice(t.data_ptr(), t.data_ptr(), 1, 3, 2, 2, 4, 0, s) == EINVAL        # k0 + kc > K
    assert lib.vd_frame_slice(t.data_ptr(), t.data_ptr(), 1, 3, 1, 1, 6, 0, s) == EINVAL        # inner % 4
    assert lib.vd_frame_slice(t.data_ptr(), t.data_ptr(), 1, 3, 1, 1, 6, 1, s) == EINVAL


@pytest.mark.parametrize("B,K,hw,C", [(1, 1, 1, 4), (2, 3, 5, 8), (2, 5, 169, 256), (2, 3, 1355, 516)])
def test_temporal_cat_forward_backward_round_trip(B, K, hw, C):
    """[B*K, hw, C] -> [B, hw, K*C]: bit-equal to the numpy transpose, the backward to its inverse, the round trip the
    identity.  (2, 3, 1355, 516) is 1,048,770 float4 units with hw odd."""
    from viddet_amd import ops
    rng = np.random.default_rng(B + K + hw + C)
    n = B * K * hw * C
    x = _f32(rng, (B, K, hw, C))
    ref = x.transpose(0, 2, 1, 3).reshape(B, hw, K * C)
    g = _f32(rng, (B, hw, K * C))
    gref = g.reshape(B, hw, K, C).transpose(0, 2, 1, 3)
    (by, y), (bg, dx), (bb, back) = _guarded(n), _guarded(n), _guarded(n)
    for t in (y, dx, back):
        t.fill_(float("nan"))
    ops.temporal_cat(dev(x), y, B, K, hw, C)
    ops.temporal_cat(dev(g), dx, B, K, hw, C, backward=True)
    ops.temporal_cat(y, back, B, K, hw, C, backward=True)
    torch.cuda.synchronize()
    assert _intact(by, n) and _intact(bg, n) and _intact(bb, n)
    assert _same_bits(y, ref) and _same_bits(dx, gref) and _same_bits(back, x)


# ---- layout and input normalisation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 9, 11), (5, 460, 460)])
def test_layout_and_preprocess_against_the_oracle(N, H, W):
    """vd_nchw_to_nhwc is a copy; vd_preprocess_u8_nhwc and vd_preprocess_u8_nchw against oracle.ops.preprocess_u8 within
    tests/test_bn_pointwise_gpu.py::test_layout_preprocess_add_fill's 1e-6, and bit-equal to each other after a transpose (they
    share vd_normalize_level).  (5, 460, 460) is 1,058,000 pixels; there every channel holds all 256 levels."""
    L, lib = _lib()
    from viddet_amd import ops
    rng = np.random.default_rng(N + H + W)
    x = _f32(rng, (N, 3, H, W))
    bo, out = _guarded(x.size)
    ops.nchw_to_nhwc(dev(x), out.view(N, H, W, 3))
    img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    if N * H * W >= 256:
        img.reshape(-1, 3)[:256] = np.arange(256, dtype=np.uint8)[:, None]
        assert all(len(np.unique(img[..., c])) == 256 for c in range(3))
    imgd = torch.from_numpy(img).cuda()
    (bh, nhwc), (bc, nchw) = _guarded(img.size), _guarded(img.size)
    ops.preprocess_u8(imgd, nhwc)
    L.check(lib.vd_preprocess_u8_nchw(imgd.data_ptr(), nchw.data_ptr(), N, H, W, L.stream_ptr()), "vd_preprocess_u8_nchw")
    torch.cuda.synchronize()
    assert _intact(bo, x.size) and _intact(bh, img.size) and _intact(bc, img.size)
    assert _same_bits(out, np.moveaxis(x, 1, -1))
    ref = np.stack([R.preprocess_u8(img[i]) for i in range(N)])              # (N, 3, H, W)
    got = nchw.cpu().numpy().reshape(N, 3, H, W)
    assert np.abs(got.astype(np.float64) - ref).max() < 1e-6
    assert _same_bits(nhwc, np.moveaxis(got, 1, -1))


# ---- max-abs slots ----------------------------------------------------------------------------------------------------------------
# vd_amax launches at most 1024 blocks: 4 * (1024 * 256 + 37) + 3 floats take the float4 body on an aligned base into a second step
AMAX_NS = [1, 3, 4, 5, 1000003, 4 * (1024 * 256 + 37) + 3]


@pytest.mark.parametrize("n", AMAX_NS)
def test_amax_body_tail_and_misaligned_base(n):
    """vd_amax with the base 16-byte aligned and one float off (the scan is then all scalar), the largest magnitude - a negative
    value - at index 0, at n - 1 (the scalar tail) and at the last float4 lane; slots that held 1e30 before the call."""
    from viddet_amd import ops, lib as L
    rng = np.random.default_rng(n)
    base = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    for off in (0, 1):
        for pos in sorted({0, n - 1, max(0, 4 * (n // 4) - 1)}):
            a = base.copy()
            a[pos] = -7.5
            buf = torch.zeros(n + 8, device="cuda")
            x = buf[off:off + n]
            x.copy_(torch.from_numpy(a))
            assert x.data_ptr() % 16 == 4 * off
            slots = torch.full((L.AMAX_FLOATS,), 1e30, device="cuda")
            ops.amax(x, slots)
            torch.cuda.synchronize()
            assert ops.amax_value(slots) == 7.5, (off, pos)


def test_amax_segments_and_merge():
    """three segments of one buffer: 100001 floats at offset 0 (the maximum in the scalar tail), 7 at an odd offset (all scalar),
    1 at a multiple of 4; then the middle one all zeros.  vd_amax_merge without b copies the 32 sub-slots and nothing else, with
    b it is their element-wise maximum."""
    from viddet_amd import ops, lib as L
    lib = L.load()
    rng = np.random.default_rng(9)
    segs = [(0, 100001), (100001, 7), (100008, 1)]
    a = rng.uniform(-1.0, 1.0, 100009).astype(np.float32)
    a[100000], a[100001 + 6], a[100008] = -5.0, -3.0, -0.25
    want = [float(np.abs(a[o:o + c]).max()) for o, c in segs]
    assert want == [5.0, 3.0, 0.25]
    arena = dev(a)
    seg = torch.tensor(segs, dtype=torch.int64, device="cuda")
    am = torch.full((3 * L.AMAX_FLOATS,), 1e30, device="cuda")
    L.check(lib.vd_amax_segments(arena.data_ptr(), seg.data_ptr(), 3, am.data_ptr(), L.stream_ptr()), "vd_amax_segments")
    torch.cuda.synchronize()
    one = lambda i: am[i * L.AMAX_FLOATS:(i + 1) * L.AMAX_FLOATS]
    assert [ops.amax_value(one(i)) for i in range(3)] == want
    arena[100001:100008] = 0.0
    am2 = torch.full((3 * L.AMAX_FLOATS,), 1e30, device="cuda")
    L.check(lib.vd_amax_segments(arena.data_ptr(), seg.data_ptr(), 3, am2.data_ptr(), L.stream_ptr()), "vd_amax_segments")
    torch.cuda.synchronize()
    assert ops.amax_value(am2[L.AMAX_FLOATS:2 * L.AMAX_FLOATS]) == 0.0
    # merge
    sa, sb = rng.uniform(0, 4, L.AMAX_FLOATS).astype(np.float32), rng.uniform(0, 4, L.AMAX_FLOATS).astype(np.float32)
    o1, o2 = torch.full((L.AMAX_FLOATS,), 1e30, device="cuda"), torch.full((L.AMAX_FLOATS,), 1e30, device="cuda")
    sad, sbd = dev(sa), dev(sb)
    L.check(lib.vd_amax_merge(sad.data_ptr(), None, o1.data_ptr(), L.stream_ptr()), "vd_amax_merge")
    L.check(lib.vd_amax_merge(sad.data_ptr(), sbd.data_ptr(), o2.data_ptr(), L.stream_ptr()), "vd_amax_merge")
    torch.cuda.synchronize()
    r1, r2 = np.full(L.AMAX_FLOATS, 1e30, np.float32), np.full(L.AMAX_FLOATS, 1e30, np.float32)
    r1[::L.AMAX_STRIDE] = sa[::L.AMAX_STRIDE]
    r2[::L.AMAX_STRIDE] = np.maximum(sa, sb)[::L.AMAX_STRIDE]
    assert _same_bits(o1, r1) and _same_bits(o2, r2)
