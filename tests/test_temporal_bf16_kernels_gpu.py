"""The temporal joins' training kernels on bf16 tensors (bf16-storage training of the k > 1 networks): vd_temporal_pool_train_bf16,
vd_temporal_pool_bwd_bf16, vd_temporal_cat / vd_frame_slice through the halved-count call, and vd_corr_bwd_bf16, against fp64
restatements.  Inputs are drawn in fp64 and rounded to bf16 first, so the oracle sees exactly the device's operands."""
import numpy as np
import pytest
import torch

from tests import corr_oracle as CO
from tests.test_corr_gpu import KERNEL_CASES
from tests.util import maxdiff

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = 2.0 ** -8              # one bf16 rounding: relative error <= 2^-9; the bounds use 2^-8 (tests/test_corr_gpu.py's form)


def _bf(a):
    """fp64 array -> (bf16 device tensor, the same values in fp64)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(BF)
    return t.cuda(), t.double().numpy()


def _lib():
    from viddet_amd import lib as L
    return L, L.load()


# inner = 8: the smallest legal one; 8 * 256 * 4096 / B is the grid stride of the capped launch: (B * inner / 8) above and not a
# multiple of 4096 * 256 exercises the strided loop's tail
INNERS = [8, 24, 13 * 13 * 256, 8 * (4096 * 256 // 2 + 37)]


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("inner", INNERS)
@pytest.mark.parametrize("type_", [0, 1])
def test_pool_forward_and_backward_on_bf16_tensors(K, inner, type_):
    L, lib = _lib()
    B = 2
    rng = np.random.default_rng(K * 7 + type_ + inner % 1000)
    x64 = rng.standard_normal((B, K, inner))
    if type_ == 0:
        x64 = np.round(x64)                           # a few bf16 levels (-3 .. 3): most positions tie
    x, xr = _bf(x64)
    y = torch.full((B, inner), float('nan'), dtype=BF, device='cuda')
    am = torch.full((B, inner), 255, dtype=torch.uint8, device='cuda')
    L.check(lib.vd_temporal_pool_train_bf16(x.data_ptr(), y.data_ptr(), am.data_ptr() if type_ == 0 else None, B, K, inner, type_,
                                            L.stream_ptr()), "vd_temporal_pool_train_bf16")
    y2 = torch.full((B, inner), float('nan'), dtype=BF, device='cuda')
    L.check(lib.vd_temporal_pool_bf16(x.data_ptr(), y2.data_ptr(), B, K, inner, type_, L.stream_ptr()), "vd_temporal_pool_bf16")
    torch.cuda.synchronize()
    got = y.double().cpu().numpy()
    assert np.array_equal(got, y2.double().cpu().numpy()), "the inference kernel's values"
    if type_ == 0:
        assert np.array_equal(got, xr.max(axis=1))
        first = xr.argmax(axis=1)                     # numpy: the first of equal maxima
        assert float(np.mean((xr == xr.max(axis=1, keepdims=True)).sum(axis=1) > 1)) > 0.3, "the data must tie"
        assert np.array_equal(am.cpu().numpy(), first.astype(np.uint8))
    else:
        ref = xr.mean(axis=1)
        assert np.all(np.abs(got - ref) <= np.abs(ref) * EPS + 1e-6)
    # backward: every element of dx written
    g, gr = _bf(rng.standard_normal((B, inner)))
    dx = torch.full((B, K, inner), float('nan'), dtype=BF, device='cuda')
    L.check(lib.vd_temporal_pool_bwd_bf16(g.data_ptr(), am.data_ptr() if type_ == 0 else None, dx.data_ptr(), B, K, inner, type_,
                                          L.stream_ptr()), "vd_temporal_pool_bwd_bf16")
    torch.cuda.synchronize()
    gd = dx.double().cpu().numpy()
    assert np.all(np.isfinite(gd))
    if type_ == 0:
        ref = np.where(np.arange(K)[None, :, None] == first[:, None, :], gr[:, None, :], 0.0)
        assert np.array_equal(gd, ref)
    else:
        ref = np.repeat(gr[:, None, :] / K, K, axis=1)
        assert np.all(np.abs(gd - ref) <= np.abs(ref) * EPS + 1e-6)


def test_pool_kernels_reject_bad_arguments():
    L, lib = _lib()
    t = torch.zeros(64, dtype=BF, device='cuda')
    a = torch.zeros(64, dtype=torch.uint8, device='cuda')
    s = L.stream_ptr()
    assert lib.vd_temporal_pool_train_bf16(t.data_ptr(), t.data_ptr(), a.data_ptr(), 1, 3, 12, 0, s) == -1      # inner % 8
    assert lib.vd_temporal_pool_train_bf16(t.data_ptr(), t.data_ptr(), None, 1, 3, 8, 0, s) == -1                # max needs argmax
    assert lib.vd_temporal_pool_train_bf16(t.data_ptr(), t.data_ptr(), a.data_ptr(), 1, 128, 8, 0, s) == -1      # K < 128
    assert lib.vd_temporal_pool_bwd_bf16(t.data_ptr(), None, t.data_ptr(), 1, 3, 8, 0, s) == -1
    assert lib.vd_corr_bwd_bf16(t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 3, 2, 2, 48, 1, 192, s) == -1       # C % 32
    assert lib.vd_corr_bwd_bf16(t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 3, 2, 2, 32, 6, 512, s) == -1       # d <= 5


@pytest.mark.parametrize("K,C,hw", [(3, 8, 5), (3, 256, 13 * 13), (5, 24, 7)])
def test_cat_and_slice_on_bf16_tensors_through_the_halved_count_call(K, C, hw):
    """vd_temporal_cat / vd_frame_slice are copies of 16-byte units: bf16 tensors go through them with the channel / inner
    count halved (C % 8 == 0), forward and backward - bit-equal permutations."""
    L, lib = _lib()
    B = 2
    rng = np.random.default_rng(C + K)
    x, _ = _bf(rng.standard_normal((B, K, hw, C)))
    y = torch.full((B, hw, K * C), float('nan'), dtype=BF, device='cuda')
    L.check(lib.vd_temporal_cat(x.data_ptr(), y.data_ptr(), B, K, hw, C // 2, 0, L.stream_ptr()), "vd_temporal_cat")
    back = torch.full((B, K, hw, C), float('nan'), dtype=BF, device='cuda')
    L.check(lib.vd_temporal_cat(y.data_ptr(), back.data_ptr(), B, K, hw, C // 2, 1, L.stream_ptr()), "vd_temporal_cat/bwd")
    torch.cuda.synchronize()
    assert torch.equal(y, x.permute(0, 2, 1, 3).reshape(B, hw, K * C))
    assert torch.equal(back, x)
    # frames [k0, k0 + kc) of every window, and the gradient of that (zeros outside the range)
    k0, kc, inner = 1, K - 2, hw * C
    sl = torch.full((B, kc, hw, C), float('nan'), dtype=BF, device='cuda')
    L.check(lib.vd_frame_slice(x.data_ptr(), sl.data_ptr(), B, K, k0, kc, inner // 2, 0, L.stream_ptr()), "vd_frame_slice")
    full = torch.full((B, K, hw, C), float('nan'), dtype=BF, device='cuda')
    L.check(lib.vd_frame_slice(sl.data_ptr(), full.data_ptr(), B, K, k0, kc, inner // 2, 1, L.stream_ptr()), "vd_frame_slice/bwd")
    torch.cuda.synchronize()
    assert torch.equal(sl, x[:, k0:k0 + kc])
    ref = torch.zeros_like(x)
    ref[:, k0:k0 + kc] = x[:, k0:k0 + kc]
    assert torch.equal(full, ref)


def _ldy(K, C, d):
    return -(-CO.corr_channels(K, C, d) // 64) * 64


def _corr_bwd(g, x, B, K, H, W, C, d):
    L, lib = _lib()
    dx = torch.full((B * K, H, W, C), float('nan'), dtype=BF, device='cuda')
    L.check(lib.vd_corr_bwd_bf16(g.data_ptr(), x.data_ptr(), dx.data_ptr(), B, K, H, W, C, d, g.shape[-1], L.stream_ptr()),
            "vd_corr_bwd_bf16")
    return dx


# tests/test_corr_gpu.py's cases (d in {0, 1, 4}, a 2 x 2 map, maps that are not multiples of the 8 x 8 tile, C 32 .. 1024) and
# one each for d = 2, 3 and 5
BWD_CASES = KERNEL_CASES + [(3, 64, 13, 13, 2), (3, 128, 10, 17, 3), (3, 64, 19, 12, 5)]


@pytest.mark.parametrize("K,C,H,W,d", BWD_CASES)
def test_corr_backward_on_bf16_tensors_against_the_restatement(K, C, H, W, d):
    """vd_corr_bwd_bf16 against the fp64 gradient of tests/corr_oracle.py::corr on bf16-representable x and dy.  Per frame t,
    with s = max|dr[:, t]|: maxdiff <= (2^-8 + 1e-5) * s - the fp32 kernel's 1e-5 * s (tests/test_corr_gpu.py) plus one bf16
    rounding of the stored gradient.  Every element of dx is written (NaN-filled before the launch), two runs are
    bit-identical, and - as in vd_corr_bwd, which never reads them either - garbage in dy's pad columns [Cc, ldy) does
    not change dx."""
    B = 2
    rng = np.random.default_rng(K * 1000 + C + d)
    x, x5n = _bf(rng.standard_normal((B, K, H, W, C)))          # device layout (frame b*K + k, NHWC)
    x5 = np.moveaxis(x5n, -1, 2)                                # (B, K, C, H, W)
    yr, bw = CO.corr(x5, d)
    Cc, ldy = yr.shape[1], _ldy(K, C, d)
    gfull, gn = _bf(np.moveaxis(rng.standard_normal(yr.shape), 1, -1))      # (B, H, W, Cc)
    dr = bw(np.moveaxis(gn, -1, 1))                             # (B, K, C, H, W)
    g = torch.zeros((B, H, W, ldy), dtype=BF, device='cuda')
    g[..., :Cc] = gfull
    xd = x.reshape(B * K, H, W, C)
    dx = _corr_bwd(g, xd, B, K, H, W, C, d)
    dx2 = _corr_bwd(g, xd, B, K, H, W, C, d)
    g[..., Cc:] = float('nan')                                  # the pad columns are never read
    if ldy > Cc:
        g[..., Cc:][::2] = 3.0e38
    dx3 = _corr_bwd(g, xd, B, K, H, W, C, d)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx.float()).all()), "every element of dx is written"
    assert torch.equal(dx, dx2), "two backward runs are bit-identical"
    assert torch.equal(dx, dx3), "dy's pad columns do not reach dx"
    gotd = np.moveaxis(dx.double().cpu().numpy().reshape(B, K, H, W, C), -1, 2)
    mid = K // 2
    for t in range(K):
        s = max(1e-6, float(np.abs(dr[:, t]).max()))
        md = maxdiff(gotd[:, t], dr[:, t])
        print("corr bwd bf16 K=%d C=%d %dx%d d=%d frame %d: maxdiff / s = %.3e (bound %.3e)" % (K, C, H, W, d, t, md / s, EPS + 1e-5))
        assert md <= (EPS + 1e-5) * s, ("centre" if t == mid else "side", t, md / s)
