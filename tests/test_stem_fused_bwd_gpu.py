"""GPU: the stem's weight gradient with the BatchNorm-backward apply pass inside it (vd_stem_wgrad_bn, vd_stem.hip).

The reference is the two-launch path the fused kernels replace, which is still in the library: vd_bn_bwd_apply[_bf16] into a
buffer, then vd_stem_wgrad[_bf16] on that buffer.  Pixel order, MFMA sequence, partial tiles and reduction are shared and
the dz arithmetic is one inlined function (vd_bn_math.h), so the weight gradient must be equal bit for bit - at kernel
level on shapes that take every path of the two kernels, and for a whole training step of the network under
VD_STEM_FUSE_BWD = 1 / 0."""
import functools

import numpy as np
import pytest
import torch

from oracle import ops as R
from tests.test_conv_gpu import TOL
from tests.util import dev, maxdiff

pytestmark = pytest.mark.gpu

SLOPE = 0.1
# (N, H, W): partial row group + odd width + one ragged 16-pixel batch | exact row group and batch | a row that crosses a
# batch | a window over 64 KB of LDS (W > 900): the run form (k_stem_wgrad) instead of the row form
SHAPES = [(2, 5, 7), (2, 8, 16), (1, 9, 33), (1, 3, 902)]
PITCHES = [(32, 48), (48, 32), (40, 36)]          # (row pitch of z, of dy); 36 bf16 elements: rows not 16-byte aligned


@functools.lru_cache(maxsize=None)
def _operands(n, h, w):
    """fp32 host operands of one shape: frames, z, dy [n,h,w,32], the per-channel vectors, fp64 sums2 and the count"""
    rng = np.random.default_rng(1000 * n + 10 * h + w)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    x = f32(rng.standard_normal((n, 3, h, w)))
    z, dy = f32(rng.standard_normal((n, h, w, 32))), f32(rng.standard_normal((n, h, w, 32)))
    scale = f32(rng.uniform(0.5, 1.5, 32) * np.where(np.arange(32) % 3 == 0, -1.0, 1.0))     # every third channel negative:
    shift = f32(rng.standard_normal(32) * 0.7)                                                 # the branch follows u, not z
    mean, invstd = f32(rng.standard_normal(32) * 0.3), f32(rng.uniform(0.5, 2.0, 32))
    count = 2.0 * n * h * w                           # SyncBN over two ranks: not the local pixel count
    sums2 = rng.standard_normal(64) * 0.2 * count     # fp64 [sum g | sum g xhat]
    u = z * scale + shift
    assert (u[..., scale < 0] > 0).any() and (u[..., scale < 0] < 0).any() and (u[..., scale > 0] > 0).any() and (u[..., scale > 0] < 0).any()
    return dict(x=x, z=z, dy=dy, scale=scale, shift=shift, mean=mean, invstd=invstd, sums2=sums2, count=count)


def _pitched(t, ld):
    """t [n,h,w,32] in rows of ld elements; the pad columns hold NaN: reading one poisons the result"""
    if ld == t.shape[-1]:
        return t.contiguous()
    out = torch.full(t.shape[:-1] + (ld,), float("nan"), dtype=t.dtype, device=t.device)
    out[..., :t.shape[-1]] = t
    return out


def _two_launch_and_fused(shape, storage):
    """[(pitches, fused dwp)], the two-launch dwp"""
    from viddet_amd import ops, lib as L
    n, h, w = shape
    o = _operands(n, h, w)
    dt = torch.bfloat16 if storage == "bf16" else torch.float32
    x = dev(o["x"])
    z, dy = dev(o["z"]).to(dt), dev(o["dy"]).to(dt)
    vec = [dev(o[k]) for k in ("scale", "shift", "mean", "invstd")]
    sums2 = torch.from_numpy(o["sums2"]).cuda()
    ws = torch.empty(max(16, L.load().vd_stem_wgrad_ws_bytes(n, h, w)), dtype=torch.uint8, device="cuda")
    dz = torch.full((n, h, w, 32), 3.0, dtype=dt, device="cuda")
    ref = torch.full((32, 32), 5.0, device="cuda")
    ops.bn_bwd_apply(z, dy, *vec, sums2, o["count"], n * h * w, 32, dz, slope=SLOPE)
    ops.stem_wgrad(x, dz, ref, ws)
    got = []
    for ldz, ldy in PITCHES:
        dwp = torch.full((32, 32), 7.0, device="cuda")
        ops.stem_wgrad_bn(x, _pitched(z, ldz), _pitched(dy, ldy), *vec, sums2, o["count"], dwp, ws, slope=SLOPE)
        got.append(((ldz, ldy), dwp))
    torch.cuda.synchronize()
    return got, ref, dz


@pytest.mark.parametrize("vec", ["0", "1"])          # VD_STEM_BN_VEC: one element per lane / 16-byte vectors through LDS
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_weight_gradient_has_the_bits_of_the_two_launch_path(monkeypatch, shape, storage, vec):
    monkeypatch.setenv("VD_STEM_BN_VEC", vec)
    got, ref, _ = _two_launch_and_fused(shape, storage)
    assert bool(torch.isfinite(ref).all()) and float(ref[:, :27].abs().min()) > 0.0
    for pitches, dwp in got:
        assert torch.equal(dwp, ref), (shape, storage, pitches, float((dwp - ref).abs().max()))
        assert float(dwp[:, 27:].abs().max()) == 0.0


def test_fused_weight_gradient_matches_the_fp64_oracle():
    """one shape against conv2d_backward of the oracle on dz computed in fp64 from the same operands, at the tolerance of
    the stem weight gradient in tests/test_conv_gpu.py"""
    n, h, w = SHAPES[0]
    o = _operands(n, h, w)
    got, _, _ = _two_launch_and_fused(SHAPES[0], "fp32")
    z, dy = o["z"].astype(np.float64), o["dy"].astype(np.float64)
    sc, sh, mu, iv = [o[k].astype(np.float64) for k in ("scale", "shift", "mean", "invstd")]
    mg, mgx = o["sums2"][:32] / o["count"], o["sums2"][32:] / o["count"]
    u = z * sc + sh
    g = np.where(u > 0, dy, dy * SLOPE)
    dz = sc * (g - mg - (z - mu) * iv * mgx)
    _, dw = R.conv2d_backward(o["x"].astype(np.float64), np.zeros((32, 3, 3, 3)), np.moveaxis(dz, -1, 1), 1, 1)
    dwk = np.zeros((32, 32))
    for ky in range(3):
        for kx in range(3):
            for c in range(3):
                dwk[:, (ky * 3 + kx) * 3 + c] = dw[:, c, ky, kx]
    for pitches, dwp in got:
        assert maxdiff(dwp.cpu().numpy(), dwk) < TOL * np.sqrt(n * h * w), pitches


def _train_step(monkeypatch, fuse, storage, freeze=False):
    from oracle import net as ON
    from tests.test_model_gpu import _targets
    from viddet_amd.model import yolo3_darknet53
    monkeypatch.setenv("VD_AUTOTUNE", "0")             # pinned tiles: the two plans run the same conv kernels
    monkeypatch.setenv("VD_STEM_FUSE_BWD", fuse)
    b, c, size = 2, 3, 64
    P = ON.init_params(c, seed=31, obj_bias=-1.0)
    net = yolo3_darknet53(["c%d" % i for i in range(c)], freeze_base=freeze)
    for k, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[k].astype(np.float32)))
    if storage == "bf16":
        net.set_storage("bf16")
    rng = np.random.default_rng(31)
    x = rng.standard_normal((b, 3, size, size)).astype(np.float32)
    gt, tg = _targets(rng, b, c, size, 3)
    out = [t.clone() for t in net(dev(x), dev(gt), *[dev(t) for t in tg])]
    net.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad().clone() for k, p in net.collect_params().items() if p.span is not None and p.grad_req != 'null'}
    return net, out, grads


def _stem_records(net, sfx):
    """(apply records on the stem's z, stem weight-gradient records as entry-point names) of the last training plan"""
    tp = net._last_train
    stem = [n for n in net.conv_nodes if n.stem][0]
    zptr = tp['bufs']['z:' + stem.dst].data_ptr()
    recs = [r for seg in tp['bwd'] if hasattr(seg, 'recs') for r in seg.recs if r[0]]
    applies = [r for r in recs if r[0].startswith('vd_bn_bwd_apply') and r[2][0] == zptr]
    wgrads = [r[1].__name__ for r in recs if r[0] == 'vd_stem_wgrad' + sfx]
    return applies, wgrads


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_training_step_is_bit_identical_with_and_without_the_fusion(monkeypatch, storage):
    sfx = "_bf16" if storage == "bf16" else ""
    net1, out1, g1 = _train_step(monkeypatch, "1", storage)
    net0, out0, g0 = _train_step(monkeypatch, "0", storage)
    assert len(out1) == 4 and all(torch.equal(a, b) for a, b in zip(out1, out0))
    assert set(g1) == set(g0) and len(g1) > 200
    for k in g1:
        assert torch.equal(g1[k], g0[k]), k
    stem1 = [n for n in net1.conv_nodes if n.stem][0]
    assert torch.equal(net1.grads, net0.grads) and float(stem1.gwp.view(32, 32)[:, :27].abs().min()) > 0.0
    a1, w1 = _stem_records(net1, sfx)
    a0, w0 = _stem_records(net0, sfx)
    assert len(a1) == 0 and w1 == ['vd_stem_wgrad_bn' + sfx], (len(a1), w1)
    assert len(a0) == 1 and w0 == ['vd_stem_wgrad' + sfx], (len(a0), w0)
    b1, b0 = net1._last_train['bufs'], net0._last_train['bufs']
    for nm in ('dz', 'dz2'):          # the next-largest cell (64 channels at half the side) sizes the scratch
        assert 2 * b1[nm].numel() == b0[nm].numel() == b0['z:' + net0.conv_nodes[0].dst].numel(), nm


def test_frozen_backbone_emits_neither_the_apply_pass_nor_the_stem_weight_gradient(monkeypatch):
    net, out, _ = _train_step(monkeypatch, "1", "fp32", freeze=True)
    applies, wgrads = _stem_records(net, "")
    assert applies == [] and wgrads == []
    assert all(bool(torch.isfinite(t).all()) for t in out)
