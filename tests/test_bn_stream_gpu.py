"""GPU: the unrolled streaming forms of vd_bn_apply_leaky / vd_bn_bwd_apply (vd_bn.hip) and their launch geometry.

What the unroll adds to the kernels that tests/test_bn_fused_gpu.py, tests/test_bn_pointwise_gpu.py and
tests/test_pointwise_edges_gpu.py already pin: the ragged end (a predicate on each of the U accesses of a thread), groups of
blocks that share a run where the vector-column count does not divide 256, and the 8-channel bf16 forms with their two fallbacks.

Shapes are chosen from the grid the launcher uses.  vd_bn_stream_grid gives the block count and the unroll factor U of a launch;
the test derives the block count again from the rule in vd_bn.hip and requires the two to agree: a group of step = cvec /
gcd(256, cvec) blocks owns one contiguous "run" of U * step * 256 vectors, and the grid is one group per run (it does not
depend on the device: a grid sized by the CU count was measured and lost).  A tensor [M, C] has M * cvec vectors
(cvec = C / 4, or C / 8 in the 8-channel bf16 form), so the nearest sizes to a whole number of runs are ONE ROW more and one row
less, not one vector: a run is a multiple of cvec.

References are numpy fp64 on the fp32 / bf16 values the device reads, evaluated in row chunks.  The bounds are those of
tests/test_bn_fused_gpu.py::test_streaming_kernels_keep_their_channel_column, unchanged: fp32 outputs 1e-4 (apply) / 2e-4
(backward) absolute times max |scale|; bf16 outputs 1e-5 + max |ref| * 2^-8, the maximum taken over the chunk of rows under
comparison, which is never above that file's maximum over the whole tensor.

The published max-abs equals the max |.| of the device's own output exactly.  Every output lies between two guard bands."""
import math

import numpy as np
import pytest
import torch

from tests.util import dev

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS_BF = 2.0 ** -8
GUARD = 64
SENT = -7.0e30
SLOPE = 0.1
CHUNK_ELEMS = 1 << 20         # elements per chunk of the fp64 reference

SHAPES = ["sub_wave", "one_block", "runs_plus_row", "runs_minus_row", "runs_2p3", "runs_many"]
# (C, storage, misaligned): cvec 8; 24 (does not divide 256); 256; 512 (larger than a block).  bf16: C = 36 takes the 4-channel
# fallback by channel count, a base pointer 8 bytes off takes it by alignment
CONFIGS = [(C, "fp32", False) for C in (32, 96, 1024, 2048)] + [(C, "bf16", False) for C in (32, 96, 1024, 2048, 36)] + \
          [(96, "bf16", True)]
IDS = ["C%d-%s%s" % (C, s, "-off8" if m else "") for C, s, m in CONFIGS]


def _vec_width(C, bf16, misaligned):
    """channels per thread and access of the launch: 8 for aligned bf16 tensors with C % 8 == 0 (VD_BN_BF16X8 permitting), else 4"""
    import os
    if bf16 and not misaligned and C % 8 == 0 and os.environ.get("VD_BN_BF16X8", "1") != "0" and os.environ.get("VD_BN_STREAM", "1") != "0":
        return 8
    return 4


def _grid(nv, cvec):
    """(blocks, U) of the launch over nv vectors: from the library, and checked against the rule it documents"""
    import ctypes
    from viddet_amd import lib as L
    u = ctypes.c_int(0)
    nb = L.load().vd_bn_stream_grid(nv, cvec, ctypes.byref(u))
    assert nb > 0 and u.value >= 1
    step = cvec // math.gcd(256, cvec)
    if u.value > 1:                 # the unrolled form (VD_BN_STREAM=0 keeps the grid-stride kernels, U = 1)
        assert u.value == L.BN_STREAM_UNROLL
        assert nb == -(-nv // (u.value * step * 256)) * step, (nb, nv, step)
    assert (nb * 256) % cvec == 0
    return nb, u.value, step


def _rows(shape, C, V):
    """M of a named shape for channel count C in the V-channel form"""
    cvec = C // V
    if shape == "sub_wave":
        return 3                                     # M = 3: 24 float4 at C = 32, fewer than one wave
    if shape == "one_block":
        return 256 // cvec if 256 % cvec == 0 else -(-256 // cvec)     # exactly 256 vectors where cvec divides 256
    _, u, step = _grid(cvec, cvec)
    run = u * step * 256                             # vectors of one group of blocks
    assert run % cvec == 0
    rows = run // cvec
    # one row past three whole runs (only j = 0 of the last group, and of some of its threads), one row short of them, between
    # 2 and 3 runs, and 41.3 runs (more groups than one XCD round of blocks)
    return {"runs_plus_row": 3 * rows + 1, "runs_minus_row": 3 * rows - 1, "runs_2p3": -(-23 * rows // 10),
            "runs_many": -(-413 * rows // 10)}[shape]


def _guarded2d(M, C, dtype, off8=False):
    """an [M, C] output between two guard bands of sentinels; off8: the interior starts 8 bytes past a 16-byte boundary"""
    extra = (8 // torch.empty((), dtype=dtype).element_size()) if off8 else 0
    buf = torch.full((M * C + 2 * GUARD + extra,), SENT, dtype=dtype, device="cuda")
    view = buf[GUARD + extra:GUARD + extra + M * C].view(M, C)
    assert view.data_ptr() % 16 == (8 if off8 else 0)
    return buf, view, GUARD + extra


def _intact(buf, lo, n):
    s = torch.tensor(SENT, dtype=buf.dtype, device=buf.device)         # the sentinel as the storage type rounds it
    return bool((buf[:lo] == s).all()) and bool((buf[lo + n:] == s).all())


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _place(t, off8):
    """t on the device; off8: 8 bytes into a 16-byte aligned allocation"""
    if not off8:
        return t.cuda()
    e = 8 // t.element_size()
    buf = torch.empty(t.numel() + e, dtype=t.dtype, device="cuda")
    v = buf[e:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


def _channel_vectors(C):
    """per-channel vectors that differ strongly from channel to channel (a wrong column is off by far more than a bound)"""
    c = np.arange(C, dtype=np.float64)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    scale = f(1.0 + (c % 61) * 0.25 + c / 256)
    shift = f(((c * 5) % 11 - 5.0) * 0.37)
    mean = f(((c * 7) % 13 - 6.0) * 0.21)
    invstd = f(0.5 + (c % 9) * 0.3)
    mg, mgx = ((c * 3) % 7 - 3.0) * 0.11, ((c * 5) % 9 - 4.0) * 0.07
    return scale, shift, mean, invstd, mg, mgx


_DATA = {}


def _tensors(n, dt):
    """three seeded tensors of n elements in the storage type (shared by every case with that element count; never written)"""
    key = (n, dt)
    if key not in _DATA:
        if len(_DATA) >= 2:
            _DATA.clear()
        g = torch.Generator(device="cuda").manual_seed(n % 1000003)
        _DATA[key] = tuple((torch.randn(n, device="cuda", generator=g) * s).to(dt) for s in (1.5, 1.0, 0.7))
    return _DATA[key]


def _chunks(M, C):
    step = max(1, CHUNK_ELEMS // C)
    for r0 in range(0, M, step):
        yield r0, min(M, r0 + step)


def _check(gots, ref_fn, M, C, bf16):
    """gots {name: [M, C] device tensor} against ref_fn(r0, r1) -> {name: (ref, fp32 absolute bound)}, chunk by chunk in one pass over
    the inputs; prints the worst error / bound ratio of each"""
    cpu = {k: g.detach().cpu() for k, g in gots.items()}
    worst = {k: 0.0 for k in gots}
    for k, g in cpu.items():
        assert bool(torch.isfinite(g.float()).all()), k
    for r0, r1 in _chunks(M, C):
        refs = ref_fn(r0, r1)
        for k, g in cpu.items():
            ref, tol = refs[k]
            if bf16:
                tol = 1e-5 + float(np.abs(ref).max()) * EPS_BF
            err = np.abs(g[r0:r1].double().numpy() - ref)
            bad = err > tol
            worst[k] = max(worst[k], float(err.max()) / tol)
            assert not bad.any(), (k, r0 + int(np.argwhere(bad)[0][0]), int(np.argwhere(bad)[0][1]), float(err[bad].max()))
    for k in gots:
        print("%-12s worst err / bound %.3f" % (k, worst[k]))


def _setup(shape, C, storage, off8):
    bf16 = storage == "bf16"
    dt = BF if bf16 else torch.float32
    V = _vec_width(C, bf16, off8)
    M = _rows(shape, C, V)
    z, res, dy = [t.view(M, C) for t in _tensors(M * C, dt)]
    return bf16, dt, M, z, res, dy


@pytest.mark.parametrize("C,storage,off8", CONFIGS, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_apply_leaky_over_ragged_trips(shape, C, storage, off8):
    """vd_bn_apply_leaky / _bf16 with and without the residual, with and without amax_out (fp32 only: the bf16 entry has none)"""
    from viddet_amd import ops, lib as L
    bf16, dt, M, z, res, _ = _setup(shape, C, storage, off8)
    zc, rc = z.cpu(), res.cpu()
    scale, shift = _channel_vectors(C)[:2]
    zd, rd = (_place(zc, off8) if off8 else z), res
    sc, sh = dev(scale), dev(shift)

    def ref_fn(r0, r1):
        zr, rr = zc[r0:r1].double().numpy(), rc[r0:r1].double().numpy()
        u = zr * scale + shift
        act = np.where(u > 0, u, SLOPE * u)
        tol = 1e-4 * float(np.abs(scale).max())
        return {"apply": (act, tol), "apply+res": (act + rr, tol)}

    gots = {}
    for with_res in (False, True):
        name = "apply+res" if with_res else "apply"
        for with_amax in ((False,) if bf16 else (False, True)):
            buf, y, lo = _guarded2d(M, C, dt, off8)
            slot = torch.zeros(L.AMAX_FLOATS, device="cuda") if with_amax else None
            ops.bn_apply_leaky(zd, sc, sh, rd if with_res else None, y, M, C, slope=SLOPE, amax_out=slot)
            torch.cuda.synchronize()
            assert _intact(buf, lo, M * C), "guard bands"
            if with_amax:       # the same output as without the slots, bit for bit, and their max is its max-abs
                assert torch.equal(_bits(y), _bits(gots[name]))
                assert ops.amax_value(slot) == float(y.abs().max())
            else:
                gots[name] = y
    _check(gots, ref_fn, M, C, bf16)


@pytest.mark.parametrize("C,storage,off8", CONFIGS, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bwd_apply_over_ragged_trips(shape, C, storage, off8):
    """vd_bn_bwd_apply / _bf16; sums2 = count * (per-channel means of g and g xhat), chosen per channel, not reduced from the data"""
    from viddet_amd import ops, lib as L
    bf16, dt, M, z, _, dy = _setup(shape, C, storage, off8)
    zc, dc = z.cpu(), dy.cpu()
    scale, shift, mean, invstd, mg, mgx = _channel_vectors(C)
    count = float(M)
    sums2 = np.concatenate([mg, mgx]) * count
    # what the device makes of them: fl(fl(sums2) * fl(1 / count)) is within 3u of these
    mgr, mgxr = sums2[:C] / count, sums2[C:] / count
    zd, dyd = (_place(zc, off8) if off8 else z), dy
    sc, sh, mu, iv = dev(scale), dev(shift), dev(mean), dev(invstd)
    s2 = torch.from_numpy(sums2).cuda()

    def ref_fn(r0, r1):
        zr, dr = zc[r0:r1].double().numpy(), dc[r0:r1].double().numpy()
        u = zr * scale + shift
        g = np.where(u > 0, dr, SLOPE * dr)
        xh = (zr - mean) * invstd
        ref = scale * (g - mgr - xh * mgxr)
        tol = 2e-4 * float(np.abs(scale).max())
        return {"bwd": (ref, tol)}

    gots = {}
    for with_amax in ((False,) if bf16 else (False, True)):
        buf, dx, lo = _guarded2d(M, C, dt, off8)
        slot = torch.zeros(L.AMAX_FLOATS, device="cuda") if with_amax else None
        ops.bn_bwd_apply(zd, dyd, sc, sh, mu, iv, s2, count, M, C, dx, slope=SLOPE, amax_out=slot)
        torch.cuda.synchronize()
        assert _intact(buf, lo, M * C), "guard bands"
        if with_amax:
            assert torch.equal(_bits(dx), _bits(gots["bwd"]))
            assert ops.amax_value(slot) == float(dx.abs().max())
        else:
            gots["bwd"] = dx
    _check(gots, ref_fn, M, C, bf16)


def _split_rows(C, V):
    """M of at least 300.3 runs and an odd split row at about 0.37 of it: the whole tensor, the head and the tail run on
    different grids with different ragged ends.  The whole tensor is at least 128 MiB, from which size on the launcher loads
    the streams that are not read again soon with the nontemporal policy; the head and the tail are smaller and use plain loads."""
    cvec = C // V
    _, u, step = _grid(cvec, cvec)
    rows = u * step * 256 // cvec
    M = max((3003 * rows) // 10 + 1, (1 << 27) // (C * (2 if V == 8 else 4)) + 7)      # and no less than 128 MiB (see there)
    M1 = ((37 * M) // 100) | 1
    assert len({_grid(m * cvec, cvec)[0] for m in (M, M1, M - M1)}) == 3
    return M, M1


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_apply_leaky_does_not_depend_on_the_launch_geometry(storage):
    """the output on [M, C] is bit for bit the outputs on two row slices run as launches of their own (with residual and amax;
    the max-abs of the whole is the larger of the parts')"""
    from viddet_amd import ops, lib as L
    C, bf16 = 96, storage == "bf16"
    dt = BF if bf16 else torch.float32
    M, M1 = _split_rows(C, _vec_width(C, bf16, False))
    z, res, _ = [t.view(M, C) for t in _tensors(M * C, dt)]
    scale, shift = _channel_vectors(C)[:2]
    sc, sh = dev(scale), dev(shift)
    outs, amaxes = [], []
    for r0, r1 in ((0, M), (0, M1), (M1, M)):
        y = torch.empty(r1 - r0, C, dtype=dt, device="cuda")
        slot = None if bf16 else torch.zeros(L.AMAX_FLOATS, device="cuda")
        ops.bn_apply_leaky(z[r0:r1], sc, sh, res[r0:r1], y, r1 - r0, C, slope=SLOPE, amax_out=slot)
        torch.cuda.synchronize()
        outs.append(y)
        amaxes.append(None if bf16 else ops.amax_value(slot))
    assert torch.equal(_bits(outs[0]), _bits(torch.cat(outs[1:])))
    if not bf16:
        assert amaxes[0] == max(amaxes[1:])


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_bwd_apply_does_not_depend_on_the_launch_geometry(storage):
    """as above for vd_bn_bwd_apply, with the same sums2 and count in all three launches"""
    from viddet_amd import ops, lib as L
    C, bf16 = 96, storage == "bf16"
    dt = BF if bf16 else torch.float32
    M, M1 = _split_rows(C, _vec_width(C, bf16, False))
    z, _, dy = [t.view(M, C) for t in _tensors(M * C, dt)]
    scale, shift, mean, invstd, mg, mgx = _channel_vectors(C)
    sc, sh, mu, iv = dev(scale), dev(shift), dev(mean), dev(invstd)
    count = float(M)
    s2 = torch.from_numpy(np.concatenate([mg, mgx]) * count).cuda()
    outs, amaxes = [], []
    for r0, r1 in ((0, M), (0, M1), (M1, M)):
        dx = torch.empty(r1 - r0, C, dtype=dt, device="cuda")
        slot = None if bf16 else torch.zeros(L.AMAX_FLOATS, device="cuda")
        ops.bn_bwd_apply(z[r0:r1], dy[r0:r1], sc, sh, mu, iv, s2, count, r1 - r0, C, dx, slope=SLOPE, amax_out=slot)
        torch.cuda.synchronize()
        outs.append(dx)
        amaxes.append(None if bf16 else ops.amax_value(slot))
    assert torch.equal(_bits(outs[0]), _bits(torch.cat(outs[1:])))
    if not bf16:
        assert amaxes[0] == max(amaxes[1:])
