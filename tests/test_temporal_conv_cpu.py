"""CPU: the cases of tests/test_temporal_conv_gpu.py CAN fail, and the host-side tap lists of frame-window convs.

A kernel-level test of the frame predicate (frame n % Kfr + dz inside [0, Kfr), written out in four kernels) is only worth
its run time if a wrong predicate cannot pass it.  Breaking the predicate in a kernel to see that would read outside the
tensors, so the condition is put on the INPUTS here: for every forward case of the GPU tests, the two results a wrong
predicate would give - (a) windows leak into each other, (b) frame taps ignored - differ from the right reference by at
least 100 x the tolerance the GPU test applies, on every frame (a) or (b) should change."""
import ctypes as C

import numpy as np
import pytest

from tests import temporal_conv_oracle as T


def _per_frame_max(d):
    """(B, C, K, H, W) -> max |.| per frame b*K + t"""
    return np.abs(d).max(axis=(1, 3, 4)).reshape(-1)


@pytest.mark.parametrize("run", T.forward_runs(), ids=lambda r: "%s-K%s-%s%s%s" % (T.case_id(r[0]), r[1], r[4], "-epi" if r[2] else "", "-xf" if r[3] else ""))
def test_wrong_frame_predicates_cannot_pass(run):
    c, K, epi, xf, kind = run
    o = T.operands(c)
    K = o["K"] if K is None else K
    nfr = o["B"] * o["K"]
    ref_of = (lambda v: T.forward_epilogue(c, K, xf, v)) if epi else (lambda v: T.forward(c, K, xf, v))
    ref = ref_of("right")
    assert ref.shape == (nfr // K, c.co, K, o["H"], o["W"])
    leak_frames = T.frames_changed_by_leak(nfr // K, K)
    for variant, frames in (("leak", leak_frames), ("centre", list(range(nfr)) if K > 1 else [])):
        wrong = ref_of(variant)
        if kind == "rms":
            # a whole-tensor relative rms cannot exceed ~1, so 100 x its bound of 1e-2 is out of reach of ANY input: here the
            # wrong results must miss the bound itself by the largest factor the measure allows on these frames (> 25 x)
            rel = float(np.sqrt(((wrong - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean()))
            assert rel > 25 * T.RMS_BOUND, (variant, rel)
            continue
        tol = T.TOL if kind == "f32" else T.TOL + float(np.abs(ref).max()) * 2.0 ** -8
        per = _per_frame_max(wrong - ref)
        # (K = 1 with frame taps: only dz = 0 survives, so "taps ignored" IS the right answer and every frame can leak)
        assert frames or (K == 1 and variant == "centre")
        if frames:
            assert per[frames].min() >= 100 * tol, (variant, float(per[frames].min()), 100 * tol)
        # and nothing else moves: the two wrong results are wrong exactly where they should be
        others = [f for f in range(nfr) if f not in frames]
        assert (per[others].max() if others else 0.0) < 1e-12, variant


def test_layout_round_trip_and_window_reading():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 5, 6, 3, 4))
    f = T.fold(x)
    assert f.shape == (12, 3, 4, 5)
    assert np.array_equal(f[1 * 6 + 2, :, :, 3], x[1, 3, 2])                  # frame b*K + t, channels last
    assert np.array_equal(T.unfold(f, 6), x)
    y = T.rewindow(x, 3)                                                       # the same frames as 4 windows of 3
    assert y.shape == (4, 5, 3, 3, 4) and np.array_equal(y[3, :, 1], x[1, :, 4])
    assert T.frames_changed_by_leak(3, 3) == [2, 3, 5, 6] and T.frames_changed_by_leak(2, 1) == [0, 1]


def test_forward_taps_are_in_kz_ky_kx_order():
    from viddet_amd import ops
    for k, pad in ((3, 1), (1, 0)):
        taps = ops.fwd_taps(k, pad, 3, 1)
        assert len(taps) == 3 * k * k
        for kz in range(3):
            for ky in range(k):
                for kx in range(k):
                    assert taps[(kz * k + ky) * k + kx] == (ky - pad, kx - pad, kz - 1)     # (dy, dx, dz) of OIDHW tap t
    assert ops.fwd_taps(3, 1) == [(ky - 1, kx - 1, 0) for ky in range(3) for kx in range(3)]


def test_data_gradient_plans_flip_the_frame_taps():
    from viddet_amd import ops
    for k, pad in ((3, 1), (1, 0)):
        plans = ops.dgrad_plans(k, pad, 1, 13, 11, kd=3, pad_d=1)
        assert len(plans) == 1
        pl = plans[0]
        assert (pl["py"], pl["px"], pl["Hg"], pl["Wg"]) == (0, 0, 13, 11)
        assert sorted(pl["tap_ids"]) == list(range(3 * k * k))                  # every weight tap exactly once
        for (dy, dx, dz), t in zip(pl["taps"], pl["tap_ids"]):
            kz, ky, kx = t // (k * k), (t // k) % k, t % k
            assert (dy, dx, dz) == (pad - ky, pad - kx, 1 - kz)                 # dz = pad_d - kz
    # stride 2 in space, frame taps unchanged: four parity plans, together every tap once, dz = pad_d - kz in each
    plans = ops.dgrad_plans(3, 1, 2, 8, 8, kd=3, pad_d=1)
    assert sorted(t for pl in plans for t in pl["tap_ids"]) == list(range(27))
    assert all(dz == 1 - t // 9 for pl in plans for (_, _, dz), t in zip(pl["taps"], pl["tap_ids"]))


def test_weight_gradient_workspace_does_not_depend_on_the_window_length():
    """ops.wgrad_ws_bytes asks the library with Kfr = 1.  The library's size depends on Kfr in one place only: the halo-ring
    kernel (another split count) serves 9-tap launches with Kfr = 1 and nothing else, so a launch with frame taps (T = 27
    or T = 3) never takes it and its size is the same for every window length."""
    from viddet_amd import ops, lib as L
    lib = L.load()
    for (B, K, H, W) in (T.SHAPES["workload"], T.SHAPES["tiny"], (16, 3, 26, 26), (64, 3, 13, 13)):
        for kern in ("333", "311"):
            kd, k, pad_d, pad = T.KERNELS[kern]
            for ci, co in ((64, 96), (128, 128), (256, 512)):
                sizes = {}
                for kfr in (1, K):
                    d = L.WgradDesc()
                    d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.Co, d.ldd = B * K, H, W, ci, H, W, co, co
                    d.in_stride, d.Kfr, d.splits = 1, kfr, 0
                    ops._set_taps(d, ops.fwd_taps(k, pad, kd, pad_d))
                    for fl in (0, L.MATH_SPLIT, L.MATH_BF16, L.MATH_F16X2, L.MATH_F16X2 | L.WGRAD_HALO, L.STORE_BF16 | L.MATH_BF16,
                               L.STORE_BF16 | L.MATH_BF16 | L.WGRAD_HALO):
                        d.flags = fl
                        d.amax_in = d.amax_dout = 1 if fl & L.MATH_F16X2 else None
                        assert not lib.vd_conv_wgrad_uses_halo(C.byref(d))
                        sizes[(kfr, fl)] = int(lib.vd_conv_wgrad_ws_bytes(C.byref(d)))
                assert all(sizes[(1, fl)] == sizes[(K, fl)] for (_, fl) in sizes), sizes
                fp32_flags = (0, L.MATH_SPLIT, L.MATH_BF16, L.MATH_F16X2, L.MATH_F16X2 | L.WGRAD_HALO)
                assert ops.wgrad_ws_bytes(B * K, H, W, ci, H, W, co, k, 1, pad, kd, pad_d) >= max(sizes[(K, fl)] for fl in fp32_flags)
