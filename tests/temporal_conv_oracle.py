"""fp64 references for the frame-window (temporal) convolutions at kernel level.  TEST INFRASTRUCTURE ONLY, no GPU.

The 3-D (3,3,3) and 2+1-D (3,1,1) neck convs of the window networks (models/definitions/layers.py:73-79, nn.Conv3D) run through
the tap-list kernels with a frame offset per tap (dz) and a window length (Kfr): frame n of the device tensor [B*K, H, W, C] is
frame n % K of window n // K, and a tap whose frame n % K + dz leaves [0, K) reads zeros.  Here: the layout conversions, the
case tables shared by tests/test_temporal_conv_cpu.py and tests/test_temporal_conv_gpu.py, and every reference those compare
with - oracle/ops.py conv3d / conv3d_backward (checked against torch in tests/test_oracle_cpu.py) plus the epilogues, the
in-load transform, the fused statistics and the fused BatchNorm-backward sums restated in fp64.

Every reference is cached per (case, window length): the tile variants of one case share one CPU computation, and nothing
that is returned may be modified by a caller."""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

from oracle import ops as R

# name: (B windows, K frames per window, H, W)
SHAPES = {
    "workload": (3, 3, 13, 13),   # 169 rows per frame: frames and windows end inside every M tile size
    "ragged": (3, 5, 5, 7),       # 35 rows per frame: a 128-row tile spans > 3 frames and crosses a window boundary; K = 5
    "tiny": (11, 3, 2, 2),        # 4 rows per frame, 132 rows: a tile holds > 10 whole windows; wgrad's one_wrap == false path
    "pair": (4, 2, 7, 5),         # K = 2: each frame has exactly one temporal neighbour
    "single": (5, 1, 6, 6),       # K = 1 with frame taps: only dz = 0 survives
    "long": (2, 9, 5, 7),         # longer windows, same kernels; also read as 6 windows of 3 (window length honoured)
    "streamk": (36, 3, 13, 13),   # "workload" with B raised until the persistent stream-K grids apply (18252 rows)
}
# name: (kd, k, pad_d, pad) - the (3,3,3) / pad (1,1,1) conv (T = 27) and the (3,1,1) / pad (1,0,0) conv (T = 3)
KERNELS = {"333": (3, 3, 1, 1), "311": (3, 1, 1, 0)}

Case = namedtuple("Case", "shape ci co kern bf16")
Case.__new__.__defaults__ = (False,)


def case_id(c):
    return "%s-%dto%d-%s%s" % (c.shape, c.ci, c.co, c.kern, "-bf16" if c.bf16 else "")


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
def fold(x):
    """oracle (B, C, K, H, W) -> device layout [B*K, H, W, C] (frame b*K + t), numpy"""
    b, c, k, h, w = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 3, 4, 1).reshape(b * k, h, w, c))


def unfold(a, K):
    """device layout [N, H, W, C] (numpy or torch) -> oracle (N // K, C, K, H, W), float64"""
    if torch.is_tensor(a):
        a = a.detach().float().cpu().numpy()
    a = np.asarray(a, dtype=np.float64)
    n, h, w, c = a.shape
    assert n % K == 0
    return a.reshape(n // K, K, h, w, c).transpose(0, 4, 1, 2, 3)


def rewindow(x, K):
    """the same frames read as windows of K: (B, C, K0, H, W) -> (B*K0 // K, C, K, H, W)"""
    return unfold(fold(x), K)


def bf16_round(a):
    """round to bf16, return float64 (tests/test_bf16_gpu.py::_bf16_round)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy().astype(np.float64)


def leaky(u, slope=0.1):
    return np.where(u > 0, u, slope * u)


def _c(v):
    return v.reshape(1, -1, 1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(c):
    """every operand a test of this case may use, from one seed per case.  Tensors (B, C, K, H, W) / weight OIDHW, float64;
    the bf16 variant rounds the TENSOR operands (x, w, dy, res, prev, bs_z) to bf16-representable values."""
    B, K, H, W = SHAPES[c.shape]
    kd, k, pad_d, pad = KERNELS[c.kern]
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    rnd = bf16_round if c.bf16 else (lambda a: a)
    o = dict(B=B, K=K, H=H, W=W, kd=kd, k=k, pad_d=pad_d, pad=pad)
    o["x"] = rnd(rng.standard_normal((B, c.ci, K, H, W)))
    o["w"] = rnd(rng.standard_normal((c.co, c.ci, kd, k, k)) / np.sqrt(c.ci * kd * k * k))      # outputs O(1)
    o["dy"] = rnd(rng.standard_normal((B, c.co, K, H, W)))
    # forward epilogue: the shift and the residual at a quarter of the output's scale - they add to max|ref| (the bf16-output
    # tolerance) and not to what a wrong frame predicate changes (tests/test_temporal_conv_cpu.py holds the cases to that ratio)
    o["res"] = rnd(0.25 * rng.standard_normal((B, c.co, K, H, W)))
    o["scale"], o["shift"] = rng.uniform(0.5, 1.5, c.co), 0.25 * rng.standard_normal(c.co)
    # in-load transform: shifts away from 0, so that leaky(b) leaking into a padded pixel or frame shows at O(1)
    o["in_scale"] = rng.uniform(0.5, 1.5, c.ci)
    o["in_shift"] = rng.uniform(0.5, 1.5, c.ci) * rng.choice([-1.0, 1.0], c.ci)
    # data gradient: the gradient it accumulates into, and the BatchNorm of the producer of x (fused backward reductions)
    o["prev"] = rnd(rng.standard_normal((B, c.ci, K, H, W)))
    o["bs_z"] = rnd(rng.standard_normal((B, c.ci, K, H, W)) * 1.5)
    o["bs_scale"], o["bs_shift"] = rng.uniform(0.5, 1.5, c.ci), rng.standard_normal(c.ci) * 0.3
    o["bs_mean"], o["bs_invstd"] = rng.standard_normal(c.ci) * 0.1, rng.uniform(0.5, 2.0, c.ci)
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


def _frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs if len(arrs) > 1 else arrs[0]


# ---------------------------------------------------------------------------------------------------------------------
# references (fp64)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward(c, K=None, xf=False, variant="right"):
    """raw conv output (B', Co, K', H, W) of the case's frames read as windows of K (default: the case's own K).
    xf: the activation operand is leaky(x * in_scale + in_shift), padding exactly 0 in space and in time.
    variant: "right"; "leak" = the WRONG result of windows leaking into each other (all frames one sequence); "centre" = the
    WRONG result of frame taps being ignored (the centre kz slice as a 2-D conv of every frame)."""
    o = operands(c)
    K = o["K"] if K is None else K
    x = o["x"]
    if xf:
        x = leaky(x * _c(o["in_scale"]) + _c(o["in_shift"]))
    if variant == "right":
        z = R.conv3d(rewindow(x, K), o["w"], o["pad_d"], o["pad"])
    elif variant == "leak":
        z = rewindow(R.conv3d(rewindow(x, o["B"] * o["K"]), o["w"], o["pad_d"], o["pad"]), K)
    else:
        assert variant == "centre"
        z = R.conv3d(rewindow(x, K), o["w"][:, :, o["pad_d"]:o["pad_d"] + 1], 0, o["pad"])
    return _frozen(np.ascontiguousarray(z))


def epilogue(c, z, K=None):
    """affine + LeakyReLU 0.1 + residual on a raw output z of forward(c, K)"""
    o = operands(c)
    K = o["K"] if K is None else K
    return leaky(z * _c(o["scale"]) + _c(o["shift"])) + rewindow(o["res"], K)


@functools.lru_cache(maxsize=None)
def forward_epilogue(c, K=None, xf=False, variant="right"):
    return _frozen(epilogue(c, forward(c, K, xf, variant), K))


@functools.lru_cache(maxsize=None)
def statistics(c, K=None):
    """per-channel sum and sum of squares of the raw output (the fused BatchNorm statistics)"""
    z = forward(c, K)
    return _frozen(z.sum(axis=(0, 2, 3, 4)), (z ** 2).sum(axis=(0, 2, 3, 4)))


@functools.lru_cache(maxsize=None)
def backward(c, K=None, xf=False):
    """(dx, dw) of the conv for the output gradient dy; dx (B', Ci, K', H, W), dw OIDHW.  xf: with the activation operand
    leaky(x * in_scale + in_shift) (the weight gradient's in-load transform; dx is then the gradient of that tensor)"""
    o = operands(c)
    K = o["K"] if K is None else K
    x = leaky(o["x"] * _c(o["in_scale"]) + _c(o["in_shift"])) if xf else o["x"]
    dx, dw = R.conv3d_backward(rewindow(x, K), o["w"], rewindow(o["dy"], K), o["pad_d"], o["pad"])
    return _frozen(np.ascontiguousarray(dx), np.ascontiguousarray(dw))


@functools.lru_cache(maxsize=None)
def backward_bn_sums(c, K=None):
    """the accumulated gradient g_all = dx + prev and the fused BatchNorm-backward sums of the producer of x: with
    g = g_all * leaky'(z * scale + shift) and xhat = (z - mean) * invstd, concat(sum g, sum g * xhat) per channel
    (tests/test_bf16_train_gpu.py::test_data_gradient_with_fused_batchnorm_backward_reductions)"""
    o = operands(c)
    K = o["K"] if K is None else K
    g_all = backward(c, K)[0] + rewindow(o["prev"], K)
    z = rewindow(o["bs_z"], K)
    u = z * _c(o["bs_scale"]) + _c(o["bs_shift"])
    g = np.where(u > 0, g_all, 0.1 * g_all)
    sums = np.concatenate([g.sum(axis=(0, 2, 3, 4)), (g * (z - _c(o["bs_mean"])) * _c(o["bs_invstd"])).sum(axis=(0, 2, 3, 4))])
    return _frozen(g_all, sums)


def frames_changed_by_leak(B, K):
    """frames (b*K + t) that differ when windows leak: the first and last frame of each window, except the outer ends of the
    batch; for K = 1 every frame is both"""
    n = B * K
    return [f for f in range(n) if (f % K == 0 and f > 0) or (f % K == K - 1 and f < n - 1)]


# ---------------------------------------------------------------------------------------------------------------------
# the forward cases of tests/test_temporal_conv_gpu.py, one table per test group: (case, window length or None, epilogue?,
# in-load transform?, tolerance kind).  tests/test_temporal_conv_cpu.py checks on each that a kernel with a wrong frame
# predicate could not pass.  Tolerance kinds: "f32" = 2e-4 absolute; "bf16out" = 2e-4 + max|ref| * 2^-8 (a bf16 output);
# "rms" = relative rms error < 1e-2 (bf16 products: tests/test_split_math_gpu.py::test_bf16_products_forward_and_gradients)
# ---------------------------------------------------------------------------------------------------------------------
TOL = 2e-4
RMS_BOUND = 1e-2

C_ = Case
FP32_TILE0 = [C_("workload", 128, 96, "333"), C_("workload", 128, 96, "311"), C_("ragged", 64, 96, "333"), C_("ragged", 64, 96, "311"),
              C_("tiny", 64, 128, "333"), C_("tiny", 64, 128, "311"), C_("pair", 64, 96, "333"), C_("pair", 64, 96, "311"),
              C_("single", 128, 128, "333"), C_("single", 128, 128, "311"), C_("long", 64, 128, "333"), C_("long", 64, 128, "311")]
EVERY_TILE = [C_("workload", 128, 96, "333"), C_("workload", 128, 96, "311"), C_("ragged", 64, 96, "333"), C_("ragged", 64, 96, "311")]
STREAMK = C_("streamk", 64, 256, "333", True)         # bf16-representable operands: the fp32 and the bf16 kernel share the reference
XF_CASES = [C_("ragged", 64, 96, "333"), C_("ragged", 64, 96, "311"), C_("pair", 64, 96, "333"), C_("pair", 64, 96, "311")]
STATS_CASES = [C_("workload", 128, 96, "333"), C_("tiny", 64, 128, "333")]
BF16_EVERY_TILE = [C_("workload", 64, 96, "333", True), C_("workload", 128, 96, "311", True)]
BF16_CI32 = [C_("ragged", 32, 96, "333", True), C_("ragged", 32, 96, "311", True)]
BF16_SPLITK = C_("workload", 64, 128, "333", True)
# (case, fp32 output?): four rows per frame of "tiny" cannot tell a wrong tap from one bf16 rounding of the output by 100 x
BF16_STATS = [(C_("workload", 64, 96, "333", True), False), (C_("tiny", 64, 128, "333", True), True)]
WINDOW_CASES = [C_("long", 64, 128, "333"), C_("long", 64, 128, "333", True)]
WINDOW_LENGTHS = (9, 3)


def forward_runs():
    """every (case, K, epilogue, xf, tolerance kind) a forward GPU test compares with its reference"""
    runs = []
    for c in FP32_TILE0 + EVERY_TILE:
        runs += [(c, None, False, False, "f32"), (c, None, True, False, "f32")]
    for c in EVERY_TILE:
        runs += [(c, None, False, False, "rms")]
    runs += [(STREAMK, None, False, False, "f32"), (STREAMK, None, True, False, "f32"), (STREAMK, None, False, False, "bf16out")]
    runs += [(c, None, False, True, "f32") for c in XF_CASES]
    runs += [(c, None, False, False, "f32") for c in STATS_CASES]
    for c in BF16_EVERY_TILE + BF16_CI32 + [BF16_SPLITK]:
        runs += [(c, None, e, False, t) for e in (False, True) for t in ("f32", "bf16out")]
    runs += [(c, None, False, False, "f32" if f32 else "bf16out") for c, f32 in BF16_STATS]
    for c in WINDOW_CASES:
        runs += [(c, K, False, False, "bf16out" if c.bf16 else "f32") for K in WINDOW_LENGTHS]
    seen, out = set(), []
    for r in runs:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out
