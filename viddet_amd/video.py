"""Image-side training augmentations of the reference's video pipeline, on NumPy arrays (k,h,w,c).

Mirrors (paths under /root/reference):
  random_expand          models/transforms/video.py:12-65
  random_color_distort   models/transforms/video.py:68-158
  imresize               gluoncv.data.transforms.image.imresize -> mx.image.imresize (called at
                         models/definitions/yolo/transforms.py:229,332; interp codes 0-4, 9, 10)

The random decisions are drawn in the reference's order from the reference's two sources - NumPy's global RNG and
Python's `random` module (the hue angle and the expand ratio / offsets use the latter) - through an `Rng` pair, so a
caller that seeds both (or passes the global modules) consumes exactly the numbers the reference's code would.

[UPSTREAM-UNVERIFIED] mx.image.imresize is an OpenCV cv::resize call; OpenCV is not available offline.  The kernels
below follow OpenCV's sampling convention (pixel centres: src = (dst + 0.5) * scale - 0.5, replicated borders; bicubic
a = -0.75; Lanczos a = 4; INTER_AREA = coverage-weighted box average when shrinking), in float arithmetic - not OpenCV's
fixed-point uint8 paths, so uint8 results can differ from cv2 by one grey level.
"""
import functools
import random as _pyrandom

import numpy as np


class Rng:
    """The two random sources the reference's transforms draw from: `np` (numpy.random module or a RandomState) and
    `py` (the random module or a random.Random).  Default: the global modules, as in the reference."""

    def __init__(self, np_rng=None, py_rng=None):
        self.np = np.random if np_rng is None else np_rng
        self.py = _pyrandom if py_rng is None else py_rng

    @classmethod
    def seeded(cls, seed):
        return cls(np.random.RandomState(seed), _pyrandom.Random(seed))


def expand_params(h, w, rng=None, max_ratio=4, keep_ratio=True):
    """The decisions of `random_expand` for (h,w) frames, without pixels: (offset_x, offset_y, new_width, new_height).
    Draws: random.uniform(1, max_ratio) [, a second one if not keep_ratio], random.randint(0, oh - h),
    random.randint(0, ow - w)."""
    rng = Rng() if rng is None else rng
    ratio_x = rng.py.uniform(1, max_ratio)
    ratio_y = ratio_x if keep_ratio else rng.py.uniform(1, max_ratio)
    oh, ow = int(h * ratio_y), int(w * ratio_x)
    off_y = rng.py.randint(0, oh - h)
    off_x = rng.py.randint(0, ow - w)
    return off_x, off_y, ow, oh


def random_expand(src, max_ratio=4, fill=0, keep_ratio=True, rng=None):
    """video.py:12-65: place the (k,h,w,c) frames on a larger canvas filled with `fill`.
    Returns (canvas, (offset_x, offset_y, new_width, new_height)).  Draws: those of `expand_params`."""
    if max_ratio <= 1:
        return src, (0, 0, src.shape[1], src.shape[0])          # (:39-40, the reference's own index slip kept)
    k, h, w, c = src.shape
    off_x, off_y, ow, oh = expand_params(h, w, rng, max_ratio, keep_ratio)
    if np.isscalar(fill):
        dst = np.full((k, oh, ow, c), fill, dtype=src.dtype)
    else:
        fill = np.asarray(fill, dtype=src.dtype)
        if c != fill.size:
            raise ValueError("Channel and fill size mismatch, {} vs {}".format(c, fill.size))
        dst = np.tile(fill.reshape(1, 1, 1, c), (k, oh, ow, 1))
    dst[:, off_y:off_y + h, off_x:off_x + w, :] = src
    return dst, (off_x, off_y, ow, oh)


_TYIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.321], [0.211, -0.523, 0.311]])
_ITYIQ = np.array([[1.0, 0.956, 0.621], [1.0, -0.272, -0.647], [1.0, -1.107, 1.705]])


def hue_matrix(alpha):
    """video.py:131-146: the 3x3 the frames are right-multiplied by for a hue rotation of alpha * pi."""
    u, w = np.cos(alpha * np.pi), np.sin(alpha * np.pi)
    bt = np.array([[1.0, 0.0, 0.0], [0.0, u, -w], [0.0, w, u]])
    return np.dot(np.dot(_ITYIQ, bt), _TYIQ).T


_GRAY = (0.299, 0.587, 0.114)


def color_distort_params(rng=None, brightness_delta=32, contrast_low=0.5, contrast_high=1.5, saturation_low=0.5,
                         saturation_high=1.5, hue_delta=18):
    """The decisions of `random_color_distort`, without pixels: the operations that were drawn, in the order they apply, as
    [(name, parameter)] - ('brightness', float32 delta), ('contrast', float32 factor), ('saturation', float32 factor),
    ('hue', python float angle).  Draw order: brightness gate (np.uniform) [+ delta], order coin (np.randint(0, 2)), then
    contrast / saturation / hue - or saturation / hue / contrast - each a gate (np.uniform(0, 1) > 0.5) followed, if taken, by
    its parameter (np.uniform; the hue angle from random.uniform)."""
    rng = Rng() if rng is None else rng
    ops = []

    def brightness():
        if rng.np.uniform(0, 1) > 0.5:
            ops.append(("brightness", np.float32(rng.np.uniform(-brightness_delta, brightness_delta))))

    def contrast():
        if rng.np.uniform(0, 1) > 0.5:
            ops.append(("contrast", np.float32(rng.np.uniform(contrast_low, contrast_high))))

    def saturation():
        if rng.np.uniform(0, 1) > 0.5:
            ops.append(("saturation", np.float32(rng.np.uniform(saturation_low, saturation_high))))

    def hue():
        if rng.np.uniform(0, 1) > 0.5:
            ops.append(("hue", rng.py.uniform(-hue_delta, hue_delta)))

    brightness()
    if rng.np.randint(0, 2):
        contrast(), saturation(), hue()
    else:
        saturation(), hue(), contrast()
    return ops


def apply_color_ops(src, ops):
    """The float32 arithmetic of video.py:68-158 for a list of `color_distort_params` operations."""
    x = np.asarray(src).astype(np.float32)
    for name, p in ops:
        if name == "brightness":
            x = x + p
        elif name == "contrast":
            x = x * p
        elif name == "saturation":
            gray = (x * np.array(_GRAY, np.float32)).sum(axis=-1, keepdims=True)
            x = x * p + gray * (np.float32(1.0) - p)
        elif name == "hue":
            x = np.dot(x, hue_matrix(p).astype(np.float32))
        else:
            raise ValueError("colour operation %r" % (name,))
    return x.astype(np.float32)


def color_affine(ops):
    """The operations of `color_distort_params` composed into one affine map of RGB, in fp64: (M (3,3), b (3,)) with
    out_c = sum_i x_i M[i][c] + b[c].  Each operation is affine (brightness x + d, contrast x * a, saturation
    x * a + gray * (1 - a), hue x . hue_matrix(alpha)), with the float32 parameters `apply_color_ops` uses."""
    M, b = np.eye(3), np.zeros(3)
    for name, p in ops:
        if name == "brightness":
            b = b + float(p)
            continue
        if name == "contrast":
            A = np.eye(3) * float(p)
        elif name == "saturation":
            g = np.array(_GRAY, np.float32).astype(np.float64)
            A = np.eye(3) * float(p) + np.outer(g, np.ones(3)) * float(np.float32(1.0) - p)
        elif name == "hue":
            A = hue_matrix(p).astype(np.float32).astype(np.float64)
        else:
            raise ValueError("colour operation %r" % (name,))
        M, b = M @ A, b @ A
    return M, b


def random_color_distort(src, brightness_delta=32, contrast_low=0.5, contrast_high=1.5, saturation_low=0.5,
                         saturation_high=1.5, hue_delta=18, rng=None):
    """video.py:68-158 on frames in [0, 255]; returns float32.  Draws: those of `color_distort_params` (no draw depends on a
    pixel, so they are all taken first)."""
    ops = color_distort_params(rng, brightness_delta, contrast_low, contrast_high, saturation_low, saturation_high, hue_delta)
    return apply_color_ops(src, ops)


# --------------------------------------------------------------------------------------------
# imresize
# --------------------------------------------------------------------------------------------
def _cubic_w(t, a=-0.75):
    t = np.abs(t)
    return np.where(t <= 1, ((a + 2) * t - (a + 3)) * t * t + 1, np.where(t < 2, ((a * t - 5 * a) * t + 8 * a) * t - 4 * a, 0.0))


def _lanczos_w(t, a=4):
    t = np.asarray(t, dtype=np.float64)
    out = np.where(np.abs(t) < a, np.sinc(t) * np.sinc(t / a), 0.0)
    return out


@functools.lru_cache(maxsize=256)
def _axis_taps(n_in, n_out, interp):
    """Sparse resampling operator of one axis: (idx (n_out, T) int64, w (n_out, T) float64) with
    out[d] = sum_k w[d, k] * in[idx[d, k]]; indices are clipped to the axis (replicated border: OpenCV's convention), so
    one source pixel may appear under several taps.  Cached per (n_in, n_out, interp): the training loader draws from a
    handful of shapes (train_yolov3.py:262-271)."""
    scale = n_in / n_out
    d = np.arange(n_out)
    if interp == 0:                                          # nearest: floor(dst * scale)
        return np.minimum((d * scale).astype(np.int64), n_in - 1)[:, None], np.ones((n_out, 1))
    if interp == 2 and n_out < n_in:                         # area, shrinking: coverage of [d*scale, (d+1)*scale)
        lo, hi = d * scale, np.minimum((d + 1) * scale, n_in)
        T = int(np.ceil(scale)) + 1
        j = np.floor(lo).astype(np.int64)[:, None] + np.arange(T)[None, :]
        w = np.clip(np.minimum(hi[:, None], j + 1) - np.maximum(lo[:, None], j), 0.0, None)
        w /= w.sum(axis=1, keepdims=True)
        return np.clip(j, 0, n_in - 1), w
    f = (d + 0.5) * scale - 0.5
    if interp in (1, 2):                                     # bilinear (area when enlarging = bilinear)
        taps, wf = 2, lambda t: np.maximum(0.0, 1.0 - np.abs(t))
    elif interp == 3:
        taps, wf = 4, _cubic_w
    elif interp == 4:
        taps, wf = 8, _lanczos_w
    else:
        raise ValueError("interp %r" % (interp,))
    j = (np.floor(f).astype(np.int64) - (taps // 2 - 1))[:, None] + np.arange(taps)[None, :]
    w = wf(f[:, None] - j)
    if interp == 4:
        w = w / w.sum(axis=1, keepdims=True)
    return np.clip(j, 0, n_in - 1), w


def _axis_weights(n_in, n_out, interp):
    """Dense (n_out, n_in) form of `_axis_taps` (tests; small shapes)."""
    idx, w = _axis_taps(n_in, n_out, interp)
    W = np.zeros((n_out, n_in))
    np.add.at(W, (np.arange(n_out)[:, None].repeat(idx.shape[1], 1), idx), w)
    return W


def _resample_axis(x, axis, idx, w):
    """out = sum_k w[:, k] * take(x, idx[:, k], axis): T gathers of the whole array, no (n_out, n_in) matrix."""
    shape = [1] * x.ndim
    shape[axis] = idx.shape[0]
    out = None
    for k in range(idx.shape[1]):
        t = np.take(x, idx[:, k], axis=axis) * w[:, k].reshape(shape)
        out = t if out is None else out + t
    return out


def resolve_interp(h0, w0, h, w, interp):
    """interp 9 -> area (2) when both axes shrink, bicubic (3) when both enlarge, bilinear (1) otherwise; every other code
    is returned as it is."""
    if interp == 9:
        return 2 if (h < h0 and w < w0) else (3 if (h > h0 and w > w0) else 1)
    return interp


def resize_tables(h0, w0, h, w, interp=9):
    """The tap tables of an (h0,w0) -> (h,w) imresize in the form the device kernel takes (vd_resize_u8_nchw):
    (interp_used, idx_y (h,Ty) int32, w_y (h,Ty) float32, idx_x (w,Tx) int32, w_x (w,Tx) float32), contiguous - `_axis_taps`
    of each axis after interp 9 is resolved by imresize's rule, cast.  Separable interpolations only (1-4, 9)."""
    interp = resolve_interp(h0, w0, h, w, interp)
    if interp not in (1, 2, 3, 4):
        raise ValueError("resize_tables: interp %r has no tap tables (1 bilinear, 2 area, 3 bicubic, 4 Lanczos, 9)" % (interp,))
    iy, wy = _axis_taps(h0, h, interp)
    ix, wx = _axis_taps(w0, w, interp)
    return (interp, np.ascontiguousarray(iy, dtype=np.int32), np.ascontiguousarray(wy, dtype=np.float32),
            np.ascontiguousarray(ix, dtype=np.int32), np.ascontiguousarray(wx, dtype=np.float32))


def imresize(img, w, h, interp=1, rng=None):
    """(h0,w0,c) image -> (h,w,c).  interp: 0 nearest, 1 bilinear, 2 area, 3 bicubic, 4 Lanczos (8x8), 9 = area when
    shrinking, bicubic when enlarging, bilinear otherwise, 10 = one of 0-4 at random.  uint8 in -> uint8 out (rounded,
    saturated); float in -> float32 out, unclipped."""
    img = np.asarray(img)
    h0, w0 = img.shape[:2]
    if interp == 10:
        interp = int((Rng() if rng is None else rng).np.randint(0, 5))
    interp = resolve_interp(h0, w0, h, w, interp)
    if (h, w) == (h0, w0):
        return img.copy()
    x = img.astype(np.float64)
    if interp == 0:
        ys = np.minimum((np.arange(h) * (h0 / h)).astype(np.int64), h0 - 1)
        xs = np.minimum((np.arange(w) * (w0 / w)).astype(np.int64), w0 - 1)
        out = x[ys][:, xs]
    else:
        # separable: the axis that shrinks more goes first (fewer elements for the second pass)
        ty, tx = _axis_taps(h0, h, interp), _axis_taps(w0, w, interp)
        if w * h0 <= h * w0:
            out = _resample_axis(_resample_axis(x, 1, *tx), 0, *ty)
        else:
            out = _resample_axis(_resample_axis(x, 0, *ty), 1, *tx)
    if img.dtype == np.uint8:
        return np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out.astype(np.float32)


# --------------------------------------------------------------------------------------------
# NV12 (what video decoders hand out) <-> packed RGB
# --------------------------------------------------------------------------------------------
# A frame (H0*3/2, W0) uint8: H0 rows of luma Y, then H0/2 rows of interleaved chroma pairs U V, one pair per 2 x 2 block.
# NV12_MATRICES[(matrix, range)] = (off, gain, ru, rv, gu, gv, bu): the luma offset and, as round(256 * c) of the
# standard's real coefficient c, the luma gain and the chroma matrix row by row - R takes (ru, rv) of (U, V), G (gu, gv),
# B (bu, 0): no standard gives blue a V term.  ONE definition: nv12_to_rgb computes with these integers and the device
# kernel (vd_resize_nv12_nchw) is handed the same seven, so whatever the table says is what both sides compute.
# Real coefficients, with (Kr, Kb) = (0.299, 0.114) for BT.601 and (0.2126, 0.0722) for BT.709, Kg = 1 - Kr - Kb:
#   rv = 2 (1 - Kr), bu = 2 (1 - Kb), gu = -Kb bu / Kg, gv = -Kr rv / Kg, ru = 0; limited range scales the luma gain by
#   255 / 219 (Y in 16 .. 235) and the chroma coefficients by 255 / 224 (U, V in 16 .. 240).
NV12_MATRICES = {
    ("bt601", "limited"): (16, 298, 0, 409, -100, -208, 516),      # 1.164384; 1.596027, -0.391762, -0.812968, 2.017232
    ("bt601", "full"): (0, 256, 0, 359, -88, -183, 454),           # 1;        1.402,    -0.344136, -0.714136, 1.772
    ("bt709", "limited"): (16, 298, 0, 459, -55, -136, 541),       # 1.164384; 1.792741, -0.213249, -0.532909, 2.112402
    ("bt709", "full"): (0, 256, 0, 403, -48, -120, 475),           # 1;        1.5748,   -0.187324, -0.468124, 1.8556
}
_KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def nv12_matrix(matrix="bt601", range="limited"):
    """The seven integers of NV12_MATRICES[(matrix, range)]; an unknown name is refused."""
    if (matrix, range) not in NV12_MATRICES:
        raise ValueError("NV12: unknown matrix / range %r / %r (matrix 'bt601' or 'bt709', range 'limited' or 'full')"
                         % (matrix, range))
    return NV12_MATRICES[(matrix, range)]


def nv12_frame_size(hn, w0):
    """(H0, W0) of NV12 frames stored as (.., hn, w0): hn = H0 * 3 / 2 with H0 and W0 even; anything else is refused."""
    if hn < 3 or hn % 3 or w0 < 2 or w0 % 2:                  # (hn = 3 m gives H0 = 2 m: even)
        raise ValueError("NV12 frames are (.., H0*3/2, W0) with H0 and W0 even (one chroma pair per 2 x 2 block), got "
                         "%d rows (H0 = %s) of W0 = %d" % (hn, hn * 2 // 3 if hn % 3 == 0 else "%d*2/3" % hn, w0))
    return hn * 2 // 3, w0


def _check_rgb_even(h0, w0):
    if h0 < 2 or w0 < 2 or h0 % 2 or w0 % 2:
        raise ValueError("NV12 needs an even frame size (one chroma pair per 2 x 2 block), got H0=%d W0=%d" % (h0, w0))


def nv12_to_rgb(frames, matrix="bt601", range="limited"):
    """(.., H0*3/2, W0) uint8 NV12 -> (.., H0, W0, 3) uint8 RGB in exact integer arithmetic.  Chroma is taken nearest: pixel
    (y, x) uses the pair at (y >> 1, x >> 1).  C = Y - off, D = U - 128, E = V - 128 and per channel
    clip((gain * C + cu * D + cv * E + 128) >> 8, 0, 255) in int32: the shift is an arithmetic (floor) shift of the possibly
    negative sum, and it comes before the clip."""
    off, gain, ru, rv, gu, gv, bu = nv12_matrix(matrix, range)
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim < 2:
        raise ValueError("nv12_to_rgb takes uint8 frames (.., H0*3/2, W0), got %s %r" % (frames.dtype, frames.shape))
    h0, w0 = nv12_frame_size(frames.shape[-2], frames.shape[-1])
    c = frames[..., :h0, :].astype(np.int32) - off
    uv = frames[..., h0:, :].astype(np.int32) - 128
    d = np.repeat(np.repeat(uv[..., 0::2], 2, axis=-2), 2, axis=-1)
    e = np.repeat(np.repeat(uv[..., 1::2], 2, axis=-2), 2, axis=-1)
    y = gain * c + 128
    rgb = np.stack([y + ru * d + rv * e, y + gu * d + gv * e, y + bu * d], axis=-1)
    return np.clip(rgb >> 8, 0, 255).astype(np.uint8)


def rgb_to_nv12(frames, matrix="bt601", range="limited"):
    """The host inverse, for synthetic data and tests: (.., H0, W0, 3) uint8 RGB -> (.., H0*3/2, W0) uint8 NV12 in fp64
    with the standard's real coefficients; the chroma of a 2 x 2 block is the mean of its four pixels' chroma; rounded
    (half to even) and clipped to 0 .. 255."""
    nv12_matrix(matrix, range)
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim < 3 or frames.shape[-1] != 3:
        raise ValueError("rgb_to_nv12 takes uint8 frames (.., H0, W0, 3), got %s %r" % (frames.dtype, frames.shape))
    h0, w0 = frames.shape[-3], frames.shape[-2]
    _check_rgb_even(h0, w0)
    kr, kb = _KR_KB[matrix]
    off, sy, sc = (16.0, 219.0 / 255.0, 224.0 / 255.0) if range == "limited" else (0.0, 1.0, 1.0)
    x = frames.astype(np.float64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    luma = kr * r + (1.0 - kr - kb) * g + kb * b
    lead = frames.shape[:-3]

    def chroma(diff, k):                                     # (B - Y') / (2 (1 - Kb)) and its red twin, 2 x 2 means
        v = 128.0 + sc * diff / (2.0 * (1.0 - k))
        return v.reshape(lead + (h0 // 2, 2, w0 // 2, 2)).mean(axis=(-3, -1))

    out = np.empty(lead + (h0 * 3 // 2, w0), dtype=np.float64)
    out[..., :h0, :] = off + sy * luma
    out[..., h0:, 0::2] = chroma(b - luma, kb)
    out[..., h0:, 1::2] = chroma(r - luma, kr)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def identity_tables(h, w):
    """Tap tables, in `resize_tables`' form, of a frame already at its target size: one tap of weight 1 per axis."""
    return (np.arange(h, dtype=np.int32).reshape(h, 1), np.ones((h, 1), np.float32),
            np.arange(w, dtype=np.int32).reshape(w, 1), np.ones((w, 1), np.float32))
