"""NV12 -> RGB restated independently of viddet_amd/video.py nv12_to_rgb: explicit per-pixel loops in Python ints (unbounded,
`>>` on a negative int floors, as the arithmetic shift of an int32 does).  Only the seven integers come from the package."""
import numpy as np


def nv12_to_rgb_loops(frame, coef):
    """frame (H0*3/2, W0) uint8, coef = (off, gain, ru, rv, gu, gv, bu) -> (H0, W0, 3) uint8"""
    off, gain, ru, rv, gu, gv, bu = (int(c) for c in coef)
    hn, w0 = frame.shape
    h0 = hn * 2 // 3
    assert h0 * 3 == hn * 2 and h0 % 2 == 0 and w0 % 2 == 0
    px = frame.tolist()
    out = np.zeros((h0, w0, 3), dtype=np.uint8)
    for y in range(h0):
        for x in range(w0):
            c = px[y][x] - off
            d = px[h0 + (y >> 1)][(x >> 1) * 2] - 128               # the pair of the pixel's 2 x 2 block: U then V
            e = px[h0 + (y >> 1)][(x >> 1) * 2 + 1] - 128
            for ch, (cu, cv) in enumerate(((ru, rv), (gu, gv), (bu, 0))):
                v = (gain * c + cu * d + cv * e + 128) >> 8         # shift first (floor) ...
                out[y, x, ch] = min(max(v, 0), 255)                 # ... then clip
    return out
