"""Loop-form oracles of viddet_amd/motion.py: plain Python loops over Python ints, written from the definition's
words and sharing no code with it."""
import numpy as np


def signature_oracle(frames, cell, fmt):
    frames = np.asarray(frames)
    if fmt == "nv12":
        F, rows, W0 = frames.shape
        H0 = rows * 2 // 3
    else:
        F, H0, W0, _ = frames.shape
    Gh, Gw = H0 // cell, W0 // cell
    out = np.zeros((F, Gh, Gw), np.uint16)
    for f in range(F):
        for gy in range(Gh):
            for gx in range(Gw):
                s = 0
                for y in range(gy * cell, gy * cell + cell):
                    for x in range(gx * cell, gx * cell + cell):
                        if fmt == "nv12":
                            s += int(frames[f, y, x])
                        else:
                            r, g, b = (int(v) for v in frames[f, y, x])
                            s += (77 * r + 150 * g + 29 * b + 128) >> 8
                out[f, gy, gx] = s
    return out


def match_oracle(sig, clip_start=None, radius=8, gate=0.75, cell=4):
    sig = [[[int(v) for v in row] for row in frame] for frame in np.asarray(sig)]
    F, Gh, Gw = len(sig), len(sig[0]), len(sig[0][0])
    R = radius
    gq = int(np.float32(gate) * np.float32(256))
    motion = np.zeros((F, 2), np.int32)
    sad = np.zeros((F, 2), np.int64)
    cs = [0, F] if clip_start is None else [int(v) for v in clip_start]
    first = set(cs[:-1])
    for t in range(F):
        if t in first:
            continue
        best = None
        zero = None
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                s = 0
                for gy in range(R, Gh - R):
                    cur, prev = sig[t][gy], sig[t - 1][gy - dy]
                    for gx in range(R, Gw - R):
                        s += abs(cur[gx] - prev[gx - dx])
                key = (s, dx * dx + dy * dy, dy, dx)
                if best is None or key < best:
                    best = key
                if dx == 0 and dy == 0:
                    zero = s
        sad[t] = best[0], zero
        if best[0] * 256 <= zero * gq:
            motion[t] = best[3] * cell, best[2] * cell
    return motion, sad


def shift_oracle(mask, boxes, motion, clip_start, sx, sy, sign):
    """stabilise (sign -1) / restore (+1) row by row, the running sum in Python ints wrapped to int32"""
    boxes = np.asarray(boxes, np.float32)
    out = boxes.copy()
    F, N = boxes.shape[:2]
    cs = [0, F] if clip_start is None else [int(v) for v in clip_start]
    f32 = np.float32
    for a, b in zip(cs[:-1], cs[1:]):
        cx = cy = 0
        for t in range(a, b):
            cx = (cx + int(motion[t][0]) + 2 ** 31) % 2 ** 32 - 2 ** 31
            cy = (cy + int(motion[t][1]) + 2 ** 31) % 2 ** 32 - 2 ** 31
            ox, oy = f32(cx) * f32(sx), f32(cy) * f32(sy)
            for i in range(N):
                if mask[t][i]:
                    x1, y1, x2, y2 = boxes[t, i]
                    out[t, i] = (x1 + ox, y1 + oy, x2 + ox, y2 + oy) if sign > 0 else (x1 - ox, y1 - oy, x2 - ox, y2 - oy)
    return out
