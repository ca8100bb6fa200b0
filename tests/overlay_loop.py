"""The overlay written a second time, from the rules of DESIGN.md 41, the other way round: a per-primitive painter in plain
Python loops that draws bottom to top and overwrites - ground truth, trails, rings, tags, inside a layer the highest row first -
where viddet_amd.overlay resolves every pixel top layer first.  It shares no code with the definition but the font, the
palette and video.rgb_to_nv12 (which are data, and another module's function)."""
import math

import numpy as np

from viddet_amd.overlay import FONT_5X7, default_palette
from viddet_amd.video import rgb_to_nv12

f32 = np.float32
GREEN, BLACK, WHITE = (0, 255, 0), (0, 0, 0), (255, 255, 255)


def _scaled(v, src, dst, hi):
    with np.errstate(over="ignore"):
        p = float(f32(v) * (f32(dst) / f32(src)))
    if math.isinf(p):
        return hi if p > 0 else 0
    return int(min(max(math.floor(p), 0), hi))


def _text(cls, score, track, names):
    name = names[cls] if names is not None and cls < len(names) else str(cls)
    out = ("#%d " % track if track >= 0 else "") + name
    if score is not None:
        q = min(999, max(0, int(f32(f32(score) * f32(100.0)) + f32(0.5))))
        out += " " + str(q // 100) + "." + str(q % 100).rjust(2, "0")
    return out[:32]


def _ink(rgb):
    return BLACK if 299 * rgb[0] + 587 * rgb[1] + 114 * rgb[2] >= 128000 else WHITE


class _Canvas:
    def __init__(self, h, w):
        self.h, self.w = h, w
        self.colour = {}                                          # (x, y) -> rgb, overwritten by whatever is drawn later

    def dot(self, x, y, rgb):
        if 0 <= x < self.w and 0 <= y < self.h:
            self.colour[(x, y)] = tuple(int(c) for c in rgb)

    def ring(self, box, t, rgb):
        x0, y0, x1, y1 = box
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                if min(x - x0, x1 - x, y - y0, y1 - y) < t:
                    self.dot(x, y, rgb)

    def tag(self, box, text, s, rgb):
        x0, y0 = box[0], box[1]
        top = y0 - 9 * s if y0 - 9 * s >= 0 else y0
        for y in range(top, top + 9 * s):
            for x in range(x0, x0 + 6 * s * len(text) + s):
                self.dot(x, y, rgb)
        ink = _ink(rgb)
        for k, ch in enumerate(text):
            glyph = FONT_5X7[ord(ch) - 32]
            for gy in range(7):
                for gx in range(5):
                    if (int(glyph[gy]) >> (4 - gx)) & 1:
                        for yy in range(s):
                            for xx in range(s):
                                self.dot(x0 + s + 6 * s * k + gx * s + xx, top + s + gy * s + yy, ink)

    def square(self, c, t, rgb):
        for y in range(c[1] - t // 2, c[1] - t // 2 + t):
            for x in range(c[0] - t // 2, c[0] - t // 2 + t):
                self.dot(x, y, rgb)

    def segment(self, a, b, t, rgb):
        dx, dy = b[0] - a[0], b[1] - a[1]
        dd = dx * dx + dy * dy
        if dd == 0:
            return
        for y in range(min(a[1], b[1]) - t, max(a[1], b[1]) + t + 1):
            for x in range(min(a[0], b[0]) - t, max(a[0], b[0]) + t + 1):
                vx, vy = x - a[0], y - a[1]
                dot, cross = vx * dx + vy * dy, vx * dy - vy * dx
                if 0 <= dot <= dd and 4 * cross * cross <= t * t * dd:          # Python integers: no width to overflow
                    self.dot(x, y, rgb)


def overlay_loop(frames, ids, scores, bboxes, track=None, gt=None, clip_start=None, net_size=None, thresh=0.5, thickness=2,
                 scale=1, trail=8, color_by=None, class_names=None, palette=None, fmt="rgb", matrix="bt601", range_="limited"):
    frames = np.asarray(frames)
    F = frames.shape[0]
    h0, w0 = (frames.shape[1] * 2 // 3, frames.shape[2]) if fmt == "nv12" else frames.shape[1:3]
    hn, wn = net_size or (h0, w0)
    pal = default_palette() if palette is None else palette
    by_track = (color_by or ("track" if track is not None else "class")) == "track"
    ids = np.asarray(ids, f32).reshape(F, -1)
    scores = np.asarray(scores, f32).reshape(F, -1)
    N = ids.shape[1]
    t, s = thickness, scale
    out = frames.copy()
    painted = np.zeros(F, np.int32)
    yuv_of = {}                                                   # a colour's (3,2) NV12 image of a constant 2 x 2 block

    def px(b):
        return (_scaled(b[0], wn, w0, w0 - 1), _scaled(b[1], hn, h0, h0 - 1), _scaled(b[2], wn, w0, w0 - 1),
                _scaled(b[3], hn, h0, h0 - 1))

    def drawn(f, i):
        b = bboxes[f][i]
        return bool(ids[f, i] >= 0 and scores[f, i] >= f32(thresh) and all(math.isfinite(float(v)) for v in b)
                    and b[0] <= b[2] and b[1] <= b[3])

    def centre(f, i):
        b = px(bboxes[f][i])
        return (b[0] + b[2]) // 2, (b[1] + b[3]) // 2

    def clip_first(f):
        return max([int(c) for c in clip_start if 0 <= int(c) <= f] or [0]) if clip_start is not None else 0

    for f in range(F):
        cv = _Canvas(h0, w0)
        if gt is not None:
            for g in reversed(range(len(gt[f]))):
                row = gt[f][g]
                if not (row[4] >= 0 and all(math.isfinite(float(v)) for v in row[:4]) and row[0] <= row[2] and row[1] <= row[3]):
                    continue
                cv.ring(px(row), t, GREEN)
                cv.tag(px(row), _text(int(row[4]), None, -1, class_names), s, GREEN)
        rows = [i for i in range(N) if drawn(f, i)]
        info = {}
        for i in rows:
            u = int(track[f][i]) if track is not None else -1
            c = int(ids[f, i])
            info[i] = (u, c, tuple(int(v) for v in pal[(u if by_track and u >= 0 else c) % 256]))
        for i in reversed(rows):
            u, c, rgb = info[i]
            if u < 0:
                continue
            vs = [centre(f, i)]
            for d in range(1, trail + 1):
                if f - d < clip_first(f):
                    break
                same = [j for j in range(N) if drawn(f - d, j) and int(track[f - d][j]) == u]
                if same:
                    vs.append(centre(f - d, same[0]))
            for a, b in zip(vs, vs[1:]):
                cv.segment(a, b, t, rgb)
            for v in vs:
                cv.square(v, t, rgb)
        for i in reversed(rows):
            cv.ring(px(bboxes[f][i]), t, info[i][2])
        for i in reversed(rows):
            u, c, rgb = info[i]
            cv.tag(px(bboxes[f][i]), _text(c, scores[f, i], u, class_names), s, rgb)
        painted[f] = len(cv.colour)
        for (x, y), rgb in cv.colour.items():
            if fmt == "nv12":
                if rgb not in yuv_of:
                    yuv_of[rgb] = rgb_to_nv12(np.full((2, 2, 3), rgb, np.uint8), matrix, range_)
                yuv = yuv_of[rgb]
                out[f, y, x] = yuv[0, 0]
                if y % 2 == 0 and x % 2 == 0:
                    out[f, h0 + y // 2, x:x + 2] = yuv[2]
            else:
                out[f, y, x] = rgb
    return out, painted
