"""Detections, tracks and ground truth drawn onto video frames: the definition.

`overlay_host` is normative; `ops.overlay` (vd_overlay.hip) equals it bit for bit.  The reference draws with OpenCV
(detect_yolo3.py visualise_predictions, utils/image.py cv_plot_bbox); OpenCV is no dependency of this project, so the picture
is defined here, in NumPy.  Two float32 steps - the scaling of a box to source pixels and the two decimals of a score - are
followed by integer arithmetic alone, so the result is exact.

The picture of a frame, bottom to top: ground truth (green rings with a tag of the class name), trails, rings, tags.  Inside a
layer the lower row index (the higher score) is on top.  A pixel takes the colour of the topmost primitive covering it and is
otherwise untouched.  The rules, one by one, are the functions below: `valid_rows`, `pixel_boxes`, `on_ring`, `tag_box`,
`glyph_pixel`, `label_text`, `on_segment`, `on_square`; `overlay_records` holds the trail's vertices.

Two steps, as the device takes them: `overlay_records` turns every (frame, row) and every ground-truth row into one fixed-size
record (REC_DTYPE, 128 bytes: the pixel box, the tag box, its text and colours, the trail's vertices), `paint_records` resolves
every pixel against the records top layer first.
"""
import numpy as np

from .video import nv12_frame_size, nv12_matrix, rgb_to_nv12

MAX_ROWS = 128           # rows and ground-truth rows per frame (vd_overlay.hip)
MAX_SIZE = 8192          # H0, W0
MAX_TRAIL = 16
MAX_TEXT = 32
MAX_NAME = 15
COL_GT, COL_BLACK, COL_WHITE = 256, 257, 258     # palette words behind the 256 colours: ground truth, the two glyph colours
PALETTE_WORDS = 259

REC_DTYPE = np.dtype([("box", "<i2", (4,)),      # px0, py0, px1, py1 (inclusive)
                      ("tag", "<i2", (4,)),      # tx0, ty0, tx1, ty1 (inclusive, not cut at the frame's edges)
                      ("col", "<u2"),            # palette word of the row's colour
                      ("gcol", "<u2"),           # ... of its glyphs: COL_BLACK or COL_WHITE
                      ("valid", "u1"),
                      ("len", "u1"),             # characters of the text
                      ("nv", "<i2"),             # vertices of the trail
                      ("text", "u1", (MAX_TEXT,)),
                      ("vx", "<i2", (MAX_TRAIL + 1, 2)),     # (x, y): the row's own centre, then the earlier frames' in order
                      ("pad", "<i4")])
assert REC_DTYPE.itemsize == 128

# The 5x7 font of ASCII 32..126, written for this project: seven rows per glyph, top first, two hex digits each; bit 4 is the
# left column.
_FONT_HEX = (
    "00000000000000" "04040404040004" "0a0a0a00000000" "0a0a1f0a1f0a0a" "040f140e051e04" "18190204081303" "0c12140815120d"
    "04040800000000" "02040808080402" "08040202020408" "0004150e150400" "0004041f040400" "000000000c0408" "0000001f000000"
    "00000000000c0c" "00010204081000" "0e11131519110e" "040c040404040e" "0e11010204081f" "1f02040201110e" "02060a121f0202"
    "1f101e0101110e" "0608101e11110e" "1f010204080808" "0e11110e11110e" "0e11110f01020c" "000c0c000c0c00" "000c0c000c0408"
    "02040810080402" "00001f001f0000" "08040201020408" "0e110102040004" "0e11010d15150e" "0e1111111f1111" "1e11111e11111e"
    "0e11101010110e" "1c12111111121c" "1f10101e10101f" "1f10101e101010" "0e11101711110f" "1111111f111111" "0e04040404040e"
    "0702020202120c" "11121418141211" "1010101010101f" "111b1515111111" "11111915131111" "0e11111111110e" "1e11111e101010"
    "0e11111115120d" "1e11111e141211" "0f10100e01011e" "1f040404040404" "1111111111110e" "11111111110a04" "1111111515150a"
    "11110a040a1111" "1111110a040404" "1f01020408101f" "0e08080808080e" "00100804020100" "0e02020202020e" "040a1100000000"
    "0000000000001f" "08040200000000" "00000e010f110f" "1010161911111e" "00000e1010110e" "01010d1311110f"
    "00000e111f100e" "0609081c080808" "000f11110f010e" "10101619111111" "04000c0404040e" "0200060202120c" "10101214181412"
    "0c04040404040e" "00001a15151111" "00001619111111" "00000e1111110e" "00001e111e1010" "00000d130f0101" "00001619101010"
    "00000e100e011e" "08081c08080906" "0000111111130d" "00001111110a04" "0000111115150a" "0000110a040a11"
    "000011110f010e" "00001f0204081f" "02040408040402" "04040404040404" "08040402040408" "00000815020000")
FONT_5X7 = np.frombuffer(bytes.fromhex(_FONT_HEX), dtype=np.uint8).reshape(95, 7).copy()
FONT_5X7.setflags(write=False)


def _label_colour_map():
    pal = np.zeros((256, 3), np.uint8)
    for i in range(256):
        c, rgb = i % 255 + 1, [0, 0, 0]
        for j in range(8):
            for ch in range(3):
                rgb[ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
        pal[i] = rgb
    pal.setflags(write=False)
    return pal


_PALETTE = _label_colour_map()


def default_palette():
    """(256,3) uint8 RGB, a fixed table: entry i is colour i % 255 + 1 of the bit-spreading label colour map (the bits of
    the index go to the three channels in turn, most significant first), so neighbouring indices differ strongly and none is
    black."""
    return _PALETTE.copy()


def check_params(net_size=None, thresh=0.5, thickness=2, scale=1, trail=8, color_by=None, class_names=None, palette=None,
                 fmt="rgb", matrix="bt601", range="limited", tracked=False, who="overlay"):
    """The parameters of the table in DESIGN.md 41, checked and filled in -> a dict.  color_by None: 'track' with a track
    table, else 'class'."""
    def integer(name, v, lo, hi):
        if isinstance(v, bool) or not hasattr(v, "__index__") or not lo <= int(v) <= hi:
            raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (who, name, lo, hi, v))
        return int(v)

    t = integer("thickness", thickness, 1, 8)
    s = integer("scale", scale, 1, 4)
    L = integer("trail", trail, 0, MAX_TRAIL)
    thresh = float(thresh)
    if thresh != thresh:
        raise ValueError("%s: thresh must be a number, got NaN" % who)
    if color_by is None:
        color_by = "track" if tracked else "class"
    if color_by not in ("class", "track"):
        raise ValueError("%s: color_by %r is neither 'class' nor 'track'" % (who, color_by))
    if fmt not in ("rgb", "nv12"):
        raise ValueError("%s: fmt %r is neither 'rgb' nor 'nv12'" % (who, fmt))
    nv12_matrix(matrix, range)
    if class_names is not None:
        class_names = tuple(class_names)
        for n in class_names:
            if not isinstance(n, str) or len(n) > MAX_NAME or any(not 32 <= ord(ch) <= 126 for ch in n):
                raise ValueError("%s: class_names are at most %d printable ASCII characters each, got %r" % (who, MAX_NAME, n))
    if palette is None:
        palette = _PALETTE
    else:
        palette = np.asarray(palette)
        if palette.dtype != np.uint8 or palette.shape != (256, 3):
            raise ValueError("%s: palette must be (256,3) uint8, got %s %r" % (who, palette.dtype, palette.shape))
    if net_size is not None:
        hn, wn = (integer("net_size", v, 1, 1 << 20) for v in net_size)
        net_size = (hn, wn)
    return dict(net_size=net_size, thresh=thresh, thickness=t, scale=s, trail=L, color_by=color_by, class_names=class_names,
                palette=palette, fmt=fmt, matrix=matrix, range=range)


def frame_size(shape, fmt, who="overlay"):
    """(F, H0, W0) of frames (F,H0,W0,3) RGB or (F,H0*3/2,W0) NV12; sizes beyond MAX_SIZE are refused."""
    if fmt == "nv12":
        if len(shape) != 3:
            raise ValueError("%s: NV12 frames are (F,H0*3/2,W0) uint8, got %r" % (who, tuple(shape)))
        try:
            h0, w0 = nv12_frame_size(shape[1], shape[2])
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e)) from None
    else:
        if len(shape) != 4 or shape[3] != 3:
            raise ValueError("%s: RGB frames are (F,H0,W0,3) uint8, got %r" % (who, tuple(shape)))
        h0, w0 = shape[1], shape[2]
    if not (1 <= h0 <= MAX_SIZE and 1 <= w0 <= MAX_SIZE):
        raise ValueError("%s: H0=%d W0=%d, frames of 1 .. %d pixels a side are taken" % (who, h0, w0, MAX_SIZE))
    return int(shape[0]), int(h0), int(w0)


# ------------------------------------------------------------------------------------------------ the rules, one by one
def class_ints(ids):
    """float class ids -> int64: truncated, 2^31 - 1 from 2^31 on; -1 where the id is not >= 0 (NaN included)"""
    ids = np.asarray(ids, np.float32)
    ok = ids >= 0
    big = ids >= np.float32(2147483648.0)
    with np.errstate(invalid="ignore"):
        c = np.where(ok & ~big, ids, 0).astype(np.int64)
    return np.where(ok, np.where(big, 0x7fffffff, c), -1)


def valid_rows(ids, scores, bboxes, thresh):
    """(F,N) bool: id >= 0, score >= thresh as a float32 comparison, four finite box values, x1 <= x2 and y1 <= y2"""
    ids, scores, b = np.asarray(ids, np.float32), np.asarray(scores, np.float32), np.asarray(bboxes, np.float32)
    with np.errstate(invalid="ignore"):
        return ((ids >= 0) & (scores >= np.float32(thresh)) & np.isfinite(b).all(-1) & (b[..., 0] <= b[..., 2])
                & (b[..., 1] <= b[..., 3]))


def pixel_boxes(bboxes, net_size, size):
    """(..,4) float boxes in net_size = (Hn, Wn) coordinates -> (..,4) int64 px0, py0, px1, py1 in a frame of size = (H0, W0):
    sx = float32(W0) / float32(Wn), then int(clamp(floor(v * sx), 0, W0 - 1)), every step one float32 operation.  Boxes that
    are not finite give rubbish (no row that holds one is valid)."""
    b = np.asarray(bboxes, np.float32)
    (hn, wn), (h0, w0) = net_size, size
    sx = np.float32(w0) / np.float32(wn)
    sy = np.float32(h0) / np.float32(hn)
    out = np.zeros(b.shape, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (s, hi) in enumerate(((sx, w0 - 1), (sy, h0 - 1), (sx, w0 - 1), (sy, h0 - 1))):
            v = np.floor(b[..., k] * s)
            v = np.minimum(np.maximum(v, np.float32(0)), np.float32(hi))
            out[..., k] = np.where(np.isfinite(v), v, 0).astype(np.int64)
    return out


def on_ring(X, Y, box, t):
    """the outline that grows inward: inside the box and within t pixels of one of its edges"""
    px0, py0, px1, py1 = (int(v) for v in box)
    inside = (X >= px0) & (X <= px1) & (Y >= py0) & (Y <= py1)
    return inside & ((X < px0 + t) | (X > px1 - t) | (Y < py0 + t) | (Y > py1 - t))


def on_segment(X, Y, a, b, t):
    """with d = b - a and v = p - a: 0 <= v.d <= d.d and 4 (v x d)^2 <= t^2 d.d, in int64; a zero-length segment holds nothing"""
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    dx, dy = bx - ax, by - ay
    dd = dx * dx + dy * dy
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    if dd == 0:
        return np.zeros(np.broadcast(X, Y).shape, bool)
    vx, vy = X - ax, Y - ay
    dot = vx * dx + vy * dy
    cr = vx * dy - vy * dx
    return (dot >= 0) & (dot <= dd) & (4 * cr * cr <= t * t * dd)


def on_square(X, Y, c, t):
    """the t x t square of a vertex: its top-left corner is (cx - (t >> 1), cy - (t >> 1))"""
    x0, y0 = int(c[0]) - (t >> 1), int(c[1]) - (t >> 1)
    return (X >= x0) & (X < x0 + t) & (Y >= y0) & (Y < y0 + t)


def tag_box(px0, py0, length, s):
    """(tx0, ty0, tx1, ty1), inclusive and not cut: 6 s length + s wide and 9 s high, its left edge px0, its top py0 - 9 s
    where that is >= 0, else py0"""
    ty0 = py0 - 9 * s if py0 - 9 * s >= 0 else py0
    return int(px0), int(ty0), int(px0) + 6 * s * length + s - 1, int(ty0) + 9 * s - 1


def in_tag(X, Y, tag):
    return (X >= tag[0]) & (X <= tag[2]) & (Y >= tag[1]) & (Y <= tag[3])


def glyph_pixel(X, Y, tag, text, s):
    """inside a tag: is the pixel one of a glyph's?  Character k's cell starts at (tx0 + s + 6 s k, ty0 + s); the glyph fills
    its left 5 s x 7 s, every font pixel an s x s block.  A byte outside 32..126 has no glyph."""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    rx, ry = X - (tag[0] + s), Y - (tag[1] + s)
    rx, ry = np.broadcast_arrays(rx, ry)
    text = np.frombuffer(bytes(text), np.uint8)
    if len(text) == 0:
        return np.zeros(rx.shape, bool)
    ok = (rx >= 0) & (ry >= 0)
    k = np.where(ok, rx, 0) // (6 * s)
    gx = (np.where(ok, rx, 0) % (6 * s)) // s
    gy = np.where(ok, ry, 0) // s
    ok &= (k < len(text)) & (gx < 5) & (gy < 7)
    ch = text[np.minimum(k, len(text) - 1)].astype(np.int64) - 32
    ok &= (ch >= 0) & (ch < 95)
    rows = FONT_5X7[np.clip(ch, 0, 94), np.clip(gy, 0, 6)].astype(np.int64)
    return ok & (((rows >> (4 - np.clip(gx, 0, 4))) & 1) == 1)


def score_hundredths(score):
    """q of the tag: min(999, int(score * 100.0f + 0.5f)), two float32 operations; 0 where that is not positive"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.float32(score) * np.float32(100.0) + np.float32(0.5)
    if v >= np.float32(999.0):
        return 999
    return int(v) if v > 0 else 0


def label_text(cls, score=None, track=None, class_names=None):
    """The text of a tag, as bytes: "#<track id> " where the row is tracked (track >= 0), the class name (the decimal class id
    without a table, or beyond it), and with a score a space and its two decimals q / 100 . q % 100; cut to 32 characters.
    score None: the class name alone (ground truth)."""
    cls = int(cls)
    name = class_names[cls] if class_names is not None and 0 <= cls < len(class_names) else "%d" % cls
    text = ("#%d " % int(track) if track is not None and int(track) >= 0 else "") + name
    if score is not None:
        q = score_hundredths(score)
        text += " %d.%02d" % (q // 100, q % 100)
    return text.encode("ascii")[:MAX_TEXT]


def frame_clip_start(clip_start, F):
    """(F,) the first frame a trail of frame f may reach back to: the largest offset of clip_start that is <= f, else 0"""
    t0 = np.zeros(F, np.int64)
    if clip_start is not None:
        cs = np.asarray(clip_start, np.int64).reshape(-1)
        for f in range(F):
            le = cs[(cs <= f) & (cs >= 0)]
            t0[f] = le.max() if le.size else 0
    return t0


def glyph_colour(rgb):
    """black glyphs on a light colour, white ones on a dark one: 299 R + 587 G + 114 B >= 128000 is light"""
    r, g, b = (int(v) for v in rgb)
    return COL_BLACK if 299 * r + 587 * g + 114 * b >= 128000 else COL_WHITE


def palette_rgb(palette):
    """(259,3) uint8: the 256 colours, then ground truth's green, black and white"""
    return np.concatenate([np.asarray(palette, np.uint8), np.array([[0, 255, 0], [0, 0, 0], [255, 255, 255]], np.uint8)])


def palette_triples(palette, fmt="rgb", matrix="bt601", range="limited"):
    """(259,3) uint8, what a painted pixel receives: RGB, or for NV12 (Y, U, V) - video.rgb_to_nv12 of a constant 2 x 2 block
    per entry, once, so that painting does no colour arithmetic"""
    rgb = palette_rgb(palette)
    if fmt != "nv12":
        return rgb
    blocks = np.broadcast_to(rgb[:, None, None, :], (PALETTE_WORDS, 2, 2, 3))
    nv = rgb_to_nv12(np.ascontiguousarray(blocks), matrix, range)                     # (259, 3, 2)
    return np.stack([nv[:, 0, 0], nv[:, 2, 0], nv[:, 2, 1]], axis=-1)


def palette_words(palette, fmt="rgb", matrix="bt601", range="limited"):
    """(259,) uint32, the table the device takes: c0 | c1 << 8 | c2 << 16 of palette_triples, and in bit 24 whether glyphs on
    this colour are white"""
    tri = palette_triples(palette, fmt, matrix, range).astype(np.uint32)
    white = np.array([glyph_colour(c) == COL_WHITE for c in palette_rgb(palette)], np.uint32)
    return (tri[:, 0] | tri[:, 1] << 8 | tri[:, 2] << 16 | white << 24).astype(np.uint32)


def font_table():
    """(95,8) uint8, the font as the device takes it: FONT_5X7's seven row bytes and a pad byte per glyph"""
    return np.ascontiguousarray(np.pad(FONT_5X7, ((0, 0), (0, 1))))


def names_table(class_names):
    """(C,16) uint8, NUL padded: the class-name table the device takes"""
    tab = np.zeros((len(class_names), MAX_NAME + 1), np.uint8)
    for i, n in enumerate(class_names):
        tab[i, :len(n)] = np.frombuffer(n.encode("ascii"), np.uint8)
    return tab


# ------------------------------------------------------------------------------------------------ records, then pixels
def _rows2d(a, F, dtype):
    a = np.asarray(a)
    if a.ndim == 3 and a.shape[-1] == 1:
        a = a[..., 0]
    if a.ndim != 2 or a.shape[0] != F:
        raise ValueError("overlay: ids, scores and track are (F,N[,1]) with F=%d, got %r" % (F, a.shape))
    return a.astype(dtype)


def overlay_records(ids, scores, bboxes, track=None, gt=None, clip_start=None, size=None, **params):
    """The first step: (rec (F,N), rec_gt (F,G)) of REC_DTYPE for frames of size = (H0, W0); G = 0 without gt.  An invalid
    row's record is all zero; so are the bytes of a record that its row does not use."""
    bboxes = np.asarray(bboxes, np.float32)
    if bboxes.ndim != 3 or bboxes.shape[-1] != 4:
        raise ValueError("overlay: bboxes must be (F,N,4), got %r" % (bboxes.shape,))
    F, N = bboxes.shape[:2]
    p = check_params(tracked=track is not None, **params)
    h0, w0 = size
    net = p["net_size"] or (h0, w0)
    t, s, L = p["thickness"], p["scale"], p["trail"]
    ids, scores = _rows2d(ids, F, np.float32), _rows2d(scores, F, np.float32)
    trk = None if track is None else _rows2d(track, F, np.int64)
    if N > MAX_ROWS:
        raise ValueError("overlay: N=%d rows per frame, at most %d are taken" % (N, MAX_ROWS))
    pal = palette_rgb(p["palette"])
    valid = valid_rows(ids, scores, bboxes, p["thresh"])
    cls = class_ints(ids)
    pb = pixel_boxes(bboxes, net, (h0, w0))
    cx, cy = (pb[..., 0] + pb[..., 2]) >> 1, (pb[..., 1] + pb[..., 3]) >> 1
    t0 = frame_clip_start(clip_start, F)
    rec = np.zeros((F, N), REC_DTYPE)
    for f in range(F):
        for i in range(N):
            if not valid[f, i]:
                continue
            r = rec[f, i]
            u = int(trk[f, i]) if trk is not None else -1
            text = label_text(cls[f, i], scores[f, i], u, p["class_names"])
            col = (u & 255) if (p["color_by"] == "track" and u >= 0) else int(cls[f, i]) & 255
            r["box"] = pb[f, i]
            r["tag"] = tag_box(pb[f, i, 0], pb[f, i, 1], len(text), s)
            r["col"], r["gcol"], r["valid"], r["len"] = col, glyph_colour(pal[col]), 1, len(text)
            r["text"][:len(text)] = np.frombuffer(text, np.uint8)
            if u >= 0:                                            # the trail: the row's own centre, then the earlier frames'
                vx = [(cx[f, i], cy[f, i])]
                for d in range(1, L + 1):
                    g = f - d
                    if g < t0[f]:
                        break
                    hit = np.nonzero(valid[g] & (trk[g] == u))[0]
                    if hit.size:
                        vx.append((cx[g, hit[0]], cy[g, hit[0]]))
                r["nv"] = len(vx)
                r["vx"][:len(vx)] = np.array(vx)
    if gt is None:
        return rec, np.zeros((F, 0), REC_DTYPE)
    gt = np.asarray(gt, np.float32)
    if gt.ndim != 3 or gt.shape[0] != F or gt.shape[2] < 5:
        raise ValueError("overlay: gt must be (F,G,>=5) rows x1, y1, x2, y2, class with F=%d, got %r" % (F, gt.shape))
    G = gt.shape[1]
    if G > MAX_ROWS:
        raise ValueError("overlay: G=%d ground-truth rows per frame, at most %d are taken" % (G, MAX_ROWS))
    gvalid = valid_rows(gt[..., 4], np.zeros((F, G), np.float32), gt[..., :4], 0.0)
    gcls = class_ints(gt[..., 4])
    gpb = pixel_boxes(gt[..., :4], net, (h0, w0))
    rec_gt = np.zeros((F, G), REC_DTYPE)
    for f in range(F):
        for g in range(G):
            if not gvalid[f, g]:
                continue
            r = rec_gt[f, g]
            text = label_text(gcls[f, g], None, None, p["class_names"])
            r["box"] = gpb[f, g]
            r["tag"] = tag_box(gpb[f, g, 0], gpb[f, g, 1], len(text), s)
            r["col"], r["gcol"], r["valid"], r["len"] = COL_GT, glyph_colour(pal[COL_GT]), 1, len(text)
            r["text"][:len(text)] = np.frombuffer(text, np.uint8)
    return rec, rec_gt


def _window(x0, y0, x1, y1, h0, w0):
    """the part of an inclusive rectangle inside the frame, as index arrays (Y column, X row), or None"""
    x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), w0 - 1), min(int(y1), h0 - 1)
    if x0 > x1 or y0 > y1:
        return None
    return np.arange(y0, y1 + 1)[:, None], np.arange(x0, x1 + 1)[None, :]


def resolve_records(rec, rec_gt, size, thickness=2, scale=1):
    """One frame's records -> (H0,W0) int16: the palette word of the topmost primitive covering each pixel, -1 where none
    does.  Top layer first; a pixel that has its colour is never looked at again."""
    h0, w0 = size
    t, s = thickness, scale
    idx = np.full((h0, w0), -1, np.int16)

    def put(win, mask, colour):
        Y, X = win
        sub = idx[Y, X]
        m = mask & (sub < 0)
        idx[Y, X] = np.where(m, colour, sub)

    def put_tag(r):
        win = _window(*r["tag"], h0, w0)
        if win is not None:
            Y, X = win
            glyph = glyph_pixel(X, Y, r["tag"], bytes(r["text"][:r["len"]]), s)
            put(win, np.ones(glyph.shape, bool), np.where(glyph, r["gcol"], r["col"]).astype(np.int16))

    def put_ring(r):
        win = _window(*r["box"], h0, w0)
        Y, X = win
        put(win, on_ring(X, Y, r["box"], t), np.int16(r["col"]))

    rows = [r for r in rec if r["valid"]]
    for r in rows:
        put_tag(r)
    for r in rows:
        put_ring(r)
    for r in rows:
        nv = int(r["nv"])
        if nv == 0:
            continue
        v = r["vx"][:nv].astype(np.int64)
        win = _window(v[:, 0].min() - t, v[:, 1].min() - t, v[:, 0].max() + t, v[:, 1].max() + t, h0, w0)
        if win is None:
            continue
        Y, X = win
        mask = np.zeros(np.broadcast(X, Y).shape, bool)
        for k in range(nv):
            mask |= on_square(X, Y, v[k], t)
            if k:
                mask |= on_segment(X, Y, v[k - 1], v[k], t)
        put(win, mask, np.int16(r["col"]))
    for r in rec_gt:
        if r["valid"]:
            put_tag(r)
            put_ring(r)
    return idx


def paint_records(frames, rec, rec_gt, **params):
    """The second step: the frames painted from their records -> (out, painted)."""
    p = check_params(**params)
    frames = np.asarray(frames)
    if frames.dtype != np.uint8:
        raise ValueError("overlay: frames must be uint8, got %s" % frames.dtype)
    F, h0, w0 = frame_size(frames.shape, p["fmt"])
    tri = palette_triples(p["palette"], p["fmt"], p["matrix"], p["range"])
    out = frames.copy()
    painted = np.zeros(F, np.int32)
    for f in range(F):
        idx = resolve_records(rec[f], rec_gt[f], (h0, w0), p["thickness"], p["scale"])
        hit = idx >= 0
        painted[f] = hit.sum()
        if p["fmt"] == "nv12":
            out[f, :h0][hit] = tri[idx[hit], 0]
            chit, cidx = hit[0::2, 0::2], idx[0::2, 0::2]
            uv = out[f, h0:].reshape(h0 // 2, w0 // 2, 2)         # a view: chroma pair (cy, cx) follows luma pixel (2cy, 2cx)
            uv[chit] = tri[cidx[chit], 1:]
        else:
            out[f][hit] = tri[idx[hit]]
    return out, painted


def overlay_host(frames, ids, scores, bboxes, track=None, gt=None, clip_start=None, **params):
    """The definition.  frames (F,H0,W0,3) uint8 RGB, or with fmt='nv12' (F,H0*3/2,W0); ids, scores (F,N[,1]) and bboxes
    (F,N,4) in net_size = (Hn, Wn) coordinates (the frames' own size where it is not given); track (F,N) integer, -1 an
    untracked row; gt (F,G,>=5) rows x1, y1, x2, y2, class, a class < 0 padding; clip_start: V+1 ascending frame offsets, a
    trail stays inside its clip.  Returns (out, painted): the painted frames, and per frame the number of pixels that took a
    primitive's colour (for NV12: luma pixels)."""
    frames = np.asarray(frames)
    fmt = params.get("fmt", "rgb")
    F, h0, w0 = frame_size(frames.shape, fmt)
    if np.asarray(bboxes).shape[0] != F:
        raise ValueError("overlay: %d frames but rows of %d" % (F, np.asarray(bboxes).shape[0]))
    rec, rec_gt = overlay_records(ids, scores, bboxes, track, gt, clip_start, size=(h0, w0), **params)
    params = dict(params)
    params.pop("tracked", None)
    return paint_records(frames, rec, rec_gt, **params)


def parse_option(overlay, who="detect_video"):
    """detect_video's `overlay`: None -> None; True -> {}; a dict -> a copy, its keys checked"""
    if overlay is None or overlay is False:
        return None
    if overlay is True:
        return {}
    if not isinstance(overlay, dict):
        raise ValueError("%s: overlay must be None, True or a dict of its parameters, got %r" % (who, overlay))
    known = {"thresh", "thickness", "scale", "trail", "color_by", "class_names", "palette", "inplace", "gt"}
    bad = sorted(set(overlay) - known)
    if bad:
        raise ValueError("%s: overlay does not take %s (it takes %s)" % (who, ", ".join(bad), ", ".join(sorted(known))))
    check_params(**{k: v for k, v in overlay.items() if k not in ("inplace", "gt")}, who=who + ": overlay")
    return dict(overlay)
