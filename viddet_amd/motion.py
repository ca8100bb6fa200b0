"""Camera-motion compensation of the clip trackers: the definition.

Every linker of the clip pipeline takes a box's position in the last frame as evidence for its position in this one.  Under a
panning or shaking camera all objects of a frame jump together and that evidence is wrong for all of them.  The translation
of the whole picture between two frames is estimated from the pixels, summed up along the clip, and taken off the boxes: in
that stabilised coordinate frame the trackers run as they are - the Kalman filter and the IoU are translation-covariant - and
what they estimate is put back into image coordinates.  This is the translation-only form of the camera-motion compensation
of BoT-SORT (Aharon et al., "BoT-SORT: Robust Associations Multi-Pedestrian Tracking", 2022), with block matching on a
coarse luma grid in place of its sparse optical flow.

The definitions below are normative: NumPy, integer arithmetic everywhere below the final box shift, so sums may be formed in
any order.  The device entry points vd_motion_sig, vd_motion_match and vd_motion_shift (viddet_amd/csrc/vd_motion.hip;
ops.motion_signature, ops.motion_match, ops.motion_shift) equal them bit for bit.

  luma       RGB (F,H0,W0,3) uint8: y = (77 R + 150 G + 29 B + 128) >> 8.  NV12 (F,H0*3/2,W0): the Y plane's byte; chroma is
             never read.
  signature  (F,Gh,Gw) uint16, Gh = H0 // cell, Gw = W0 // cell: the sum of the luma over every cell x cell block of pixels;
             the pixels right of Gw*cell and below Gh*cell are not read.  cell is 2, 4, 8 or 16: at most 16*16*255 = 65280.
  match      for every frame t that is not the first of its clip and every displacement (dx,dy) in [-R, R]^2, R = radius:
                 SAD(dx,dy) = sum over gy in [R, Gh-R), gx in [R, Gw-R) of | sig[t][gy,gx] - sig[t-1][gy-dy, gx-dx] |
             The winner is the least key (SAD, dx*dx + dy*dy, dy, dx); sad[t] = (SAD(winner), SAD(0,0)).  It is accepted iff
                 SAD(winner) * 256 <= SAD(0,0) * int(float32(gate) * float32(256))
             and then motion[t] = (dx*cell, dy*cell) in source pixels, else (0,0).  The first frame of a clip, and a frame
             that no clip covers, gets zeros in both.  Content at pixel p of frame t-1 appears at p + motion[t] in frame t: a
             camera that steps to the right gives a negative x.
  stabilise  C[t], the int32 running sum of motion inside the clip; every row whose id is >= 0 (a NaN is not) has
                 off = (float32(C[t].x) * sx, float32(C[t].y) * sy)
             subtracted from its corners, x1 - off.x, y1 - off.y, x2 - off.x, y2 - off.y: one float32 multiply and one
             float32 subtract each.  The other rows keep their bits.  sx = float32(W) / float32(W0) is the network's width
             over the source's (sy alike), formed once on the host.
  restore    the same offset added where track >= 0; the other rows keep their bits.

gate = 0.75 is a provisional default, not tuned: on frames without a common motion the best of 289 displacements still
undercuts SAD(0,0) by some margin (0.80 to 0.86 of it on uncorrelated synthetic frames, tools/motion_probe.py), and the gate
has to lie below that.

This module imports NumPy only.
"""
import numpy as np

_F = np.float32
CELLS = (2, 4, 8, 16)
MAX_RADIUS = 16
MAX_GRID = 4096                                     # cells a side: a SAD stays below 2**40
DEFAULTS = dict(cell=4, radius=8, gate=0.75)
FORMATS = ("rgb", "nv12")


def check_params(cell=4, radius=8, gate=0.75, who="motion"):
    """(cell, radius as ints, gate as a float32); a ValueError names the argument that is not usable"""
    if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or int(cell) not in CELLS:
        raise ValueError("%s: cell must be 2, 4, 8 or 16, got %r" % (who, cell))
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError("%s: radius must be an integer in [1, %d], got %r" % (who, MAX_RADIUS, radius))
    try:
        g = _F(gate)
    except (TypeError, ValueError):
        g = _F("nan")
    if isinstance(gate, bool) or not (g > 0 and g <= 1):
        raise ValueError("%s: gate must be a number in (0, 1], got %r" % (who, gate))
    return int(cell), int(radius), g


def gate_q(gate):
    """the gate as the integer the comparison uses: int(float32(gate) * float32(256))"""
    return int(_F(gate) * _F(256))


def grid_size(H0, W0, cell):
    return int(H0) // int(cell), int(W0) // int(cell)


def check_grid(Gh, Gw, radius, who="motion"):
    """the interior [R, G-R) must hold a cell on both axes; a ValueError names radius"""
    if Gh <= 2 * radius or Gw <= 2 * radius:
        raise ValueError("%s: radius=%d needs a signature of more than %d x %d cells, got %d x %d" %
                         (who, radius, 2 * radius, 2 * radius, Gh, Gw))
    if Gh > MAX_GRID or Gw > MAX_GRID:
        raise ValueError("%s: a signature of %d x %d cells, at most %d a side are taken" % (who, Gh, Gw, MAX_GRID))


def frame_size(shape, fmt):
    """(F, H0, W0) of frames of that shape: (F,H0,W0,3) for 'rgb', (F,H0*3/2,W0) for 'nv12'"""
    if fmt not in FORMATS:
        raise ValueError("motion: fmt must be 'rgb' or 'nv12', got %r" % (fmt,))
    if fmt == "rgb":
        if len(shape) != 4 or shape[3] != 3:
            raise ValueError("motion: RGB frames must be (F,H0,W0,3), got %r" % (tuple(shape),))
        return int(shape[0]), int(shape[1]), int(shape[2])
    if len(shape) != 3 or shape[1] % 3 or (shape[1] // 3 * 2) % 2 or shape[2] % 2:
        raise ValueError("motion: NV12 frames must be (F,H0*3/2,W0) with H0 and W0 even, got %r" % (tuple(shape),))
    return int(shape[0]), int(shape[1]) // 3 * 2, int(shape[2])


def _clips(clip_start, F):
    if clip_start is None:
        return [(0, F)]
    cs = [int(v) for v in np.asarray(clip_start).reshape(-1)]
    if len(cs) < 2 or cs[0] != 0 or cs[-1] != F or any(b < a for a, b in zip(cs, cs[1:])):
        raise ValueError("clip_start must be V+1 ascending offsets from 0 to F=%d, got %r" % (F, cs))
    return list(zip(cs[:-1], cs[1:]))


def luma_host(frames, fmt="rgb"):
    """frames -> (F,H0,W0) uint8 luma"""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8:
        raise ValueError("motion: frames must be uint8, got %s" % frames.dtype)
    F, H0, W0 = frame_size(frames.shape, fmt)
    if fmt == "nv12":
        return frames[:, :H0, :]
    f = frames.astype(np.int32)
    return ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8).astype(np.uint8)


def signature_host(frames, cell=4, fmt="rgb"):
    """frames -> (F,Gh,Gw) uint16: the luma summed over cell x cell blocks"""
    cell, _, _ = check_params(cell=cell, who="signature_host")
    y = luma_host(frames, fmt)
    F, H0, W0 = y.shape
    Gh, Gw = grid_size(H0, W0, cell)
    if Gh < 1 or Gw < 1:
        raise ValueError("signature_host: frames of %d x %d hold no cell of %d pixels" % (H0, W0, cell))
    y = y[:, :Gh * cell, :Gw * cell].astype(np.int64).reshape(F, Gh, cell, Gw, cell)
    return y.sum(axis=(2, 4)).astype(np.uint16)


def sad_table(cur, prev, radius):
    """(D,D) int64, D = 2*radius + 1: SAD(dx,dy) at [dy + radius, dx + radius] of two (Gh,Gw) signatures"""
    R = radius
    Gh, Gw = cur.shape
    c = cur[R:Gh - R, R:Gw - R].astype(np.int64)
    p = prev.astype(np.int64)
    out = np.empty((2 * R + 1, 2 * R + 1), dtype=np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            out[dy + R, dx + R] = np.abs(c - p[R - dy:Gh - R - dy, R - dx:Gw - R - dx]).sum()
    return out


def match_host(sig, clip_start=None, radius=8, gate=0.75, cell=4):
    """sig (F,Gh,Gw) uint16 -> (motion (F,2) int32 as (x, y) in source pixels, sad (F,2) int64 as (best, zero))"""
    cell, R, g = check_params(cell, radius, gate, "match_host")
    sig = np.asarray(sig)
    if sig.dtype != np.uint16 or sig.ndim != 3:
        raise ValueError("match_host: sig must be (F,Gh,Gw) uint16, got %s %r" % (sig.dtype, sig.shape))
    F, Gh, Gw = sig.shape
    check_grid(Gh, Gw, R, "match_host")
    gq = gate_q(g)
    motion = np.zeros((F, 2), dtype=np.int32)
    sad = np.zeros((F, 2), dtype=np.int64)
    d = np.arange(-R, R + 1, dtype=np.int64)
    d2 = d[:, None] ** 2 + d[None, :] ** 2
    for t0, t1 in _clips(clip_start, F):
        for t in range(t0 + 1, t1):
            tab = sad_table(sig[t], sig[t - 1], R)
            # the least (SAD, dx*dx + dy*dy, dy, dx): one integer key, the table is [dy, dx]
            key = ((tab << 10 | d2) << 6 | (d[:, None] + R)) << 6 | (d[None, :] + R)
            iy, ix = np.unravel_index(int(np.argmin(key)), key.shape)
            best, zero = int(tab[iy, ix]), int(tab[R, R])
            sad[t] = best, zero
            if best * 256 <= zero * gq:
                motion[t] = (ix - R) * cell, (iy - R) * cell
    return motion, sad


def motion_host(frames, clip_start=None, cell=4, radius=8, gate=0.75, fmt="rgb"):
    """signature_host then match_host -> (motion, sad)"""
    return match_host(signature_host(frames, cell, fmt), clip_start, radius, gate, cell)


def cumulate(motion, clip_start=None):
    """C (F,2) int32: the running sum of motion inside every clip (wrapping as int32 does)"""
    motion = np.asarray(motion, dtype=np.int32)
    C = np.zeros_like(motion)
    for t0, t1 in _clips(clip_start, motion.shape[0]):
        if t1 > t0:
            C[t0:t1] = np.cumsum(motion[t0:t1].astype(np.int64), axis=0).astype(np.int32)
    return C


def _shift(mask, bboxes, C, sx, sy, add):
    b = np.array(bboxes, dtype=_F, copy=True)
    F = b.shape[0]
    with np.errstate(all="ignore"):
        off = np.stack([C[:, 0].astype(_F) * _F(sx), C[:, 1].astype(_F) * _F(sy)], axis=1).astype(_F)   # (F,2)
        off4 = np.concatenate([off, off], axis=1)[:, None, :]                                            # (F,1,4)
        moved = (b + off4 if add else b - off4).astype(_F)
    m = np.asarray(mask).reshape(F, -1)
    b[m] = moved[m]
    return b


def stabilise_host(ids, bboxes, motion, clip_start, sx, sy):
    """bboxes (F,N,4) float32 in the stabilised frame: the clip's accumulated motion taken off every row with id >= 0"""
    ids = np.asarray(ids, dtype=_F)
    with np.errstate(invalid="ignore"):
        return _shift(ids >= 0, bboxes, cumulate(motion, clip_start), sx, sy, False)


def restore_host(track, tbox, motion, clip_start, sx, sy):
    """tbox (F,N,4) float32 back in image coordinates: the accumulated motion added where track >= 0"""
    return _shift(np.asarray(track) >= 0, tbox, cumulate(motion, clip_start), sx, sy, True)


# ------------------------------------------------------------------ the option of detect_video
def split_gmc(track):
    """The `gmc` key of a `track=` option, which track.parse_option does not know: track -> (track without the key, its value
    or None)"""
    if not isinstance(track, dict) or "gmc" not in track:
        return track, None
    rest = dict(track)
    return rest, rest.pop("gmc")


def parse_option(gmc, tracked, smooth, tubelet, who):
    """The `gmc` key of `who`'s track option (detect_video): None / False -> None; True or {'cell':, 'radius':, 'gate':} -> the
    dict with the defaults filled in.  tracked: the call links tracks; smooth, tubelet: the call has those passes on.  A
    ValueError names what is not usable."""
    if gmc is None or gmc is False:
        return None
    kw = {} if gmc is True else dict(gmc)
    unknown = sorted(set(kw) - set(DEFAULTS))
    if unknown:
        raise ValueError("%s: gmc takes cell, radius and gate, got %s" % (who, ", ".join(unknown)))
    kw = dict(DEFAULTS, **kw)
    kw["cell"], kw["radius"], g = check_params(kw["cell"], kw["radius"], kw["gate"], who + " with gmc")
    kw["gate"] = float(g)
    if not tracked:
        raise ValueError("%s: gmc needs track: it stabilises the boxes the tracker links" % who)
    for name, on in (("smooth", smooth), ("tubelet", tubelet)):
        if on:
            raise ValueError("%s: gmc beside %s is not taken: that pass emits boxes, and their way through the stabilised frame "
                             "has no definition yet" % (who, name))
    return kw
