"""Training augmentation with the pixels on the device.

The host keeps every decision of YOLO3VideoTrainTransform - the random draws, the constrained crop's IoU trials, the boxes
and the targets - and describes what they do to the pixels in a record per sample (`augment_record`): one colour affine,
two tap tables in source coordinates and the canvas fill.  `Loader._collate` gathers the records of a batch and the
untouched uint8 frames into an `AugmentBatch`; `augment_on_device` uploads it in one copy and runs vd_augment_u8_nchw
(viddet_amd/csrc/vd_augment.hip), which returns the normalised float batch the training step takes.

This module imports NumPy only (the loader's worker processes import it); torch is imported by `augment_on_device`.
"""
import numpy as np

from .video import _axis_taps, color_affine

MAX_TAPS = 32            # vd_augment_u8_nchw takes at most this many taps per axis
FILL_TAP = -1            # tap index of a tap that lies on the expansion canvas


def check_source_size(h0, w0, H, W):
    """Refuse a source whose WORST crop would need more taps than the kernel takes: the 4x expansion cropped whole and
    shrunk with the area interpolation, ceil(4 * max(w0 / W, h0 / H)) + 1 taps.  Decided from the size alone, so a run
    cannot stop on an unlucky draw."""
    need = int(np.ceil(4 * max(w0 / W, h0 / H))) + 1
    if need > MAX_TAPS:
        raise ValueError("device_augment: a %dx%d (width x height) source resized to %dx%d can need %d taps per axis (the 4x "
                         "expansion cropped whole, area interpolation); vd_augment_u8_nchw takes at most %d"
                         % (w0, h0, W, H, need, MAX_TAPS))


def _source_taps(n_crop, n_out, interp, shift, n_src):
    """`_axis_taps` of a crop of n_crop pixels resized to n_out, moved into source coordinates: canvas index = crop index +
    crop origin, source index = canvas index - expansion offset (shift = origin - offset); outside the source -> FILL_TAP."""
    idx, w = _axis_taps(int(n_crop), int(n_out), int(interp))
    idx = idx + int(shift)
    idx = np.where((idx < 0) | (idx >= n_src), FILL_TAP, idx)
    return np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(w, dtype=np.float32)


class AugmentRecord:
    """What one sample's decisions do to its pixels: color (12,) fp32 = M (3x3 row-major) then b; idx_y (H,Ty) int32 / w_y (H,Ty)
    fp32 and idx_x (W,Tx) / w_x (W,Tx) in source coordinates (FILL_TAP = canvas); fill (3,) fp32; window = the sample is a
    (K,h0,w0,3) window, not one (h0,w0,3) frame.  `params` keeps the decisions themselves (tests, probes)."""

    __slots__ = ("color", "idx_y", "w_y", "idx_x", "w_x", "fill", "window", "params")

    def __init__(self, color, idx_y, w_y, idx_x, w_x, fill, window=False, params=None):
        self.color, self.idx_y, self.w_y, self.idx_x, self.w_x = color, idx_y, w_y, idx_x, w_x
        self.fill, self.window, self.params = fill, bool(window), params

    def __getstate__(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __setstate__(self, state):
        for k, v in zip(self.__slots__, state):
            setattr(self, k, v)


def augment_record(h0, w0, H, W, ops=(), expand=None, crop=None, interp=1, flip=False, fill=(0.0, 0.0, 0.0), window=False):
    """The record of explicit decisions on an (h0,w0) source resized to (H,W): `ops` as video.color_distort_params returns
    them, `expand` = (offset_x, offset_y, canvas_width, canvas_height) or None, `crop` = (x0, y0, width, height) on the canvas
    (None = all of it), interp 0..4, flip = reverse x.  The colour affine is composed in fp64 and cast."""
    off_x, off_y, cw0, ch0 = (0, 0, w0, h0) if expand is None else [int(v) for v in expand]
    x0, y0, cw, ch = (0, 0, cw0, ch0) if crop is None else [int(v) for v in crop]
    M, b = color_affine(ops)
    color = np.concatenate([M.reshape(9), b]).astype(np.float32)
    idx_y, w_y = _source_taps(ch, H, interp, y0 - off_y, h0)
    idx_x, w_x = _source_taps(cw, W, interp, x0 - off_x, w0)
    if flip:
        idx_x, w_x = np.ascontiguousarray(idx_x[::-1]), np.ascontiguousarray(w_x[::-1])
    if idx_y.shape[1] > MAX_TAPS or idx_x.shape[1] > MAX_TAPS:
        raise ValueError("augment_record: a %dx%d crop resized to %dx%d has Ty=%d / Tx=%d taps; vd_augment_u8_nchw takes at "
                         "most %d" % (cw, ch, W, H, idx_y.shape[1], idx_x.shape[1], MAX_TAPS))
    params = dict(ops=list(ops), expand=None if expand is None else (off_x, off_y, cw0, ch0), crop=(x0, y0, cw, ch),
                  interp=int(interp), flip=bool(flip))
    return AugmentRecord(color, idx_y, w_y, idx_x, w_x, np.asarray(fill, dtype=np.float32), window, params)


def _pad_taps(idx, w, T):
    """(n,t) tables -> (n,T) with fill taps of weight 0 behind them (they change no sum)."""
    n, t = idx.shape
    if t == T:
        return idx, w
    return (np.concatenate([idx, np.full((n, T - t), FILL_TAP, np.int32)], axis=1),
            np.concatenate([w, np.zeros((n, T - t), np.float32)], axis=1))


class AugmentBatch:
    """The batch `augment_on_device` takes: `raw` (all frames, flat uint8), `src_off` (N,) int64 byte offsets into it, `src_hw`
    (N,2) int32 (h0, w0), `color` (N,12) fp32, `idx_y` / `w_y` (N,H,Ty), `idx_x` / `w_x` (N,W,Tx) padded to the batch's largest
    Ty / Tx with zero-weight fill taps, `fill` (3,) fp32, and K, H, W; `window` = samples are (K,h0,w0,3) windows.  Sources of
    one batch may differ in size; K is the same for all."""

    def __init__(self, frames, records):
        if len(frames) != len(records) or not records:
            raise ValueError("AugmentBatch: one record per sample needed")
        fr = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        fr = [f if f.ndim == 4 else f[np.newaxis] for f in fr]
        self.window = records[0].window
        self.K = fr[0].shape[0]
        self.H, self.W = records[0].idx_y.shape[0], records[0].idx_x.shape[0]
        for f, r in zip(fr, records):
            if f.ndim != 4 or f.shape[3] != 3 or f.shape[0] != self.K or r.window != self.window:
                raise ValueError("AugmentBatch: every sample must be (K,h0,w0,3) uint8 with one K, got %r" % (f.shape,))
            if (r.idx_y.shape[0], r.idx_x.shape[0]) != (self.H, self.W):
                raise ValueError("AugmentBatch: the records of one batch must have one target size")
            if not np.array_equal(r.fill, records[0].fill):
                raise ValueError("AugmentBatch: the records of one batch must have one fill colour")
        self.N = len(fr)
        sizes = np.array([f.size for f in fr], dtype=np.int64)
        self.src_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.src_hw = np.array([f.shape[1:3] for f in fr], dtype=np.int32)
        self.raw = np.concatenate([f.reshape(-1) for f in fr])
        self.color = np.stack([r.color for r in records]).astype(np.float32)
        self.Ty, self.Tx = max(r.idx_y.shape[1] for r in records), max(r.idx_x.shape[1] for r in records)
        ty = [_pad_taps(r.idx_y, r.w_y, self.Ty) for r in records]
        tx = [_pad_taps(r.idx_x, r.w_x, self.Tx) for r in records]
        self.idx_y, self.w_y = np.stack([t[0] for t in ty]), np.stack([t[1] for t in ty])
        self.idx_x, self.w_x = np.stack([t[0] for t in tx]), np.stack([t[1] for t in tx])
        self.fill = np.asarray(records[0].fill, dtype=np.float32)

    @property
    def shape(self):
        """shape of the float batch `augment_on_device` returns"""
        return (self.N, self.K, 3, self.H, self.W) if self.window else (self.N, 3, self.H, self.W)

    def __len__(self):
        return self.N

    SECTIONS = ("src_off", "src_hw", "color", "idx_y", "w_y", "idx_x", "w_x", "fill", "raw")

    def packed(self):
        """(buffer uint8, {name: (byte offset, dtype, shape)}): every array in one host buffer, each section 16-byte aligned,
        the frames last - one host-to-device copy per batch."""
        lay, pos = {}, 0
        for name in self.SECTIONS:
            a = getattr(self, name)
            lay[name] = (pos, a.dtype, a.shape)
            pos += (a.nbytes + 15) // 16 * 16
        buf = np.zeros(pos, dtype=np.uint8)
        for name in self.SECTIONS:
            a = getattr(self, name)
            buf[lay[name][0]:lay[name][0] + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        return buf, lay


def augment_on_device(batch):
    """AugmentBatch -> the augmented, normalised float batch on the current device: (B,3,H,W), or (B,K,3,H,W) for windows, fp32
    (vd_augment_u8_nchw; one packed upload, one launch)."""
    import torch
    from . import ops
    if not isinstance(batch, AugmentBatch):
        raise TypeError("augment_on_device takes the AugmentBatch a Loader of YOLO3VideoTrainTransform(device_augment=True) "
                        "yields as its first column, got %s" % type(batch).__name__)
    if batch.Ty > MAX_TAPS or batch.Tx > MAX_TAPS:
        raise ValueError("augment_on_device: Ty=%d / Tx=%d taps, vd_augment_u8_nchw takes at most %d" % (batch.Ty, batch.Tx, MAX_TAPS))
    if not torch.cuda.is_available():
        raise RuntimeError("augment_on_device needs the GPU: the augmentation kernel has no CPU fallback")
    buf, lay = batch.packed()
    dev = torch.from_numpy(buf).cuda()
    sec = {name: dev[off:] for name, (off, _, _) in lay.items()}       # views: only their addresses are used
    out = torch.empty((batch.N * batch.K, 3, batch.H, batch.W), dtype=torch.float32, device=dev.device)
    ops.augment_u8_nchw(sec["raw"], sec["src_off"], sec["src_hw"], sec["color"], sec["idx_y"], sec["w_y"], batch.Ty,
                        sec["idx_x"], sec["w_x"], batch.Tx, sec["fill"], out, batch.N, batch.K, batch.H, batch.W)
    return out.view(batch.shape)
