"""Host-side mirror of the reference's yolo3_darknet53 network object for the MI355X kernel library.

Mirrors (paths under /root/reference):
  yolo3_darknet53 factory            models/definitions/yolo/wrappers.py:9-110
  Darknet-53 2-D backbone            models/definitions/darknet/three_darknet.py:100-123,152-264
  YOLODetectionBlockV3               models/definitions/yolo/yolo3.py:218-263
  YOLOOutputV3                       models/definitions/yolo/yolo3.py:43-199
  YOLOV3T (wiring, NMS, losses)      models/definitions/yolo/yolo3.py:959-1302
  _conv2d / _upsample                models/definitions/layers.py:11-20,63-70
  yolo3_3ddarknet / Darknet3D        models/definitions/yolo/wrappers.py:113-130, darknet/three_darknet.py:19-70,100-226
                                     (--conv_types 21: the (2+1)-D backbone of frame windows)

The network is a static list of nodes; for every (mode, batch, H, W) a *launch program* — a flat
list of pre-built C-ABI calls (descriptor structs built once) — is compiled and replayed.  All
arithmetic runs in libviddet_hip.so; torch provides device memory, streams and (for N>1 ranks)
torch.distributed collectives only.  There is no autograd tape: the backward program is the fixed
reverse schedule of this one graph.
"""
import ctypes as C
import math
import os
import re
from collections import OrderedDict

import numpy as np
import torch

from . import lib as L
from . import ops
from .lib import ConvDesc, WgradDesc, EPI_AFFINE, EPI_LEAKY, EPI_RESIDUAL
from .ops import round_up, fwd_taps, dgrad_plans

from .consts import BN_EPS, BN_MOMENTUM, LEAKY_SLOPE   # layers.py:68-69


class Slot:
    """Late-bound pointer argument of a launch record (set right before a program runs)."""

    def __init__(self):
        self.value = None


class Program:
    """A flat replayable list of C-ABI launches; the stream is bound at run time (the last argument of
    every vd_* entry point), so a program can be replayed eagerly or inside a HIP graph capture.
    A record may name a side stream (`stream=`) and python records (`add_py`) carry event record / wait
    calls, which is how the weight-gradient GEMMs run beside the rest of the backward pass."""

    def __init__(self):
        self.recs = []
        self.meta = []          # per-record info (kind, algorithmic flops) for the roofline accounting
        self.keep = []          # descriptor structs / tensors the records point into
        self.streams = []       # per-record side stream (torch.cuda.Stream) or None = current stream

    def add(self, fname, *args, meta=None, stream=None, label=None):
        """`label`: the name the record is listed under where that is a kernel family, not the entry point (the fused stem
        weight gradient vd_stem_wgrad_bn is a `vd_stem_wgrad` record to everything that counts or times records by name)"""
        fn = getattr(L.load(), fname)
        self.recs.append((label or fname, fn, args))
        self.meta.append(meta)
        self.streams.append(stream)

    def add_py(self, fn):
        self.recs.append((None, fn, ()))
        self.meta.append(None)
        self.streams.append(None)

    def add_coll(self, fn):
        """a collective (SyncBN's statistics all-reduce) as a record of the program: enqueued in place between the launches
        it sits between - the replay loop never leaves the program for it - and replayed by run_timed as well, so the ranks
        of a job stay in step whichever replay form they run"""
        self.recs.append((None, fn, ()))
        self.meta.append(dict(kind='collective'))
        self.streams.append(None)

    def hold(self, *objs):
        self.keep.extend(objs)

    def run(self):
        s = L.stream_ptr()
        for (fname, fn, args), st in zip(self.recs, self.streams):
            if fname is None:
                fn()
                continue
            a = [x.value if isinstance(x, Slot) else x for x in args]
            rc = fn(*a, s if st is None else C.c_void_p(st.cuda_stream))
            if rc != 0:
                L.check(rc, fname)

    def run_timed(self, select):
        """Replay (everything on the current stream, side streams ignored so that each launch is timed alone)
        with a (start, stop) event pair around every record whose entry point is in `select`.
        Returns [(fname, meta, start, stop)]."""
        s = L.stream_ptr()
        out = []
        for (fname, fn, args), meta in zip(self.recs, self.meta):
            if fname is None:
                if meta and meta.get('kind') == 'collective':
                    fn()
                continue
            a = [x.value if isinstance(x, Slot) else x for x in args]
            if fname in select:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn(*a, s)
                e1.record()
                if fname in ("vd_conv_igemm", "vd_conv_wgrad"):     # which product arithmetic this record runs in
                    d = args[0]._obj
                    meta = dict(meta or {}, split=bool(d.flags & L.MATH_SPLIT), bf16=bool(d.flags & L.MATH_BF16),
                                f16x2=bool(d.flags & L.MATH_F16X2), nohalo=bool(d.flags & L.MATH_NOHALO), tile=int(getattr(d, "tile", 0)),
                                streamk=bool(fname == "vd_conv_igemm" and L.load().vd_conv_igemm_streamk(args[0])))
                    if fname == "vd_conv_wgrad":                # the halo-ring kernel (vd_wgrad_halo.hip) or the generic one
                        meta["wgrad_halo"] = bool(L.load().vd_conv_wgrad_uses_halo(args[0]))
                    if fname == "vd_conv_igemm" and meta.get("bytes"):
                        # operands the fused epilogue reads besides input / weights: the residual (or accumulated
                        # gradient) rows, and the producer's z rows of the fused BatchNorm-backward reductions
                        out_bytes = 4.0 * d.N * d.Hg * d.Wg * d.Co
                        extra = (out_bytes if d.residual else 0.0) + (out_bytes if getattr(d, "bs_part", None) else 0.0)
                        meta["bytes_epilogue_reads"] = extra
                        meta["bytes"] = meta["bytes"] + extra
                if fname == "vd_conv_igemm_bf16":
                    form = int(L.load().vd_conv_igemm_bf16_streamk(args[0], args[1]))
                    meta = dict(meta or {}, tile=int(args[0]._obj.tile), nohalo=bool(args[0]._obj.flags & L.MATH_NOHALO),
                                streamk=form == 1, splitk=form == 2)
                out.append((fname, meta, e0, e1))
            else:
                rc = fn(*a, s)
            if rc != 0:
                L.check(rc, fname)
        return out


class TuneCache(dict):
    """The plan-time autotuner's choices (launch-record signature -> arithmetic / tile), persisted.

    A choice made by timing differs between boxes and runs (launch-to-launch noise under the power limit is of the order
    of the differences between tiles), and with it the summation order of every convolution: two runs of one seed were not
    bit-identical, ranks of one job could disagree, and every process start paid the tuning again (38 of the 39.5 s of a
    driver bench run).  So the table lives in a JSON file: `VD_TUNE_CACHE` (a path), default
    viddet_amd/tune/gfx950_<hash>.json where <hash> identifies the kernel sources the choices were timed on (another
    library build never reads them).  Read on first use, written (atomically, by rank 0) whenever a plan build added
    entries; `VD_TUNE_CACHE=off` keeps it in memory only.  Under torch.distributed every rank adopts rank 0's choice for
    a new entry (`agree`), so the ranks of a job run the same kernels."""

    def __init__(self):
        super().__init__()
        self._loaded, self._dirty, self.tuned, self.hits, self._synced_world = False, False, 0, 0, 1

    @staticmethod
    def library_id():
        import hashlib
        here = os.path.dirname(os.path.abspath(__file__))
        # the conv kernels' sources (the public header is not part of it: declarations of other entry points change there
        # without touching a tile; descriptor layouts are guarded by the ABI revision)
        srcs = [os.path.join(here, "csrc", f) for f in ("vd_conv.hip", "vd_conv_igemm.h", "vd_conv_sk.hip", "vd_conv_par.hip",
                                                         "vd_conv_bf16.hip", "vd_conv_igemm_bf16.h", "vd_conv_bf16_sk.hip", "vd_conv_c32_bf16.hip",
                                                         "vd_wgrad_halo.hip", "vd_common.h")]
        h = hashlib.sha256()
        if all(os.path.exists(f) for f in srcs):
            for f in srcs:
                h.update(open(f, "rb").read())
        else:
            h.update(open(L.LIB_PATH, "rb").read())
        # library switches that change what a timed launch runs (the default keeps the hash of the sources alone)
        for sw in ("VD_WGRAD_RESERVE",):
            if os.environ.get(sw):
                h.update(("%s=%s" % (sw, os.environ[sw])).encode())
        return h.hexdigest()[:12]

    def path(self):
        p = os.environ.get("VD_TUNE_CACHE", "")
        if p.lower() in ("off", "0", "none"):
            return None
        if p:
            return p
        return os.path.join(os.path.dirname(os.path.abspath(__file__)), "tune", "gfx950_%s.json" % self.library_id())

    @staticmethod
    def _world():
        if not torch.distributed.is_available() or not torch.distributed.is_initialized():
            return 1
        return torch.distributed.get_world_size()

    @staticmethod
    def device_arch():
        """gcnArchName of the current device without its feature suffixes ('gfx950'), None without a GPU"""
        if not torch.cuda.is_available():
            return None
        return str(torch.cuda.get_device_properties(torch.cuda.current_device()).gcnArchName).split(":")[0]

    def _read_file(self):
        import ast
        import json
        out = {}
        p = self.path()
        if p is None or not os.path.exists(p):
            return out
        try:
            doc = json.load(open(p))
            if doc.get("library") not in (None, self.library_id()):
                return out                               # timed on other kernels
            arch = self.device_arch()
            if arch is not None and doc.get("device") not in (None, arch):
                return out                               # timed on another device
            for k, v in doc.get("entries", {}).items():
                out[ast.literal_eval(k)] = tuple(v) if isinstance(v, list) else v
        except (OSError, ValueError, SyntaxError) as e:   # an unreadable table is a cold start, not an error
            print("viddet_amd: ignoring tuning table %s (%s)" % (p, e), flush=True)
            return {}
        return out

    def load(self):
        """Read the table.  Under torch.distributed ONLY rank 0 reads the file and every rank adopts its entries (one
        broadcast at first use): ranks that read their own copies - another node's file system, another VD_TUNE_CACHE,
        a file rank 0 has rewritten since - would disagree on hit or miss, and the ranks that miss would enter `agree`'s
        broadcast alone.  After this every lookup gives the same answer on every rank, so `agree` is entered by all or none."""
        self._loaded = True
        world = self._world()
        self._synced_world = world
        if world > 1 and os.environ.get("VD_TUNE_AGREE", "1") != "0":
            box = [self._read_file() if torch.distributed.get_rank() == 0 else None]
            torch.distributed.broadcast_object_list(box, src=0)
            dict.clear(self)                              # rank 0's table, nothing else
            entries = box[0]
        else:
            entries = self._read_file()
        for key, v in entries.items():
            if not dict.__contains__(self, key):
                dict.__setitem__(self, key, v)

    def __contains__(self, key):
        # (a process group that came up after the first lookup: sync once more - every rank is in the same position)
        if not self._loaded or self._synced_world != self._world():
            self.load()
        hit = dict.__contains__(self, key)
        self.hits += int(hit)
        return hit

    def __setitem__(self, key, value):
        dict.__setitem__(self, key, value)
        self._dirty = True
        self.tuned += 1

    def clear(self):
        dict.clear(self)
        self._loaded = False                             # entries on disk come back on the next lookup

    def agree(self, best):
        """rank 0's choice for a new entry, on every rank (all ranks build the same plans in the same order)."""
        if os.environ.get("VD_TUNE_AGREE", "1") == "0" or not torch.distributed.is_available() or \
                not torch.distributed.is_initialized() or torch.distributed.get_world_size() == 1:
            return best
        box = [best]
        torch.distributed.broadcast_object_list(box, src=0)
        return tuple(box[0]) if isinstance(box[0], list) else box[0]

    def save(self):
        import json
        if not self._dirty:
            return
        self._dirty = False
        p = self.path()
        if p is None:
            return
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_rank() != 0:
            return
        try:
            os.makedirs(os.path.dirname(p) or ".", exist_ok=True)
            doc = {"library": self.library_id(), "device": self.device_arch() or "gfx950",
                   "entries": {repr(k): (list(v) if isinstance(v, tuple) else v) for k, v in sorted(self.items(), key=lambda kv: repr(kv[0]))}}
            tmp = "%s.%d.tmp" % (p, os.getpid())
            with open(tmp, "w") as f:
                json.dump(doc, f, indent=0)
            os.replace(tmp, p)
        except OSError as e:
            print("viddet_amd: could not write tuning table %s (%s)" % (p, e), flush=True)


_TUNE_CACHE = TuneCache()


def ev_record(e, st=None):
    """python record of a Program: record event e on stream st (None = the stream the program runs on)"""
    def f():
        e.record(st if st is not None else torch.cuda.current_stream())
    return f


def ev_wait(e, st=None):
    """python record of a Program: stream st (None = the stream the program runs on) waits for event e"""
    def f():
        (st if st is not None else torch.cuda.current_stream()).wait_event(e)
    return f


def _bf16_pitch(c):
    """row pitch of a head tensor in bf16-storage training: the K dimension of its data gradient (32 or runs of 64)"""
    return c if (c == 32 or c % 64 == 0) else round_up(c, 64)



def fp32_math():
    """Arithmetic of the fp32 convolution products (include/viddet_hip.h VD_MATH_SPLIT): 'native' = fp32 MFMA,
    'split' = three-way bf16 operand split on the bf16 matrix pipe (fp32-accurate), 'auto' = the
    plan-time autotuner times both per launch record and keeps the faster."""
    m = _MATH_OVERRIDE[0] or os.environ.get("VD_FP32_MATH", "auto")
    if m not in _MATH_MODES:
        raise ValueError("VD_FP32_MATH must be one of %s, got %r" % ("|".join(_MATH_MODES), m))
    return m


_MATH_OVERRIDE = [None]
# 'split2' = two-way fp16 operand split with per-tensor power-of-two scales (VD_MATH_F16X2: three MFMAs per product block
# instead of six, fp32-accurate); 'auto' times native, split and split2 per launch record
_MATH_MODES = ("native", "split", "split2", "auto", "bf16")
_ALL_MATH = L.MATH_SPLIT | L.MATH_BF16 | L.MATH_F16X2 | L.MATH_NOHALO | L.CONV_STREAMK


def _streamk_on():
    """VD_STREAMK=0: never the persistent stream-K form of k_conv_igemm (read when a plan is built).  The form changes how a
    launch is cut into workgroups, not one bit of what it computes (vd_conv_sk.hip), so this is a speed switch only."""
    return os.environ.get('VD_STREAMK', '1') != '0'


def _streamk_applies(d, fl, tile):
    """would vd_conv_igemm run this record as a stream-K grid with arithmetic `fl` and tile `tile`?"""
    if not (d.sk_ws and (fl & L.MATH_F16X2)):
        return False
    keep = (d.flags, d.tile)
    d.flags, d.tile = (d.flags & ~_ALL_MATH) | fl | L.CONV_STREAMK, tile
    try:
        return bool(L.load().vd_conv_igemm_streamk(C.byref(d)))
    finally:
        d.flags, d.tile = keep


def set_conv_math(mode):
    """Process-wide product arithmetic of the fp32-tensor convolutions for programs built from now on: None (the
    VD_FP32_MATH environment, default 'auto'), 'native', 'split', 'auto', or 'bf16' = products on bf16-rounded
    operands with fp32 accumulation (VD_MATH_BF16; the mixed-precision training arithmetic, bf16-accurate)."""
    assert mode is None or mode in _MATH_MODES
    _MATH_OVERRIDE[0] = mode


def _tile_candidates(d, math):
    """(flags bit, tile) candidates of one launch record."""
    if d.flags & L.CONV_PARITY4:            # the parity-fused stride-2 data gradient: fp16 split, the tiles it is built for
        return [(L.MATH_F16X2, t) for t in (5, 1, 6, 2, 12, 11)]
    cands = []
    if math in ("native", "auto"):
        if d.Co <= 32:
            cands += [(0, 7)]
        elif d.Co <= 64:
            cands += [(0, 6), (0, 8)]
        else:
            cands += [(0, t) for t in (1, 2, 3, 4, 5)]
    fls = []
    if math in ("split", "auto"):
        fls.append(L.MATH_SPLIT)
    if math in ("split2", "auto"):
        # the fp16 split needs the max-abs slots of both operands and has no in-load transform
        fls.append(L.MATH_F16X2 if (d.amax_in and d.amax_w and not d.in_scale) else L.MATH_SPLIT)
    if math == "bf16":
        fls.append(L.MATH_BF16)
    # the halo-staged loop (3x3 stride-1 geometry) is timed against the generic one
    if L.MATH_F16X2 in fls and os.environ.get("VD_HALO_AB", "1") == "1" and d.T == 9 and d.in_stride == 1 and d.Hg == d.Hi and d.Co > 32:
        fls.append(L.MATH_F16X2 | L.MATH_NOHALO)
    for fl in dict.fromkeys(fls):
        if d.Co <= 32:           # 256 x 32 tiles (9: 32x32x16 MFMA, 10: 16x16x32)
            cands += [(fl, t) for t in (9, 10, 13, 14)]
        elif d.Co <= 64:         # split tiles 1..4 on the 32x32x16 MFMA, 5..8 the same tiles on 16x16x32
            cands += [(fl, t) for t in (3, 4, 7, 8)] + ([(fl, t) for t in (15, 16)] if not (fl & L.MATH_F16X2 and not fl & L.MATH_NOHALO and d.T == 9 and d.in_stride == 1 and d.Hg == d.Hi) else [])
        else:
            # 11, 12: 128x128 as four waves (two workgroups per CU); never the halo loop, so only with the generic bit
            cands += [(fl, t) for t in (1, 2, 3, 4, 5, 6, 7, 8)] + ([(fl, t) for t in (11, 12)] if not (fl & L.MATH_F16X2 and not fl & L.MATH_NOHALO and d.T == 9 and d.in_stride == 1 and d.Hg == d.Hi) else [])
    return cands


def _bf16_tile_candidates(d, of32, *, patch_kernel, tall_tiles, halo):
    """(tiles, halo_geo) of one vd_conv_igemm_bf16 launch record for _tune_bf16_record.  What the inference and the training
    plans decide differently is the caller's word: patch_kernel - tile 16, the first-stage patch kernel of
    vd_conv_c32_bf16.hip (3x3, 32 -> 64 channels; the library falls back to the default tile where it does not apply);
    tall_tiles - the 256-row tiles 8 / 9 of wide layers; halo - whether the halo-staged loop may be timed at all."""
    one = d.T == 1           # 14 / 15: the small four-wave tiles (64x64 / 128x32, four or five workgroups per CU) for the HBM-bound 1x1 layers
    tiles = ((10, 11, 13) + ((14,) if one else ()) + ((16,) if (d.T == 9 and d.Co == 64 and patch_kernel and not of32) else ()) if d.Ci == 32
             else (12, 10, 11, 13) + ((15,) if one else ()) if d.Co <= 32
             else (10, 11, 13, 2, 3, 4, 5) + ((14,) if one else ()) if d.Co <= 64
             else (1, 2, 3, 4, 5, 6, 7) + ((8, 9) if (d.Co > 128 and tall_tiles) else ()) + ((14,) if one else ()))
    # 3x3 stride-1 'same' geometry: the halo-staged loop (8-wave tiles; the library falls back by itself where it does not
    # apply) is timed against the generic one
    return tiles, bool(halo and d.T == 9 and d.in_stride == 1 and d.Hg == d.Hi and d.Ci % 64 == 0)


def autotune_desc(d, reps=3):
    """Pick the fastest k_conv_igemm variant (product arithmetic x tile shape) for one launch descriptor (timed in
    place on its own buffers with events on the launch stream; cached per problem signature).  VD_AUTOTUNE=0 keeps
    the kernel's heuristic tile.  Tuning launches only rewrite buffers every real run rewrites first."""
    math = fp32_math()
    base = d.flags & ~_ALL_MATH
    if os.environ.get("VD_AUTOTUNE", "1") == "0":
        f16 = L.MATH_F16X2 if (d.amax_in and d.amax_w and not d.in_scale) else L.MATH_SPLIT
        d.flags = base | {"split": L.MATH_SPLIT, "split2": f16, "bf16": L.MATH_BF16}.get(math, 0)
        if d.flags & L.MATH_F16X2 and d.T >= 9 and d.sk_ws and _streamk_on():
            d.flags |= L.CONV_STREAMK                     # (the library ignores it where the form does not apply)
        if os.environ.get("VD_TILE_ALT", "0") == "1":
            # a second, equally deterministic tile set (the last candidate of the launch record's list instead of the
            # kernel's heuristic tile): other M-tile heights, hence other groupings of the BatchNorm partial sums and
            # split-K slabs - the control of tests/test_training_loop_gpu.py
            alt = [t for fl, t in _tile_candidates(d, math if math != "auto" else "native") if fl == (d.flags & _ALL_MATH)]
            if alt:
                d.tile = alt[-1]
        return
    lib = L.load()
    s = L.stream_ptr()
    key = (math, d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.in_stride, d.T, d.Co, d.out_stride, base, bool(d.in_scale),
           bool(d.stats_part), bool(d.amax_in and d.amax_w), bool(d.amax_out), d.Kfr, bool(d.bs_part))
    if key in _TUNE_CACHE:
        fl, d.tile = _TUNE_CACHE[key]
        d.flags = base | fl
        return
    cands = _tile_candidates(d, math)
    best = cands[0]
    if len(cands) > 1:
        def time_of(fl, c, n):
            d.flags, d.tile = base | fl, c
            L.check(lib.vd_conv_igemm(C.byref(d), s), 'vd_conv_igemm/tune')
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                lib.vd_conv_igemm(C.byref(d), s)
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1) / n
            if os.environ.get("VD_TUNE_VERBOSE") == "1":
                print("igemm tune %s math %d tile %d: %.4f ms (%d launches)" % (key[1:11], fl, c, t, n), flush=True)
            return t
        ranked = sorted((time_of(fl, c, reps), (fl, c)) for fl, c in cands)
        # the persistent stream-K form of the three fastest tiles (same bits, another cut of the launch into workgroups)
        if _streamk_on():
            sk = [(fl | L.CONV_STREAMK, c) for _, (fl, c) in ranked[:3] if _streamk_applies(d, fl, c)]
            ranked = sorted(ranked + [(time_of(fl, c, reps), (fl, c)) for fl, c in sk])
        best = ranked[0][1]
        # candidates within 4 % of the fastest are re-timed with more launches: the first pass is 3 launches each, and
        # launch-to-launch noise under the power limit is of that order
        close = [fc for t, fc in ranked if t <= 1.04 * ranked[0][0]][:3]
        if len(close) > 1:
            best = min((time_of(fl, c, 3 * reps), (fl, c)) for fl, c in close)[1]
    best = _TUNE_CACHE.agree(tuple(best))
    d.flags, d.tile = base | best[0], best[1]
    _TUNE_CACHE[key] = best


def _wgrad_halo_applies(d, flags):
    """would vd_conv_wgrad run the halo-ring kernel (vd_wgrad_halo.hip) for this record with `flags` | VD_WGRAD_HALO?
    The library ignores the flag elsewhere; this keeps such launches out of the timing loop."""
    keep = d.flags
    d.flags = flags | L.WGRAD_HALO
    try:
        return bool(L.load().vd_conv_wgrad_uses_halo(C.byref(d)))
    finally:
        d.flags = keep


def autotune_wgrad_bf16(d, ws_ptr, ws_bytes, reps=2):
    """bf16-stored operands: generic kernel vs the halo ring, timed in place (the flag is ignored where it does not apply)"""
    d.flags = L.STORE_BF16 | L.MATH_BF16
    if os.environ.get("VD_WGRAD_HALO", "1") != "1" or not _wgrad_halo_applies(d, L.STORE_BF16 | L.MATH_BF16):
        return
    if os.environ.get("VD_AUTOTUNE", "1") == "0":
        d.flags |= L.WGRAD_HALO
        return
    key = ('wgrad_bf16', d.N, d.Hi, d.Wi, d.Ci, d.Co)
    if key not in _TUNE_CACHE:
        lib = L.load()
        s = L.stream_ptr()
        best, best_t = 0, None
        for fl in (0, L.WGRAD_HALO):
            d.flags = L.STORE_BF16 | L.MATH_BF16 | fl
            L.check(lib.vd_conv_wgrad(C.byref(d), ws_ptr, ws_bytes, s), 'vd_conv_wgrad/tune')
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                lib.vd_conv_wgrad(C.byref(d), ws_ptr, ws_bytes, s)
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1)
            if os.environ.get("VD_TUNE_VERBOSE") == "1":
                print("wgrad bf16 tune %s halo %d: %.4f ms" % (key[1:], fl, t / reps), flush=True)
            if best_t is None or t < best_t:
                best, best_t = fl, t
        _TUNE_CACHE[key] = _TUNE_CACHE.agree(best)
    d.flags = L.STORE_BF16 | L.MATH_BF16 | _TUNE_CACHE[key]


def autotune_wgrad(d, ws_ptr, ws_bytes, reps=2):
    """Product arithmetic of one weight-gradient launch record (fp32 MFMA vs the split forms), timed in place."""
    math = fp32_math()
    d.flags = 0
    if d.Co < 64 or math == "native":
        return
    if math == "bf16":
        d.flags = L.MATH_BF16
        return
    f16 = L.MATH_F16X2 if (d.amax_in and d.amax_dout and not d.in_scale) else L.MATH_SPLIT
    # the halo-ring kernel (vd_wgrad_halo.hip) where the library takes it: 3x3 / stride 1 / Co >= 128, fp16 split
    halo = L.WGRAD_HALO if (f16 == L.MATH_F16X2 and os.environ.get("VD_WGRAD_HALO", "1") == "1" and _wgrad_halo_applies(d, f16)) else 0
    if math in ("split", "split2") or os.environ.get("VD_AUTOTUNE", "1") == "0":
        d.flags = (f16 | halo) if math in ("split2", "auto") else L.MATH_SPLIT
        return
    key = ('wgrad', d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.in_stride, d.T, d.Co, d.Kfr, bool(d.in_scale), f16 | halo)
    if key not in _TUNE_CACHE:
        lib = L.load()
        s = L.stream_ptr()
        best, best_t = 0, None
        for fl in dict.fromkeys((0, L.MATH_SPLIT, f16, f16 | halo)):
            d.flags = fl
            L.check(lib.vd_conv_wgrad(C.byref(d), ws_ptr, ws_bytes, s), 'vd_conv_wgrad/tune')
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                lib.vd_conv_wgrad(C.byref(d), ws_ptr, ws_bytes, s)
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1)
            if os.environ.get("VD_TUNE_VERBOSE") == "1":
                print("wgrad tune %s flags %d: %.4f ms" % (key[1:11], fl, t / reps), flush=True)
            if best_t is None or t < best_t:
                best, best_t = fl, t
        _TUNE_CACHE[key] = _TUNE_CACHE.agree(best)
    d.flags = _TUNE_CACHE[key]


def _tune_bf16_record(d, of32, key, tiles, halo_geo, splitk=False):
    """Time the tile variants of one vd_conv_igemm_bf16 launch record in place - generic loop, halo-staged loop where it
    exists, and the persistent stream-K form of the three fastest (VD_CONV_STREAMK: same bits) - and keep the best as
    (tile, flag bits) under `key`.  splitk (inference plans only - the form is deterministic but has another summation
    order than the one-tile launch): launches with too few tiles for the chip also time the split-K grid (VD_CONV_SPLITK)
    of every tile that has one."""
    lib = L.load()
    s = L.stream_ptr()
    mask = L.MATH_NOHALO | L.CONV_STREAMK | L.CONV_SPLITK
    base = d.flags & ~mask
    if key not in _TUNE_CACHE:
        verbose = os.environ.get("VD_TUNE_VERBOSE") == "1"

        def time_of(c, fl):
            d.tile, d.flags = c, base | fl
            L.check(lib.vd_conv_igemm_bf16(C.byref(d), of32, s), 'vd_conv_igemm_bf16/tune')
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                lib.vd_conv_igemm_bf16(C.byref(d), of32, s)
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1)
            if verbose:
                fl_ = 2.0 * d.N * d.Hg * d.Wg * d.Co * d.T * d.Ci * 3 / t / 1e9
                print("bf16 tune %s tile %d %s%s: %.3f ms %.0f TF" % (key[1:10], c, "generic" if fl & L.MATH_NOHALO else "halo",
                                                                   " split-K" if fl & L.CONV_SPLITK else " stream-K" if fl & L.CONV_STREAMK else "",
                                                                   t / 3, fl_), flush=True)
            return t
        ranked = []
        for c in tiles:
            for fl in ((0, L.MATH_NOHALO) if (halo_geo and c in (2, 3, 5, 6, 7, 10)) else (L.MATH_NOHALO,)):
                ranked.append((time_of(c, fl), (c, fl)))
        ranked.sort()
        if _streamk_on() and d.sk_ws and not of32:
            classic = list(ranked)
            for _, (c, fl) in classic[:3]:
                d.tile, d.flags = c, base | fl | L.CONV_STREAMK
                if lib.vd_conv_igemm_bf16_streamk(C.byref(d), of32) == 1:
                    ranked.append((time_of(c, fl | L.CONV_STREAMK), (c, fl | L.CONV_STREAMK)))
            if splitk and os.environ.get("VD_SPLITK", "1") != "0":
                for _, (c, fl) in classic:
                    d.tile, d.flags = c, base | fl | L.CONV_SPLITK
                    if lib.vd_conv_igemm_bf16_streamk(C.byref(d), of32) == 2:
                        ranked.append((time_of(c, fl | L.CONV_SPLITK), (c, fl | L.CONV_SPLITK)))
            ranked.sort()
        _TUNE_CACHE[key] = _TUNE_CACHE.agree(ranked[0][1] if ranked else (2, L.MATH_NOHALO))
    d.tile, d.flags = _TUNE_CACHE[key][0], base | _TUNE_CACHE[key][1]


def autotune_program(prog, reps=3):
    for (fname, fn, args) in prog.recs:
        if fname == 'vd_conv_igemm':
            autotune_desc(args[0]._obj, reps)
    _TUNE_CACHE.save()


class Parameter:
    """Gluon-Parameter-like handle (name, shape in the reference's layout, wd_mult, lr_mult, grad_req).  The three
    attributes are live, as in Gluon: `grad_req = 'null'` (wrappers.py:55-57 freeze_base) removes the parameter from the
    backward schedule and from the optimiser (no gradient, no update, no weight decay); `wd_mult` / `lr_mult` scale
    the optimiser's wd / lr for this parameter (train_yolov3.py:495-497 sets wd_mult = 0 with --no_wd)."""

    def __init__(self, net, name, shape, kind, node=None, trainable=True):
        self._net, self.name, self.shape, self.kind, self.node = net, name, tuple(shape), kind, node
        self._wd_mult, self._lr_mult = 1.0, 1.0
        self._grad_req = 'write' if trainable else 'null'
        self.storage = None      # view into an arena (device layout)
        self.grad_storage = None
        self.span = None         # [lo, hi) of the parameter arena (None: not in the arena, e.g. running statistics)

    @property
    def wd_mult(self):
        return self._wd_mult

    @wd_mult.setter
    def wd_mult(self, v):
        self._wd_mult = float(v)
        self._net._opt_ranges = None

    @property
    def lr_mult(self):
        return self._lr_mult

    @lr_mult.setter
    def lr_mult(self, v):
        self._lr_mult = float(v)
        self._net._opt_ranges = None

    @property
    def grad_req(self):
        return self._grad_req

    @grad_req.setter
    def grad_req(self, v):
        if v not in ('write', 'null'):
            raise NotImplementedError("grad_req %r: only 'write' and 'null' are built (the reference uses no 'add')" % (v,))
        if self.span is None and v != 'null':
            raise ValueError("%s is an auxiliary state (no gradient)" % self.name)
        if v != self._grad_req:
            self._grad_req = v
            self._net._grad_req_changed()

    # reference layout <-> device layout (conv weights are kept fwd-packed [Co_pad][T*Ci])
    def _dev_shape(self):
        """shape of the packed image's OIHW form: a consumer of a correlation join reads its input with zero channels
        appended (CorrNode), so its device rows are longer than the reference's by that padding"""
        n = self.node
        if n is None or n.cin == n.ref_cin:
            return self.shape
        return (self.shape[0], n.cin) + self.shape[2:]

    def data(self):
        if self.kind == 'conv_weight':
            shp = self._dev_shape()
            out = torch.empty(shp, device=self.storage.device)
            ops.unpack_weight(self.storage, out)
            return out if shp == self.shape else out[:, :self.shape[1]].contiguous()
        if self.kind == 'stem_weight':
            co = self.shape[0]
            return self.storage.view(co, 32)[:, :27].reshape(co, 3, 3, 3).permute(0, 3, 1, 2).contiguous().view(self.shape)
        if self.kind in ('gru_weight', 'gru_bias'):
            return self._gru_read(self.storage)
        return self.storage[:int(np.prod(self.shape))].view(self.shape).clone()

    # a GRU cell's 3*Ch output channels are three gate blocks (r, z, o); on the device each block is padded to the width
    # the state tensor has (GruNode.chp), and the h2h weight's input channels to the same width - zero rows / columns
    def _gru_read(self, st):
        n = self.node
        ch, chp = n.gate_ch, n.cout // 3
        if self.kind == 'gru_bias':
            return st[:3 * chp].view(3, chp)[:, :ch].reshape(-1).clone()
        full = torch.empty((3 * chp, n.cin) + self.shape[2:], device=st.device)
        ops.unpack_weight(st, full)
        return torch.cat([full[g * chp:g * chp + ch, :n.ref_cin] for g in range(3)], dim=0).contiguous()

    def grad(self):
        if self.kind == 'conv_weight':
            shp = self._dev_shape()
            out = torch.empty(shp, device=self.grad_storage.device)
            ops.unpack_weight(self.grad_storage, out)
            return out if shp == self.shape else out[:, :self.shape[1]].contiguous()
        if self.kind == 'stem_weight':
            co = self.shape[0]
            return self.grad_storage.view(co, 32)[:, :27].reshape(co, 3, 3, 3).permute(0, 3, 1, 2).contiguous().view(self.shape)
        if self.kind in ('gru_weight', 'gru_bias'):
            return self._gru_read(self.grad_storage)
        return self.grad_storage[:int(np.prod(self.shape))].view(self.shape).clone()

    def set_data(self, value):
        v = torch.as_tensor(np.asarray(value.detach().cpu() if torch.is_tensor(value) else value), dtype=torch.float32)
        assert tuple(v.shape) == self.shape, "%s: shape %s != %s" % (self.name, tuple(v.shape), self.shape)
        v = v.to(self.storage.device).contiguous()
        if self.kind == 'conv_weight':
            shp = self._dev_shape()
            if shp != self.shape:                  # the padded input channels get zero weights
                vp = torch.zeros(shp, device=v.device)
                vp[:, :self.shape[1]] = v
                v = vp
            co_pad = self.storage.numel() // (int(np.prod(shp[1:])))
            ops.pack_weight_fwd(v, self.storage, co_pad)
        elif self.kind == 'stem_weight':
            co = self.shape[0]
            tmp = torch.zeros(co, 32, device=v.device)
            tmp[:, :27] = v.reshape(co, 3, 3, 3).permute(0, 2, 3, 1).reshape(co, 27)     # ((co,3,1,3,3): the (1,3,3) stem of Darknet3D)
            self.storage.copy_(tmp.view(-1))
        elif self.kind in ('gru_weight', 'gru_bias'):
            n = self.node
            ch, chp = n.gate_ch, n.cout // 3
            self.storage.zero_()
            if self.kind == 'gru_bias':
                self.storage[:3 * chp].view(3, chp)[:, :ch].copy_(v.view(3, ch))
            else:
                vp = torch.zeros((3 * chp, n.cin) + self.shape[2:], device=v.device)
                for g in range(3):
                    vp[g * chp:g * chp + ch, :n.ref_cin] = v[g * ch:(g + 1) * ch]
                ops.pack_weight_fwd(vp, self.storage, 3 * chp)
        else:
            self.storage.zero_()
            self.storage[:v.numel()].copy_(v.view(-1))
        self._net._params_changed()


class ParameterDict(OrderedDict):
    def reset_ctx(self, ctx=None):     # train_yolov3.py:494 — parameters already live on this rank's GPU
        return None

    def select(self, pattern):
        rx = re.compile(pattern)
        out = ParameterDict()
        for k, v in self.items():
            if rx.match(k):
                out[k] = v
        return out


class ConvNode:
    def __init__(self, name, src, dst, cin, cout, k, stride, div_in, bn=True, residual=None, stem=False, head=False,
                 kd=1, fr=1):
        self.name, self.src, self.dst = name, src, dst
        self.cin, self.cout, self.k, self.stride = cin, cout, k, stride
        self.ref_cin = cin                         # input channels of the reference's weight (< cin behind a CorrNode)
        self.pad = k // 2
        self.kd, self.pad_d = kd, kd // 2          # temporal kernel depth (Conv3D over the K frames of a window)
        self.fr = fr                               # frames per sample carried by this node's tensors (K or 1)
        self.div_in = div_in                       # input spatial = H / div_in
        self.div_out = div_in * stride
        self.bn, self.residual, self.stem, self.head = bn, residual, stem, head
        self.co_pad = round_up(cout, 32) if head else cout
        self.ci_eff = 32 if stem else cin           # stem weights are kept as [32][32]: 27 taps x channels padded to 32
        self.T = 1 if stem else kd * k * k

    def taps(self):
        return [(0, 0, 0)] if self.stem else fwd_taps(self.k, self.pad, self.kd, self.pad_d)

    def weight_shape(self):
        if self.kd > 1 or getattr(self, 'conv3d', False):
            return (self.cout, self.ref_cin, self.kd, self.k, self.k)
        return (self.cout, self.ref_cin, self.k, self.k)


class UpcatNode:
    def __init__(self, name, up, route, dst, cu, cr, div_out, fr=1):
        self.name, self.up, self.route, self.dst, self.cu, self.cr, self.div_out = name, up, route, dst, cu, cr, div_out
        self.fr = fr


class PoolNode:
    """TemporalPooling over the K frames of a window (layers.py:161-205): (B*K, h, w, C) -> (B, h, w, C)."""

    def __init__(self, name, src, dst, K, type_):
        # type 0 = max, 1 = mean, 2 = 'cat' (channel stacking: dst has K * C channels)
        self.name, self.src, self.dst, self.K = name, src, dst, K
        self.type = {'max': 0, 'mean': 1, 'cat': 2}[type_]


class CorrNode:
    """Corr(d, K, kernal_size=1, stride=1, keep='all') over the K frames of a window (layers.py:93-132): (B*K, h, w, C) ->
    (B, h, w, ldy) = [the K frames' channels stacked | one (2d+1)^2-channel correlation map per frame t != K/2 against the
    centre frame | zeros up to ldy = round_up(Cc, 64)] (vd_corr.hip).  The zero tail keeps the channel count of the
    consumers' operand a multiple of 64; their weights carry zero rows there (Parameter._dev_shape)."""

    def __init__(self, name, src, dst, K, d, C_):
        self.name, self.src, self.dst, self.K, self.d, self.C = name, src, dst, K, d, C_
        self.Cc = K * C_ + (K - 1) * (2 * d + 1) ** 2
        self.ldy = round_up(self.Cc, 64)


class GruNode:
    """RNN(k, type='gru', channels=ch, kernel=(s, s), bi=True) over the K frames of a window (layers.py:267-306; the cell is
    restated from MXNet's Conv2DGRUCell / BidirectionalCell): (B*K, h, w, cin) -> (B*K, h, w, chp), frame t
    of the output = (hl_t + hr_t) / 2 of two independent cells run forwards and backwards in time.  Each cell owns two
    bias-only convolutions (i2h on the K frames at once, h2h on one step's state), kept as ConvNodes outside the node list
    so that the arena, the max-abs slots, the optimiser ranges and the gradient buckets treat them like any conv; their
    3*ch output channels are three gate blocks (r, z, o), each padded to chp on the device (zero rows, zero bias)."""

    def __init__(self, name, pname, src, dst, K, cin, ch, ksz, div, chp):
        self.name, self.pname, self.src, self.dst, self.K = name, pname, src, dst, K
        self.cin, self.ch, self.chp, self.k, self.div = cin, ch, chp, ksz, div
        self.cells = []
        for cname in ('l_cell', 'r_cell'):
            i2h = ConvNode("%s.%s.i2h" % (pname, cname), src, "gru:%s.%s.I" % (name, cname), cin, 3 * chp, ksz, 1, div, bn=False, fr=K)
            # (fr = K: the weight-gradient launch over the frames that had a state bounds the workspace sizes)
            h2h = ConvNode("%s.%s.h2h" % (pname, cname), None, "gru:%s.%s.H" % (name, cname), chp, 3 * chp, ksz, 1, div, bn=False, fr=K)
            h2h.ref_cin = ch
            for cn, kind in ((i2h, 'i2h'), (h2h, 'h2h')):
                cn.gru, cn.gate_ch = self, ch
                cn.pw, cn.pb = "%s.%s.%s_weight" % (pname, cname, kind), "%s.%s.%s_bias" % (pname, cname, kind)
            self.cells.append((cname, i2h, h2h))

    def key(self, cname, what):
        return "gru:%s.%s.%s" % (self.name, cname, what)


class SelNode:
    """x.slice_axis(axis=1, begin=k0, end=k0+kc) on folded frames (yolo3_temporal.py:437-446): frames [k0, k0+kc) of every
    K-frame window of `src` -> `dst` (kc frames per window)."""

    def __init__(self, name, src, dst, K, k0, kc):
        self.name, self.src, self.dst, self.K, self.k0, self.kc = name, src, dst, K, k0, kc


class AddNode:
    """dst = a + b (yolo3_temporal.py:440,445: the per-frame stage output plus the strided 2+1-D side branch)."""

    def __init__(self, name, a, b, dst, fr):
        self.name, self.a, self.b, self.dst, self.fr = name, a, b, dst, fr


class TdwNode:
    """The temporal half of the backbone's _conv21d cell (three_darknet.py:19-38,41-70): Conv3DRepPad, a depthwise (3,1,1)
    conv over the K frames of a window with repeat padding (front: frame 0, tail: frame K-2), no bias, and NO BatchNorm or
    activation behind it (:36).  (B*K, h, w, C) -> (B*K, h, w, C), + `residual` when it closes a DarknetBasicBlockV3
    (:120-123).  One streaming kernel each way (vd_tdw.hip).  Its weight (C,1,3,1,1) lives in the weight range of the arena
    behind the conv weights: weight decay, --no_wd, lr_mult, grad_req and the optimiser treat it as a weight."""

    def __init__(self, name, pname, src, dst, C_, div, K, residual=None):
        self.name, self.pname, self.src, self.dst, self.C, self.div, self.K, self.residual = name, pname, src, dst, C_, div, K, residual
        self.fr = K


# ---- graph analysis: pure functions of the node list (no device)
def node_inputs(n):
    """The tensors node n reads, in the order its operands are named."""
    if isinstance(n, (ConvNode, TdwNode)):
        ins = [n.src, n.residual]
    elif isinstance(n, UpcatNode):
        ins = [n.up, n.route]
    elif isinstance(n, AddNode):
        ins = [n.a, n.b]
    else:                                          # PoolNode, CorrNode, SelNode, GruNode
        ins = [n.src]
    return [t for t in ins if t]


def consumers_of(nodes):
    """tensor -> the nodes that read it, in node order (the first entry is the earliest forward consumer)"""
    out = {}
    for m in nodes:
        for t in node_inputs(m):
            out.setdefault(t, []).append(m)
    return out


def single_conv_consumers(nodes):
    """the rule of YOLOV3.single_conv_consumer_tensors: BatchNorm cells without residual (the stem and the routes apart)
    whose output has exactly one read, as the operand of a convolution"""
    use = consumers_of(nodes)
    return {n.dst for n in nodes if isinstance(n, ConvNode) and n.bn and not n.residual and not n.stem
            and len(use.get(n.dst, ())) == 1 and isinstance(use[n.dst][0], ConvNode) and use[n.dst][0].src == n.dst
            and n.dst not in [r[0] for r in ROUTE_TENSORS]}


def grad_required(nodes, trainable, is_input):
    """tensor -> whether backward has to produce its gradient.  grad_req 'null' (wrappers.py:55-57): a tensor needs a
    gradient only if a trainable parameter sits in its producer or anywhere upstream of it.  With the backbone frozen
    nothing below the three route tensors does, so the whole backbone drops out of the backward schedule (as MXNet's
    autograd prunes it) and its weight-gradient launches never run.  `trainable(c)`: a ConvNode (a GruNode's cell convs
    included) or a TdwNode owns a trainable parameter; `is_input(t)`: t is a network input, the only tensors that may be
    read without a producer."""
    need = {}
    for m in nodes:
        ins = node_inputs(m)
        for t in ins:
            if t not in need:
                assert is_input(t), "%s reads %s, which nothing produces" % (m.name, t)
                need[t] = False
        if isinstance(m, GruNode):
            own = any(trainable(cn) for _, i2h, h2h in m.cells for cn in (i2h, h2h))
        else:
            own = isinstance(m, (ConvNode, TdwNode)) and trainable(m)
        need[m.dst] = bool(own or any(need[t] for t in ins))
    return need


def check_conv_types(conv_types, k):
    """--conv_types: six integers, the stem then the five stages (three_darknet.py:152-199,243-244).  Returns None for the
    plain 2-D network (all 2), the list for a Darknet3D with a non-empty prefix of 21; everything else is refused by name."""
    if conv_types is None:
        return None
    try:
        ct = [int(c) for c in conv_types]
    except (TypeError, ValueError):
        raise NotImplementedError("conv_types %r: six integers out of 2 and 21 are built" % (conv_types,))
    if len(ct) != 6:
        raise NotImplementedError("conv_types needs 6 entries (the stem and the five stages), got %d: %r" % (len(ct), ct))
    if any(c == 3 for c in ct):
        raise NotImplementedError("conv_types 3 (3x3x3 convolutions in the backbone, an 81-tap stem) is outside the built "
                                  "scope; 2 and 21 are built: %r" % (ct,))
    if any(c not in (2, 21) for c in ct):
        raise NotImplementedError("conv_types entries must be 2 or 21, got %r" % (ct,))
    if all(c == 2 for c in ct):
        return None
    n21 = ct.index(2) if 2 in ct else 6
    if n21 == 0 or any(c == 21 for c in ct[n21:]):
        raise NotImplementedError("conv_types %r: a 21 after a 2 - the trunk is pooled over time once, where the 2-D stages "
                                  "begin (three_darknet.py:174-176), so the 21 entries must be a prefix" % (ct,))
    if not (k and int(k) >= 2):
        raise NotImplementedError("conv_types %r needs a window of K >= 2 frames (k = %r): K = 1 is refused, the tail pad of "
                                  "the temporal conv is frame K-2 (three_darknet.py:62)" % (ct, k))
    return ct


def _darknet3d_trunk(nodes, T, tensors, conv_types, K):
    """Darknet3D with return_features=True (three_darknet.py:152-226) on windows of K frames folded into the batch.  The
    parameter names are YOLOV3TB's `d_model.features.{i}`; the temporal pool occupies an index of `features` (:176), so the
    indices behind it are the 2-D network's plus one.  Returns the routes a, b, c (single-frame maps, :205-226)."""
    feat = lambda i: "d_model.features.%d" % i

    def cell21(name, src, dst, cin, cout, stride, div, residual=None, stem=False):
        """_conv21d(cout, 3, 1, strides) (:19-38): (1,3,3) conv + BN + LeakyReLU on every frame, then the temporal conv"""
        sp = T(dst + '.s', cout, div * stride, fr=K)
        n1 = ConvNode(name, src, sp, cin, cout, 3, stride, div, stem=stem, fr=K)
        n1.conv3d = True
        nodes.append(n1)
        out = T(dst, cout, div * stride, fr=K)
        n1.tdw = TdwNode('tdw.' + dst, name + ".3.conv.weight", sp, out, cout, div * stride, K, residual)
        nodes.append(n1.tdw)
        return out

    T('in', 3, 1, fr=K)
    cur = cell21(feat(0), 'in', 'f0', 3, 32, 1, 1, stem=True)
    idx, div, fr = 1, 1, K
    routes = []

    def pool_trunk():
        nxt = T(cur + '.pool', tensors[cur][0], div)
        pn = PoolNode('pool.trunk', cur, nxt, K, 'max')
        pn.feature_index = idx
        nodes.append(pn)
        if routes and routes[-1] == cur:            # conv_swap == 4 (:211-214): the pool is the last feature of route a
            routes[-1] = nxt
        return nxt

    for gi, (nlayer, ch) in enumerate(zip([1, 2, 8, 8, 4], [64, 128, 256, 512, 1024])):
        t21 = conv_types[gi + 1] == 21
        if not t21 and fr > 1:                                                       # :174-176
            cur, fr, idx = pool_trunk(), 1, idx + 1
        if t21:
            cur = cell21(feat(idx), cur, 'f%d' % idx, ch // 2, ch, 2, div)           # :187-189, strides (1,2,2)
        else:
            nxt = T('f%d' % idx, ch, div * 2)
            nodes.append(ConvNode(feat(idx), cur, nxt, ch // 2, ch, 3, 2, div))
            cur = nxt
        div, idx = div * 2, idx + 1
        for _ in range(nlayer):                                                      # DarknetBasicBlockV3 (:100-123)
            mid = T('f%d.m' % idx, ch // 2, div, fr=fr)
            n0 = ConvNode(feat(idx) + ".body.0", cur, mid, ch, ch // 2, 1, 1, div, fr=fr)
            n0.conv3d = t21                          # _conv3d 1x1x1: per-frame arithmetic, 5-D weight
            nodes.append(n0)
            if t21:
                cur = cell21(feat(idx) + ".body.1", mid, 'f%d' % idx, ch // 2, ch, 1, div, residual=cur)
            else:
                nxt = T('f%d' % idx, ch, div)
                nodes.append(ConvNode(feat(idx) + ".body.1", mid, nxt, ch // 2, ch, 3, 1, div, residual=cur))
                cur = nxt
            idx += 1
        if gi >= 2:
            routes.append(cur)
    if fr > 1:                                                                       # :197-199 the whole trunk was 2+1-D
        cur = pool_trunk()
        routes[-1] = cur
    for i, r in enumerate(routes):                   # :219,224-225 a route that left the trunk with K frames: its own max
        if tensors[r][3] > 1:
            pr = T('route%d.pool' % i, tensors[r][0], tensors[r][1])
            nodes.append(PoolNode('pool.route%d' % i, r, pr, K, 'max'))
            routes[i] = pr
    return routes


def _feature_name(f):
    if f < 15:
        return "stages.0.%d" % f
    if f < 24:
        return "stages.1.%d" % (f - 15)
    return "stages.2.%d" % (f - 24)


ROUTE_TENSORS = (('f14', 256, 8), ('f23', 512, 16), ('f28', 1024, 32))   # features[:15], [15:24], [24:] (wrappers.py:58)


def build_graph(num_class, k=1, k_join_type=None, k_join_pos=None, block_conv_type='2', noback=False,
                temporal_out=False, temporal_side=False, corr_pos=None, corr_d=0, rnn_pos=None, conv_types=None, frames=1):
    """Node list of YOLOV3T over Darknet-53 (wrappers.py:54-58,101-103; three_darknet.py:252-258;
    yolo3.py:1003-1054 wiring, :1095-1177 forward).  k>1: the backbone is TimeDistributed (K frames folded
    into the batch, layers.py:241-250); 'early' joins pool each stage output over K, 'late' joins keep K frames
    through the neck (2-D blocks per frame, or 3-D / 2+1-D convs across the K axis, yolo3.py:229-262) and pool
    the tips right before the prediction convs (:1134-1138)."""
    nodes, tensors = [], OrderedDict()     # tensors[name] = (channels, div, pitch, frames)
    K = k if k and k > 1 else 1
    # temporal_out = YOLOV3Temporal with t_out (yolo3_temporal.py:396-470, corr_d = 0): every one of the t frames runs
    # through the backbone, the detection blocks (per frame, or 3-D / 2+1-D convs across the t axis) and its OWN
    # prediction convs - no join; TimeDistributed wrappers are created inside hybrid_forward there, so parameter
    # names carry no `.model`
    # temporal_side = YOLOV3Temporal with t_out=False (yolo3_temporal.py:326-333,436-447): the three Darknet stages run on
    # 5, 3 and 1 frames of the window; strided 2+1-D side branches (convs1 / convs2: a per-frame 3x3 stride-2 conv, then a
    # (3,1,1) conv WITHOUT temporal padding, 5 -> 3 and 3 -> 1 frames) carry the neighbours' features down and are added to
    # the stage outputs; the routes are the centre frames and the neck / heads are the plain single-frame ones.
    # corr_pos (yolo3.py:1112-1113,1139-1140): the reference's `elif` - a correlation join replaces the pooling / stacking
    # at the same place when no k_join_pos is given
    corr = K > 1 and k_join_pos is None and corr_pos is not None and not temporal_out and not temporal_side
    if corr:
        k_join_pos = corr_pos
    # rnn_pos (yolo3.py:1022-1030,1040-1042,1128-1138): 'late' - the block has no tip cell, a 3x3 bidirectional ConvGRU over
    # the K frames takes its place and the late join follows; 'out' - the neck runs per frame whatever k_join_pos says (the
    # early / late joins are guarded by `_rnn_pos != 'out'`), a 1x1 ConvGRU replaces the prediction conv and TemporalPooling
    # joins the K predictions
    rnn = rnn_pos if K > 1 and not temporal_out and not temporal_side else None
    late = K > 1 and (k_join_pos == 'late' or temporal_out or rnn == 'out')
    td_names = K > 1 and not temporal_out and not temporal_side
    pad_of = {}                            # zero channels at the end of a tensor built from a correlation join

    def corr_join(name, src, c_, d_):
        n_ = CorrNode('corr.' + name, src, name + '.corr', K, corr_d, c_)
        dst = T(n_.dst, n_.ldy, d_)
        nodes.append(n_)
        pad_of[dst] = n_.ldy - n_.Cc
        return dst, n_.ldy

    def T(name, c, div, ld=None, fr=1):
        tensors[name] = (c, div, c if ld is None else ld, fr)
        return name

    def sname(f):
        nm = _feature_name(f)
        if td_names:
            head, idx = nm.rsplit(".", 1)
            nm = "%s.model.%s" % (head, idx)
        return nm

    routes = []
    d3 = conv_types is not None
    if d3:
        # yolo3_3ddarknet (wrappers.py:113-130): Darknet3D on windows of `frames` frames, then YOLOV3TB with k = 1
        assert K == 1 and not noback and not temporal_out and not temporal_side
        routes = _darknet3d_trunk(nodes, T, tensors, conv_types, frames)
    elif noback:
        # YOLOV3_noback (yolo3.py:1730-1840): the three backbone feature maps are the inputs (net(x1, x2, x3)); only
        # transitions / yolo_blocks / yolo_outputs exist, under the same structural names as in the full network
        assert K == 1, "YOLOV3_noback has no temporal window"
        routes = [T(nm, c_, d_) for nm, c_, d_ in ROUTE_TENSORS]
    else:
        T('in', 3, 1, fr=K)
        cur = T('f0', 32, 1, fr=K)
        nodes.append(ConvNode(sname(0), 'in', cur, 3, 32, 3, 1, 1, stem=True, fr=K))
    f = 1
    div = 1
    sfr = K                                # frames the current Darknet stage runs on
    side = None                            # output of the side branch to add to the next stage output

    def side_branch(i, src, cin, cout, d, fr):
        """convs{i} = _conv21d(channel=cout, t=3, d=3, m=cin, padding=[1,0], stride=[(1,2,2),1]) on `src` (fr frames)."""
        sp = T('cx%d.s' % i, cin, d * 2, fr=fr)
        n1 = ConvNode("convs%d.0.0" % i, src, sp, cin, cin, 3, 2, d, fr=fr)        # (1,3,3) stride (1,2,2), BN + LeakyReLU
        n1.conv3d = True
        nodes.append(n1)
        out = T('cx%d' % i, cout, d * 2, fr=fr - 2)
        n2 = ConvNode("convs%d.0.1" % i, sp, out, cin, cout, 1, 1, d * 2, kd=3, fr=fr)   # (3,1,1), no temporal padding
        n2.tvalid = True
        nodes.append(n2)
        return out

    for gi, (nlayer, ch) in enumerate(zip([] if (noback or d3) else [1, 2, 8, 8, 4], [64, 128, 256, 512, 1024])):
        if temporal_side and gi in (3, 4):
            i = gi - 2                                                               # side branch 1 / 2
            if gi == 3:
                routes.append(T('r0', tensors[cur][0], div))
                nodes.append(SelNode('sel.r0', cur, 'r0', sfr, 2, 1))                # :437 the centre frame
            side = side_branch(i, cur, tensors[cur][0], ch, div, sfr)
            if gi == 3:
                nxt = T(cur + '.s', tensors[cur][0], div, fr=3)
                nodes.append(SelNode('sel.s1', cur, nxt, sfr, 1, 3))                 # :439 frames 1..3
                cur, sfr = nxt, 3
            else:
                cur, sfr = routes[1], 1                                              # :444 frame 1 of 3 (= route 1)
        nxt = T('f%d' % f, ch, div * 2, fr=sfr)
        nodes.append(ConvNode(sname(f), cur, nxt, ch // 2, ch, 3, 2, div, fr=sfr))
        cur, div, f = nxt, div * 2, f + 1
        for _ in range(nlayer):
            mid = T('f%d.m' % f, ch // 2, div, fr=sfr)
            nxt = T('f%d' % f, ch, div, fr=sfr)
            nm = sname(f)
            nodes.append(ConvNode(nm + ".body.0", cur, mid, ch, ch // 2, 1, 1, div, fr=sfr))
            nodes.append(ConvNode(nm + ".body.1", mid, nxt, ch // 2, ch, 3, 1, div, residual=cur, fr=sfr))
            cur, f = nxt, f + 1
        if temporal_side and gi in (3, 4):
            nxt = T(cur + '.a', ch, div, fr=sfr)
            nodes.append(AddNode('add.%d' % (gi - 2), cur, side, nxt, sfr))          # :440,445 x = x + cx
            cur = nxt
            if gi == 3:
                routes.append(T('r1', ch, div))
                nodes.append(SelNode('sel.r1', cur, 'r1', 3, 1, 1))                  # :441 the middle of the three
            else:
                routes.append(cur)                                                   # :446 squeeze: one frame left
        elif f in (15, 24, 29) and not temporal_side:
            routes.append(cur)
    nfr = K if late else 1                 # frames carried through the neck
    if K > 1 and not late and not temporal_side:      # 'early' join (yolo3.py:1107-1124): pool every route over K
        pooled = []
        for i, r in enumerate(routes):
            c_, d_ = tensors[r][0], tensors[r][1]
            if corr:
                pooled.append(corr_join('route%d' % i, r, c_, d_)[0])
                continue
            pr = T('route%d.pool' % i, c_ * (K if k_join_type == 'cat' else 1), d_)
            nodes.append(PoolNode('pool.route%d' % i, r, pr, K, k_join_type))
            pooled.append(pr)
        routes = pooled
    # neck + heads, deepest first (yolo3.py:1013-1054, 1126-1177)
    A = 3 * (5 + num_class)
    x, xc = routes[2], tensors[routes[2]][0]
    heads = []
    conv3 = block_conv_type in ('3', '21')
    for i, c in enumerate([512, 256, 128]):
        d = 32 >> i
        if conv3:
            pre, cell = "yolo_blocks.%d" % i, ".conv"           # Conv wrapper registers `.conv` (layers.py:135-158)
        elif late and td_names:
            pre, cell = "yolo_blocks.%d.model" % i, ""           # TimeDistributed(block)
        else:
            pre, cell = "yolo_blocks.%d" % i, ""

        def add_cell(name, src, dst_name, cin, cout, ksz):
            """one Conv+BN+LeakyReLU cell of the detection block; 3x3 cells become 3x3x3 ('3') or
            (1,3,3)+(3,1,1) ('21') across the K frames when block_conv_type asks for it"""
            if conv3 and ksz == 3 and block_conv_type == '3':
                dst = T(dst_name, cout, d, fr=nfr)
                nodes.append(ConvNode(name + cell, src, dst, cin, cout, 3, 1, d, kd=3, fr=nfr))
                return dst
            if conv3 and ksz == 3:       # R(2+1)D: spatial then temporal, each with BN + LeakyReLU (layers.py:82-89)
                mid = T(dst_name + ".s", cout, d, fr=nfr)
                n1 = ConvNode(name + cell + ".0", src, mid, cin, cout, 3, 1, d, fr=nfr)
                n1.conv3d = True
                nodes.append(n1)
                dst = T(dst_name, cout, d, fr=nfr)
                n2 = ConvNode(name + cell + ".1", mid, dst, cout, cout, 1, 1, d, kd=3, fr=nfr)
                nodes.append(n2)
                return dst
            dst = T(dst_name, cout, d, fr=nfr)
            n1 = ConvNode(name + cell, src, dst, cin, cout, ksz, 1, d, fr=nfr)
            n1.conv3d = conv3              # 1x1x1 Conv3D: same arithmetic as the per-frame 1x1, 5-D weight
            nodes.append(n1)
            return dst

        for j in range(5):
            cout = c if j % 2 == 0 else 2 * c
            x = add_cell("%s.body.%d" % (pre, j), x, 'n%d.b%d' % (i, j), xc, cout, 1 if j % 2 == 0 else 3)
            xc = cout
        route = x
        if rnn == 'late':
            tip = T('n%d.tip' % i, 2 * c, d, fr=K)
            nodes.append(GruNode('rnn.tip%d' % i, "yolo_tips.%d.tip.rnn" % i, route, tip, K, c, 2 * c, 3, d, 2 * c))
        else:
            tip = add_cell(pre + ".tip", route, 'n%d.tip' % i, c, 2 * c, 3)
        tipc = 2 * c
        if rnn == 'out':
            # YOLOOutputV3 with rnn_shape (yolo3.py:58-60,152-155): the K tips -> K predictions -> TemporalPooling
            Ap = round_up(A, 32)
            pr = T('n%d.rnn' % i, A, d, Ap, fr=K)
            nodes.append(GruNode('rnn.out%d' % i, "yolo_outputs.%d.prediction.rnn" % i, tip, pr, K, 2 * c, A, 1, d, Ap))
            hd = T('head%d' % i, A, d, Ap)
            nodes.append(PoolNode('pool.head%d' % i, pr, hd, K, k_join_type))
            heads.append(hd)
        elif late and not temporal_out and corr:                  # yolo3.py:1139-1140: correlation join of the tip
            tip, tipc = corr_join('n%d.tip' % i, tip, 2 * c, d)
        elif late and not temporal_out:                         # yolo3.py:1134-1138: join the tip over K
            tipc = 2 * c * (K if k_join_type == 'cat' else 1)
            ptip = T('n%d.tip.pool' % i, tipc, d)
            nodes.append(PoolNode('pool.tip%d' % i, tip, ptip, K, k_join_type))
            tip = ptip
        if rnn != 'out':
            hfr = K if temporal_out else 1                      # per-frame predictions (TimeDistributed(output))
            hd = T('head%d' % i, A, d, round_up(A, 32), fr=hfr)
            nodes.append(ConvNode("yolo_outputs.%d.prediction" % i, tip, hd, tipc, A, 1, 1, d, bn=False, head=True, fr=hfr))
            heads.append(hd)
        if i < 2:
            tr = T('n%d.tr' % i, c // 2, d, fr=nfr)
            nodes.append(ConvNode("transitions.%d%s" % (i, ".model" if (late and td_names) else ""), route, tr, c, c // 2,
                                  1, 1, d, fr=nfr))
            rt = routes[1 - i]
            rc = tensors[rt][0]
            cat = T('n%d.cat' % i, c // 2 + rc, d // 2, fr=nfr)
            if rt in pad_of:                                    # [upsampled transition | route], padding stays at the end
                pad_of[cat] = pad_of[rt]
            nodes.append(UpcatNode("upcat.%d" % i, tr, rt, cat, c // 2, rc, d // 2, fr=nfr))
            x, xc = cat, c // 2 + rc
    for n in nodes:
        if isinstance(n, ConvNode) and n.src in pad_of:        # every consumer of a correlation join is a 1x1 cell
            assert n.k == 1 and n.kd == 1 and not getattr(n, 'conv3d', False), n.name
            n.ref_cin = n.cin - pad_of[n.src]
    return nodes, tensors, heads


class YOLOV3(object):
    """The network object the reference's loops drive (net(x) / net(x, *targets), set_nms, reset_class,
    collect_params, save/load_parameters, hybridize, initialize).  k=1 (YOLOV3T with k=1 == YOLOV3)."""

    def __init__(self, classes, nms_thresh=0.45, nms_topk=400, post_nms=100, ignore_iou_thresh=0.7,
                 device="cuda", syncbn_scope=None, process_group=None, k=1, k_join_type=None, k_join_pos=None,
                 block_conv_type='2', noback=False, temporal_out=False, temporal_side=False, corr_pos=None, corr_d=0,
                 rnn_pos=None, conv_types=None, agnostic=False):
        self._classes = list(classes)
        # class-agnostic detection (YOLOOutputV3(agnostic=True), yolo3.py:184-188): inference emits one candidate per anchor
        # (id 0, score = sigmoid(objectness)) into the same box_nms.  The branch sits behind `if autograd.is_training()`, so
        # the graph, the parameters and training are those of agnostic=False; only the decode + NMS tail of the inference
        # plans differs (infer_plan.InferPlan.detect_tail)
        self.agnostic = bool(agnostic)
        if self.agnostic:
            if conv_types is not None and check_conv_types(conv_types, k) is not None:
                raise NotImplementedError("agnostic with conv_types: detect_yolo3.py builds yolo3_3ddarknet without the flag "
                                          "(detect_yolo3.py:872-882); the class-agnostic tail is built for yolo3_darknet53")
            if rnn_pos == 'out':
                raise NotImplementedError("agnostic with rnn_pos 'out': its predictions come from YOLOOutputV3's own RNN "
                                          "output block (yolo3.py:1040-1042), a tail of its own that is not built agnostic")
            if temporal_out or temporal_side:
                raise NotImplementedError("agnostic with temporal / t_out: YOLOV3Temporal is not passed the flag "
                                          "(wrappers.py:96-98)")
            if noback:
                raise NotImplementedError("agnostic with the no-backbone network: YOLOV3_noback has no agnostic argument "
                                          "(wrappers.py:133-161)")
        # Darknet3D backbone on windows of k frames (yolo3_3ddarknet, wrappers.py:113-130): the neck and heads are the plain
        # single-frame ones (YOLOV3TB with k = 1), so nothing that joins or mixes frames behind the backbone combines with it
        self._conv_types = check_conv_types(conv_types, k)
        if self._conv_types is not None and (k_join_type or k_join_pos or block_conv_type != '2' or noback or temporal_out or
                                             temporal_side or corr_pos is not None or rnn_pos is not None):
            raise NotImplementedError("conv_types %r builds yolo3_3ddarknet, whose neck is the single-frame one: k_join_type / "
                                      "k_join_pos, block_conv_type, corr_pos, rnn_pos, temporal and the no-backbone network do "
                                      "not combine with it" % (self._conv_types,))
        # bidirectional ConvGRU (RNN, layers.py:267-306).  What the factory refuses is refused here too: nothing is dropped
        if rnn_pos is not None:
            if rnn_pos not in ('late', 'out'):
                raise ValueError("rnn_pos must be None, 'late' or 'out', got %r" % (rnn_pos,))
            if not (k and k > 1) or noback or temporal_out or temporal_side or block_conv_type != '2' or corr_pos is not None \
                    or (rnn_pos == 'late' and (k_join_pos != 'late' or k_join_type not in ('max', 'mean', 'cat'))) \
                    or (rnn_pos == 'out' and k_join_type not in ('max', 'mean')):
                raise NotImplementedError("rnn_pos %r needs a window k > 1 of the plain YOLOV3T network with block_conv_type '2', "
                                          "no corr_pos, and a late max / mean / cat join ('late') or a max / mean join ('out'); "
                                          "yolo3_darknet53() names the reason for each" % (rnn_pos,))
        self._rnn_pos = rnn_pos
        self._corr_pos, self._corr_d = corr_pos, int(corr_d or 0)   # correlation join (Corr, layers.py:93-132)
        self.temporal_side = bool(temporal_side)  # YOLOV3Temporal(t_out=False): strided 2+1-D side branches, one output
        self.temporal_out = bool(temporal_out)   # YOLOV3Temporal(t_out=True): per-frame detections / losses
        self._grad_scale = 1.0                   # d(reported loss)/d(sum of per-sample losses), see _forward_train
        self.noback = bool(noback)               # YOLOV3_noback: net(x1, x2, x3[, targets]) on cached backbone features
        self._k = k if k and k > 1 else 1
        self._k_join_type, self._k_join_pos, self._block_conv_type = k_join_type, k_join_pos, block_conv_type
        self.nms_thresh, self.nms_topk, self.post_nms = nms_thresh, nms_topk, post_nms
        self._ignore_iou_thresh = ignore_iou_thresh
        self._label_smooth = False
        self._target_generator = self            # train_yolov3.py:499-500 pokes net._target_generator._label_smooth
        self.device = torch.device(device)
        self.syncbn_scope = syncbn_scope         # None | 'reference' | 'all'
        self.process_group = process_group
        self._training = False
        self._recording = False
        self._programs = {}
        self._sk_ws = {}           # stream-K hand-off workspaces by stream index (_set_streamk)
        self._range_exact = set()  # operand tensors whose consumers never run the fp16-split arithmetic (see _build)
        self._fold_dirty = True
        self._stats_version = 1          # bumped whenever the BatchNorm running statistics move
        self._weights_version = 1        # bumped whenever the weights move; each training plan packs its own data-gradient
        self._pack_stream = None         # weight layouts and remembers the version they were packed from
        self._pack_event = None
        self._graph_cache = {}
        self._live = None                # the VideoSession with frames in flight, if any (open_video)
        self.use_graphs = False
        self.overlap_wgrad = os.environ.get('VD_OVERLAP', '1') != '0'   # wgrad GEMMs on a side stream (_build_train)
        self.fuse_bn_stats = os.environ.get('VD_FUSE_STATS', '1') != '0'  # BN statistics in the conv epilogue
        self.precision = 'fp32'        # inference precision: 'fp32' | 'bf16' (set_precision)
        self._dev_resize = None        # (height, width, interp): raw uint8 frames are resized on the device (set_device_resize)
        self._resize_cache = {}        # (H0, W0, H, W, interp) -> the tap tables of that resize, host and device
        self._dev_nv12 = None          # set_device_resize(source='nv12'): the seven integers of video.NV12_MATRICES[(matrix, range)]
        self.bucketed_allreduce = os.environ.get('VD_BUCKETED', '1') != '0'
        self.alias_skip_grad = os.environ.get('VD_ALIAS_SKIP', '1') != '0'    # skip gradients by alias, not by copy
        self.fuse_bn_bwd = os.environ.get('VD_FUSE_BWD', '1') != '0'          # BN backward reductions in the dgrad epilogue
        # fp32 gradients per all-reduce.  The tail bucket (everything below stage 4: ~15 M parameters, the layers whose
        # gradients come last) closes with the stem and is the one collective nothing overlaps, so buckets are kept at
        # 32 MB: large enough for the ring to reach its bandwidth, small enough that the exposed tail stays ~30 MB.
        self.bucket_elems = int(float(os.environ.get('VD_BUCKET_MB', '32')) * (1 << 18))
        self._pending_reduces = []
        self._reduced_from = 1 << 62
        self._dp_stats = {'buckets': 0, 'bucket_bytes': 0}     # all-reduce buckets queued since the last reset (bench.py)
        self._bucket_group = None      # second communicator for the gradient buckets when SyncBN collectives exist
        self._build(len(self._classes))

    # ------------------------------------------------------------------ construction
    def _build(self, num_class):
        self.num_class = num_class
        self.nodes, self.tensors, self.head_names = build_graph(num_class, 1 if self._conv_types else self._k, self._k_join_type,
                                                                self._k_join_pos, self._block_conv_type,
                                                                noback=self.noback, temporal_out=self.temporal_out,
                                                                temporal_side=self.temporal_side, corr_pos=self._corr_pos,
                                                                corr_d=self._corr_d, rnn_pos=self._rnn_pos,
                                                                conv_types=self._conv_types, frames=self._k)
        self._head_frames = self._k if self.temporal_out else 1
        self.input_tensors = [nm for nm, _, _ in ROUTE_TENSORS] if self.noback else ['in']
        self.gru_nodes = [n for n in self.nodes if isinstance(n, GruNode)]
        self.tdw_nodes = [n for n in self.nodes if isinstance(n, TdwNode)]
        # (a GruNode's four convolutions take their place in the arena order where the node stands)
        self.conv_nodes = [m for n in self.nodes for m in ([n] if isinstance(n, ConvNode) else
                                                           [cn for _, i2h, h2h in n.cells for cn in (i2h, h2h)] if isinstance(n, GruNode) else [])]
        # The loss gradient (dhead: (sigmoid - target) x mask) is sparse and saturated - after a few hundred steps most of its
        # entries sit 2^20 .. 2^30 below its largest ones, and an output of its consumers that reads only such entries (a
        # background pixel of the data gradient) would be formed from operands the fp16 split has staged with a handful of
        # bits.  Its consumers - the data and weight gradients of the three prediction convs, 2 % of the step's FLOPs - are
        # therefore range-exact BY CONSTRUCTION (3-way bf16 split / fp32 MFMA), never chosen by timing.  Every other operand
        # tensor is dense; those join this set through check_operand_ranges() when their channel scales spread too far.
        self._range_exact = set('dz:' + n.name for n in self.conv_nodes if n.head)
        # A correlation join's output mixes frame features with cost-volume maps (products of two features / C): no single
        # BatchNorm bounds its channel scales.  So the convs that read it - directly or through the concatenation behind a
        # transition, which the closure below reaches - are range-exact by construction as well (forward and weight
        # gradient: both take it as their operand).
        self._range_exact |= {n.dst for n in self.nodes if isinstance(n, CorrNode)}
        self._close_range_exact()
        self._guard = None
        # arena layout: [conv weights (fwd-packed) | bn gamma, beta, head bias]  -> wd / no_wd ranges
        off = 0
        for n in self.conv_nodes:
            n.w_off = off
            n.w_numel = n.co_pad * n.T * n.ci_eff
            off += round_up(n.w_numel, 64)
        self.n_wconv = off                           # end of the conv weights; the temporal depthwise weights follow them
        for n in self.tdw_nodes:
            n.w_off, n.w_numel = off, 3 * n.C
            off += round_up(n.w_numel, 64)
        self.n_weight = off
        for n in self.conv_nodes:
            if n.bn:
                n.gamma_off, n.beta_off = off, off + round_up(n.cout, 64)
                off += 2 * round_up(n.cout, 64)
            else:
                n.bias_off = off
                off += round_up(n.co_pad, 64)
        self.n_params = off
        dev = self.device
        self.weights = torch.zeros(off, device=dev)
        self.grads = torch.zeros(off, device=dev)
        self.momentum_buf = torch.zeros(off, device=dev)
        soff = 0
        for n in self.conv_nodes:
            if n.bn:
                n.stat_off = soff
                soff += 2 * round_up(n.cout, 64)
        self.running = torch.zeros(max(soff, 1), device=dev)
        # max-abs of every conv weight tensor (operand scale of the VD_MATH_F16X2 arithmetic): one slot set per conv,
        # refreshed by ONE launch whenever the weights moved (_refresh_wamax)
        self._wamax = torch.zeros(len(self.conv_nodes) * L.AMAX_FLOATS, device=dev)
        self._wamax_seg = torch.tensor([[n.w_off, n.w_numel] for n in self.conv_nodes], dtype=torch.int64, device=dev)
        for i, n in enumerate(self.conv_nodes):
            n.wamax = self._wamax[i * L.AMAX_FLOATS:(i + 1) * L.AMAX_FLOATS]
        self._wamax_dirty = True
        # per-node derived buffers: folded scale/shift (eval) and batch scale/shift/mean/invstd (train)
        self.aux = torch.zeros(max(1, sum(6 * round_up(n.cout, 64) for n in self.conv_nodes if n.bn)), device=dev)
        self.sums = torch.zeros(max(1, sum(4 * round_up(n.cout, 64) for n in self.conv_nodes)), dtype=torch.float64,
                                device=dev)
        aoff = doff = 0
        for n in self.conv_nodes:
            c64 = round_up(n.cout, 64)
            if n.bn:
                v = self.aux[aoff:aoff + 6 * c64]
                n.fold_scale, n.fold_shift = v[0:n.cout], v[c64:c64 + n.cout]
                n.b_scale, n.b_shift = v[2 * c64:2 * c64 + n.cout], v[3 * c64:3 * c64 + n.cout]
                n.b_mean, n.b_invstd = v[4 * c64:4 * c64 + n.cout], v[5 * c64:5 * c64 + n.cout]
                aoff += 6 * c64
            n.sums = self.sums[doff:doff + 2 * c64]
            n.sums2 = self.sums[doff + 2 * c64:doff + 4 * c64]
            doff += 4 * c64
        self._make_params()

    def _make_params(self):
        P = ParameterDict()

        def reg(name, shape, kind, node, storage, gstorage, trainable=True, off=None):
            p = Parameter(self, name, shape, kind, node, trainable)
            p.storage, p.grad_storage = storage, gstorage
            if off is not None:
                p.span = (off, off + round_up(storage.numel(), 64))
            P[name] = p
            return p

        for n in self.conv_nodes:
            wv = self.weights[n.w_off:n.w_off + n.w_numel]
            gv = self.grads[n.w_off:n.w_off + n.w_numel]
            n.wp, n.gwp = wv, gv
            if getattr(n, 'gru', None) is not None:
                # i2h_weight (3 Ch, Cin, s, s) / h2h_weight (3 Ch, Ch, s, s) in the weight range, the biases (3 Ch,) in the
                # vector range beside the head bias (--no_wd, wd_mult, lr_mult reach them there)
                reg(n.pw, (3 * n.gate_ch, n.ref_cin, n.k, n.k), 'gru_weight', n, wv, gv, off=n.w_off)
                n.bias = self.weights[n.bias_off:n.bias_off + n.co_pad]
                n.gbias = self.grads[n.bias_off:n.bias_off + n.co_pad]
                reg(n.pb, (3 * n.gate_ch,), 'gru_bias', n, n.bias, n.gbias, off=n.bias_off)
            elif n.head:
                reg(n.name + ".weight", (n.cout, n.ref_cin, 1, 1), 'conv_weight', n, wv, gv, off=n.w_off)
                n.bias = self.weights[n.bias_off:n.bias_off + n.co_pad]
                n.gbias = self.grads[n.bias_off:n.bias_off + n.co_pad]
                reg(n.name + ".bias", (n.cout,), 'vector', n, n.bias, n.gbias, off=n.bias_off)
            else:
                kind = 'stem_weight' if n.stem else 'conv_weight'
                reg(n.name + ".0.weight", n.weight_shape(), kind, n, wv, gv, off=n.w_off)
                n.gamma = self.weights[n.gamma_off:n.gamma_off + n.cout]
                n.beta = self.weights[n.beta_off:n.beta_off + n.cout]
                n.ggamma = self.grads[n.gamma_off:n.gamma_off + n.cout]
                n.gbeta = self.grads[n.beta_off:n.beta_off + n.cout]
                c64 = round_up(n.cout, 64)
                n.rmean = self.running[n.stat_off:n.stat_off + n.cout]
                n.rvar = self.running[n.stat_off + c64:n.stat_off + c64 + n.cout]
                reg(n.name + ".1.gamma", (n.cout,), 'vector', n, n.gamma, n.ggamma, off=n.gamma_off)
                reg(n.name + ".1.beta", (n.cout,), 'vector', n, n.beta, n.gbeta, off=n.beta_off)
                reg(n.name + ".1.running_mean", (n.cout,), 'vector', n, n.rmean, None, trainable=False)
                reg(n.name + ".1.running_var", (n.cout,), 'vector', n, n.rvar, None, trainable=False)
                t = getattr(n, 'tdw', None)
                if t is not None:                    # Conv3DRepPad registers its Conv3D as `.conv` (three_darknet.py:55)
                    t.w = self.weights[t.w_off:t.w_off + t.w_numel]
                    t.gw = self.grads[t.w_off:t.w_off + t.w_numel]
                    reg(t.pname, (t.C, 1, 3, 1, 1), 'vector', t, t.w, t.gw, off=t.w_off)
        self._params = P
        self._opt_ranges = None

    # ------------------------------------------------------------------ reference-style surface
    @property
    def classes(self):
        return self._classes

    def collect_params(self, select=None):
        return self._params if select is None else self._params.select(select)

    def hybridize(self, active=True):
        """The reference compiles a CachedOp here (train_yolov3.py:586); programs are always pre-compiled."""
        return None

    def set_nms(self, nms_thresh=0.45, nms_topk=400, post_nms=100):
        # yolo3.py:1208-1228
        self.nms_thresh, self.nms_topk, self.post_nms = nms_thresh, nms_topk, post_nms
        self._programs = {k: v for k, v in self._programs.items() if k[0] not in ('infer', 'infer_bf16', 'stream', 'stream_bf16')}
        self._graph_cache.clear()

    def initialize(self, init='uniform', seed=233, obj_bias=0.0):
        """'uniform': MXNet default Uniform(0.07) for conv weights, gamma=1, beta=0, bias=0, running mean 0 / var 1.
        'he': N(0, 2/(k*k*Cin)) conv weights (keeps synthetic activations O(1))."""
        g = torch.Generator(device='cpu').manual_seed(seed)
        for name, p in self._params.items():
            if name.endswith('weight'):
                if init == 'uniform':
                    v = (torch.rand(p.shape, generator=g) * 2 - 1) * 0.07
                else:
                    fan = int(np.prod(p.shape[1:]))
                    v = torch.randn(p.shape, generator=g) * math.sqrt(2.0 / fan)
                    if 'prediction' in name:
                        v *= 0.05     # raw box logits O(1): exp(raw_wh)*anchor stays a sane pixel size
                p.set_data(v)
            elif name.endswith('gamma') or name.endswith('running_var'):
                v = torch.ones(p.shape)
                if init == 'he' and name.endswith('gamma') and '.body.1.1.' in name and name.startswith('stages'):
                    v *= 0.3      # residual-branch gain < 1: 23 residual adds would otherwise double the activation
                                  # variance per block in eval mode (running var = 1) and saturate every logit
                p.set_data(v)
            elif name.endswith('bias'):
                v = torch.zeros(p.shape)
                if obj_bias != 0.0 and p.kind != 'gru_bias':
                    v.view(3, -1)[:, 4] = obj_bias
                p.set_data(v)
            else:
                p.set_data(torch.zeros(p.shape))
        self.momentum_buf.zero_()
        self.grads.zero_()

    def reset_class(self, classes, reuse_weights=None):
        """yolo3.py:1230-1302 + YOLOOutputV3.reset_class :76-129: rebuild the 3 prediction convs."""
        if self._rnn_pos == 'out':
            raise NotImplementedError("reset_class on an rnn_pos='out' network: its predictions come from the GRU cells' gate "
                                      "blocks, and the reference's own YOLOOutputV3.reset_class doubts that path; retrain it")
        old_classes, old = self._classes, {k: p.data().cpu() for k, p in self._params.items()}
        old_attr = {k: (p.grad_req, p.wd_mult, p.lr_mult) for k, p in self._params.items()}
        old_npred = 5 + len(old_classes)
        if isinstance(reuse_weights, (dict, list)):
            if isinstance(reuse_weights, dict):
                m = {}
                for k, v in reuse_weights.items():
                    if isinstance(v, str):
                        if v not in old_classes:
                            raise ValueError("{} not found in old class names {}".format(v, old_classes))
                        v = old_classes.index(v)
                    elif v < 0 or v >= len(old_classes):
                        raise ValueError("Index {} out of bounds for old class names".format(v))
                    if isinstance(k, str):
                        if k not in classes:
                            raise ValueError("{} not found in new class names {}".format(k, classes))
                        k = list(classes).index(k)
                    elif k < 0 or k >= len(classes):
                        raise ValueError("Index {} out of bounds for new class names".format(k))
                    m[k] = v
                reuse_weights = m
            else:
                reuse_weights = {list(classes).index(x): old_classes.index(x) for x in reuse_weights
                                 if x in classes and x in old_classes}
        self._classes = list(classes)
        self._programs.clear()
        self._graph_cache.clear()
        self._build(len(self._classes))
        new_npred = 5 + len(self._classes)
        g = torch.Generator(device='cpu').manual_seed(233)
        for name, p in self._params.items():
            if "yolo_outputs" not in name:
                p.set_data(old[name])
                # every parameter but the rebuilt prediction convs is the same object in the reference: it keeps its
                # grad_req ('null' under freeze_base) and multipliers
                if p.span is not None:
                    p.grad_req, p.wd_mult, p.lr_mult = old_attr[name]
                continue
            new = (torch.rand(p.shape, generator=g) * 2 - 1) * 0.07 if name.endswith('weight') else torch.zeros(p.shape)
            if reuse_weights:
                od = old[name]
                for k, v in reuse_weights.items():
                    for a in range(3):
                        new[5 + k + a * new_npred] = od[5 + v + a * old_npred]
                        new[a * new_npred:a * new_npred + 5] = od[a * old_npred:a * old_npred + 5]
            p.set_data(new)

    def _grad_req_changed(self):
        """A parameter was frozen / unfrozen: the backward schedule and the optimiser ranges are rebuilt on next use."""
        self._programs = {k: v for k, v in self._programs.items() if k[0] != 'train'}
        self._opt_ranges = None

    def _node_trainable(self, n):
        """(weight trainable, any of gamma / beta / bias trainable) of a conv node."""
        P = self._params
        if getattr(n, 'gru', None) is not None:
            return P[n.pw].grad_req != 'null', P[n.pb].grad_req != 'null'
        if n.head:
            return P[n.name + ".weight"].grad_req != 'null', P[n.name + ".bias"].grad_req != 'null'
        return (P[n.name + ".0.weight"].grad_req != 'null',
                P[n.name + ".1.gamma"].grad_req != 'null' or P[n.name + ".1.beta"].grad_req != 'null')

    def _optimizer_ranges(self):
        """Contiguous arena ranges [(lo, hi, lr_mult, wd_mult)] of the trainable parameters, adjacent parameters with
        equal multipliers merged: two ranges (weights | gamma, beta, bias) for a fully trainable network."""
        if self._opt_ranges is None:
            ps = sorted((p for p in self._params.values() if p.span is not None and p.grad_req != 'null'),
                        key=lambda p: p.span[0])
            out = []
            for p in ps:
                lo, hi = p.span
                if out and out[-1][1] == lo and out[-1][2] == p.lr_mult and out[-1][3] == p.wd_mult and \
                        (lo != self.n_weight):
                    out[-1][1] = hi
                else:
                    out.append([lo, hi, p.lr_mult, p.wd_mult])
            self._opt_ranges = [tuple(r) for r in out]
        return self._opt_ranges

    def _params_changed(self):
        self._fold_dirty = True
        self._weights_version += 1
        self._wamax_dirty = True

    def _refresh_wamax(self):
        if self._wamax_dirty:
            L.check(L.load().vd_amax_segments(self.weights.data_ptr(), self._wamax_seg.data_ptr(), len(self.conv_nodes),
                                              self._wamax.data_ptr(), L.stream_ptr()), 'vd_amax_segments')
            self._wamax_dirty = False

    # ------------------------------------------------------------------ buffers
    def _buffers(self, key, B, H, W, train, bf16=False):
        """Activation (and in training gradient) tensors of one input shape.  bf16: the tensors of bf16-storage training -
        bf16 activations and gradients, no max-abs slots; the head logits stay fp32 and the heads take the bf16 pitch
        (_bf16_pitch), zero-filled so that the logits' pad columns stay 0."""
        # VD_STEM_FUSE_BWD (train_plan.stem_fuse_bwd, default on): no plan stores the stem's dz, which sizes the dz scratch
        stem_dz = train and not train_plan.stem_fuse_bwd()
        ck = ('buf', B, H, W, train) + (('bf16',) if bf16 else ()) + (('stem_dz',) if stem_dz else ())
        if ck in self._programs:
            return self._programs[ck]
        dev = self.device
        dt = torch.bfloat16 if bf16 else torch.float32
        zeroed = set(self.head_names) | {'d:' + h for h in self.head_names} if bf16 else set()
        bufs = {}
        for name, (c, div, ld, fr) in self.tensors.items():
            if name == 'in':
                bufs['in'] = torch.empty(B * fr, 3, H, W, device=dev)      # (B,K,3,H,W) folded: frame n = b*K + k
            elif name in zeroed:
                bufs[name] = torch.zeros(B * fr, H // div, W // div, _bf16_pitch(ld), device=dev)
            else:
                bufs[name] = torch.empty(B * fr, H // div, W // div, ld, dtype=dt, device=dev)
        if self.noback:
            for nm, c_, d_ in ROUTE_TENSORS:                                   # NCHW staging of the three inputs
                bufs['in:' + nm] = torch.empty(B, c_, H // d_, W // d_, device=dev)
        for g in self.gru_nodes:
            # per direction: I = i2h of the folded frames (backward: dI in place), H = h2h of a step (training keeps every
            # step's: backward recomputes the gates from I and H and writes dH in place), h = the states, step-major
            # [K][B] so that one step is a contiguous B-frame operand, dh = the state gradient carried between steps
            h_, w_ = H // g.div, W // g.div
            for cname, i2h, h2h in g.cells:
                bufs[i2h.dst] = torch.empty(B * g.K, h_, w_, 3 * g.chp, device=dev)
                bufs[h2h.dst] = torch.empty(B * g.K if train else B, h_, w_, 3 * g.chp, device=dev)
                bufs[g.key(cname, 'h')] = torch.empty(B * g.K, h_, w_, g.chp, device=dev)
                if train:
                    bufs[g.key(cname, 'dh')] = torch.empty(B, h_, w_, g.chp, device=dev)
        # max-abs slots (operand scales of the fp16-split arithmetic): one set per activation tensor, and in training
        # per conv node for the gradient dz it consumes; zeroed by the first record of every forward program
        if not bf16:
            names = [nm for nm in self.tensors if nm != 'in'] + (['dz:' + n.name for n in self.conv_nodes] if train else [])
            bufs['amax'] = torch.zeros(len(names) * L.AMAX_FLOATS, device=dev)
            for i, nm in enumerate(names):
                bufs['amax:' + nm] = bufs['amax'][i * L.AMAX_FLOATS:(i + 1) * L.AMAX_FLOATS]
        for n in self.conv_nodes:
            if getattr(n, 'tvalid', False):        # the 'same'-padded temporal conv output the valid frames are taken from
                bufs['zf:' + n.dst] = torch.empty(B * n.fr, H // n.div_out, W // n.div_out, n.cout, device=dev)
                if train:
                    bufs['dzf:' + n.dst] = torch.empty_like(bufs['zf:' + n.dst])
                else:
                    bufs['zs:' + n.dst] = torch.empty_like(bufs[n.dst])
        if train:
            for n in self.nodes:
                if isinstance(n, PoolNode) and n.type == 0:
                    # the winning frame of a max join: int32 beside fp32 tensors, one byte beside bf16 ones (K < 128)
                    bufs['am:' + n.dst] = torch.empty(bufs[n.dst].shape, dtype=torch.uint8 if bf16 else torch.int32, device=dev)
            for n in self.conv_nodes:
                if n.bn:
                    bufs['z:' + n.dst] = torch.empty_like(bufs[n.dst])
            for name in self.tensors:
                if name != 'in':
                    bufs['d:' + name] = (torch.zeros_like if 'd:' + name in zeroed else torch.empty_like)(bufs[name], dtype=dt)
            mx = max(bufs[n.dst].numel() for n in self.conv_nodes)
            # the two dz scratch buffers: the largest cell that stores a dz (the fused stem does not: TrainPlan.stem_fused)
            mz = mx if stem_dz else max(bufs[n.dst].numel() for n in self.conv_nodes
                                        if not (n.stem and n.bn and not getattr(n, 'tvalid', False)))
            bufs['dz'] = torch.empty(mz, dtype=dt, device=dev)
            bufs['dz2'] = torch.empty(mz, dtype=dt, device=dev)
            bufs['tmp'] = torch.empty(mx, dtype=dt, device=dev)
        # The plan-time autotuner times candidate kernels in place on these buffers.  Fresh allocations are zero pages, and on
        # all-zero operands the chip holds a ~20 % higher clock - for every candidate, but not equally: stand-alone the 256x128
        # tiles on the two MFMA shapes tie at 310 TF on zeros and differ by 8 % (255 vs 275) on real data.  Tune on noise.
        for nm, t in bufs.items():
            if torch.is_tensor(t) and t.dtype == dt and not nm.startswith('amax') and nm not in zeroed:
                t.normal_()
        self._programs[ck] = bufs
        return bufs

    def _grid(self, H, W):
        assert H == W, "square inputs only (the reference resizes to data_shape x data_shape)"
        assert H % 32 == 0, "input side must be a multiple of 32"
        return [H // 32, H // 16, H // 8]

    # ------------------------------------------------------------------ program builders
    def _conv_desc(self, n, bufs, B, H, W, out, *, scale=None, shift=None, residual=None, leaky=False, amax_out=False):
        d = ConvDesc()
        x = bufs[n.src]
        Hi, Wi = H // n.div_in, W // n.div_in
        Ho, Wo = H // n.div_out, W // n.div_out
        d.in_, d.wp, d.out = x.data_ptr(), n.wp.data_ptr(), out.data_ptr()
        d.N, d.Hi, d.Wi, d.Ci = B * n.fr, Hi, Wi, n.ci_eff
        d.Hg, d.Wg, d.in_stride = Ho, Wo, n.stride
        ops._set_taps(d, n.taps())
        d.Kfr = n.fr if n.kd > 1 else 1
        d.Ho, d.Wo, d.Co = Ho, Wo, n.co_pad
        d.out_stride, d.out_oy, d.out_ox = 1, 0, 0
        d.ldo = d.ldr = n.co_pad
        flags = 0
        if scale is not None or shift is not None:
            flags |= EPI_AFFINE
            d.scale = scale.data_ptr() if scale is not None else None
            d.shift = shift.data_ptr() if shift is not None else None
        if leaky:
            flags |= EPI_LEAKY
        if residual is not None:
            flags |= EPI_RESIDUAL
            d.residual = residual.data_ptr()
        d.flags, d.slope = flags, LEAKY_SLOPE
        d.amax_in, d.amax_w = self._amax_or_none(bufs, n.src), n.wamax.data_ptr()
        self._set_streamk(d, 0)
        if amax_out:                                   # inference: the epilogue publishes the max-abs of what it writes
            d.amax_out = bufs['amax:' + n.dst].data_ptr()
        return d

    def _amax_or_none(self, bufs, name):
        """max-abs slots of an operand tensor for the fp16-split arithmetic, or None where that arithmetic must not be used
        for its consumers (`_range_exact`): without the slots a launch record runs the 3-way bf16 split or the fp32 MFMA,
        whose operands keep fp32's exponent range"""
        if name in self._range_exact:
            return None
        return bufs['amax:' + name].data_ptr()

    def _close_range_exact(self):
        """Close `_range_exact` over the tensors that only re-arrange a range-exact one: the output of a concatenation, a
        temporal pool (max / mean / channel stacking), a frame selection or an add carries its sources' channels on, so it
        is range-exact as soon as ANY source is - the conv behind `n0.cat` reads the very channels the guard flagged in
        `n0.tr`.  One walk in node order (a source is produced before its reader).  A ConvNode's fused residual is NOT
        followed: the cell's dst is leaky(bn(z)) + residual, a tensor with a BatchNorm of its own, which the guard
        examines itself (the same holds for a TdwNode's residual: its operand name is the guard's for that cell).
        Returns the nodes whose dst joined, in node order."""
        added = []
        for n in self.nodes:
            if isinstance(n, (UpcatNode, PoolNode, SelNode, AddNode)) and n.dst not in self._range_exact and \
                    any(t in self._range_exact for t in node_inputs(n)):
                self._range_exact.add(n.dst)
                added.append(n)
        return added

    def _concat_ranges(self, ups, thresh, ratios, flags, at):
        """The guard's second source: a concatenation whose two sides differ in SCALE with no BatchNorm vector showing it
        (every channel of the transition uniformly small against the route: two flat vectors, and the merged max-abs slot
        keeps the larger side only).  For each UpcatNode of `ups`: min / max of the two sources' max-abs (each reduced over
        its sub-slots) into ratios[at + j], the flag (ratio < thresh) into flags[at + j] - on the device, read with the
        guard's flags.  The slots are those of the last fp32 training step; without one, and for a side that is all zeros
        (nothing to lose: zero is staged exactly), nothing is flagged."""
        flags[at:].zero_()
        ratios[at:].fill_(1.0)
        tp = getattr(self, '_last_train', None)
        if not ups or tp is None or tp.get('storage', 'fp32') != 'fp32':
            return
        bufs = tp['bufs']
        side = lambda t: bufs['amax:' + t].view(-1)[::L.AMAX_STRIDE][:L.AMAX_SLOTS].max()
        for j, n in enumerate(ups):
            if n.dst in self._range_exact:
                continue
            a, b = side(n.up), side(n.route)
            lo, hi = torch.minimum(a, b), torch.maximum(a, b)
            ratios[at + j] = torch.where(lo > 0, lo / hi.clamp_min(1e-37), torch.ones_like(lo))
            flags[at + j] = ((lo > 0) & (lo < thresh * hi)).to(torch.int32)

    def check_operand_ranges(self, thresh=2.0 ** -16):
        """The data-driven half of the fp16 split's range rule (include/viddet_hip.h vd_range_guard).  One
        small launch over the BatchNorm vectors of the network, the max-abs ratio of every concatenation's two sides
        (_concat_ranges), then a read of the flags (synchronises: call it where the host waits anyway - train_yolov3.py does
        at every log line).  A tensor whose per-channel scales spread over more than 1 / thresh joins `_range_exact`, and
        with it every tensor derived from it (_close_range_exact); the plans are dropped and rebuilt with the range-exact
        arithmetic for their consumers.  Returns {tensor name: min / max channel-scale ratio} of the newly flagged tensors;
        a derived tensor carries the smallest ratio of the sources that brought it in."""
        bn = [n for n in self.conv_nodes if n.bn]
        if not bn:
            return {}
        ups = [n for n in self.nodes if isinstance(n, UpcatNode)]
        if getattr(self, '_guard', None) is None:
            arr = (L.GuardItem * len(bn))()
            for i, n in enumerate(bn):
                arr[i].gamma, arr[i].beta, arr[i].scale, arr[i].C = n.gamma.data_ptr(), n.beta.data_ptr(), n.b_scale.data_ptr(), n.cout
            items = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
            nf = 2 * len(bn) + len(ups)                    # [per BatchNorm: activation, gradient | per concatenation]
            self._guard = (items, torch.zeros(nf, device=self.device), torch.zeros(nf, dtype=torch.int32, device=self.device))
        items, ratios, flags = self._guard
        L.check(L.load().vd_range_guard(items.data_ptr(), len(bn), float(thresh), ratios.data_ptr(), flags.data_ptr(), L.stream_ptr()),
                'vd_range_guard')
        self._concat_ranges(ups, float(thresh), ratios, flags, 2 * len(bn))
        if torch.distributed.is_available() and torch.distributed.is_initialized() and \
                torch.distributed.get_world_size(self.process_group) > 1:
            # every rank takes the union: without SyncBN the ranks' invstd differ, and the ranks must run the same plans
            torch.distributed.all_reduce(flags, op=torch.distributed.ReduceOp.MAX, group=self.process_group)
        fl, ra = flags.cpu().numpy(), ratios.cpu().numpy()
        new = {}
        for i, n in enumerate(bn):
            # (the operand tensor behind a _conv21d cell is its temporal conv's output: per-channel taps, same channel scales)
            for k, name in ((0, n.tdw.dst if getattr(n, 'tdw', None) is not None else n.dst), (1, 'dz:' + n.name)):
                if k == 1 and n.stem:
                    # no launch reads the stem's dz max-abs slot: no data gradient flows into the frames, its weight
                    # gradient is an fp32 MFMA kernel (vd_stem.hip), and the fused one never stores a dz at all
                    continue
                if fl[2 * i + k] and name not in self._range_exact:
                    new[name] = float(ra[2 * i + k])
        for j, n in enumerate(ups):
            if fl[2 * len(bn) + j] and n.dst not in self._range_exact:
                new[n.dst] = float(ra[2 * len(bn) + j])
        if new:
            self._range_exact.update(new)
            # the derived tensors that join with them, so that the caller's log line names every tensor that moved (the set
            # was closed before this call, so each of them has a source among the new names)
            for n in self._close_range_exact():
                new[n.dst] = min(new[t] for t in node_inputs(n) if t in new)
            self._drop_plans()
        return new

    def _set_streamk(self, d, stream_idx):
        """give a conv record the stream-K hand-off workspace of the stream it runs on (0 = the program's main stream,
        1.. = the parity streams of a stride-2 data gradient): launches that may overlap never share one"""
        if not _streamk_on():
            return
        ws = self._sk_ws.get(stream_idx)
        if ws is None:
            ws = self._sk_ws[stream_idx] = ops.streamk_workspace(self.device)
        d.sk_ws, d.sk_ws_bytes = ws.data_ptr(), ws.numel()

    def _syncbn_exchange(self, t):
        """the SyncBN collective of one layer and direction: sum all-reduce of its fp64 [2C] vector over the ranks"""
        def f():
            if getattr(self, '_syncbn_suppress', False):          # (bench.py times a step without the exchanges)
                return
            torch.distributed.all_reduce(t, group=self.process_group)
            if getattr(self, '_dp_stats', None) is not None:
                self._dp_stats['syncbn_exchanges'] = self._dp_stats.get('syncbn_exchanges', 0) + 1
        return f

    def _add_sel_add_fwd(self, prog, n, bufs, B, bf16=False):
        """Forward launches of a SelNode / AddNode (the same in inference and training).  bf16 (inference only): the slice
        copies 4-byte words, two elements each, and no max-abs records follow."""
        am = lambda t: bufs['amax:' + t].data_ptr()
        if isinstance(n, SelNode):
            xs, o = bufs[n.src], bufs[n.dst]
            prog.add('vd_frame_slice', xs.data_ptr(), o.data_ptr(), B, n.K, n.k0, n.kc, xs[0].numel() // (2 if bf16 else 1), 0)
            if not bf16:
                prog.add('vd_amax_merge', am(n.src), None, am(n.dst))
        else:
            a, b_, o = bufs[n.a], bufs[n.b], bufs[n.dst]
            prog.add('vd_add_bf16' if bf16 else 'vd_add', a.data_ptr(), b_.data_ptr(), o.data_ptr(), o.numel())
            if not bf16:
                prog.add('vd_amax', o.data_ptr(), o.numel(), am(n.dst))

    # ------------------------------------------------------------------ bidirectional ConvGRU (GruNode)
    def _gru_conv_desc(self, cn, x, out, N, H, W, sidx, amax_in=None):
        """forward record of one of a GRU cell's convolutions (stride 1, 'same', bias in the epilogue) on N frames of `x`.
        No arithmetic flag is set here: autotune_program, at the end of the plan build, picks it per record (autotune_desc),
        and a record without max-abs slots for its operand (amax_in None: the state) can only get the fp32 MFMA or the
        3-way bf16 split there, never the fp16 split (_tile_candidates) - the range-exact arithmetics."""
        d = ConvDesc()
        Hc, Wc = H // cn.div_in, W // cn.div_in
        d.in_, d.wp, d.out = x.data_ptr(), cn.wp.data_ptr(), out.data_ptr()
        d.N, d.Hi, d.Wi, d.Ci = N, Hc, Wc, cn.cin
        d.Hg, d.Wg, d.in_stride = Hc, Wc, 1
        ops._set_taps(d, cn.taps())
        d.Kfr, d.Ho, d.Wo, d.Co = 1, Hc, Wc, cn.co_pad
        d.out_stride, d.out_oy, d.out_ox = 1, 0, 0
        d.ldo = d.ldr = cn.co_pad
        d.flags, d.slope, d.shift = EPI_AFFINE, LEAKY_SLOPE, cn.bias.data_ptr()
        d.amax_in, d.amax_w = amax_in, cn.wamax.data_ptr()
        self._set_streamk(d, sidx)
        return d

    @staticmethod
    def _gru_meta(cn, N, H, W, kind):
        """roofline record of a GRU conv launch over N frames (the form of _flops)"""
        px = N * (H // cn.div_in) * (W // cn.div_in)
        return dict(kind=kind, node=cn.name, k=cn.k, stride=1, flops=2.0 * cn.cin * cn.cout * cn.k * cn.k * px,
                    bytes=4.0 * (px * cn.cin + px * cn.cout + cn.cout * cn.cin * cn.k * cn.k))

    def _add_gru_fwd(self, prog, g, bufs, B, H, W, train, side=None):
        """Forward launches of a GruNode.  Per direction ONE i2h conv over the B*K folded frames, then per step one h2h conv
        on the B frames of the previous state (none at the first step: the state is zero, the gate kernel takes the h2h
        bias) and one gate launch; then the average of the two directions into the folded output.  Training: the reverse
        direction's chain runs on `side`; inference keeps one stream (no parallel branches in a captured graph) and one
        H slab."""
        K, hw = g.K, (H // g.div) * (W // g.div)
        x = bufs[g.src]
        par = train and side is not None
        if par:
            e_x, e_r = torch.cuda.Event(), torch.cuda.Event()
            prog.add_py(ev_record(e_x))
            prog.add_py(ev_wait(e_x, side))
            prog.hold(e_x, e_r)
        for di, (cname, i2h, h2h) in reversed(list(enumerate(g.cells))):      # the side stream's chain is queued first
            st = side if (par and di == 1) else None
            sidx = 4 if st is not None else 0                                # (0..3: main stream and the parity streams)
            I, Hb, hs = bufs[i2h.dst], bufs[h2h.dst], bufs[g.key(cname, 'h')]
            d = self._gru_conv_desc(i2h, x, I, B * K, H, W, sidx, self._amax_or_none(bufs, g.src))
            prog.hold(d)
            prog.add('vd_conv_igemm', C.byref(d), meta=self._gru_meta(i2h, B * K, H, W, 'fwd'), stream=st)
            for s_ in range(K):
                t = s_ if di == 0 else K - 1 - s_
                Hs = None
                if s_ > 0:
                    Hs = Hb[s_ * B:(s_ + 1) * B] if train else Hb
                    d = self._gru_conv_desc(h2h, hs[(s_ - 1) * B:s_ * B], Hs, B, H, W, sidx)
                    prog.hold(d)
                    prog.add('vd_conv_igemm', C.byref(d), meta=self._gru_meta(h2h, B, H, W, 'fwd'), stream=st)
                prog.add('vd_gru_gate_fwd', I.data_ptr(), Hs.data_ptr() if s_ > 0 else None, h2h.bias.data_ptr(),
                         hs[(s_ - 1) * B:].data_ptr() if s_ > 0 else None, hs[s_ * B:].data_ptr(), B, K, t, hw, g.chp,
                         meta=dict(kind='gru_gate_fwd', node=g.name, flops=14.0 * B * hw * g.chp,
                                   bytes=4.0 * B * hw * g.chp * (8 if s_ > 0 else 4)), stream=st)
            if st is not None:
                prog.add_py(ev_record(e_r, side))
        if par:
            prog.add_py(ev_wait(e_r))
        y = bufs[g.dst]
        prog.add('vd_gru_avg', bufs[g.key('l_cell', 'h')].data_ptr(), bufs[g.key('r_cell', 'h')].data_ptr(), y.data_ptr(), B, K,
                 hw * g.chp, bufs['amax:' + g.dst].data_ptr(),
                 meta=dict(kind='gru_avg', node=g.name, flops=2.0 * B * K * hw * g.chp, bytes=12.0 * B * K * hw * g.chp))

    def _add_tdw_fwd(self, prog, n, bufs, B, H, W):
        """y = tdw(x, w) [+ residual] with the max-abs of y for the convs that read it (the same in inference and training)"""
        hw = (H // n.div) * (W // n.div)
        prog.add('vd_tdw_fwd', bufs[n.src].data_ptr(), n.w.data_ptr(), bufs[n.residual].data_ptr() if n.residual else None,
                 bufs[n.dst].data_ptr(), B, n.K, hw, n.C, bufs['amax:' + n.dst].data_ptr(),
                 meta=dict(kind='tdw_fwd', node=n.name, flops=6.0 * B * n.K * hw * n.C,
                           bytes=4.0 * B * n.K * hw * n.C * (3 if n.residual else 2)))

    def _add_input_stage(self, prog, bufs, B, H, W):
        """The first records of every fp32 program: the max-abs slots are zeroed; then the layout change of the network
        inputs - none for the frame batch (the stem kernel reads NCHW directly); the three cached feature maps of the
        no-backbone variant go NCHW -> NHWC."""
        prog.add('vd_fill', bufs['amax'].data_ptr(), 0.0, bufs['amax'].numel())
        if self.noback:
            for nm, c_, d_ in ROUTE_TENSORS:
                prog.add('vd_nchw_to_nhwc', bufs['in:' + nm].data_ptr(), bufs[nm].data_ptr(), B, c_, H // d_, W // d_)
                prog.add('vd_amax', bufs[nm].data_ptr(), bufs[nm].numel(), bufs['amax:' + nm].data_ptr())

    def _add_stem(self, prog, n, bufs, B, H, W, out, *, scale=None, shift=None, leaky=False, bf16=False, stats=None):
        """vd_stem_conv: the 3 -> 32 stem straight from the NCHW batch (vd_stem.hip)."""
        flags = (EPI_AFFINE if scale is not None else 0) | (EPI_LEAKY if leaky else 0)
        prog.add('vd_stem_conv', bufs['in'].data_ptr(), n.wp.data_ptr(), out.data_ptr(), out.shape[-1], bufs['in'].shape[0], H, W,
                 scale.data_ptr() if scale is not None else None, shift.data_ptr() if shift is not None else None,
                 LEAKY_SLOPE, flags, 1 if bf16 else 0, stats, meta=self._flops(n, B, H, W, 'fwd'))

    def _stage_inputs(self, bufs, x):
        if self.noback:
            for (nm, _, _), t in zip(ROUTE_TENSORS, x):
                bufs['in:' + nm].copy_(t.reshape(bufs['in:' + nm].shape))
        elif x.dtype == torch.uint8 and self._dev_nv12 is not None:
            # NV12 frames (B,H0*3/2,W0) or windows (B,K,H0*3/2,W0): converted, resized and normalised in one kernel
            n_ = bufs['in'].shape[0]
            assert x.numel() == n_ * x.shape[-2] * x.shape[-1], "NV12 input must be (B[,K],H0*3/2,W0)"
            self._preprocess_u8(self._frames_to_device(x), bufs['in'], n_)
        elif x.dtype == torch.uint8:
            # uint8 frames (B,H,W,3) or windows (B,K,H,W,3) straight from the loader: /255, normalise and NHWC -> planar in
            # one kernel (transforms.py:239-245), a quarter of the host-to-device bytes
            n_, h_, w_ = bufs['in'].shape[0], bufs['in'].shape[2], bufs['in'].shape[3]
            if self._dev_resize is not None:                      # frames of any size, resized on the way (set_device_resize)
                h_, w_ = x.shape[-3], x.shape[-2]
            assert x.shape[-1] == 3 and x.numel() == n_ * h_ * w_ * 3, "uint8 input must be (B[,K],H,W,3)"
            self._preprocess_u8(x.to(self.device).contiguous(), bufs['in'], n_)
        else:
            bufs['in'].copy_(x.reshape(bufs['in'].shape))

    def _preprocess_u8(self, xd, dst, n):
        """n uint8 frames (..,H0,W0,3) on the device -> the first n rows of the NCHW input tensor `dst`, normalised: one
        vd_preprocess_u8_nchw launch, or - device resize on and the frames not yet the size of dst - one vd_resize_u8_nchw
        launch that resamples them on the way (its output is vd_preprocess_u8_nchw of the resized uint8 frames, bit for bit)"""
        if self._dev_nv12 is not None:
            return self._preprocess_nv12(xd, dst, n)
        h, w = dst.shape[2], dst.shape[3]
        h0, w0 = xd.shape[-3], xd.shape[-2]
        if self._dev_resize is None or (h0, w0) == (h, w):       # (imresize returns a copy of a frame of the target size)
            L.check(L.load().vd_preprocess_u8_nchw(xd.data_ptr(), dst.data_ptr(), n, h, w, L.stream_ptr()), 'vd_preprocess_u8_nchw')
            return
        t = self._resize_tables(h0, w0)
        if t['dev'] is None:
            t['dev'] = [torch.from_numpy(a).to(self.device) for a in t['host']]
        iy, wy, ix, wx = t['dev']
        L.check(L.load().vd_resize_u8_nchw(xd.data_ptr(), dst.data_ptr(), None, n, h0, w0, h, w, iy.data_ptr(), wy.data_ptr(),
                                           iy.shape[1], ix.data_ptr(), wx.data_ptr(), ix.shape[1], L.stream_ptr()),
                'vd_resize_u8_nchw')

    def _frames_to_device(self, x):
        """uint8 frames for _preprocess_u8: on the device and contiguous - NV12 frames (set_device_resize(source='nv12'))
        keep their layout, _preprocess_nv12 reads a pitched surface through its strides"""
        x = x.to(self.device)
        return x if self._dev_nv12 is not None else x.contiguous()

    def _preprocess_nv12(self, xd, dst, n):
        """n NV12 frames (..,H0*3/2,W0) uint8 on the device -> the first n rows of `dst`: one vd_resize_nv12_nchw launch, a
        frame already at the target size included (identity tap tables).  A tensor with last stride 1, rows at least W0
        apart and frames at least a frame's rows apart - a contiguous one, or the view (N,H0*3/2,P)[..., :W0] of a pitched
        decoder surface - goes to the kernel through its strides as pitch / frame_stride; any other layout is made
        contiguous first."""
        from .video import nv12_frame_size
        hn, w0 = xd.shape[-2], xd.shape[-1]
        h0, _ = nv12_frame_size(hn, w0)
        xd = xd.reshape(-1, hn, w0)                               # windows (B,K,..): B*K frames, a view where the strides allow
        pitch, fstride = xd.stride(1), xd.stride(0)
        if xd.stride(2) != 1 or pitch < w0 or (xd.shape[0] > 1 and fstride < hn * pitch):
            xd = xd.contiguous()
            pitch, fstride = xd.stride(1), xd.stride(0)
        if xd.shape[0] == 1:                                      # (a single frame's stride says nothing)
            fstride = hn * pitch
        assert xd.shape[0] >= n
        t = self._resize_tables(h0, w0, identity=(h0, w0) == (dst.shape[2], dst.shape[3]))
        if t['dev'] is None:
            t['dev'] = [torch.from_numpy(a).to(self.device) for a in t['host']]
        iy, wy, ix, wx = t['dev']
        in_bytes = (n - 1) * fstride + (hn - 1) * pitch + w0      # up to the last frame's last chroma byte, nothing behind it
        L.check(L.load().vd_resize_nv12_nchw(xd.data_ptr(), in_bytes, fstride, pitch, h0 * pitch, dst.data_ptr(), None, n, h0, w0,
                                             dst.shape[2], dst.shape[3], iy.data_ptr(), wy.data_ptr(), iy.shape[1], ix.data_ptr(),
                                             wx.data_ptr(), ix.shape[1], *self._dev_nv12, L.stream_ptr()),
                'vd_resize_nv12_nchw')

    def _build_infer(self, B, H, W):
        """the fp32 inference plan (infer_plan.InferPlan) -> (prog, bufs, outputs)"""
        return infer_plan.InferPlan(self, H, W, False).build(B)

    def _refresh_fold(self):
        if not self._fold_dirty:
            return
        for n in self.conv_nodes:
            if n.bn:
                ops.bn_fold_eval(n.gamma, n.beta, n.rmean, n.rvar, BN_EPS, n.fold_scale, n.fold_shift)
        self._fold_dirty = False

    # ------------------------------------------------------------------ bf16 inference
    def set_precision(self, precision):
        """'fp32' (reference precision) or 'bf16' (BASELINE configs[1]): bf16 storage + bf16 MFMA with fp32
        accumulation and fp32 epilogue for inference; the prediction heads stay fp32."""
        assert precision in ('fp32', 'bf16')
        if precision == 'bf16' and getattr(self, '_conv_types', None):
            raise NotImplementedError("bf16 inference is not built for conv_types networks: the temporal-conv kernels "
                                      "(vd_tdw.hip) are fp32 only")
        if precision == 'bf16' and self._rnn_pos:
            raise NotImplementedError("bf16 inference is not built for rnn_pos networks: the ConvGRU gate kernels (vd_gru.hip) "
                                      "and the recurrent state are fp32 only")
        self.precision = precision

    def _build_infer_bf16(self, B, H, W):
        """bf16 inference plan of every network variant: the plain net (BASELINE configs[1]), k > 1 windows (TimeDistributed
        backbone = frames folded into the batch, temporal pooling / stacking, 3-D and 2+1-D neck convs through Kfr), the
        no-backbone net (its three fp32 feature maps converted on the way in) and YOLOV3Temporal (frame selections, sums,
        valid-frame convs, per-frame heads) -> (prog, bufs, outputs, packs)."""
        return infer_plan.InferPlan(self, H, W, True).build(B)

    def _refresh_bf16(self, packs):
        """Re-derive the bf16 weight images and the padded fp32 scale/shift vectors after a parameter change."""
        self._refresh_fold()
        lib = L.load()
        s = L.stream_ptr()
        for n, wb, co_p, ci_p in packs:
            L.check(lib.vd_pack_weight_bf16(n.wp.data_ptr(), wb.data_ptr(), n.co_pad, co_p, n.ci_eff, ci_p, n.T, s),
                    'vd_pack_weight_bf16')
            if n.bn:
                n.bf_scale[:n.cout].copy_(n.fold_scale)
                n.bf_shift[:n.cout].copy_(n.fold_shift)

    def _tune_bf16(self, prog):
        if os.environ.get("VD_AUTOTUNE", "1") == "0":
            return
        for (fname, fn, args) in prog.recs:
            if fname != 'vd_conv_igemm_bf16':
                continue
            d, of32 = args[0]._obj, args[1]
            base = d.flags & ~(L.MATH_NOHALO | L.CONV_STREAMK | L.CONV_SPLITK)
            key = ('bf16', d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.in_stride, d.T, d.Co, base, of32, d.Kfr)
            _tune_bf16_record(d, of32, key, *_bf16_tile_candidates(d, of32, patch_kernel=True, tall_tiles=True, halo=True),
                              splitk=True)
        _TUNE_CACHE.save()

    def _bf16_current(self, state, packs, progs):
        """The bf16 weight images of ONE plan, current: every plan owns its images, re-packed when the weights / running
        statistics moved since THIS plan last packed them (a net-wide flag would leave the other shapes' plans stale);
        the plan's records are tuned once, after the first pack.  `state` (a dict of the plan) remembers the version."""
        version = (self._weights_version, self._stats_version)
        if state.get('packs_version') != version:
            self._refresh_bf16(packs)
            if 'packs_version' not in state:
                for prog in progs:
                    self._tune_bf16(prog)
            state['packs_version'] = version

    # ------------------------------------------------------------------ inference
    def _in_shape(self, x):
        """(B, H, W) of the image batch a call refers to (the no-backbone inputs are the stride-8/16/32 maps)."""
        if self.noback:
            return x[0].shape[0], x[0].shape[-2] * 8, x[0].shape[-1] * 8
        if self._dev_resize is not None:            # raw (B[,K],H0,W0,3) frames, resized to the target on the device
            if self._dev_nv12 is not None:          # NV12 (B[,K],H0*3/2,W0): two planes, no channel axis
                if x.dtype != torch.uint8:
                    raise ValueError("set_device_resize(source='nv12') is on: the network takes NV12 frames, uint8 "
                                     "(B[,K],H0*3/2,W0), got a %s tensor %s" % (str(x.dtype).replace("torch.", ""), tuple(x.shape)))
                if x.dim() >= 4 and x.shape[-1] == 3:
                    raise ValueError("set_device_resize(source='nv12') is on: the network takes NV12 frames (B[,K],H0*3/2,W0), "
                                     "got packed RGB frames %s - set source='rgb' for those" % (tuple(x.shape),))
                if x.dim() not in (3, 4):
                    raise ValueError("set_device_resize(source='nv12') is on: expected NV12 frames (B[,K],H0*3/2,W0), got %s"
                                     % (tuple(x.shape),))
                from .video import nv12_frame_size
                h0, w0 = nv12_frame_size(x.shape[-2], x.shape[-1])
                self._resize_tables(h0, w0, identity=(h0, w0) == self._dev_resize[:2])
                return x.shape[0], self._dev_resize[0], self._dev_resize[1]
            if x.dtype != torch.uint8:
                raise ValueError("set_device_resize is on: the network takes raw uint8 frames (B[,K],H0,W0,3); a float batch is "
                                 "already normalised at its own size - switch it off with set_device_resize(None)")
            self._resize_tables(x.shape[-3], x.shape[-2])
            return x.shape[0], self._dev_resize[0], self._dev_resize[1]
        if x.dtype == torch.uint8:                  # (B[,K],H,W,3) frames, normalised on the device
            return x.shape[0], x.shape[-3], x.shape[-2]
        return x.shape[0], x.shape[-2], x.shape[-1]

    def set_device_resize(self, width, height=None, interp=9, source='rgb', matrix='bt601', range='limited'):
        """Resize raw uint8 frames to (height, width) on the device (vd_resize.hip); width None switches it off
        (the default: every call behaves as without it).  On: uint8 inputs (B,H0,W0,3), (B,K,H0,W0,3) and detect_video's
        (T,H0,W0,3) have any one source size per call and go through video.imresize's resample (interp 9: area when both axes
        shrink, bicubic when both grow, bilinear otherwise) inside the kernel that normalises them; the plans are those of
        the target size.  Float inputs are refused while it is on.

        source='nv12' (DESIGN.md 23): the frames are NV12, as video decoders hand them out - uint8 (B,H0*3/2,W0),
        (B,K,H0*3/2,W0) and detect_video's (T,H0*3/2,W0), on the host or already on the device, a pitched surface through
        its strides (_preprocess_nv12) - converted to RGB by video.nv12_to_rgb's integer arithmetic with
        NV12_MATRICES[(matrix, range)] inside the same launch (vd_resize_nv12_nchw); a frame of the target size goes
        through it too.  The result is bit-equal to source='rgb' on nv12_to_rgb of the frames."""
        if width is None:
            self._dev_resize = self._dev_nv12 = None
            return
        if source not in ('rgb', 'nv12'):
            raise ValueError("set_device_resize: source %r is neither 'rgb' nor 'nv12'" % (source,))
        coef = None
        if source == 'nv12':
            from .video import nv12_matrix
            try:
                coef = nv12_matrix(matrix, range)
            except ValueError as e:
                raise ValueError("set_device_resize: %s" % e) from None
        if self.noback:
            raise NotImplementedError("set_device_resize with noback: the no-backbone network takes cached feature maps, not "
                                      "frames - there is nothing to resize")
        width, height = int(width), int(width if height is None else height)
        if width < 32 or height < 32 or width % 32 or height % 32:
            raise ValueError("set_device_resize: width and height must be positive multiples of 32 (the network's stride), got "
                             "width=%d height=%d" % (width, height))
        from .video import resolve_interp
        if resolve_interp(2, 2, 1, 1, interp) not in (1, 2, 3, 4):
            raise ValueError("set_device_resize: interp %r is not a separable interpolation (1 bilinear, 2 area, 3 bicubic, "
                             "4 Lanczos, 9 = by direction)" % (interp,))
        self._dev_resize = (height, width, interp)
        self._dev_nv12 = coef

    def _resize_tables(self, h0, w0, identity=False):
        """The tap tables of the (h0, w0) -> target resize, cached on the net per (H0, W0, H, W, interp): {'host': the four
        arrays of video.resize_tables, 'dev': their uploads (made by the first launch that needs them)}.  Refuses, before
        anything touches the GPU, a resize whose taps the kernel does not take.  identity: the one-tap tables of a frame
        already at the target size (the NV12 kernel converts such a frame too), under the key (.., 'identity')."""
        h, w, interp = self._dev_resize
        key = (int(h0), int(w0), h, w, 'identity' if identity else interp)
        t = self._resize_cache.get(key)
        if t is None:
            from .video import resize_tables, identity_tables
            tabs = identity_tables(h, w) if identity else resize_tables(key[0], key[1], h, w, interp)[1:]
            ty, tx = tabs[0].shape[1], tabs[2].shape[1]
            if ty > 16 or tx > 16:
                raise ValueError("set_device_resize: a %dx%d -> %dx%d resize has Ty=%d / Tx=%d taps per output pixel, "
                                 "vd_resize_u8_nchw takes at most 16 (area shrinking up to 15x)" % (key[0], key[1], h, w, ty, tx))
            t = self._resize_cache[key] = dict(host=tabs, dev=None)
        return t

    def _forward_infer(self, x):
        B, H, W = self._in_shape(x)
        assert 0 < self.nms_thresh < 1, "nms_thresh outside (0,1) (NMS disabled) is not implemented"
        if self.precision == 'bf16':
            key = ('infer_bf16', B, H, W)
            if key not in self._programs:
                self._programs[key] = self._build_or_evict(lambda: self._build_infer_bf16(B, H, W))
            prog, bufs, o, packs = self._programs[key]
            self._bf16_current(bufs, packs, [prog])
        else:
            key = ('infer', B, H, W)
            if key not in self._programs:
                self._programs[key] = self._build_or_evict(lambda: self._build_infer(B, H, W))
            prog, bufs, o = self._programs[key]
            self._refresh_fold()
        self._stage_inputs(bufs, x)
        self._refresh_wamax()
        if self.use_graphs:
            g = self._graph_cache.get(key)
            if g is None:
                prog.run()                       # warm-up outside capture (function attributes etc.)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    prog.run()
                self._graph_cache[key] = g
            g.replay()
        else:
            prog.run()
        self.last_rows, self.last_overflow = o['rows'], o['overflow']
        if self.temporal_out:                    # (B, t, 100, .) as TimeDistributed(output) stacks them
            K = self._k
            return (o['ids'].view(B, K, -1, 1), o['scores'].view(B, K, -1, 1), o['bboxes'].view(B, K, -1, 4))
        return o['ids'], o['scores'], o['bboxes']

    # ------------------------------------------------------------------ streaming video detection
    def _stream_refusal(self):
        """Why this network cannot detect on a clip frame by frame (None: it can).  Decided from the constructor's
        arguments first, so that every refusal carries the name the caller used; _stream_split() then checks the graph."""
        if self._conv_types:
            return ("conv_types %r: the (2+1)-D backbone mixes the frames of a window inside the backbone itself (the temporal "
                    "depthwise convs, vd_tdw.hip), so no part of it is per-frame" % (self._conv_types,))
        if self.noback:
            return ("noback: the no-backbone network takes cached feature maps, not frames: it has no window, no join and no "
                    "per-frame prefix to run once")
        if self.temporal_out or self.temporal_side:
            return ("temporal / t_out: YOLOV3Temporal has no pooled or stacked join to split at - its side branches are temporal "
                    "convs over the window's frames (t_out: every frame keeps its own predictions)")
        if self._rnn_pos:
            return ("rnn_pos %r: the ConvGRU carries a state across the K frames of a window ahead of the join, so a frame's "
                    "features depend on the window it is seen in" % (self._rnn_pos,))
        if self._corr_pos:
            return ("corr_pos %r: the correlation join compares every frame with the centre frame of ITS window (vd_corr.hip "
                    "reads a materialised window); it has no form that reads a ring" % (self._corr_pos,))
        if self._block_conv_type != '2':
            return ("block_conv_type %r: the neck's 3-D / 2+1-D convs mix the frames of a window ahead of the late join, so "
                    "the neck is not per-frame" % (self._block_conv_type,))
        if self._k > 1 and (self._k_join_type not in ('max', 'mean', 'cat') or self._k_join_pos not in ('early', 'late')):
            return ("k_join_type %r / k_join_pos %r: a window k > 1 needs a max | mean | cat join, early or late, to split at"
                    % (self._k_join_type, self._k_join_pos))
        return None

    def _stream_split(self):
        """Split the inference graph at the joins: (prefix, suffix).  The prefix is every node whose output a PoolNode
        transitively needs - re-made as nodes over single frames (fr = 1; they share the parameters) - the suffix the joins
        and everything behind them.  Asserts that the prefix is per-frame arithmetic and that the suffix sees the prefix
        through the joins only."""
        import copy
        pools = [n for n in self.nodes if isinstance(n, PoolNode)]
        assert pools, "no join to split at"
        need = {p.src for p in pools}
        for n in reversed(self.nodes):
            if not isinstance(n, PoolNode) and n.dst in need:
                need.update(node_inputs(n))
        prefix, suffix = [], []
        for n in self.nodes:
            if isinstance(n, PoolNode) or n.dst not in need:
                suffix.append(n)
                continue
            ok = (isinstance(n, ConvNode) and n.kd == 1 and not getattr(n, 'tvalid', False)) or isinstance(n, UpcatNode)
            assert ok and n.fr == self._k, "%s (%s) upstream of a join is not per-frame" % (n.name, type(n).__name__)
            m = copy.copy(n)
            m.fr = 1
            prefix.append(m)
        for n in suffix:
            if isinstance(n, PoolNode):
                assert n.K == self._k and self.tensors[n.src][3] == self._k and self.tensors[n.dst][3] == 1, n.name
            else:
                assert isinstance(n, (ConvNode, UpcatNode)) and n.fr == 1 and not (set(node_inputs(n)) & need), \
                    "%s behind the joins reads a per-frame tensor" % n.name
        return prefix, suffix

    def _build_stream(self, Bc, H, W, S):
        """The two programs of detect_video (infer_plan.InferPlan.build_stream), in the precision set on the net."""
        return infer_plan.InferPlan(self, H, W, self.precision == 'bf16').build_stream(Bc, S)

    def _stage_frames(self, dst, frames, a, b):
        """frames [a, b) of the clip -> the first rows of the NCHW input tensor `dst`, normalised as net(x) does; the rows
        behind them repeat the last one (a padded row must hold real data: the fp32 operand scales are per tensor)"""
        n = b - a
        if frames.dtype == torch.uint8:
            self._preprocess_u8(self._frames_to_device(frames[a:b]), dst, n)
        else:
            dst[:n].copy_(frames[a:b])
        if n < dst.shape[0]:
            dst[n:].copy_(dst[n - 1:n].expand(dst.shape[0] - n, -1, -1, -1))

    def detect_video(self, frames, step=1, chunk=8, seq_nms=None, track=None, tubelet=None, smooth=None, stitch=None,
                     overlay=None):
        """Detect on every frame of ONE clip: frames (T,3,H,W) float or (T,H,W,3) uint8 -> ids (T,post_nms,1), scores
        (T,post_nms,1), bboxes (T,post_nms,4), what net(windows) returns on the T windows the VID dataset would build
        (stream_window_slots: imgnetvid.py:486-506) - with the per-frame part of the network run ONCE per frame.

        The graph is split at the joins (_stream_split).  The prefix runs on the frames that are not yet in a ring of
        S = chunk + 2*(K//2)*step slots per join source (slot = frame mod S); per chunk of output frames the slot table of
        its windows is uploaded, the joins read the ring in place (vd_stream.hip) and the suffix runs at batch `chunk`.  A
        shorter last chunk runs the same programs on padded rows (repeats of its last real row) whose outputs are dropped.
        Honours set_precision, set_nms and agnostic; k = 1 is plain batched detection in chunks.  `stream_stats` counts the
        frames that went through each part in the last call; last_rows / last_overflow cover the T frames.  With
        `stream_keep_heads` set on the net, `stream_heads` keeps the three raw head tensors of the T frames (k > 1).

        seq_nms: None (the default: the call as it always was), True, or a dict of link_thresh / nms_thresh / rescore - the
        finished clip's rows go through sequence NMS on the device (ops.seq_nms): the rescored, re-sorted
        tensors are returned, last_rows follows the permutation and last_plain holds the three tensors ahead of it.  A
        further key `clip` (a number) clips the boxes to [0, clip] first, as detect_yolo3.py clips the boxes it saves.

        track: None (the default), True, or a dict of sigma_l / sigma_h / sigma_iou / t_min / max_age (and `clip`, as above) -
        the rows the call returns are linked into tracks on the device (ops.track; with seq_nms: the rescored,
        re-sorted rows).  The returned tensors are what the call returns without it; last_tracks = (track, tlen, tscore),
        each (T,post_nms), holds the result and is None after a call without `track`.  A further key `method`: 'iou' (the
        default, the IOU tracker) or 'sort' (SORT: Kalman prediction and an optimal assignment, ops.track_sort, DESIGN.md 34;
        the missing parameters then take viddet_amd.sort's defaults, sigma_iou 0.3 and max_age 1) or 'byte' (BYTE: SORT with
        a second association of the low-score rows, ops.track_byte; it takes sigma_d, sigma_new and sigma_iou2
        as well, and the missing parameters take viddet_amd.byte's defaults); with 'sort' and 'byte' last_track_boxes
        (T,post_nms,4) holds the filtered box of every tracked row, otherwise it is None.  With 'sort', a further key
        `appearance`: True or {'level': 8 | 16 | 32, 'sigma_app': a, 'sigma_prox': p} - every chunk's rows get an int8
        descriptor pooled from the backbone's route tensor of that stride under their boxes (ops.roi_embed; the plain plan's
        buffer with k = 1, the feature ring of an early join with k > 1) and the tracker links on the fused cost of geometry
        and appearance (ops.track_sort_app).  last_embeddings (T,post_nms,C) int8 holds the descriptors and is
        None after a call without the key; with 'keep_maps': True (tests) last_app_maps holds a clone of the maps every
        launch read, in frame order.  Refused with 'iou' and 'byte', beside seq_nms (it permutes the rows ahead of the
        tracker), with a late join (its ring holds neck tips, not routes) and by open_video.  With any method, a further key
        `gmc`: True or {'cell': 2 | 4 | 8 | 16, 'radius': 1..16, 'gate': g} - camera-motion compensation: the
        translation of the whole picture between consecutive frames is estimated from the uint8 frames' luma (RGB, or NV12
        under set_device_resize(source='nv12'); ops.motion_signature in slices of `chunk` frames - a host clip is uploaded
        a second time, slice by slice - then one ops.motion_match), summed along the clip and taken off the boxes the tracker
        and `stitch` link (ops.motion_shift, after the `clip` clamp); last_track_boxes is put back into image coordinates.
        The three returned tensors are those of the call without the key; last_motion = (motion (T,2) int32 in source
        pixels, sad (T,2) int64) and is None after a call without it.  Composes with seq_nms (which runs ahead, on image
        coordinates) and overlay; refused beside smooth and tubelet (they emit boxes), with float frames, with a frame too
        small for `radius`, and by open_video.

        tubelet: None (the default), True, or a dict of rescore / max_gap / drop_untracked; needs `track` - the rows the tracker
        saw (those of Seq-NMS where that is on, clipped where track's `clip` is given) go through the tubelet pass on the device
        (ops.tubelet): the rows of a track take its score, the frames it skipped get an interpolated box, every
        frame is re-sorted, and those three tensors are returned.  last_pre_tubelet holds the three tensors ahead of the pass,
        last_tracks stays ops.track's result on them, last_tubelet = (perm, track_out, dropped), last_rows follows perm (-1 on
        filled and empty rows).  A call without it sets last_tubelet to None.  open_video takes no such argument: a hole is
        known only once its track resumes, after the frame has been given out.

        smooth: None (the default), True, or {'max_gap': g}; needs `track` - the boxes the tracker saw are smoothed along its
        tracks on the device (ops.smooth, DESIGN.md 37: the Rauch-Tung-Striebel smoother of SORT's Kalman filter, every box
        estimated from the frames before and after it; a track is cut where it skips more than max_gap frames).  The order is
        Seq-NMS -> track -> smooth -> tubelet: the smoothed boxes replace the tracker's in what is returned and in what the
        tubelet pass gets; ids and scores are untouched.  last_pre_smooth holds the boxes ahead of the pass, last_smooth its
        slen (T,post_nms); both are None after a call without it.  last_tracks and last_track_boxes are as without it.

        stitch: None (the default), True, or {'max_gap': g, 'sigma_iou': s}; needs `track` - the fragments a tracker leaves
        where an object was missed for more than max_age frames are re-linked on the device (ops.stitch, DESIGN.md 38: every
        track's filter state at its last row is extrapolated over up to max_gap frames and matched to the first rows of later
        tracks).  The order is Seq-NMS -> track -> stitch -> smooth -> tubelet, so the later passes take the stitched table.
        last_pre_stitch holds the tracker's (track, tlen, tscore), last_tracks the stitched triple, last_stitch = (stitches,
        overflow), each (1,); last_track_boxes stays the tracker's.  A call without it sets last_stitch and last_pre_stitch to
        None.  open_video takes no such argument: a fragment's successor is known only later.

        overlay: None (the default), True, or a dict of thresh / thickness / scale / trail / color_by / class_names / palette /
        gt / inplace; needs uint8 frames - what the call returns is drawn onto the frames on the device (ops.overlay, DESIGN.md
        41): rings, tags of class, score and track id, trails along the final track table (last_tubelet[1] where the tubelet
        pass ran, else last_tracks[0]; none without `track`), ground truth `gt` (T,G,>=5) in green underneath.  The boxes are
        in the network's coordinates (set_device_resize's target, else the frames' own size) and the frames keep their source
        size; NV12 frames follow set_device_resize(source='nv12')'s matrix and range.  last_overlay = (frames_out, painted):
        a painted copy of the frames on the device (with inplace, device frames only: the caller's tensor itself) and the
        painted pixels of every frame; None after a call without it.  The three returned tensors are those of the call without
        it.  open_video takes no such argument: a session gives its frames back before their rows."""
        from .live import detect_video
        return detect_video(self, frames, step, chunk, seq_nms, track, tubelet, smooth, stitch, overlay)

    def open_video(self, step=1, chunk=8, track=None, smooth=None):
        """A live.VideoSession on this net: detect_video(step, chunk, track) on a clip whose frames arrive a few at a time and
        whose length nobody knows - session.push(frames) returns the detections that are final by now, session.flush() ends
        the clip.  Refused where detect_video is, in the same words, and while another session of this net has
        frames in flight.  Seq-NMS has no online form and is no option here; nor is the tubelet pass: a hole is
        known only once its track resumes, after the frame has been given out.  The `smooth` option of detect_video (DESIGN.md
        37) is none here either: a frame's smoothed box needs the frames after it - but smooth={'lag': L} or {'lag': L,
        'max_gap': g} (L in [0, 15]; needs `track`; True is refused, a latency must be chosen) is its fixed-lag form
        (ops.SmoothLagState): every frame comes out L frames later, its boxes smoothed along the online tracker's
        tracks against the frames before it and the L frames after it; session.last_pre_smooth / last_smooth hold the boxes
        ahead of the pass and slen.  Nor is `stitch` an option: a fragment's
        successor is known only later.  track={'method': 'sort'} and
        track={'method': 'byte'} raise NotImplementedError unless the dict also says 'online': True (a bool, this method's
        word alone): the session then carries that tracker from push to push on the device (ops.KalmanTrackState, DESIGN.md
        39) and keeps the filtered boxes of the emitted frames in session.last_track_boxes."""
        if self._live is not None:
            raise RuntimeError("open_video: %r has frames in flight on this net: flush() it first" % (self._live,))
        from .live import VideoSession
        return VideoSession(self, step, chunk, track, smooth)

    def extract_features(self, x):
        """extract_base_features.py:127-130: f1 = features[:15](x), f2 = features[15:24](f1), f3 = features[24:](f2) in
        inference mode (BatchNorm on running statistics) -> three NCHW fp32 tensors (B,256,H/8,W/8), (B,512,H/16,W/16),
        (B,1024,H/32,W/32), the inputs of the no-backbone network."""
        if self.noback or self._k > 1 or self._conv_types:
            raise NotImplementedError("extract_features is the per-frame Darknet-53 trunk of the full k=1 network")
        B, H, W = self._in_shape(x)
        key = ('features', B, H, W)
        if key not in self._programs:
            self._programs[key] = infer_plan.InferPlan(self, H, W, False).build_features(B)
        prog, bufs = self._programs[key]
        self._refresh_fold()
        self._refresh_wamax()
        self._stage_inputs(bufs, x)
        prog.run()
        return tuple(bufs[nm].permute(0, 3, 1, 2).contiguous() for nm, _, _ in ROUTE_TENSORS)

    # ------------------------------------------------------------------ training forward / backward
    def _syncbn(self, n):
        if not self.syncbn_scope or not torch.distributed.is_available() or not torch.distributed.is_initialized():
            return False
        # (VD_FORCE_DIST=1, bench.py / tests: the exchange runs on a single rank too - the RCCL call pattern of an N-rank job)
        if torch.distributed.get_world_size(self.process_group) < 2 and os.environ.get("VD_FORCE_DIST", "0") != "1":
            return False
        if self.syncbn_scope == 'all':
            return True
        # 'reference': --syncbn only reaches the stem and the 5 stride-2 convs
        return n.stem or n.stride == 2

    def _build_train(self, B, H, W):
        """The training plan at one shape (train_plan.TrainPlan): forward with the BatchNorm statistics, the loss, then the
        fixed reverse pass, as segments of launch records, with the buffers and workspaces they point into."""
        return train_plan.TrainPlan(self, B, H, W).build()

    # ------------------------------------------------------------------ bf16-STORAGE training (BASELINE configs[4])
    def set_storage(self, storage):
        """Storage type of the TRAINING activations and their gradients: 'fp32' (default: the reference's arithmetic,
        train_yolov3.py:623-636) or 'bf16' - conv outputs, cell outputs and both gradient families are bf16 tensors, the
        convolutions run one bf16 MFMA per product block with fp32 accumulation (vd_conv_igemm_bf16 / VD_STORE_BF16),
        BatchNorm statistics come from the fp32 accumulators; master weights, weight gradients, BatchNorm vectors, head
        logits, losses and the optimiser stay fp32.  No reference counterpart: judged against the fp32 oracle at a stated
        bf16 tolerance (tests/test_bf16_train_gpu.py, test_model_gpu.py)."""
        if storage not in ('fp32', 'bf16'):
            raise ValueError("storage must be 'fp32' or 'bf16'")
        if storage == 'bf16' and getattr(self, '_conv_types', None):
            raise NotImplementedError("bf16-storage training is not built for conv_types networks: the temporal-conv kernels "
                                      "(vd_tdw.hip) are fp32 only")
        if storage == 'bf16' and getattr(self, '_rnn_pos', None):
            raise NotImplementedError("bf16-storage training is not built for rnn_pos networks: the ConvGRU gate kernels "
                                      "(vd_gru.hip) and the recurrent state are fp32 only")
        if storage == 'bf16' and (self.noback or self.temporal_out or getattr(self, 'temporal_side', False)):
            raise NotImplementedError("bf16-storage training is built for yolo3_darknet53 and the k > 1 windows of YOLOV3T (every "
                                      "join, neck and correlation variant), not for the noback, temporal_out and temporal_side "
                                      "networks")
        self.storage = storage

    def _tune_bf16_desc(self, d, of32):
        """Tile (and halo / generic loop) of one vd_conv_igemm_bf16 launch record, timed in place; persisted like the others."""
        if os.environ.get("VD_AUTOTUNE", "1") == "0":
            return
        base = d.flags & ~(L.MATH_NOHALO | L.CONV_STREAMK)
        key = ('bf16', d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.in_stride, d.T, d.Co, base, of32, d.out_stride, bool(d.stats_part),
               bool(d.bs_part)) + ((d.Kfr,) if d.Kfr > 1 else ())      # (frame taps: the 3-D / 2+1-D neck convs of a window)
        # training: the patch kernel is the forward with fused statistics; no 256-row tiles under the fused BatchNorm-
        # backward reductions; the halo loop only for an unstrided output (a parity launch of a stride-2 data gradient has none)
        _tune_bf16_record(d, of32, key, *_bf16_tile_candidates(d, of32, patch_kernel=bool(d.stats_part and not d.bs_part),
                                                               tall_tiles=not d.bs_part, halo=d.out_stride == 1))

    @staticmethod
    def _flops(n, B, H, W, kind, esz=4):
        """Algorithmic FLOPs of one conv launch: 2*Cin*Cout*k*k*Ho*Wo per image; `esz` = bytes per element."""
        px_in = B * n.fr * (H // n.div_in) * (W // n.div_in)
        px_out = B * n.fr * (H // n.div_out) * (W // n.div_out)
        return dict(kind=kind, node=n.name, k=n.k, stride=n.stride,
                    flops=2.0 * n.cin * n.cout * n.kd * n.k * n.k * px_out,
                    # algorithmic bytes: every operand tensor once (input, output/gradient, weights)
                    bytes=float(esz) * (px_in * n.cin + px_out * n.cout + n.cout * n.cin * n.kd * n.k * n.k))

    @staticmethod
    def _corr_meta(n, B, xs, kind, esz=4):
        """roofline record of a correlation launch: 2 flops per (pixel, displacement, channel) and side frame (x2 backward:
        both operands' gradients); bytes = the operands read once and the result written once"""
        px = B * xs.shape[1] * xs.shape[2]
        D2 = (2 * n.d + 1) ** 2
        flops = 2.0 * px * (n.K - 1) * D2 * n.C * (2 if kind == 'bwd' else 1)
        byt = float(esz) * px * (n.K * n.C + n.ldy) * (2 if kind == 'bwd' else 1)
        return dict(kind='corr_' + kind, flops=flops, bytes=byt)

    def _ones(self, c):
        """c ones (_zeros: c zeros): the first c elements of one 1024-element constant, wide enough for every tensor of
        today's networks (1024 channels); a wider one fails here, when the plan is built"""
        assert c <= 1024, "constant vectors hold 1024 channels, asked for %d" % c
        if not hasattr(self, '_const'):
            self._const = (torch.ones(1024, device=self.device), torch.zeros(1024, device=self.device))
        return self._const[0]

    def _zeros(self, c):
        self._ones(c)
        return self._const[1]

    def _refresh_dgrad(self, tp, overlap=False):
        """Re-pack the data-gradient weight layout after the weights moved. With overlap=True (start of a training
        step) the 72 small pack launches run on a side stream beside the forward pass; backward() waits on the event.
        A bf16-storage plan first gets the bf16 image of the weight arena its forward convs read, on the main stream:
        the forward pass needs it before anything else."""
        if tp.get('dgrad_version') == self._weights_version:
            return
        if tp['wb_arena'] is not None:
            L.check(L.load().vd_pack_weight_bf16(self.weights.data_ptr(), tp['wb_arena'].data_ptr(), 1, 1, self.n_weight,
                                                 self.n_weight, 1, L.stream_ptr()), 'vd_pack_weight_bf16')
        ev = None
        if overlap and self.overlap_wgrad:
            if self._pack_stream is None:
                self._pack_stream = torch.cuda.Stream()
            cur = torch.cuda.current_stream()
            self._pack_stream.wait_stream(cur)          # the optimiser's weight update is on the main stream
            with torch.cuda.stream(self._pack_stream):
                for n, plan, wpk in tp['dgrad_packs']:
                    self._pack_dgrad(n, plan, wpk)
                ev = torch.cuda.Event()
                ev.record(self._pack_stream)
        else:
            for n, plan, wpk in tp['dgrad_packs']:
                self._pack_dgrad(n, plan, wpk)
        self._pack_event = ev
        tp['dgrad_version'] = self._weights_version

    @staticmethod
    def _pack_dgrad(n, plan, wpk):
        if wpk.dtype == torch.bfloat16:     # bf16 storage: straight to bf16 [cin][T * K pitch]
            T = len(plan['taps'])
            arr = (C.c_int32 * T)(*plan['tap_ids'])
            L.check(L.load().vd_pack_weight_dgrad_bf16(n.wp.data_ptr(), wpk.data_ptr(), n.co_pad, wpk.numel() // (n.cin * T),
                                                       n.cin, n.kd, n.k, n.k, arr, T, 1, L.stream_ptr()), 'vd_pack_weight_dgrad_bf16')
        elif plan.get('fused_s2'):          # the one-launch form of a stride-2 data gradient (VD_CONV_PARITY4)
            ops.pack_weight_dgrad_s2(n.wp, wpk, Co=n.co_pad, Co_pad=n.co_pad, Ci=n.cin)
        else:
            ops.pack_weight_dgrad(n.wp, wpk, Co=n.co_pad, Co_pad=n.co_pad, Ci=n.cin, kd=n.kd, kh=n.k, kw=n.k,
                                  tap_ids=plan['tap_ids'], src_packed=True)

    @staticmethod
    def _run_segments(segs):
        for s in segs:
            if isinstance(s, Program):
                s.run()
            else:
                s()

    def single_conv_consumer_tensors(self):
        """Outputs of Conv+BN+LeakyReLU cells (no residual) that are read by exactly one node, a convolution: the cells whose
        forward BatchNorm apply could move into the consumer's operand gather (bench.py reports their share)."""
        if getattr(self, '_scc', None) is None:
            self._scc = single_conv_consumers(self.nodes)
        return self._scc

    def _drop_plans(self, keep=None):
        """Forget every cached plan (programs, activation / gradient buffers, graphs) except `keep`, and return their
        memory to the driver."""
        for k in [k for k in self._programs if k != keep]:
            del self._programs[k]
        self._graph_cache.clear()
        self._last_train = None
        import gc
        gc.collect()
        torch.cuda.empty_cache()

    def _build_or_evict(self, build):
        """Build a plan; when it does not fit beside the cached ones, drop those and build again.  The retry runs AFTER the
        except block: inside it the live exception's traceback still holds the failed build's frame - its half-allocated
        buffers - so empty_cache() could not return them and the second build needed room for one and a half plans."""
        try:
            return build()
        except torch.cuda.OutOfMemoryError:
            pass
        self._drop_plans(keep=None)
        return build()

    def _forward_train(self, x, gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t):
        B, H, W = self._in_shape(x)
        bf16s = getattr(self, 'storage', 'fp32') == 'bf16'
        key = ('train_bf16' if bf16s else 'train', B, H, W)
        if key not in self._programs:
            # every input shape owns its plan and buffers (random-shape training visits ten); when the next one does not
            # fit beside the others, drop those and build again - their kernel choices stay in the tuning cache
            self._programs[key] = self._build_or_evict(lambda: self._build_train(B, H, W))
        tp = self._programs[key]
        f32 = lambda t: t.to(device=self.device, dtype=torch.float32).contiguous()
        gt, obj, ctr, scl, wgt, cls = [f32(t) for t in (gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t)]
        if self.temporal_out:
            # yolo3_temporal.py:521-533: frame t of window b is matched against ITS targets (args sliced on axis 1);
            # folded here as image b*t_len + t, the order the frames already have
            K = self._k
            for t in (gt, obj, ctr, scl, wgt, cls):
                if t.dim() < 3 or t.shape[0] != B or t.shape[1] != K:
                    raise ValueError("per-frame targets are (B,%d,...) tensors, got %s" % (K, tuple(t.shape)))
            gt, obj, ctr, scl, wgt, cls = [t.reshape((B * K,) + tuple(t.shape[2:])) for t in (gt, obj, ctr, scl, wgt, cls)]
        tp['live'] = (gt, obj, ctr, scl, wgt, cls)
        s = tp['slots']
        s['gt'].value, s['M'].value = gt.data_ptr(), int(gt.shape[1])
        s['obj'].value, s['ctr'].value, s['scl'].value = obj.data_ptr(), ctr.data_ptr(), scl.data_ptr()
        s['wgt'].value, s['cls'].value = wgt.data_ptr(), cls.data_ptr()
        s['smooth'].value = 1 if self._label_smooth else 0
        self._stage_inputs(tp['bufs'], x)
        self._refresh_wamax()
        self._refresh_dgrad(tp, overlap=True)
        self._run_segments(tp['fwd'])
        self._fold_dirty = True            # running stats moved
        self._stats_version += 1
        self._last_train = tp
        L_ = tp['losses']
        if self.temporal_out:
            # :535 [F.mean(F.concat(*l, dim=0)) for l in losses]: four scalars, means over the B*t per-frame losses.
            # backward() computes the gradient of the SUM of the per-frame losses; the 1/(B*t) of the mean is a
            # common factor of the whole gradient and is applied with the optimiser's rescale (sgd_step)
            self._grad_scale = 1.0 / float(L_.shape[0])
            m = L_.mean(dim=0)
            return m[0], m[1], m[2], m[3]
        self._grad_scale = 1.0
        return L_[:, 0], L_[:, 1], L_[:, 2], L_[:, 3]

    def backward(self):
        """autograd.backward(sum_losses) (train_yolov3.py:631): gradient of the sum of all four losses over the
        local batch wrt every parameter, written into the gradient arena."""
        tp = self._last_train
        self._refresh_dgrad(tp)            # only if the weights moved between the forward and this call
        if self._pack_event is not None:
            torch.cuda.current_stream().wait_event(self._pack_event)
            self._pack_event = None
        self._run_segments(tp['bwd'])

    # ------------------------------------------------------------------ call protocol
    def __call__(self, x, *args):
        if self.noback:
            # YOLOV3_noback.hybrid_forward(x1, x2, x3, *args) (yolo3.py:1782): three feature maps, then the targets
            if len(args) < 2:
                raise TypeError("the no-backbone network is called as net(x1, x2, x3[, gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t])")
            feats, args = (x, args[0], args[1]), args[2:]
            for t, (nm, c_, d_) in zip(feats, ROUTE_TENSORS):
                if t.dim() != 4 or t.shape[1] != c_:
                    raise ValueError("expected a (B,%d,H/%d,W/%d) feature map, got %s" % (c_, d_, d_, tuple(t.shape)))
            if len(args) == 0:
                return self._forward_infer(feats)
            if len(args) != 6:
                raise TypeError("training call takes (x1, x2, x3, gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t)")
            return self._forward_train(feats, *args)
        if self._dev_nv12 is not None:              # NV12 frames (B[,K],H0*3/2,W0); _in_shape refuses every other mistake by name
            if x.dtype == torch.uint8 and not (x.dim() >= 4 and x.shape[-1] == 3) and \
                    (x.dim() != (4 if self._k > 1 else 3) or (self._k > 1 and x.shape[1] != self._k)):
                raise ValueError("set_device_resize(source='nv12') is on: expected NV12 frames (B,%sH0*3/2,W0), got %s"
                                 % ("%d," % self._k if self._k > 1 else "", tuple(x.shape)))
        elif x.dtype == torch.uint8:
            if x.dim() != (5 if self._k > 1 else 4) or x.shape[-1] != 3 or (self._k > 1 and x.shape[1] != self._k):
                raise ValueError("expected uint8 frames (B,%sH,W,3), got %s" % ("%d," % self._k if self._k > 1 else "", tuple(x.shape)))
        elif self._k > 1:
            if x.dim() != 5 or x.shape[1] != self._k or x.shape[2] != 3:
                raise ValueError("expected a (B,%d,3,H,W) window batch, got %s" % (self._k, tuple(x.shape)))
        elif x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("expected a (B,3,H,W) batch, got %s" % (tuple(x.shape),))
        if len(args) == 0:
            return self._forward_infer(x)
        if len(args) != 6:
            raise TypeError("training call takes (x, gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t)")
        return self._forward_train(x, *args)

    # ------------------------------------------------------------------ optimiser / DP hooks
    def _dp_active(self):
        return torch.distributed.is_available() and torch.distributed.is_initialized() and \
            (torch.distributed.get_world_size(self.process_group) > 1 or os.environ.get("VD_FORCE_DIST") == "1")

    def _bucket_launcher(self, lo, hi, side):
        def f():
            if not self._dp_active() or getattr(self, '_dp_suppress', False):     # (bench.py times a collective-free backward)
                return
            self._dp_stats['buckets'] += 1
            self._dp_stats['bucket_bytes'] += 4 * (hi - lo)
            st = side if side is not None else torch.cuda.current_stream()
            with torch.cuda.stream(st):
                h = torch.distributed.all_reduce(self.grads[lo:hi], group=self._bucket_group or self.process_group,
                                                 async_op=True)
            self._pending_reduces.append(h)
            self._reduced_from = min(self._reduced_from, lo)
        return f

    def allreduce_grads(self):
        """kvstore-'local' replacement (train_yolov3.py:530): RCCL sum all-reduce of the flat gradient arena.
        With bucketing (default) the conv-weight range was already queued in ~32 MB pieces during backward();
        here the handles are awaited and the remaining small range (gamma, beta, head bias) is reduced."""
        if not self._dp_active() or getattr(self, '_dp_suppress', False):
            return
        wt = [m.w_off for m in self.conv_nodes if self._node_trainable(m)[0]]
        wt_lo = min(wt) if wt else self.n_weight             # frozen prefix (freeze_base): zeros, never reduced
        if self._pending_reduces:
            for h in self._pending_reduces:
                h.wait()
            self._pending_reduces = []
            lo = self._reduced_from
            self._reduced_from = self.n_params
            if lo > wt_lo:                               # anything before the first bucket (not expected)
                torch.distributed.all_reduce(self.grads[wt_lo:lo], group=self.process_group)
            torch.distributed.all_reduce(self.grads[self.n_wconv:], group=self.process_group)
        else:
            torch.distributed.all_reduce(self.grads[wt_lo:], group=self.process_group)

    def sgd_step(self, lr, momentum, wd, batch_size, no_wd=False):
        """gluon.Trainer('sgd').step(batch_size) (train_yolov3.py:527-530,634) over the trainable parameters only
        (grad_req 'null' => no update and no weight decay, wrappers.py:55-57), with each parameter's lr_mult / wd_mult;
        `no_wd=True` is shorthand for wd_mult = 0 on gamma / beta / bias (--no_wd, :495-497)."""
        rescale = self._grad_scale / float(batch_size)
        nw = self.n_weight
        for lo, hi, lr_mult, wd_mult in self._optimizer_ranges():
            wd_ = 0.0 if (no_wd and lo >= nw) else wd * wd_mult
            ops.sgd_momentum(self.weights[lo:hi], self.grads[lo:hi], self.momentum_buf[lo:hi], lr * lr_mult, momentum,
                             wd_, rescale)
        self._params_changed()

    # ------------------------------------------------------------------ checkpoints
    def state_arrays(self):
        return OrderedDict((k, p.data().cpu().numpy()) for k, p in self._params.items())

    def save_parameters(self, path):
        from .params_io import save_params
        save_params(path, self.state_arrays())

    def inflate_from_2d(self, src):
        """get_darknet's transfer of 2-D weights (three_darknet.py:289-318), extended to the whole detector: `src` is a
        k = 1 yolo3_darknet53 network or its {name: array} dict.  Spatial and 1x1x1 weights are the 2-D weights with a unit
        time axis (the reference divides by shape[-3] = 1), BatchNorm parameters and running statistics are copied, every
        temporal weight becomes 1/3 in its three taps, the neck and heads are copied by name.  A window of K equal frames
        then reproduces the 2-D network (the three taps see the same frame whatever the padding repeats)."""
        if not self._conv_types:
            raise NotImplementedError("inflate_from_2d is the weight transfer of a conv_types network (yolo3_3ddarknet)")
        if isinstance(src, YOLOV3):
            if src._k != 1 or src.noback or getattr(src, '_conv_types', None):
                raise ValueError("inflate_from_2d takes the plain k = 1 yolo3_darknet53 network")
            src = {k_: p.data() for k_, p in src.collect_params().items()}
        pool_at = [n.feature_index for n in self.nodes if isinstance(n, PoolNode) and n.name == 'pool.trunk'][0]
        to2d = {}
        for f in range(29):                  # features index of the 2-D network -> this network's (the pool takes one)
            to2d["d_model.features.%d." % (f + (1 if f >= pool_at else 0))] = _feature_name(f) + "."
        for name, p in self._params.items():
            if name.endswith(".3.conv.weight"):
                p.set_data(torch.full(p.shape, 1.0 / p.shape[2]))
                continue
            key = name
            if name.startswith("d_model."):
                pre = name[:name.index(".", len("d_model.features.")) + 1]
                key = to2d[pre] + name[len(pre):]
            if key not in src:
                raise KeyError("inflate_from_2d: %s (for %s) is missing in the 2-D network" % (key, name))
            v = torch.as_tensor(np.asarray(src[key].detach().cpu() if torch.is_tensor(src[key]) else src[key]), dtype=torch.float32)
            if len(p.shape) == 5 and v.dim() == 4:
                v = v.unsqueeze(2)
            p.set_data(v)

    def load_parameters(self, path, allow_missing=False, ignore_extra=False):
        from .params_io import load_params
        arrs = load_params(path)
        for k, p in self._params.items():
            if k in arrs:
                p.set_data(torch.from_numpy(np.ascontiguousarray(arrs[k], dtype=np.float32)))
            elif not allow_missing and not re.search(r"(anchor|offset)", k):
                raise KeyError("parameter %s missing in %s" % (k, path))
        if not ignore_extra:
            extra = [k for k in arrs if k not in self._params and not re.search(r"(anchor|offset)", k)]
            if extra:
                raise KeyError("unexpected parameters in %s: %s" % (path, extra[:5]))


def yolo3_darknet53(classes, pretrained_base=False, norm_layer=None, norm_kwargs=None, freeze_base=False,
                    k=None, k_join_type=None, k_join_pos=None, block_conv_type='2', temporal=False, t_out=False,
                    corr_d=None, corr_pos=None, rnn_pos=None, agnostic=False, **kwargs):
    """wrappers.py:9-110 -> YOLOV3T (yolo3.py:959-1054).  norm_layer='syncbn' (the reference passes
    SyncBatchNorm) selects the SyncBN collective.  k>1 builds the temporal-window variants; `t_out=True`
    (--temp --mult_out) builds YOLOV3Temporal with per-frame outputs (yolo3_temporal.py:286-555, t = k = 5)."""
    k = 1 if k is None else int(k)
    if agnostic:
        # class-agnostic detection (wrappers.py:101-103 hands `agnostic` to YOLOV3T): what is refused is refused by name
        if temporal or t_out:
            raise NotImplementedError("agnostic with temporal / t_out: YOLOV3Temporal is not passed the flag (wrappers.py:96-98)")
        if rnn_pos == 'out':
            raise NotImplementedError("agnostic with rnn_pos 'out': its predictions come from YOLOOutputV3's own RNN output "
                                      "block (yolo3.py:1040-1042), a tail of its own that is not built agnostic")
        kwargs = dict(kwargs, agnostic=True)
    if rnn_pos is not None:
        # the bidirectional ConvGRU (RNN, layers.py:267-306; yolo3.py:978-988): what is built, and what is refused by name
        if rnn_pos not in ('late', 'out'):
            raise ValueError("rnn_pos must be None, 'late' or 'out', got %r" % (rnn_pos,))
        if temporal or t_out:
            raise NotImplementedError("rnn_pos with temporal / t_out: YOLOV3Temporal has no RNN (yolo3_temporal.py)")
        if k < 2:
            raise NotImplementedError("rnn_pos needs a window of k > 1 frames: the GRU runs over the K frames (k = %d)" % k)
        if block_conv_type != '2':
            raise NotImplementedError("rnn_pos with block_conv_type %r: the reference swaps axes 1 and 2 of the RNN output "
                                      "there, so the join would pool over channels; block_conv_type '2' only" % (block_conv_type,))
        if corr_pos is not None:
            raise NotImplementedError("rnn_pos with corr_pos: the correlation join and the RNN are not combined (the "
                                      "reference's `elif` never reaches Corr behind a late join, and 'out' skips every join)")
        if rnn_pos == 'late' and (k_join_pos != 'late' or k_join_type not in ('max', 'mean', 'cat')):
            raise NotImplementedError("rnn_pos 'late' needs k_join_pos 'late' and k_join_type max / mean / cat "
                                      "(yolo3.py:986-988)")
        if rnn_pos == 'out' and k_join_type not in ('max', 'mean'):
            raise NotImplementedError("rnn_pos 'out' needs k_join_type max or mean: TemporalPooling joins the K predictions "
                                      "and asserts it (layers.py:168), got %r" % (k_join_type,))
        if rnn_pos == 'out':
            k_join_pos = k_join_pos or 'late'                     # not read: 'out' guards every early / late join
    if temporal or t_out:                                         # wrappers.py:96-98
        if corr_d:
            raise NotImplementedError("YOLOV3Temporal with a correlation branch (corr_d) is outside the built scope")
        assert k == 5, "Currently only support t=5 but will increase to more later"        # yolo3_temporal.py:399
        assert block_conv_type in ('2', '3', '21')
        scope = (norm_kwargs or {}).get('scope', 'all') if norm_layer == 'syncbn' else None
        if not t_out:
            # --temp without --mult_out (yolo3_temporal.py:326-333,436-447): strided 2+1-D side branches, ONE output for the
            # centre frame.  The detection blocks get the squeezed (B,C,h,w) routes, so only the 2-D blocks are defined
            # (a 3-D block would be handed a 4-D tensor in the reference as well).
            if block_conv_type != '2':
                raise NotImplementedError("YOLOV3Temporal(t_out=False) squeezes the frame axis before the detection blocks: "
                                          "block_conv_type must be '2'")
            net = YOLOV3(classes, syncbn_scope=scope, k=k, temporal_side=True, **kwargs)
        else:
            net = YOLOV3(classes, syncbn_scope=scope, k=k, block_conv_type=block_conv_type, temporal_out=True, **kwargs)
        if freeze_base:
            for name, p in net.collect_params('stages.*').items():
                p.grad_req = 'null'
        return net
    # yolo3.py:978-985
    if block_conv_type in ('3', '21'):
        assert k > 1, "k must be greater than 1 to use 3D or 2+1D convolutions"
        assert k_join_pos == 'late', "only 'late' pooling can be used when using 3D or 2+1D convolutions"
        assert k_join_type is not None, "please specify a k_join_type: max, mean, or cat"
    assert block_conv_type in ('2', '3', '21')
    assert k_join_type in [None, 'max', 'mean', 'cat']
    assert k_join_pos in [None, 'early', 'late']
    assert corr_pos in [None, 'early', 'late']
    corr = {}
    if k > 1:
        # yolo3.py:1106-1113,1134-1140: `if k_join_pos == pos: join  elif corr_pos == pos: Corr` at each position
        if k_join_pos is None and corr_pos is not None:
            corr = dict(corr_pos=corr_pos, corr_d=int(corr_d or 0))    # k_join_type is not read on this path
            k_join_type = None
        elif k_join_pos is not None and corr_pos is not None and corr_pos != k_join_pos:
            # the join of one position would hand a (B, K*C | C, h, w) tensor to the TimeDistributed blocks of the other
            raise NotImplementedError("k_join_pos %r with corr_pos %r: the reference feeds a 4-D tensor to a TimeDistributed "
                                      "block" % (k_join_pos, corr_pos))
        elif k_join_type is None or k_join_pos is None:
            raise NotImplementedError("k>1 needs k_join_type (max|mean|cat) and k_join_pos (early|late), or corr_pos")
    scope = None
    if norm_layer == 'syncbn':
        scope = (norm_kwargs or {}).get('scope', 'all')
    net = YOLOV3(classes, syncbn_scope=scope, k=k, k_join_type=k_join_type, k_join_pos=k_join_pos,
                 block_conv_type=block_conv_type, rnn_pos=rnn_pos, **corr, **kwargs)
    if freeze_base:                          # wrappers.py:55-57: every Darknet parameter leaves the gradient / update
        for name, p in net.collect_params('stages.*').items():
            p.grad_req = 'null'
    return net


def yolo3_3ddarknet(classes, pretrained_base=False, norm_layer=None, norm_kwargs=None, freeze_base=False,
                    conv_types=(2, 2, 2, 2, 2, 2), k=None, **kwargs):
    """wrappers.py:113-130 -> YOLOV3TB (yolo3.py:1305-1439, k = 1) over Darknet3D (three_darknet.py:126-226): a Darknet-53
    whose stem and first stages are (2+1)-D (`conv_types`: the stem, then the five stages; 21 = a per-frame (1,3,3) conv + BN +
    LeakyReLU followed by a depthwise (3,1,1) conv with repeat padding), run on windows of `k` frames and max-pooled over time
    where the 2-D stages begin.  conv_types all 2 is yolo3_darknet53.  norm_layer='syncbn' reaches the stem and the five
    stride-2 convs only: the blocks are built with plain BatchNorm (three_darknet.py:193), which is scope 'reference'.
    `net.inflate_from_2d(src)` starts it from a trained 2-D detector (get_darknet, three_darknet.py:289-318)."""
    ct = check_conv_types(conv_types, 2 if k is None else k)       # (all 2: no window is needed)
    if ct is not None and kwargs.get('agnostic'):
        raise NotImplementedError("agnostic with conv_types %r: detect_yolo3.py builds yolo3_3ddarknet without the flag "
                                  "(detect_yolo3.py:872-882); the class-agnostic tail is built for yolo3_darknet53" % (ct,))
    if ct is None:
        return yolo3_darknet53(classes, pretrained_base=pretrained_base, norm_layer=norm_layer, norm_kwargs=norm_kwargs,
                               freeze_base=freeze_base, k=k, **kwargs)
    check_conv_types(ct, k)
    scope = None
    if norm_layer == 'syncbn':
        scope = (norm_kwargs or {}).get('scope', 'reference')
        if scope != 'reference':
            raise NotImplementedError("conv_types %r with syncbn scope %r: the blocks of Darknet3D are built with plain "
                                      "BatchNorm (three_darknet.py:193); scope 'reference' only" % (ct, scope))
    net = YOLOV3(classes, syncbn_scope=scope, k=int(k), conv_types=ct, **kwargs)
    if freeze_base:                          # wrappers.py:118-120: every Darknet3D parameter, temporal weights included
        for name, p in net.collect_params('d_model.*').items():
            p.grad_req = 'null'
    return net


def yolo3_no_backbone(classes, norm_layer=None, norm_kwargs=None, **kwargs):
    """wrappers.py:133-161 -> YOLOV3_noback (yolo3.py:1730-1870): neck + heads on cached Darknet-53 feature maps,
    called as net(x1, x2, x3[, targets]) with x1 (B,256,H/8,W/8), x2 (B,512,H/16,W/16), x3 (B,1024,H/32,W/32).
    Parameter names are the transitions.* / yolo_blocks.* / yolo_outputs.* subset of the full network's."""
    scope = None
    if norm_layer == 'syncbn':
        scope = (norm_kwargs or {}).get('scope', 'all')
    return YOLOV3(classes, syncbn_scope=scope, noback=True, **kwargs)


from . import infer_plan, train_plan  # noqa: E402  (last: they import the node classes, Program and the tuners from this module)
