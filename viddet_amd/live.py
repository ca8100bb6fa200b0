"""Streaming video detection on the host: the engine (StreamEngine), detect_video on a whole clip and live
sessions, detect_video on a clip whose frames arrive a few at a time and whose length nobody knows.

`net.open_video(step, chunk, track)` returns a VideoSession.  `push(frames)` takes the next frames and returns the detections
that are final by now, `flush()` ends the clip.  Over any way of cutting a clip into pushes followed by one flush, the
concatenated results are torch.equal to `net.detect_video(clip, step, chunk)`: both run the one engine, in exactly the
launch groups stream.StreamPlanner forms - the fp32 operand scales are per tensor, so any other grouping would round
differently.  With `track`, the emitted rows go through a resumable tracker on the device
(ops.TrackState, vd_track_push; with track={'method': 'sort' | 'byte', 'online': True} ops.KalmanTrackState, vd_track_kf_push,
DESIGN.md 39) whose state survives from push to push.  With `smooth={'lag': L}` the tracked frames go through a fixed-lag
smoother on the device as well (ops.SmoothLagState, vd_track_smooth_push) and come out L frames later.
"""
import numpy as np
import torch

from . import ops
from .appearance import LEVELS as APP_LEVELS
from .appearance import parse_option as parse_appearance
from .appearance import split_appearance
from .motion import check_grid as check_motion_grid
from .motion import frame_size as motion_frame_size
from .motion import grid_size as motion_grid_size
from .motion import parse_option as parse_gmc
from .motion import split_gmc
from .overlay import parse_option as parse_overlay
from .seq_nms import parse_option as parse_seq_nms
from .smooth import parse_option as parse_smooth
from .smooth_lag import parse_option as parse_smooth_lag
from .stitch import parse_option as parse_stitch
from .stream import StreamPlanner
from .track import parse_option as parse_track
from .track import split_online
from .tubelet import parse_option as parse_tubelet


def frame_shape(net, frames, nv12_name, name, d):
    """The frames detect_video ("a clip (T,...") and VideoSession.push ("frames (n,...") accept -> net._in_shape's (n, H, W)"""
    u8 = frames.dtype == torch.uint8
    if net._dev_nv12 is not None and u8:                          # NV12 (n,H0*3/2,W0); _in_shape checks the rest
        if frames.dim() != 3 or frames.shape[0] < 1:
            raise ValueError("set_device_resize(source='nv12') is on: expected %s (%s,H0*3/2,W0) uint8, got %s"
                             % (nv12_name, d, tuple(frames.shape)))
    elif frames.dim() != 4 or frames.shape[0] < 1 or (frames.shape[-1] if u8 else frames.shape[1]) != 3:
        raise ValueError("expected %s (%s,3,H,W), or (%s,H,W,3) uint8, got %s" % (name, d, d, tuple(frames.shape)))
    return net._in_shape(frames)


class StreamEngine:
    """The device half of streaming detection, the one place where the feature ring is written and read:
    detect_video and VideoSession both run their launch groups here.

    run(acts, frames, base, T, hw) runs the actions of `plan` (a stream.StreamPlanner on the net's K, `step` and `chunk`) in
    order.  frames: the clip's frames from frame `base` on, wherever they live - every group is sliced out of them and staged
    from there (net._stage_frames), the clip is never moved to the device as a whole.  T: the clip's length, None while it is
    open.  hw: (H, W) of the network's input.  ('prefix', a, b): frames [a, b) go through the prefix program, their rows
    into the ring slots a % S ..; ('suffix', t0, n): the slot table of the windows of frames [t0, t0 + n) is uploaded and the
    suffix program runs (K = 1: the plain plan at batch `chunk`, a shorter last chunk padded with repeats of its last frame).
    Returns the dict of emitted tensors - ids, scores, bboxes, rows, overflow - as new tensors over the m >= 0 frames of the
    suffix actions.  `stats` counts the frames through each part; with keep_heads, `heads` collects the three raw head
    tensors of every K > 1 suffix launch.  With `appearance` (appearance.parse_option's dict) every suffix action
    is followed by ops.roi_embed on the route tensor of that level - the plain plan's buffer (K = 1) or the feature ring of
    the early join, read in place through the frames' slots - with the program's own ids and bboxes; `embs` collects the
    descriptors of the emitted frames and, with keep_maps, `app_maps` a clone of the maps every launch read, in frame order."""

    def __init__(self, net, step, chunk, appearance=None):
        self.net, self.chunk = net, chunk
        self.plan = StreamPlanner(net._k, step, chunk)
        self.stats = dict(prefix_frames=0, suffix_frames=0, chunks=0)
        self.heads = []
        self.app, self.embs, self.app_maps = appearance, [], []

    def _programs(self, H, W):
        """the two programs at this clip's size, current (K > 1)"""
        net, S = self.net, self.plan.S
        bf16 = net.precision == 'bf16'
        key = ('stream_bf16' if bf16 else 'stream', self.chunk, H, W, S)
        if key not in net._programs:
            net._programs[key] = net._build_or_evict(lambda: net._build_stream(self.chunk, H, W, S))
        sp = net._programs[key]
        if bf16:
            net._bf16_current(sp, sp['packs'], [sp['pre'], sp['suf']])
        else:
            net._refresh_fold()
        net._refresh_wamax()
        return sp

    def _prefix(self, sp, frames, base, a, b):
        S, m = self.plan.S, b - a
        self.net._stage_frames(sp['pb']['in'], frames, a - base, b - base)
        sp['pre'].run()
        for t in sp['srcs']:                                      # rows -> slots (a run of frames wraps at most once: m <= S)
            ring, src = sp['sb']['ring:' + t], sp['pb'][t]
            s0 = a % S
            m0 = min(m, S - s0)
            ring[s0:s0 + m0].copy_(src[:m0])
            if m0 < m:
                ring[:m - m0].copy_(src[m0:m])
        self.stats['prefix_frames'] += m

    def _embed(self, fmap, o, map_index, n):
        """the descriptors of a suffix launch's rows off `fmap` (the level's route tensor: the plan's buffer or the ring)"""
        from .model import ROUTE_TENSORS
        _, c, stride = ROUTE_TENSORS[APP_LEVELS[self.app["level"]]]
        maps = fmap[..., :c]                                      # the plans pad a pixel's pitch: a view, read in place
        self.embs.append(ops.roi_embed(maps, o['ids'], o['bboxes'], stride, map_index=map_index)[:n])
        if self.app["keep_maps"]:                                 # tests: what the launch read, in frame order
            self.app_maps.append((maps[:n] if map_index is None else maps[map_index[:n].long()]).clone())

    def _suffix(self, sp, frames, base, t0, n, T, hw, keep_heads):
        net = self.net
        if net._k == 1:
            # no join, no prefix: the plain plan at batch `chunk`, a shorter last chunk padded with repeats of its last frame
            x = frames[t0 - base:t0 - base + n]
            if n < self.chunk:
                x = torch.cat([x, x[-1:].expand((self.chunk - n,) + tuple(x.shape[1:]))], dim=0)
            net._forward_infer(x)
            prog = net._programs[('infer_bf16' if net.precision == 'bf16' else 'infer', self.chunk) + tuple(hw)]
            o = prog[2]
            if self.app is not None:
                self._embed(prog[1][self._app_name()], o, None, n)
        else:
            sp['slots'].copy_(torch.from_numpy(self.plan.slots(t0, n, T)))
            sp['suf'].run()
            o = sp['o']
            if keep_heads:                                        # tests: the raw head tensors of every chunk
                self.heads.append([sp['sb'][h][:n].clone() for h in net.head_names])
            if self.app is not None:                              # frame t lives in slot t % S; a padded row repeats the last
                S = self.plan.S
                slot = [min(t0 + i, t0 + n - 1) % S for i in range(self.chunk)]
                self._embed(sp['sb']['ring:' + self._app_name()], o, torch.tensor(slot, dtype=torch.int32).to(net.device), n)
        self.stats['suffix_frames'] += n
        self.stats['chunks'] += 1
        return {k: o[k][:n].clone() for k in ('ids', 'scores', 'bboxes', 'rows', 'overflow')}

    def _app_name(self):
        from .model import ROUTE_TENSORS
        return ROUTE_TENSORS[APP_LEVELS[self.app["level"]]][0]

    def run(self, acts, frames, base, T, hw, keep_heads=False):
        net = self.net
        sp = self._programs(*hw) if net._k > 1 and acts else None
        outs = []
        for kind, a, b in acts:
            if kind == 'prefix':
                self._prefix(sp, frames, base, a, b)
            else:
                outs.append(self._suffix(sp, frames, base, a, b, T, hw, keep_heads))
        if outs:
            return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}
        dev, P = net.device, net.post_nms
        return dict(ids=torch.empty(0, P, 1, device=dev), scores=torch.empty(0, P, 1, device=dev),
                    bboxes=torch.empty(0, P, 4, device=dev), rows=torch.empty(0, P, dtype=torch.int32, device=dev),
                    overflow=torch.empty(0, dtype=torch.int32, device=dev))


def _follow(rows, perm):
    """last_rows behind a pass that permutes the rows of every frame: the old row of every output row, -1 where it has none"""
    old = torch.gather(rows, 1, perm.clamp(min=0).long())
    return torch.where(perm >= 0, old, torch.full_like(old, -1))


def _draw(net, frames, res, ovl, track, hw):
    """detect_video's `overlay`: the rows the call returns drawn onto a copy of the caller's frames (ops.overlay),
    or with inplace onto the device frames themselves -> (frames_out, painted)"""
    kw = {k: v for k, v in ovl.items() if k not in ("inplace", "gt")}
    if net._dev_nv12 is not None:                                 # the frames are NV12: the session's matrix and range
        from .video import NV12_MATRICES
        matrix, rng = next(k for k, v in NV12_MATRICES.items() if v == tuple(net._dev_nv12))
        kw.update(fmt="nv12", matrix=matrix, range=rng)
    rgb = kw.get("fmt") != "nv12"                                 # (RGB goes contiguous; an NV12 surface keeps its strides)
    if not frames.is_cuda:
        src = frames.to(net.device)
        src = out = src.contiguous() if rgb else src              # the upload is the copy: painted in place
    elif ovl.get("inplace"):
        src = out = frames
    else:
        src, out = (frames.contiguous() if rgb else frames), None
    gt = ovl.get("gt")
    if gt is not None:
        gt = torch.as_tensor(gt, dtype=torch.float32).to(net.device).contiguous()
    return ops.overlay(src, res[0].contiguous(), res[1].contiguous(), res[2].contiguous(), track=track, gt=gt, out=out,
                       net_size=tuple(hw), **kw)


def _camera_motion(net, frames, gmc, chunk, fmt):
    """detect_video's `gmc`: the signature of the clip in slices of `chunk` frames - a host clip is uploaded
    slice by slice and is never on the device as a whole - then one ops.motion_match over it -> (motion, sad, cum)"""
    T, H0, W0 = motion_frame_size(tuple(frames.shape), fmt)
    Gh, Gw = motion_grid_size(H0, W0, gmc["cell"])
    sig = torch.empty(T, Gh, Gw, dtype=torch.uint16, device=net.device)
    for a in range(0, T, chunk):
        x = frames[a:a + chunk]
        x = x if x.is_cuda else x.to(net.device)
        if fmt == "rgb":
            x = x.contiguous()
        ops.motion_signature(x, cell=gmc["cell"], fmt=fmt, out=sig[a:a + x.shape[0]])
    return ops.motion_match(sig, radius=gmc["radius"], gate=gmc["gate"], cell=gmc["cell"])


def detect_video(net, frames, step=1, chunk=8, seq_nms=None, track=None, tubelet=None, smooth=None, stitch=None, overlay=None):
    """YOLOV3.detect_video (its docstring is the description): a clip whose end is known is one push and one flush of the
    planner, run on the engine with the caller's frames at base 0; then Seq-NMS -> track -> stitch -> smooth ->
    tubelet on the finished clip, and the overlay of what is returned."""
    why = net._stream_refusal()
    if why is not None:
        raise NotImplementedError("detect_video with " + why)
    if net._live is not None:
        raise RuntimeError("detect_video: %r has frames in flight on this net (they share the feature ring): flush() it first"
                           % (net._live,))
    seq = parse_seq_nms(seq_nms, net.post_nms, "detect_video")
    track, gmc = split_gmc(track)
    track, app = split_appearance(track)
    trk = parse_track(track, net.post_nms, "detect_video")
    gmc = parse_gmc(gmc, trk is not None, smooth not in (None, False), tubelet not in (None, False), "detect_video")
    app = parse_appearance(app, None if trk is None else trk[2], seq is not None, "detect_video")
    if app is not None and net._k > 1 and net._k_join_pos != 'early':
        raise NotImplementedError("detect_video with track's appearance and k_join_pos %r: the ring of the late join holds the "
                                  "neck's tips, not the backbone's route tensors the descriptor is pooled from"
                                  % (net._k_join_pos,))
    tub_kw = parse_tubelet(tubelet, trk is not None, "detect_video")
    smo_kw = parse_smooth(smooth, trk is not None, "detect_video")
    sti_kw = parse_stitch(stitch, trk is not None, "detect_video")
    ovl = parse_overlay(overlay, "detect_video")
    if ovl is not None:
        if frames.dtype != torch.uint8:
            raise ValueError("detect_video: overlay needs uint8 frames (the pixels it draws on), got %s: float frames are "
                             "already normalised" % frames.dtype)
        if ovl.get("inplace") and not frames.is_cuda:
            raise ValueError("detect_video: overlay's inplace needs frames on the device; host frames are painted on their upload")
    gmc_fmt = None
    if gmc is not None:                                           # refused by name before any GPU work
        if frames.dtype != torch.uint8:
            raise ValueError("detect_video: gmc needs uint8 frames (the pixels the camera motion is read from), got %s: float "
                             "frames are already normalised" % frames.dtype)
        gmc_fmt = "nv12" if net._dev_nv12 is not None else "rgb"
        _, h0, w0 = motion_frame_size(tuple(frames.shape), gmc_fmt)
        check_motion_grid(*motion_grid_size(h0, w0, gmc["cell"]), gmc["radius"], "detect_video with gmc")
    net.last_overlay = None
    net.last_motion = None
    net.last_tracks = net.last_track_boxes = None
    net.last_embeddings = net.last_app_maps = None
    net.last_tubelet = net.last_pre_tubelet = None
    net.last_smooth = net.last_pre_smooth = None
    net.last_stitch = net.last_pre_stitch = None
    if net._k > 1:
        net._stream_split()                                       # the graph's own word, before anything touches the GPU
    step, chunk = int(step), int(chunk)
    if step < 1 or chunk < 1:
        raise ValueError("detect_video needs step >= 1 and chunk >= 1, got step=%d chunk=%d" % (step, chunk))
    T, H, W = frame_shape(net, frames, "an NV12 clip", "a clip", "T")
    assert 0 < net.nms_thresh < 1, "nms_thresh outside (0,1) (NMS disabled) is not implemented"
    eng = StreamEngine(net, step, chunk, appearance=app)
    acts = eng.plan.push(T) + eng.plan.flush()
    out = eng.run(acts, frames, 0, T, (H, W), keep_heads=getattr(net, 'stream_keep_heads', False))
    net.stream_stats = eng.stats
    net.stream_heads = [torch.cat(h) for h in zip(*eng.heads)] if eng.heads else None
    net.last_rows, net.last_overflow = out['rows'], out['overflow']
    res = out['ids'], out['scores'], out['bboxes']
    if app is not None:
        net.last_embeddings = torch.cat(eng.embs)
        net.last_app_maps = torch.cat(eng.app_maps) if app["keep_maps"] else None
    num_class = 1 if net.agnostic else net.num_class
    if seq is not None:
        net.last_plain = res                                      # the rows ahead of Seq-NMS
        boxes = res[2] if seq[1] is None else res[2].clamp(0, float(seq[1]))
        ids, scores, bboxes, perm = ops.seq_nms(res[0], res[1], boxes, num_class=num_class, **seq[0])
        net.last_rows = _follow(net.last_rows, perm)
        res = ids, scores, bboxes
    if trk is not None:
        boxes = res[2] if trk[1] is None else res[2].clamp(0, float(trk[1]))
        if gmc is not None:                                       # the tracker and stitch link in the stabilised frame
            motion, sad, cum = _camera_motion(net, frames, gmc, chunk, gmc_fmt)
            net.last_motion = motion, sad
            _, h0, w0 = motion_frame_size(tuple(frames.shape), gmc_fmt)
            gsx, gsy = float(np.float32(W) / np.float32(w0)), float(np.float32(H) / np.float32(h0))
            boxes = ops.motion_shift(res[0].contiguous(), boxes.contiguous(), cum, gsx, gsy, -1)
        if app is not None:                                       # SORT on the fused cost of geometry and appearance
            *links, net.last_track_boxes = ops.track_sort_app(res[0], res[1], boxes, net.last_embeddings, num_class=num_class,
                                                              sigma_app=app["sigma_app"], sigma_prox=app["sigma_prox"], **trk[0])
            net.last_tracks = tuple(links)
        elif trk[2] in ("sort", "byte"):                          # SORT, BYTE: the triple as ever, the filtered boxes beside it
            link = ops.track_sort if trk[2] == "sort" else ops.track_byte
            *links, net.last_track_boxes = link(res[0], res[1], boxes, num_class=num_class, **trk[0])
            net.last_tracks = tuple(links)
        else:
            net.last_tracks = ops.track(res[0], res[1], boxes, num_class=num_class, **trk[0])
        if gmc is not None and net.last_track_boxes is not None:  # the filtered boxes back in image coordinates
            net.last_track_boxes = ops.motion_shift(net.last_tracks[0], net.last_track_boxes, cum, gsx, gsy, 1)
        if sti_kw is not None:                                    # the fragments re-linked: the later passes take these ids
            net.last_pre_stitch = net.last_tracks
            *links, stitches, overflow = ops.stitch(res[0], res[1], boxes, net.last_tracks[0], num_class=num_class, **sti_kw)
            net.last_tracks, net.last_stitch = tuple(links), (stitches, overflow)
        if smo_kw is not None:                                    # the boxes the tracker saw, smoothed along its tracks
            net.last_pre_smooth = boxes
            boxes, net.last_smooth = ops.smooth(res[0], res[1], boxes, net.last_tracks[0], num_class=num_class, **smo_kw)
            res = res[0], res[1], boxes
        if tub_kw is not None:
            net.last_pre_tubelet = res[0], res[1], boxes          # the rows the tracker saw
            out_t = ops.tubelet(res[0], res[1], boxes, net.last_tracks[0], num_class=num_class, **tub_kw)
            net.last_rows = _follow(net.last_rows, out_t[3])
            net.last_tubelet = out_t[3], out_t[4], out_t[5]
            res = out_t[0], out_t[1], out_t[2]
    if ovl is not None:                                           # what the call returns, with the final track table
        table = None if trk is None else net.last_tubelet[1] if net.last_tubelet is not None else net.last_tracks[0]
        net.last_overlay = _draw(net, frames, res, ovl, table, (H, W))
    return res


class VideoSession:
    """One open-ended clip on `net` (YOLOV3.open_video makes it; detect_video's docstring describes step and chunk).

    push(frames): what detect_video accepts - (n,3,H,W) float, (n,H,W,3) uint8, or NV12 (n,H0*3/2,W0) uint8 under
    set_device_resize(source='nv12') - on the host or the device, n >= 1.  Returns (t0, ids, scores, bboxes) for the m >= 0
    frames [t0, t0 + m) whose detections are final now: new tensors (m,post_nms,1), (m,post_nms,1), (m,post_nms,4), never views
    of a program's buffers.  m == 0 is normal: a frame is emitted only once the (K//2)*step frames ahead of it have been seen
    and its chunk is full.  The first push of a clip fixes the frame size and dtype; another one raises ValueError.

    flush(): ends the clip - the remaining frames come out with the VID rule's end clamp (the last frame repeats), in the same
    form - and leaves the session at the start of a new clip: frame counter 0, tracker state fresh.

    last_rows (m,post_nms) int32 and last_overflow (m,) int32 cover the frames just emitted; frames_in / frames_out count the
    clip's frames taken and emitted; stream_stats accumulates detect_video's counters over the clip (it keeps the finished
    clip's totals after flush(), until the next clip's first push).

    track: None, True or detect_video's dict (sigma_l, sigma_h, sigma_iou, t_min, max_age, clip).  Every batch of emitted
    frames is pushed to an ops.TrackState; last_tracks = (track, tlen, tscore), each (m,post_nms), is track_online_host's
    triple for those frames: ids counted over the clip, lengths and maxima so far.  Nothing is decided online: sigma_h and
    t_min (kept in track_decide) are for track.finalize_tracks on the concatenated triples of the finished clip, which gives
    detect_video(track=...)'s last_tracks.  Without a further word the session carries the IOU tracker only:
    track={'method': 'sort'} and track={'method': 'byte'} raise NotImplementedError.  With
    'online': True in the dict (a bool; open_video's word alone, detect_video does not take it) the session carries that
    tracker: the emitted frames go to an ops.KalmanTrackState (vd_track_kf_push), last_tracks is the triple of
    sort_online_host / byte_online_host and last_track_boxes (None for 'iou') their tbox (m,post_nms,4);
    finalize_tracks(*triples, tbox=boxes, **track_decide) on the finished clip gives detect_video's last_tracks and
    last_track_boxes.  'method': 'iou' with 'online': True is the session as ever: that tracker is always online.

    smooth: None, or {'lag': L} / {'lag': L, 'max_gap': g} with L in [0, 15]; needs `track` ('iou' as it is, 'sort' / 'byte'
    with 'online': True).  True is refused: a latency must be chosen.  The fixed-lag form of detect_video's smooth (DESIGN.md
    40): every emitted batch goes to the tracker as ever, then the boxes the tracker saw (clamped by `clip`) and its ids go to
    an ops.SmoothLagState (vd_track_smooth_push).  push / flush then return (t0, ids, scores, bboxes) for the frames whose
    SMOOTHED boxes are final - L frames later than without the option; the ids, scores, rows, overflow, track triples and
    tbox of the frames still waiting are held back on the device and come out with their frame, so last_rows, last_overflow,
    last_tracks and last_track_boxes always describe the frames just returned, frames_out counts returned frames,
    last_pre_smooth holds those frames' boxes ahead of the pass and last_smooth their slen (both None without the option).
    Nothing is decided online: rows of a track that finalize_tracks drops later are smoothed too - the stated departure from
    detect_video(track=..., smooth=...), which smooths the decided table; where nothing is dropped and L is at least the
    clip's length less one, the two are equal bit for bit.  flush() resets both states.

    Seq-NMS is not a session option: it takes the best path through ALL frames of a clip, removes it and starts again until no
    row is alive, so no frame is final before the clip ends - it has no online form.  Run detect_video(seq_nms=...) on the
    finished clip instead.

    While a session has frames in flight (pushed, not yet flushed), the net's detect_video and open_video raise RuntimeError
    and no other session of the net accepts frames; net(x) is not affected.  Changing parameters, set_precision, set_nms or
    set_device_resize while frames are in flight is not supported: flush() first."""

    def __init__(self, net, step=1, chunk=8, track=None, smooth=None):
        why = net._stream_refusal()
        if why is not None:
            raise NotImplementedError("open_video with " + why)
        step, chunk = int(step), int(chunk)
        if step < 1 or chunk < 1:
            raise ValueError("open_video needs step >= 1 and chunk >= 1, got step=%d chunk=%d" % (step, chunk))
        self.track_decide = None
        self._trk_kw = self._trk_clip = self._trk = None
        self._trk_method = "iou"
        if split_gmc(track)[1] not in (None, False):
            raise NotImplementedError("open_video with track's gmc: the signature of the last frame is not carried from push to "
                                      "push (run detect_video on the finished clip)")
        track = split_gmc(track)[0]
        if split_appearance(track)[1] not in (None, False):
            raise NotImplementedError("open_video with track's appearance: the descriptors of a session's frames are not carried "
                                      "from push to push (run detect_video on the finished clip)")
        track, online = split_online(split_appearance(track)[0], "open_video")
        trk = parse_track(track, net.post_nms, "open_video")
        if trk is not None:
            if trk[2] != "iou" and not online:
                raise NotImplementedError("open_video with track method %r: it has no resumable form yet, only 'iou' has "
                                          "(run detect_video on the finished clip)" % (trk[2],))
            self._trk_kw, self._trk_clip, self._trk_method = trk
            self.track_decide = dict(sigma_h=self._trk_kw.pop("sigma_h"), t_min=self._trk_kw.pop("t_min"))
        self._smo_kw = parse_smooth_lag(smooth, trk is not None, "open_video")
        self._smo = self._held = None                             # the smoother's state; the frames that wait for their boxes
        if net._k > 1:
            net._stream_split()                                   # the graph's own word, before anything touches the GPU
        self.net, self.step, self.chunk = net, step, chunk
        self._eng = StreamEngine(net, step, chunk)
        self._plan = self._eng.plan
        self._buf = None                                          # the frames [_buf0, frames_in) that wait for their group
        self._buf0 = 0
        self._shape = None                                        # (shape of a frame, dtype), fixed by the clip's first push
        self._hw = None
        self.frames_out = 0
        self.last_rows = self.last_overflow = self.last_tracks = self.last_track_boxes = None
        self.last_pre_smooth = self.last_smooth = None

    def __repr__(self):
        return "<VideoSession step=%d chunk=%d: %d frames in, %d out>" % (self.step, self.chunk, self.frames_in, self.frames_out)

    @property
    def frames_in(self):
        return self._plan.frames_in

    @property
    def stream_stats(self):
        return self._eng.stats

    def _run(self, acts, frames, T, last=False):
        """the planner's actions on `frames` (the clip's frames from _buf0 on) -> (t0, ids, scores, bboxes) of the frames they emit
        (with smooth: of the frames whose smoothed boxes are final by now; last: the clip ends here, all of them)"""
        net = self.net
        out = self._eng.run(acts, frames, self._buf0, T, self._hw)
        self.last_rows, self.last_overflow = out['rows'], out['overflow']
        if self._trk_kw is not None:
            if self._trk is None:
                num_class = 1 if net.agnostic else net.num_class
                if self._trk_method == "iou":
                    self._trk = ops.TrackState(1, net.post_nms, num_class, device=net.device, **self._trk_kw)
                else:                                             # SORT, BYTE: the filter states travel with the tracks
                    self._trk = ops.KalmanTrackState(1, net.post_nms, num_class, method=self._trk_method, device=net.device,
                                                     **self._trk_kw)
            boxes = out['bboxes'] if self._trk_clip is None else out['bboxes'].clamp(0, float(self._trk_clip))
            if self._trk_method == "iou":
                self.last_tracks = self._trk.push(out['ids'], out['scores'], boxes)
            else:                                                 # the triple as ever, the filtered boxes beside it
                *links, self.last_track_boxes = self._trk.push(out['ids'], out['scores'], boxes)
                self.last_tracks = tuple(links)
            if self._smo_kw is not None:
                return self._smooth(out, boxes, last)
        t0 = self.frames_out
        self.frames_out += out['ids'].shape[0]
        return t0, out['ids'], out['scores'], out['bboxes']

    def _smooth(self, out, boxes, last):
        """the frames the engine just emitted (`boxes`: as the tracker saw them) behind the ones that wait; the frames whose
        smoothed boxes are final leave the queue, every last_* word cut to them"""
        net = self.net
        if self._smo is None:
            self._smo = ops.SmoothLagState(1, net.post_nms, 1 if net.agnostic else net.num_class, device=net.device, **self._smo_kw)
        new = dict(ids=out['ids'], scores=out['scores'], pre=boxes, rows=out['rows'], overflow=out['overflow'])
        for k, t in zip(("track", "tlen", "tscore"), self.last_tracks):
            new[k] = t
        if self.last_track_boxes is not None:
            new["tbox"] = self.last_track_boxes
        held = new if self._held is None else {k: torch.cat([self._held[k], new[k]]) for k in new}
        t0, sbox, slen = self._smo.push(out['ids'], out['scores'], boxes.contiguous(), new["track"])
        if last:
            _, sbox2, slen2 = self._smo.flush()
            sbox, slen = torch.cat([sbox, sbox2]), torch.cat([slen, slen2])
        m = sbox.shape[0]
        give = {k: t[:m] for k, t in held.items()}
        self._held = {k: t[m:] for k, t in held.items()} if m < held['ids'].shape[0] else None
        self.last_rows, self.last_overflow = give['rows'], give['overflow']
        self.last_tracks = give['track'], give['tlen'], give['tscore']
        self.last_track_boxes = give.get('tbox')
        self.last_pre_smooth, self.last_smooth = give['pre'], slen
        assert t0 == self.frames_out, "the smoother gave out frame %d, the session is at %d" % (t0, self.frames_out)
        self.frames_out += m
        return t0, give['ids'], give['scores'], sbox

    # ------------------------------------------------------------------ the public two
    def push(self, frames):
        net = self.net
        if net._live is not None and net._live is not self:
            raise RuntimeError("push: the net has another video session with frames in flight (%r): flush() it first" % (net._live,))
        _, H, W = frame_shape(net, frames, "NV12 frames", "frames", "n")
        shape = (tuple(frames.shape[1:]), frames.dtype)
        if self.frames_in == 0:
            assert 0 < net.nms_thresh < 1, "nms_thresh outside (0,1) (NMS disabled) is not implemented"
            self._shape, self._hw = shape, (H, W)
            self._eng.stats = dict(prefix_frames=0, suffix_frames=0, chunks=0)
        elif shape != self._shape:
            raise ValueError("push: this clip's frames are %s %s (its first push fixed that), got %s %s; flush() starts a new clip"
                             % (self._shape[0], str(self._shape[1]).replace("torch.", ""), shape[0], str(shape[1]).replace("torch.", "")))
        net._live = self
        n = int(frames.shape[0])
        frames = frames.to(net.device)
        if self._buf is not None:
            frames = torch.cat([self._buf, frames], dim=0)        # the clip's frames from _buf0 on
        res = self._run(self._plan.push(n), frames, None)
        keep = self._plan.out if net._k == 1 else self._plan.done  # the first frame that still waits for its group
        self._buf = frames[keep - self._buf0:].clone() if keep < self.frames_in else None
        self._buf0 = keep
        return res

    def flush(self):
        net = self.net
        if self.frames_in == 0:                                   # nothing in flight: an empty clip emits nothing
            return self._run([], None, 0, last=True)
        T = self.frames_in
        res = self._run(self._plan.flush(), self._buf, T, last=True)
        self._buf, self._buf0, self._shape, self._hw = None, 0, None, None
        self.frames_out = 0
        if self._trk is not None:
            self._trk.reset()
        if self._smo is not None:                                 # flush() left it fresh
            self._held = None
        if net._live is self:
            net._live = None
        return res
