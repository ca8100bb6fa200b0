"""Live video sessions: detect_video on a clip whose frames arrive a few at a time and whose length nobody knows.

`net.open_video(step, chunk, track)` returns a VideoSession.  `push(frames)` takes the next frames and returns the detections
that are final by now, `flush()` ends the clip.  Over any way of cutting a clip into pushes followed by one flush, the
concatenated results are torch.equal to `net.detect_video(clip, step, chunk)`: the session runs detect_video's own two
programs in exactly the launch groups detect_video forms (stream.StreamPlanner) - the fp32 operand scales are per tensor, so
any other grouping would round differently.  With `track`, the emitted rows go through a resumable tracker on the device
(ops.TrackState, vd_track_push) whose state survives from push to push.
"""
import torch

from . import lib as L
from . import ops
from .stream import StreamPlanner


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
    detect_video(track=...)'s last_tracks.

    Seq-NMS is not a session option: it takes the best path through ALL frames of a clip, removes it and starts again until no
    row is alive, so no frame is final before the clip ends - it has no online form.  Run detect_video(seq_nms=...) on the
    finished clip instead.

    While a session has frames in flight (pushed, not yet flushed), the net's detect_video and open_video raise RuntimeError
    and no other session of the net accepts frames; net(x) is not affected.  Changing parameters, set_precision, set_nms or
    set_device_resize while frames are in flight is not supported: flush() first."""

    def __init__(self, net, step=1, chunk=8, track=None):
        why = net._stream_refusal()
        if why is not None:
            raise NotImplementedError("open_video with " + why)
        step, chunk = int(step), int(chunk)
        if step < 1 or chunk < 1:
            raise ValueError("open_video needs step >= 1 and chunk >= 1, got step=%d chunk=%d" % (step, chunk))
        self.track_decide = None
        self._trk_kw = self._trk_clip = self._trk = None
        if track is not None and track is not False:
            from .track import DEFAULTS, check_params
            kw = {} if track is True else dict(track)
            self._trk_clip = kw.pop("clip", None)
            unknown = sorted(set(kw) - set(DEFAULTS))
            if unknown:
                raise ValueError("open_video: track takes sigma_l, sigma_h, sigma_iou, t_min and max_age, got %s" % ", ".join(unknown))
            kw = dict(DEFAULTS, **kw)
            check_params(who="open_video with track", **kw)
            if net.post_nms > L.TRACK_MAX_ROWS:
                raise ValueError("open_video with track: post_nms=%d rows per frame, the tracker takes at most %d"
                                 % (net.post_nms, L.TRACK_MAX_ROWS))
            self.track_decide = dict(sigma_h=kw.pop("sigma_h"), t_min=kw.pop("t_min"))
            self._trk_kw = kw
        if net._k > 1:
            net._stream_split()                                   # the graph's own word, before anything touches the GPU
        self.net, self.step, self.chunk = net, step, chunk
        self._plan = StreamPlanner(net._k, step, chunk)
        self._buf = None                                          # the frames [_buf0, frames_in) that wait for their group
        self._buf0 = 0
        self._shape = None                                        # (shape of a frame, dtype), fixed by the clip's first push
        self._hw = None
        self.frames_out = 0
        self.stream_stats = dict(prefix_frames=0, suffix_frames=0, chunks=0)
        self.last_rows = self.last_overflow = self.last_tracks = None

    def __repr__(self):
        return "<VideoSession step=%d chunk=%d: %d frames in, %d out>" % (self.step, self.chunk, self.frames_in, self.frames_out)

    @property
    def frames_in(self):
        return self._plan.frames_in

    # ------------------------------------------------------------------ the two launch groups, as detect_video runs them
    def _programs(self):
        """detect_video's programs at this clip's size, current (K > 1)"""
        net = self.net
        H, W = self._hw
        bf16 = net.precision == 'bf16'
        key = ('stream_bf16' if bf16 else 'stream', self.chunk, H, W, self._plan.S)
        if key not in net._programs:
            net._programs[key] = net._build_or_evict(lambda: net._build_stream(self.chunk, H, W, self._plan.S))
        sp = net._programs[key]
        if bf16:
            net._bf16_current(sp, sp['packs'], [sp['pre'], sp['suf']])
        else:
            net._refresh_fold()
        net._refresh_wamax()
        return sp

    def _prefix(self, sp, frames, a, b):
        net, S, m = self.net, self._plan.S, b - a
        net._stage_frames(sp['pb']['in'], frames, a - self._buf0, b - self._buf0)
        sp['pre'].run()
        for t in sp['srcs']:                                      # rows -> slots (a run of frames wraps at most once: m <= S)
            ring, src = sp['sb']['ring:' + t], sp['pb'][t]
            s0 = a % S
            m0 = min(m, S - s0)
            ring[s0:s0 + m0].copy_(src[:m0])
            if m0 < m:
                ring[:m - m0].copy_(src[m0:m])
        self.stream_stats['prefix_frames'] += m

    def _suffix(self, sp, frames, t0, n, T):
        net = self.net
        if net._k == 1:
            # the plain plan at batch `chunk`, a shorter last chunk padded with repeats of its last frame
            x = frames[t0 - self._buf0:t0 - self._buf0 + n]
            if n < self.chunk:
                x = torch.cat([x, x[-1:].expand((self.chunk - n,) + tuple(x.shape[1:]))], dim=0)
            net._forward_infer(x)
            o = net._programs[('infer_bf16' if net.precision == 'bf16' else 'infer', self.chunk) + self._hw][2]
        else:
            sp['slots'].copy_(torch.from_numpy(self._plan.slots(t0, n, T)))
            sp['suf'].run()
            o = sp['o']
        self.stream_stats['suffix_frames'] += n
        self.stream_stats['chunks'] += 1
        return {k: o[k][:n].clone() for k in ('ids', 'scores', 'bboxes', 'rows', 'overflow')}

    def _run(self, acts, frames, T):
        """the planner's actions on `frames` (the clip's frames from _buf0 on) -> (t0, ids, scores, bboxes) of the frames they emit"""
        net = self.net
        sp = self._programs() if net._k > 1 and acts else None
        outs = []
        for kind, a, b in acts:
            if kind == 'prefix':
                self._prefix(sp, frames, a, b)
            else:
                outs.append(self._suffix(sp, frames, a, b, T))
        dev, P = net.device, net.post_nms
        if outs:
            out = {k: torch.cat([o[k] for o in outs]) for k in outs[0]}
        else:
            out = dict(ids=torch.empty(0, P, 1, device=dev), scores=torch.empty(0, P, 1, device=dev),
                       bboxes=torch.empty(0, P, 4, device=dev), rows=torch.empty(0, P, dtype=torch.int32, device=dev),
                       overflow=torch.empty(0, dtype=torch.int32, device=dev))
        self.last_rows, self.last_overflow = out['rows'], out['overflow']
        if self._trk_kw is not None:
            if self._trk is None:
                self._trk = ops.TrackState(1, P, 1 if net.agnostic else net.num_class, device=dev, **self._trk_kw)
            boxes = out['bboxes'] if self._trk_clip is None else out['bboxes'].clamp(0, float(self._trk_clip))
            self.last_tracks = self._trk.push(out['ids'], out['scores'], boxes)
        t0 = self.frames_out
        self.frames_out += out['ids'].shape[0]
        return t0, out['ids'], out['scores'], out['bboxes']

    # ------------------------------------------------------------------ the public two
    def push(self, frames):
        net = self.net
        if net._live is not None and net._live is not self:
            raise RuntimeError("push: the net has another video session with frames in flight (%r): flush() it first" % (net._live,))
        u8 = frames.dtype == torch.uint8
        if net._dev_nv12 is not None and u8:                      # NV12 frames (n,H0*3/2,W0); _in_shape checks the rest
            if frames.dim() != 3 or frames.shape[0] < 1:
                raise ValueError("set_device_resize(source='nv12') is on: expected NV12 frames (n,H0*3/2,W0) uint8, got %s"
                                 % (tuple(frames.shape),))
        elif frames.dim() != 4 or frames.shape[0] < 1 or (frames.shape[-1] if u8 else frames.shape[1]) != 3:
            raise ValueError("expected frames (n,3,H,W), or (n,H,W,3) uint8, got %s" % (tuple(frames.shape),))
        _, H, W = net._in_shape(frames)
        shape = (tuple(frames.shape[1:]), frames.dtype)
        if self.frames_in == 0:
            assert 0 < net.nms_thresh < 1, "nms_thresh outside (0,1) (NMS disabled) is not implemented"
            self._shape, self._hw = shape, (H, W)
            self.stream_stats = dict(prefix_frames=0, suffix_frames=0, chunks=0)
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
            return self._run([], None, 0)
        T = self.frames_in
        res = self._run(self._plan.flush(), self._buf, T)
        self._buf, self._buf0, self._shape, self._hw = None, 0, None, None
        self.frames_out = 0
        if self._trk is not None:
            self._trk.reset()
        if net._live is self:
            net._live = None
        return res
