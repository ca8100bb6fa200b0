"""Window bookkeeping of streaming video detection (YOLOV3.detect_video).  NumPy only: no GPU, no torch.

The VID dataset builds the K-frame window of every frame of a clip by one rule (/root/reference datasets/imgnetvid.py:486-506);
`stream_window_slots` restates it, `ring_size` / `chunk_slots` turn it into the slot tables of the feature ring.
`StreamPlanner` forms detect_video's launch groups while the frames of a clip still arrive (live.VideoSession).
"""
import numpy as np


def stream_window_slots(T, K, step=1):
    """int64 [T][K]: the frame indices of the window of every frame t of a T-frame clip (imgnetvid.py:486-506).

    h = K // 2 frames behind t, `step` apart and oldest first (max(0, t - j*step) for j = h .. 1: the clip's first frame
    repeats where the window reaches before it), then t, then frames ahead (min(T-1, t + j*step) for j = 1 .. h: the last
    frame repeats) until the window holds K entries - an even K has no room for the last forward frame.  K = 1: [[t]]."""
    T, K, step = int(T), int(K), int(step)
    if T < 1 or K < 1 or step < 1:
        raise ValueError("stream_window_slots needs T >= 1, K >= 1 and step >= 1, got T=%d K=%d step=%d" % (T, K, step))
    h = K // 2
    out = np.empty((T, K), dtype=np.int64)
    for t in range(T):
        w = [max(0, t - j * step) for j in range(h, 0, -1)] + [t]
        for j in range(1, h + 1):
            if len(w) == K:
                break
            w.append(min(T - 1, t + j * step))
        out[t] = w
    return out


def ring_size(K, step, chunk):
    """Slots of the feature ring: a chunk of `chunk` consecutive output frames reads the frames from (K//2)*step before its
    first to (K//2)*step behind its last, and frame f lives in slot f mod S - so S frames in a row never collide."""
    return int(chunk) + 2 * (int(K) // 2) * int(step)


class StreamPlanner:
    """The launch groups of detect_video, formed while the frames of a clip arrive (VideoSession).

    detect_video(frames, step, chunk) on a clip of T frames runs, with reach = (K//2)*step, per output chunk
    [t0, t0 + chunk): prefix groups [done, min(done + chunk, t0 + chunk + reach, T)) until done reaches
    min(t0 + chunk + reach, T), then the suffix on the min(chunk, T - t0) frames from t0 (K = 1: no prefix, the plain plan on
    every chunk).  None of that depends on T before the clip ends, so `push(n)` - n frames arrived - returns the actions whose
    frames are all there, in detect_video's order: ('prefix', a, b) for a group that T cannot cut short any more, and
    ('suffix', t0, chunk) once done >= t0 + chunk + reach.  `flush()` ends the clip: T = frames_in, the rest of
    detect_video's loops (the short groups) is returned and the planner starts a new clip.  Over any way of cutting a clip into
    pushes followed by one flush the actions are those of detect_video on the whole clip.

    frames_in: frames arrived; done: frames that went through a prefix group (K = 1: through the plan); out: the first frame
    no suffix has emitted yet; buffered = frames_in - done, the frames that wait for their group: fewer than `chunk` after
    every push."""

    def __init__(self, K, step=1, chunk=8):
        K, step, chunk = int(K), int(step), int(chunk)
        if K < 1 or step < 1 or chunk < 1:
            raise ValueError("StreamPlanner needs K >= 1, step >= 1 and chunk >= 1, got K=%d step=%d chunk=%d" % (K, step, chunk))
        self.K, self.step, self.chunk = K, step, chunk
        self.reach = (K // 2) * step
        self.S = ring_size(K, step, chunk)
        self.frames_in = self.done = self.out = 0

    @property
    def buffered(self):
        return self.frames_in - self.done

    def _advance(self, T):
        """detect_video's loops from where they stand, as far as the frames that arrived determine them (T None: the clip
        is still open)"""
        acts = []
        end = self.frames_in if T is None else T
        while self.out < end:
            t0 = self.out
            if self.K == 1:
                if T is None and self.frames_in < t0 + self.chunk:
                    break
                n = min(self.chunk, end - t0)
                self.done = t0 + n
            else:
                need = t0 + self.chunk + self.reach
                if T is not None:
                    need = min(need, T)
                while self.done < need:
                    b = min(self.done + self.chunk, need)
                    if b > self.frames_in:                        # (only while the clip is open: need <= T at its end)
                        return acts
                    acts.append(('prefix', self.done, b))
                    self.done = b
                n = min(self.chunk, end - t0)
            acts.append(('suffix', t0, n))
            self.out = t0 + n
        return acts

    def push(self, n):
        """n >= 1 frames arrived -> the actions they complete"""
        n = int(n)
        if n < 1:
            raise ValueError("StreamPlanner.push needs n >= 1 frames, got %d" % n)
        self.frames_in += n
        return self._advance(None)

    def flush(self):
        """The clip ends at frames_in -> the remaining actions; the planner is at the start of a new clip afterwards"""
        acts = self._advance(self.frames_in)
        assert self.out == self.done == self.frames_in
        self.frames_in = self.done = self.out = 0
        return acts

    def slots(self, t0, n, T=None):
        """The int32 [chunk][K] slot table of the suffix action (t0, n): chunk_slots of the windows of frames [t0, t0 + n),
        checked against the frames the ring holds when that action runs (done stands at min(t0 + chunk + reach, T) then).
        T: the clip's length once it is known (the actions of flush()), None while it is open - no window of an action that
        push() returned reaches the clip's end."""
        last = t0 + self.chunk + self.reach
        if T is not None:
            last = min(last, int(T))
        # (an open clip: frames below `last` are all a window of [t0, t0 + chunk) reaches, so `last` stands in for T)
        fr = window_rows(t0, n, last if T is None else int(T), self.K, self.step)
        return _slot_table(fr, t0, n, self.chunk, self.S, max(0, last - self.S), last)


def window_rows(t0, n, T, K, step=1):
    """stream_window_slots(T, K, step)[t0:t0 + n] without the rows around it (a stream has no short T to build them all for)"""
    t0, n, T, K, step = int(t0), int(n), int(T), int(K), int(step)
    if not (0 <= t0 and 0 < n and t0 + n <= T) or K < 1 or step < 1:
        raise ValueError("window_rows: frames [%d, %d) of a clip of %d frames, K=%d step=%d" % (t0, t0 + n, T, K, step))
    h = K // 2
    t = np.arange(t0, t0 + n, dtype=np.int64)[:, None]
    back = np.maximum(0, t - np.arange(h, 0, -1, dtype=np.int64)[None, :] * step)
    ahead = np.minimum(T - 1, t + np.arange(1, K - h, dtype=np.int64)[None, :] * step)     # K - h - 1 frames: an even K has one fewer
    return np.concatenate([back, t, ahead], axis=1)


def chunk_slots(windows, t0, n, rows, S, first, last):
    """int32 [rows][K] slot table of the output frames [t0, t0 + n) (n <= rows: the rows behind them repeat the last real one,
    so that a padded row reads valid slots).  `windows` = stream_window_slots(...); [first, last) = the frames the ring
    holds now.  Raises when a window needs a frame that is not there: the table is checked here, before it is uploaded
    (the kernels only clamp)."""
    if not (0 < n <= rows) or S < 1:
        raise ValueError("chunk_slots: bad sizes (n=%d rows=%d S=%d)" % (n, rows, S))
    fr = np.asarray(windows[t0:t0 + n], dtype=np.int64)
    if fr.shape[0] != n:
        raise ValueError("chunk_slots: frames [%d, %d) are outside the clip of %d frames" % (t0, t0 + n, len(windows)))
    return _slot_table(fr, t0, n, rows, S, first, last)


def _slot_table(fr, t0, n, rows, S, first, last):
    """chunk_slots on the window rows `fr` of the frames [t0, t0 + n) themselves"""
    if fr.min() < first or fr.max() >= last or last - first > S:
        raise ValueError("chunk_slots: the windows of frames [%d, %d) need frames [%d, %d], the ring of %d slots holds [%d, %d)"
                         % (t0, t0 + n, fr.min(), fr.max(), S, first, last))
    tab = np.concatenate([fr, np.repeat(fr[-1:], rows - n, axis=0)], axis=0) % S
    assert tab.min() >= 0 and tab.max() < S
    return np.ascontiguousarray(tab, dtype=np.int32)
