"""Window bookkeeping of streaming video detection (YOLOV3.detect_video).  NumPy only: no GPU, no torch.

The VID dataset builds the K-frame window of every frame of a clip by one rule (/root/reference datasets/imgnetvid.py:486-506);
`stream_window_slots` restates it, `ring_size` / `chunk_slots` turn it into the slot tables of the feature ring.
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
    if fr.min() < first or fr.max() >= last or last - first > S:
        raise ValueError("chunk_slots: the windows of frames [%d, %d) need frames [%d, %d], the ring of %d slots holds [%d, %d)"
                         % (t0, t0 + n, fr.min(), fr.max(), S, first, last))
    tab = np.concatenate([fr, np.repeat(fr[-1:], rows - n, axis=0)], axis=0) % S
    assert tab.min() >= 0 and tab.max() < S
    return np.ascontiguousarray(tab, dtype=np.int32)
