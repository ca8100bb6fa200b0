"""Seeded inputs of the overlay tests (tests/test_overlay_cpu.py, tests/test_overlay_gpu.py): objects that drift across a clip,
their rows shuffled per frame, some rows broken on purpose (id -1, a NaN box, a score under the threshold, x1 > x2)."""
import numpy as np


def make_case(seed, F, size, N, G=0, net_size=None, clips=None, tracked=0.8, broken=True, **params):
    """-> dict(frames (F,H0,W0,3), ids, scores (F,N,1), bboxes (F,N,4), track (F,N) int32, gt (F,G,6) or None, clip_start,
    params).  Boxes are in net_size coordinates (the frames' own size where None)."""
    rng = np.random.default_rng(seed)
    h0, w0 = size
    hn, wn = net_size or size
    frames = rng.integers(0, 256, (F, h0, w0, 3), dtype=np.uint8)
    # N objects: a start box, a velocity, a class; object k keeps track id k * 7 + 1 where it is tracked
    xy = rng.random((N, 2)) * [wn * 0.8, hn * 0.8]
    wh = rng.random((N, 2)) * [wn * 0.4, hn * 0.4] + 1.0
    vel = (rng.random((N, 2)) - 0.5) * [wn * 0.1, hn * 0.1]
    cls = rng.integers(0, 5, N)
    is_tracked = rng.random(N) < tracked
    ids = np.zeros((F, N, 1), np.float32)
    scores = np.zeros((F, N, 1), np.float32)
    bboxes = np.zeros((F, N, 4), np.float32)
    track = np.full((F, N), -1, np.int32)
    for f in range(F):
        order = rng.permutation(N)
        sc = np.sort(rng.random(N).astype(np.float32))[::-1] * 0.5 + 0.5
        for i, k in enumerate(order):
            p = xy[k] + vel[k] * f
            ids[f, i, 0] = cls[k]
            scores[f, i, 0] = sc[i]
            bboxes[f, i] = [p[0], p[1], p[0] + wh[k, 0], p[1] + wh[k, 1]]
            if is_tracked[k] and rng.random() < 0.85:             # a track misses a frame now and then
                track[f, i] = k * 7 + 1
        if broken and N > 4:                                     # (four rows are broken: a fifth is left to draw)
            j = rng.permutation(N)[:4]
            ids[f, j[0], 0] = -1.0
            bboxes[f, j[1], rng.integers(0, 4)] = np.nan
            scores[f, j[2], 0] = 0.25
            bboxes[f, j[3], [0, 2]] = bboxes[f, j[3], [2, 0]] + [1.0, -1.0]
    gt = None
    if G:
        gt = np.full((F, G, 6), -1.0, np.float32)
        for f in range(F):
            n = rng.integers(0, G + 1)
            p = rng.random((n, 2)) * [wn * 0.7, hn * 0.7]
            s = rng.random((n, 2)) * [wn * 0.5, hn * 0.5] + 2.0
            gt[f, :n, :4] = np.concatenate([p, p + s], axis=1)
            gt[f, :n, 4] = rng.integers(0, 5, n)
            gt[f, :n, 5] = rng.integers(0, 9, n)
    p = dict(net_size=(hn, wn), **params)
    return dict(frames=frames, ids=ids, scores=scores, bboxes=bboxes, track=track, gt=gt, clip_start=clips, params=p)


NAMES = ("aeroplane", "bicycle", "cat", "dog")                      # class 4 has no name: its decimal id is printed

# name -> arguments of make_case.  48 x 64 takes the dword path, 37 x 51 the byte path; two clips through clip_start.
CASES = {
    "rgb_L0": dict(seed=1, F=5, size=(48, 64), N=6, G=3, net_size=(32, 32), clips=[0, 3, 5], trail=0),
    "rgb_L3": dict(seed=2, F=5, size=(48, 64), N=8, G=2, net_size=(64, 96), clips=[0, 2, 5], trail=3, class_names=NAMES),
    "odd_L0": dict(seed=3, F=5, size=(37, 51), N=4, G=0, clips=[0, 3, 5], trail=0, color_by="class"),
    "odd_L3": dict(seed=4, F=5, size=(37, 51), N=7, G=3, net_size=(64, 64), clips=[0, 3, 5], trail=3, thickness=1),
    "thick": dict(seed=5, F=3, size=(48, 64), N=5, G=2, trail=2, thickness=8, scale=1),
    "big_text": dict(seed=6, F=3, size=(48, 64), N=4, G=1, trail=2, thickness=1, scale=4, class_names=NAMES),
    "no_track": dict(seed=7, F=3, size=(48, 64), N=5, G=2, tracked=0.0, trail=4),
}


def case(name):
    return make_case(**CASES[name])


def call_args(c, fmt="rgb"):
    """(positional, keyword) arguments of overlay_host for a case, without the frames"""
    kw = dict(c["params"], track=c["track"], gt=c["gt"], clip_start=c["clip_start"])
    if fmt != "rgb":
        kw["fmt"] = fmt
    return (c["ids"], c["scores"], c["bboxes"]), kw


def even(frames):
    """the largest even-sized corner of RGB frames (NV12 needs one)"""
    h, w = frames.shape[1] & ~1, frames.shape[2] & ~1
    return np.ascontiguousarray(frames[:, :h, :w])
