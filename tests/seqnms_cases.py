"""Inputs of the Seq-NMS tests (tests/test_seq_nms_cpu.py, tests/test_seq_nms_gpu.py): small clips built to tie, to link, to
break and to cross the sizes at which vd_seq_nms changes lanes and words."""
import numpy as np

LADDER = np.linspace(0.05, 0.95, 12).astype(np.float32)          # scores come from 12 values: most rows tie


def random_clip(T, N, classes=1, seed=0, fill=0.8, empty=(), gap=None, spread=60.0, absent=()):
    """(ids (T,N,1), scores (T,N,1), bboxes (T,N,4)) float32: N tracks drifting about 1.5 px per frame with jitter, scores from
    the ladder, about `fill` of the rows present (the others are -1 rows, anywhere in the frame).  empty: frames without a row;
    gap: a frame that every track skips; absent: classes that never occur."""
    rng = np.random.default_rng(seed)
    origin = rng.uniform(0, spread, (N, 2))
    size = rng.uniform(16, 40, (N, 2))
    present = [c for c in range(classes) if c not in absent]
    track_cls = rng.choice(present, N)
    ids = -np.ones((T, N, 1), np.float32)
    scores = -np.ones((T, N, 1), np.float32)
    bboxes = -np.ones((T, N, 4), np.float32)
    for t in range(T):
        if t in empty or t == gap:
            continue
        order = rng.permutation(N)                                 # a track sits at another row in every frame
        for r, k in enumerate(order):
            if rng.uniform() > fill:
                continue
            xy = origin[k] + 1.5 * t + rng.uniform(-1.0, 1.0, 2)
            ids[t, r, 0] = track_cls[k]
            scores[t, r, 0] = LADDER[rng.integers(0, len(LADDER))]
            bboxes[t, r] = np.concatenate([xy, xy + size[k]])
    return ids, scores, bboxes


def four_frames():
    """A 10 x 10 box moving 1 px per frame with scores .9 .2 .8 .7, and in frame 1 a second box 2 px further with score .5:
    one sequence through the .5 box (2.9 / 4 = 0.725), the .2 row dies at IoU 80 / 120, one round."""
    ids = -np.ones((4, 3, 1), np.float32)
    scores = -np.ones((4, 3, 1), np.float32)
    bboxes = -np.ones((4, 3, 4), np.float32)
    for t, s in enumerate([0.9, 0.2, 0.8, 0.7]):
        ids[t, 0], scores[t, 0], bboxes[t, 0] = 0, s, [t, 0, t + 10, 10]
    ids[1, 1], scores[1, 1], bboxes[1, 1] = 0, 0.5, [3, 0, 13, 10]
    return ids, scores, bboxes


def exact_half():
    """[0,0,10,10] and [0,0,10,20]: IoU 100 / 200, exactly 0.5.  Frame 0 holds both, frame 1 the second one."""
    ids = np.zeros((2, 2, 1), np.float32)
    scores = np.array([[[0.9], [0.6]], [[0.7], [-1.0]]], np.float32)
    bboxes = np.array([[[0, 0, 10, 10], [0, 0, 10, 20]], [[0, 0, 10, 20], [-1, -1, -1, -1]]], np.float32)
    ids[1, 1] = -1
    return ids, scores, bboxes


def dense_one_class(T=3, N=128, seed=5):
    """N rows of ONE class in every frame, packed so that many overlap: rows below and above 64 link and suppress each other"""
    rng = np.random.default_rng(seed)
    ids = np.zeros((T, N, 1), np.float32)
    scores = LADDER[rng.integers(0, len(LADDER), (T, N, 1))]
    xy = rng.uniform(0, 90, (T, N, 2)).astype(np.float32)
    bboxes = np.concatenate([xy, xy + rng.uniform(20, 36, (T, N, 2)).astype(np.float32)], axis=2)
    return ids, scores, bboxes.astype(np.float32)
