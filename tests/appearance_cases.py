"""Inputs of the appearance tests (tests/test_appearance_cpu.py, tests/test_appearance_gpu.py): the two closed-form clips that
geometry cannot decide, with the expected ids written out by hand, the seeded clips that the paper-form oracle
(tests/appearance_oracle.py) decides with a margin, and the maps and boxes of the descriptor."""
import numpy as np

E_A = np.array((127, -127, 64, -64, 0, 0, 32, -32), np.int8)               # two descriptors of cosine 0
E_B = np.array((-127, 127, 64, -64, 32, -32, 0, 0), np.int8)
E_A2 = np.array((127, -127, 64, -64, 0, 0, 32, 40), np.int8)               # E_A with one channel moved: a cosine below 1


def clip(w, h, d, v, n, cls=(0, 0)):
    """Two boxes, both scored 0.9: A has x1 = 200 - v * (n - 1 - t) and B x1 = 200 + d + v * (n - 1 - t) for t < n, both y from
    10 to 10 + h; after frame n - 1 both reverse at v px a frame for n more frames.  -> (ids, scores, bboxes), F = 2 n, N = 2."""
    F = 2 * n
    ids = np.zeros((F, 2, 1), np.float32)
    ids[:, 0, 0], ids[:, 1, 0] = cls
    scores = np.full((F, 2, 1), 0.9, np.float32)
    bboxes = np.zeros((F, 2, 4), np.float32)
    for t in range(F):
        s = abs(n - 1 - t)
        a, b = 200.0 - v * s, 200.0 + d + v * s
        bboxes[t, 0] = [a, 10.0, a + w, 10.0 + h]
        bboxes[t, 1] = [b, 10.0, b + w, 10.0 + h]
    return ids, scores, bboxes


def swap_clip():
    """After the turn the constant-velocity prediction of A overlaps B's box with IoU 55/145 and its own with 40/160: SORT swaps"""
    return clip(100.0, 200.0, 45.0, 30.0, 5)


def turn_clip():
    """The prediction overlaps the turned box with 16/64 < 0.3 (and >= 0.1): SORT closes both tracks and starts ids 2 and 3"""
    return clip(40.0, 80.0, 70.0, 12.0, 5)


def far_turn_clip():
    """The turn at 20 px a frame: the prediction, 40 px off a 40 px box, does not touch the turned box - `near` fails"""
    return clip(40.0, 80.0, 130.0, 20.0, 5)


def two_descriptors(F, a=E_A, b=E_B):
    emb = np.zeros((F, 2, len(a)), np.int8)
    emb[:, 0], emb[:, 1] = a, b
    return emb


KEPT = [[0, 1]] * 10                                                      # row 0 is track 0 and row 1 track 1 throughout
SWAPPED = [[0, 1]] * 5 + [[1, 0]] * 5
FRAGMENTED = [[0, 1]] * 5 + [[2, 3]] * 5


def walkers_app(seed, T=10, objects=6, classes=2, miss=0.15, size=(16.0, 60.0), speed=6.0, jitter=0.5, extent=400.0, C=8, turn=None,
                noise=6):
    """tests/sort_cases.py's walkers with a descriptor per object - a seeded int8 vector, every row a noisy copy of its
    object's - and, with `turn` a frame, every velocity reversed from that frame on and doubled, so that constant-velocity
    predictions miss.  -> (ids, scores, bboxes, emb), N = objects."""
    rng = np.random.RandomState(seed)
    pos = rng.uniform(0.0, extent, (objects, 2))
    vel = rng.uniform(-speed, speed, (objects, 2))
    wh = rng.uniform(size[0], size[1], (objects, 2))
    cls = rng.randint(0, classes, objects)
    score = rng.uniform(0.55, 0.95, objects)
    proto = rng.randint(-100, 101, (objects, C))
    ids = -np.ones((T, objects, 1), np.float32)
    scores = -np.ones((T, objects, 1), np.float32)
    bboxes = -np.ones((T, objects, 4), np.float32)
    emb = np.zeros((T, objects, C), np.int8)
    for t in range(T):
        order = rng.permutation(objects)
        seen = rng.uniform(size=objects) >= miss
        jit = rng.uniform(-jitter, jitter, (objects, 4))
        wobble = rng.randint(-noise, noise + 1, (objects, C))
        n = 0
        for o in order:
            if seen[o]:
                c = pos[o] + vel[o] * (t if turn is None or t < turn else turn - 2.0 * (t - turn))
                box = np.array([c[0] - wh[o, 0] / 2, c[1] - wh[o, 1] / 2, c[0] + wh[o, 0] / 2, c[1] + wh[o, 1] / 2]) + jit[o]
                ids[t, n, 0], scores[t, n, 0], bboxes[t, n] = cls[o], score[o], box
                emb[t, n] = np.clip(proto[o] + wobble[o], -127, 127)
                n += 1
    return ids, scores, bboxes, emb


def random_emb(F, N, C, seed, protos=12, noise=10, none=0.1):
    """(F,N,C) int8: every row a noisy copy of one of `protos` seeded vectors, a share `none` of the rows without a descriptor"""
    rng = np.random.RandomState(seed)
    proto = rng.randint(-110, 111, (protos, C))
    pick = rng.randint(0, protos, (F, N))
    emb = np.clip(proto[pick] + rng.randint(-noise, noise + 1, (F, N, C)), -127, 127).astype(np.int8)
    emb[rng.uniform(size=(F, N)) < none] = 0
    return emb


def feature_map(S, Hf, Wf, C, seed, leaky=True):
    """(S,Hf,Wf,C) float32: Gaussian values, leaky-rectified as a backbone's activations are"""
    f = np.random.RandomState(seed).standard_normal((S, Hf, Wf, C)).astype(np.float32)
    return np.where(f > 0, f, np.float32(0.1) * f).astype(np.float32) if leaky else f


def boxes_for(Hf, Wf, stride, N, B, seed):
    """(ids (B,N,1), bboxes (B,N,4)): the first rows are the named edge cases - inside the map, across each border, smaller than a
    cell, zero width, inverted, a NaN and an infinite coordinate, id -1, wholly outside - the others seeded boxes around the map"""
    W, H = float(Wf * stride), float(Hf * stride)
    named = [[0.3 * W, 0.2 * H, 0.8 * W, 0.9 * H], [-0.5 * W, 0.1 * H, 0.4 * W, 0.6 * H], [0.5 * W, -0.7 * H, 0.9 * W, 0.3 * H],
             [0.6 * W, 0.2 * H, 1.8 * W, 0.7 * H], [0.1 * W, 0.5 * H, 0.6 * W, 1.9 * H], [3.25, 2.5, 3.25 + 0.3 * stride, 2.5 + 0.2 * stride],
             [0.4 * W, 0.1 * H, 0.4 * W, 0.8 * H], [0.9 * W, 0.8 * H, 0.2 * W, 0.1 * H], [np.nan, 1.0, 9.0, 9.0], [1.0, 1.0, np.inf, 9.0],
             [0.2 * W, 0.2 * H, 0.7 * W, 0.7 * H], [3.0 * W, 4.0 * H, 3.5 * W, 4.5 * H], [-2.0 * W, -2.0 * H, -1.5 * W, -1.1 * H]]
    rng = np.random.RandomState(seed)
    bboxes = np.zeros((B, N, 4), np.float32)
    ids = np.zeros((B, N, 1), np.float32)
    for b in range(B):
        lo = rng.uniform(-0.3, 1.0, (N, 2)) * [W, H]
        bboxes[b] = np.concatenate([lo, lo + rng.uniform(0.02, 0.8, (N, 2)) * [W, H]], axis=1)
        ids[b, :, 0] = rng.randint(0, 3, N)
        k = min(N, len(named))
        take = named if b == 0 else named[::-1]
        bboxes[b, :k] = np.asarray(take[:k], np.float32)
        if N > 10:
            ids[b, 10 if b == 0 else len(named) - 11, 0] = -1.0
    return ids, bboxes
