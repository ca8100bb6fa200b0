"""Inputs of the camera-motion tests (tests/test_motion_cpu.py, tests/test_motion_gpu.py): the closed-form shake clip, frames
without a common motion, seeded signatures, and the two objects that a shaking camera tears off their tracks."""
import numpy as np

H, W, T = 96, 128, 12
CAM_X = [24 * (t % 2) for t in range(T)]                                   # +24 / 0
CAM_Y = [(0, 0, 8, 8, 0, 0, -8, -8)[t % 8] for t in range(T)]
CAM = np.array([CAM_X, CAM_Y], np.int64).T                                # (T,2) (x, y)
STEPS = np.concatenate([np.zeros((1, 2), np.int64), np.diff(CAM, axis=0)])  # the camera's step into frame t


def canvas(kind, seed=0, h=H + 64, w=W + 64):
    """a world canvas: 'blocks' - 8 x 8-pixel blocks of random colours - or 'pixels' - every pixel random"""
    rng = np.random.RandomState(seed)
    if kind == "blocks":
        return np.kron(rng.randint(0, 256, (h // 8, w // 8, 3)).astype(np.uint8), np.ones((8, 8, 1), np.uint8))
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


def shake_clip(kind="blocks", seed=0):
    """(T,H,W,3) uint8: crops of the canvas at the camera's positions; motion must be -STEPS exactly, with a SAD of 0"""
    c = canvas(kind, seed)
    return np.stack([c[32 + y:32 + y + H, 32 + x:32 + x + W] for x, y in CAM])


def uncorrelated(F=6, seed=3, h=H, w=W):
    """SyntheticVideo-style frames: every pixel of every frame drawn anew"""
    return np.random.default_rng(seed).integers(0, 256, (F, h, w, 3), dtype=np.uint8)


def to_nv12_luma(frames_rgb, seed=1):
    """(F,H*3/2,W) uint8 whose Y plane is the frames' luma and whose chroma is noise (it must never be read)"""
    from viddet_amd.motion import luma_host
    y = luma_host(frames_rgb)
    F, h, w = y.shape
    uv = np.random.RandomState(seed).randint(0, 256, (F, h // 2, w)).astype(np.uint8)
    return np.concatenate([y, uv], axis=1)


def signatures(F, Gh, Gw, seed, shift=True):
    """(F,Gh,Gw) uint16: seeded words up to 65280; with shift, frame t is frame t - 1 moved by a seeded step plus noise, so that the
    winners are spread over the window"""
    rng = np.random.RandomState(seed)
    big = rng.randint(0, 65281, (Gh + 64, Gw + 64)).astype(np.int64)
    out = np.empty((F, Gh, Gw), np.uint16)
    y, x = 32, 32
    for t in range(F):
        if shift and t:
            y, x = np.clip(y + rng.randint(-12, 13), 0, 64), np.clip(x + rng.randint(-12, 13), 0, 64)
        out[t] = np.clip(big[y:y + Gh, x:x + Gw] + rng.randint(-300, 301, (Gh, Gw)), 0, 65280)
    return out


def two_objects():
    """The shake clip's camera on a static 40 x 40 box and a second object of the same class that drifts 3 px a frame:
    (ids (T,2,1), scores (T,2,1), bboxes (T,2,4)) in image coordinates.  Static: the constant-velocity prediction overlaps the
    seen box with IoU 640 / 2560 = 0.25 on the x step alone."""
    ids = np.zeros((T, 2, 1), np.float32)
    scores = np.full((T, 2, 1), 0.9, np.float32)
    boxes = np.zeros((T, 2, 4), np.float32)
    for t in range(T):
        cx, cy = CAM[t]
        boxes[t, 0] = [44 - cx, 28 - cy, 84 - cx, 68 - cy]
        boxes[t, 1] = [4 + 3 * t - cx, 180 - cy, 28 + 3 * t - cx, 230 - cy]
    return ids, scores, boxes


MOTION = (-STEPS).astype(np.int32)                                        # what match_host must find on the shake clip
