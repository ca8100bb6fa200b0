"""What the streaming-detection tests compare against (tests/test_stream_cpu.py, tests/test_stream_gpu.py).

* WINDOWS: the windows of every frame of a clip, written out BY HAND from the rule of /root/reference
  datasets/imgnetvid.py:486-506 (K // 2 frames back, `step` apart, oldest first, the first frame repeated before the clip's
  start; the frame; K // 2 frames ahead, the last frame repeated behind the clip's end; an even K drops the last forward one).
* clip_reference(): the fp64 oracle network (oracle/net_temporal.py) on the T windows of a clip gathered on the host - the
  reference net.detect_video is held to, NOT the windowed device path.  Computed once per (configuration, step) and shared.
"""
import numpy as np

WINDOWS = {
    (7, 3, 1): [[0, 0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5], [4, 5, 6], [5, 6, 6]],
    (7, 3, 2): [[0, 0, 2], [0, 1, 3], [0, 2, 4], [1, 3, 5], [2, 4, 6], [3, 5, 6], [4, 6, 6]],
    (5, 5, 1): [[0, 0, 0, 1, 2], [0, 0, 1, 2, 3], [0, 1, 2, 3, 4], [1, 2, 3, 4, 4], [2, 3, 4, 4, 4]],
    (2, 3, 1): [[0, 0, 1], [0, 1, 1]],
    (1, 3, 1): [[0, 0, 0]],
    (6, 4, 1): [[0, 0, 0, 1], [0, 0, 1, 2], [0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [3, 4, 5, 5]],      # even K
    (7, 1, 1): [[0], [1], [2], [3], [4], [5], [6]],
}

C, SIZE, T, K, SEED = 2, 64, 7, 3, 43          # the network cases: two classes, 64 x 64 frames, a clip of seven

_CACHE = {}


def clip_frames():
    """fp32 (T, 3, SIZE, SIZE): the clip of the network cases, distinct frames"""
    if 'x' not in _CACHE:
        _CACHE['x'] = np.random.default_rng(SEED).standard_normal((T, 3, SIZE, SIZE)).astype(np.float32)
    return _CACHE['x']


def params(jt, jp):
    from oracle import net_temporal as OT
    key = ('P', jt, jp)
    if key not in _CACHE:
        _CACHE[key] = OT.init_params(C, K, jp, "2", seed=SEED, obj_bias=-1.0, k_join_type=jt)
    return _CACHE[key]


def clip_windows(step):
    """fp64 (T, K, 3, SIZE, SIZE): the windows gathered on the host by the hand-written table"""
    return clip_frames().astype(np.float64)[np.asarray(WINDOWS[(T, K, step)])]


def clip_reference(jt, jp, step, agnostic=False):
    """(ids, scores, boxes, rows, heads) of the oracle network on the T windows of the clip (read-only: shared)"""
    from oracle import net_temporal as OT
    key = ('ref', jt, jp, step, bool(agnostic))
    if key not in _CACHE:
        onet = OT.TemporalNet(params(jt, jp), C, K, jt, jp, "2")
        if agnostic:
            from tests import agnostic_oracle as AO
            _CACHE[key] = AO.net_detect(onet, clip_windows(step))
        else:
            _CACHE[key] = onet.detect(clip_windows(step))
    return _CACHE[key]
