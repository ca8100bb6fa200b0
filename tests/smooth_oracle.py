"""The loop form that viddet_amd.smooth.smooth_host is held to (tests/test_smooth_cpu.py): written from the textbook, not from the
definition.  The full 7-state Kalman filter of Bewley's SORT (state u, v, s, r, du, dv, ds) and the Rauch-Tung-Striebel
fixed-interval smoother over it, in float64, with matrix products and np.linalg.inv:

    predict   x- = F x,  P- = F P F^T + Q          (first Bewley's rule: if s + ds <= 0 then ds = 0)
    update    K = P- H^T (H P- H^T + R)^-1,  x = x- + K (z - H x-),  P = (I - K H) P-
    smooth    C_k = P_k F^T (P-_{k+1})^-1,  xs_k = x_k + C_k (xs_{k+1} - x-_{k+1}),  xs_last = x_last

It runs over EVERY frame of a segment's span and skips the update where the track has no member (x_k = x-_k, P_k = P-_k there).
Membership and segments are found with plain loops over frames and rows."""
import numpy as np

F_ = np.eye(7)
F_[0, 4] = F_[1, 5] = F_[2, 6] = 1.0
H_ = np.eye(4, 7)
Q_ = np.diag([1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 1e-4])
R_ = np.diag([1.0, 1.0, 10.0, 10.0])
P0_ = np.diag([10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4])


def to_z(box):
    w, h = box[2] - box[0], box[3] - box[1]
    return np.array([box[0] + w / 2.0, box[1] + h / 2.0, w * h, w / h])


def to_box(x):
    w = np.sqrt(x[2] * x[3])
    h = x[2] / w
    return np.array([x[0] - w / 2.0, x[1] - h / 2.0, x[0] + w / 2.0, x[1] + h / 2.0])


def rts_segment(frames, boxes):
    """frames: the ascending frame numbers of a segment's members, boxes: their corner boxes -> (the smoothed boxes (n,4), the
    filtered boxes (n,4)), float64"""
    frames = [int(f) for f in frames]
    at = dict(zip(frames, range(len(frames))))
    span = range(frames[0], frames[-1] + 1)
    xf, Pf, xp, Pp = [], [], [], []
    x = np.concatenate([to_z(np.asarray(boxes[0], np.float64)), np.zeros(3)])
    P = P0_.copy()
    for f in span:
        if f == frames[0]:
            xp.append(x.copy()), Pp.append(P.copy())
        else:
            x = x.copy()
            if x[2] + x[6] <= 0:
                x[6] = 0.0
            x = F_ @ x
            P = F_ @ P @ F_.T + Q_
            xp.append(x.copy()), Pp.append(P.copy())
            if f in at:
                S = H_ @ P @ H_.T + R_
                K = P @ H_.T @ np.linalg.inv(S)
                x = x + K @ (to_z(np.asarray(boxes[at[f]], np.float64)) - H_ @ x)
                P = (np.eye(7) - K @ H_) @ P
        xf.append(x.copy()), Pf.append(P.copy())
    xs = [None] * len(xf)
    xs[-1] = xf[-1]
    for k in range(len(xf) - 2, -1, -1):
        C = Pf[k] @ F_.T @ np.linalg.inv(Pp[k + 1])
        xs[k] = xf[k] + C @ (xs[k + 1] - xp[k + 1])
    pick = [f - frames[0] for f in frames]
    return np.array([to_box(xs[k]) for k in pick]), np.array([to_box(xf[k]) for k in pick])


def smooth_loop(ids, scores, bboxes, track, clip_start=None, num_class=None, max_gap=7):
    """the whole pass with loops -> (sbox (F,N,4) float64, slen (F,N))"""
    ids, scores = np.asarray(ids, np.float64), np.asarray(scores, np.float64)
    bboxes = np.asarray(bboxes, np.float64)
    Fr, N = bboxes.shape[:2]
    ids, scores = ids.reshape(Fr, N), scores.reshape(Fr, N)
    sbox = bboxes.copy()
    slen = np.zeros((Fr, N), np.int64)
    cs = [0, Fr] if clip_start is None else list(clip_start)
    for t0, t1 in zip(cs[:-1], cs[1:]):
        tracks = {}
        for t in range(t0, t1):
            seen = set()
            for i in range(N):
                present = ids[t, i] >= 0 and np.isfinite(scores[t, i]) and (num_class is None or ids[t, i] < num_class)
                u = int(track[t, i])
                if present and 0 <= u < (t1 - t0) * N and u not in seen:
                    seen.add(u)
                    tracks.setdefault(u, []).append((t, i))
        for members in tracks.values():
            segs = [[members[0]]]
            for m in members[1:]:
                if m[0] - segs[-1][-1][0] > max_gap + 1:
                    segs.append([])
                segs[-1].append(m)
            for seg in segs:
                for t, i in seg:
                    slen[t, i] = len(seg)
                if len(seg) >= 2:
                    out, _ = rts_segment([t for t, _ in seg], [bboxes[t, i] for t, i in seg])
                    for (t, i), b in zip(seg, out):
                        if np.isfinite(b).all():
                            sbox[t, i] = b
    return sbox, slen
