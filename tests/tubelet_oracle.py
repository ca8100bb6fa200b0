"""The tubelet pass as plain loops over dicts, written from the rules of DESIGN.md 32 and independent of
viddet_amd.tubelet.tubelet_host (it shares row_classes with it and nothing else): tests/test_tubelet_cpu.py holds the two
array_equal on every case."""
import numpy as np

from viddet_amd.seq_nms import row_classes

f32 = np.float32


def _lerp(a, b, w):
    with np.errstate(all="ignore"):
        d = f32(f32(b) - f32(a))
        return f32(f32(a) + f32(d * w))


def tubelet_loops(ids, scores, bboxes, track, clip_start=None, num_class=None, rescore="avg", max_gap=7, drop_untracked=False,
                  stats=None):
    ids, scores, bboxes = np.asarray(ids, f32), np.asarray(scores, f32), np.asarray(bboxes, f32)
    F, N = bboxes.shape[0], bboxes.shape[1]
    track = np.asarray(track)
    idv, scv = ids.reshape(F, N), scores.reshape(F, N)
    cls = row_classes(idv, scv, num_class)
    bounds = [0, F] if clip_start is None else [int(v) for v in clip_start]
    o_ids, o_sc, o_box = np.full((F, N), -1, f32), np.full((F, N), -1, f32), np.full((F, N, 4), -1, f32)
    o_perm, o_trk, o_drop = np.full((F, N), -1, np.int32), np.full((F, N), -1, np.int32), np.zeros(F, np.int32)
    n_tracks, n_filled, n_dropped = [], [], []
    for t0, t1 in zip(bounds[:-1], bounds[1:]):
        limit = (t1 - t0) * N
        members = {}                                   # track id -> [(frame, row)] in frame order
        owner = {}                                     # (frame, row) -> track id, members only
        for t in range(t0, t1):
            seen = set()
            for i in range(N):
                u = int(track[t, i])
                if cls[t, i] < 0 or u < 0 or u >= limit or u in seen:
                    continue
                seen.add(u)
                members.setdefault(u, []).append((t, i))
                owner[(t, i)] = u
        track_score = {}
        for u, rows in members.items():
            if rescore == "avg":
                s = f32(0)
                with np.errstate(over="ignore"):
                    for t, i in rows:
                        s = f32(s + scv[t, i])
                    s = f32(s / f32(len(rows)))
            elif rescore == "max":
                s = scv[rows[0]]
                for t, i in rows[1:]:
                    if scv[t, i] > s:
                        s = scv[t, i]
            else:
                s = None
            track_score[u] = s
        fills = {}                                     # frame -> [(track id, id, score, box)]
        for u in sorted(members):
            rows = members[u]
            for (fa, ia), (fb, ib) in zip(rows[:-1], rows[1:]):
                g = fb - fa
                if g <= 1 or g > max_gap + 1:
                    continue
                for j in range(1, g):
                    w = f32(f32(j) / f32(g))
                    box = np.array([_lerp(bboxes[fa, ia, c], bboxes[fb, ib, c], w) for c in range(4)], f32)
                    s = track_score[u] if rescore is not None else _lerp(scv[fa, ia], scv[fb, ib], w)
                    fills.setdefault(fa + j, []).append((u, idv[fa, ia], s, box))
        filled = 0
        for t in range(t0, t1):
            entries = []                               # (score, id, box, perm, track)
            for i in range(N):
                if cls[t, i] < 0:
                    continue
                u = owner.get((t, i), -1)
                if drop_untracked and u < 0:
                    continue
                s = scv[t, i] if (u < 0 or rescore is None) else track_score[u]
                entries.append((s, idv[t, i], bboxes[t, i], i, u))
            for u, id_, s, box in fills.get(t, []):    # ascending track id: the outer loop above ran sorted
                if len(entries) < N:
                    entries.append((s, id_, box, -2, u))
                    filled += 1
                else:
                    o_drop[t] += 1
            # an insertion sort, descending, that never moves an entry past an equal one
            done = []
            for e in entries:
                k = len(done)
                while k > 0 and done[k - 1][0] < e[0]:
                    k -= 1
                done.insert(k, e)
            for k, (s, id_, box, p, u) in enumerate(done):
                o_sc[t, k], o_ids[t, k], o_box[t, k], o_perm[t, k], o_trk[t, k] = s, id_, box, p, u
        n_tracks.append(len(members))
        n_filled.append(filled)
        n_dropped.append(int(o_drop[t0:t1].sum()))
    if stats is not None:
        stats.update(tracks=n_tracks, filled=n_filled, dropped=n_dropped)
    return o_ids.reshape(ids.shape), o_sc.reshape(scores.shape), o_box, o_perm, o_trk, o_drop
