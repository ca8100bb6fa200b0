"""Generates tests/golden/vid_golden.npz by running the reference's own metrics/imgnetvid.py (plain NumPy) on a synthetic
set of clips, in the build container.  Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_vid_golden.py

The reference module is loaded by path with `mxnet` replaced by a stub (metric.EvalMetric, nd.NDArray), `tqdm` by a
pass-through and its `np` by a proxy whose `array` falls back to a 1-D object array on a ragged list (the old-NumPy
behaviour the reference was written for) and that still has `np.float`.  Only arrays travel: the inputs (label rows with
track ids, detection rows, motion IoUs) and the reference's outputs (boxoverlap, parse_set's thresholds, vid_ap, ap per
class and agnostic, get()'s strings).  The conditions the fixture must meet are checked here, on the reference's outputs
and with tests/vid_eval_oracle.py, and asserted again by tests/test_vid_metric_cpu.py."""
import importlib.util
import os
import sys
import time
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"


class _NP:
    float = float

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, *a, **kw):
        try:
            return np.array(obj, *a, **kw)
        except ValueError:
            out = np.empty(len(obj), dtype=object)
            for i, o in enumerate(obj):
                out[i] = o
            return out


def load_reference():
    mx = types.ModuleType("mxnet")
    mx.metric = types.ModuleType("mxnet.metric")
    mx.metric.EvalMetric = type("EvalMetric", (), {"__init__": lambda self, name, *a, **k: setattr(self, "name", name)})
    mx.nd = types.ModuleType("mxnet.nd")
    mx.nd.NDArray = type("NDArray", (), {})
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    sys.modules.update({"mxnet": mx, "mxnet.metric": mx.metric, "mxnet.nd": mx.nd, "tqdm": tq})
    spec = importlib.util.spec_from_file_location("ref_imgnetvid_metric", os.path.join(REF, "metrics", "imgnetvid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.np = _NP()
    return mod


def build_set(seed, clips, frames, num_class):
    """label rows of SyntheticTracks clips + noisy detections with pairwise distinct scores"""
    from viddet_amd.data import SyntheticTracks
    ds = SyntheticTracks("synthetic", num_videos=clips, frames_per_video=frames, num_class=num_class, seed=seed)
    rng = np.random.default_rng([seed, 99])
    ids = ds.get_sample_ids()
    labels, dets = [], []
    W, H = 480, 360
    for sid in ids:
        rows = ds.get_label(sid)
        labels += [[sid] + r.tolist() for r in rows]
        for r in rows:
            s = np.array([r[2] - r[0] + 1, r[3] - r[1] + 1] * 2)
            for _ in range(int(rng.choice([0, 1, 1, 1, 2, 3]))):                  # none, one, or several on one ground truth
                box = r[:4] + rng.normal(0, 1, 4) * s * rng.choice([0.02, 0.06, 0.15, 0.3])
                cls = r[4] if rng.random() < 0.85 else rng.integers(0, num_class)
                dets.append([sid, cls, 0.0] + box.tolist())
        for _ in range(int(rng.integers(0, 3))):                                  # clutter, on frames without ground truth too
            xy = rng.uniform(0, (W - 20, H - 20))
            wh = np.exp(rng.uniform(np.log(10.0), np.log(250.0), 2))
            dets.append([sid, rng.integers(0, num_class), 0.0] + xy.tolist() + (xy + wh).tolist())
    dets = np.array(dets, np.float64)
    dets[:, 2] = 0.06 + 0.93 * (rng.permutation(len(dets)) + 0.5) / len(dets)     # pairwise distinct
    motion = ds.motion_ious
    return ids, np.array(labels, np.float64), motion, dets


def check_conditions(g, ap):
    """the fixture's conditions (ISSUE / DESIGN.md 25), on the reference's ap and the oracle's records"""
    from tests import vid_eval_oracle as E
    from viddet_amd.device_vid_metric import pack_images
    assert len(np.unique(g["dets"][:, 2])) == len(g["dets"]), "scores are not pairwise distinct"
    inside = ((ap > 0) & (ap < 1)).any(axis=2)
    assert inside.all(), "cells without a class with 0 < AP < 1:\n%r" % inside
    _, ds = E.load_golden_arrays(g)
    (det, gt), = pack_images(ds, E.golden_results(g), chunk_bytes=1 << 40)[0]
    rec_gt, rec_tp, rec_fp, img_nig, img_ngt, _, _ = E.match_records(det, gt, C=int(g["num_class"]))
    valid = rec_gt != -2
    codes = (rec_fp.view(np.uint32)[..., None] >> (2 * np.arange(16))) & 3
    unmatched = valid & (rec_gt == -1)
    for code in (1, 2, 3):
        assert (codes[unmatched] == code).any(), "fp rule %d is not exercised" % code
    # rule 0 by the motion comparison, not by the area gate: the cells of the all-areas range never gate
    assert (codes[unmatched & (img_ngt[:, None] > 0)][:, [4, 8, 12]] == 0).any(), "fp rule 0 (ovmax_ig > ovmax_nig) is not exercised"
    assert (codes[unmatched & (img_ngt[:, None] == 0)] == 2).any(), "no detection on a frame without ground truth"
    matched = rec_gt >= 0
    assert (matched & (rec_tp.view(np.uint32) != 0xffff)).any(), "no matched detection outside a cell"
    thr = g["thr"]
    assert (thr < 0.5).any(), "no small ground truth"
    # a detection that loses a ground truth to a higher-scored one: unmatched, yet a row of its class reaches thr for it
    lost = small = False
    from viddet_amd.vid_metric import overlaps, gt_thresholds
    for b in range(det.shape[0]):
        gv = gt[b, :, 4] >= 0
        if not gv.any():
            continue
        ov = overlaps(det[b, :, 2:6], gt[b, gv, :4])
        t = gt_thresholds(gt[b, gv, :4])
        same = det[b, :, 0][:, None] == gt[b, gv, 4][None]
        lost |= bool((unmatched[b] & ((ov >= t) & same).any(axis=1)).any())
        rows = np.nonzero(gv)[0]
        for j in np.nonzero(matched[b])[0]:
            k = int(np.nonzero(rows == rec_gt[b, j])[0][0])
            small |= bool(ov[j, k] < 0.5)
    assert lost, "no detection loses its ground truth to a higher-scored one"
    assert small, "no match below IoU 0.5 on a small ground truth"


def main():
    ref = load_reference()
    from tests import vid_eval_oracle as E
    seed, clips, frames, C = 7, 8, 24, 3
    ids, labels, motion, dets = build_set(seed, clips, frames, C)
    g = dict(sample_ids=np.array(ids, np.int64), labels=labels, dets=dets, num_class=np.int64(C),
             motion_counts=np.array([len(motion[str(s)]) for s in ids], np.int64),
             motion_values=np.concatenate([np.asarray(motion[str(s)], np.float64) for s in ids]))
    _, ds = E.load_golden_arrays(g)
    # boxoverlap on pairs: every detection against the first label row of its frame (or of the set), and label rows in pairs
    rng = np.random.default_rng(5)
    pa = np.concatenate([dets[rng.integers(0, len(dets), 200), 3:7], labels[rng.integers(0, len(labels), 56), 1:5]])
    pb = labels[rng.integers(0, len(labels), 256), 1:5]
    near = rng.integers(0, len(labels), 128)
    pa[:128] = labels[near, 1:5] + rng.normal(0, 6, (128, 4))
    pb[:128] = labels[near, 1:5]
    g["pairs"] = np.concatenate([pa, pb], axis=1)
    g["pair_iou"] = np.array([float(ref.boxoverlap(a, b)) for a, b in zip(pa, pb)])
    g["thr"] = np.concatenate([r["thr"] for r in ref.parse_set(ds, iou_thr=0.5, pixel_tolerance=10)])
    for i, n in enumerate((1, 5, 40)):
        tp = np.cumsum(rng.random(n) < 0.6).astype(np.float64)
        fp = np.cumsum(rng.random(n) < 0.4).astype(np.float64)
        g["ap_rec%d" % i], g["ap_prec%d" % i] = tp / max(tp[-1], 1.0) * 0.9, tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        g["ap_out%d" % i] = np.float64(ref.vid_ap(g["ap_rec%d" % i], g["ap_prec%d" % i]))
    results = E.golden_results(g)
    for agnostic, key in ((False, ""), (True, "_agnostic")):
        m = ref.VIDDetectionMetric(ds, agnostic=agnostic)
        by_sid = {}
        for r in results:
            by_sid.setdefault(r[0], []).append(r)
        for sid, rows in by_sid.items():
            rows = np.array(rows)
            m.update([rows[None, :, 3:7]], [rows[None, :, 1]], [rows[None, :, 2]], None, None, None, sid=sid)
        assert len(m._results) == len(results)
        t0 = time.perf_counter()
        ap = ref.vid_eval_motion(ds, m._results, m._motion_ranges, m._area_ranges, iou_threshold=0.5, agnostic=agnostic)
        g["ref_seconds" + key] = np.float64(time.perf_counter() - t0)
        names, values = m.get()
        g["ap" + key], g["names" + key], g["values" + key] = ap, np.array(names), np.array(values)
    check_conditions(g, g["ap"])
    out = os.path.join(HERE, "vid_golden.npz")
    np.savez_compressed(out, **g)
    print("%s: %d bytes, %d images, %d label rows, %d detections; the reference's vid_eval_motion took %.2f s per class, "
          "%.2f s agnostic on this CPU" % (out, os.path.getsize(out), len(ids), len(labels), len(dets), g["ref_seconds"],
                                           g["ref_seconds_agnostic"]))
    print(np.round(g["ap"], 3))


if __name__ == "__main__":
    main()
