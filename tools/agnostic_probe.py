"""Times the detection tail alone - decode + filter and NMS - in its two forms on the same head tensors: the per-class tail
(vd_yolo_decode_filter + vd_nms_topk) and the class-agnostic one (vd_yolo_decode_filter_agnostic + vd_nms_agnostic,
--model_agnostic).

Heads are random: box logits N(0, 1) (sizes x 0.5), class logits N(-2, 2), objectness logits N(mu, 2) with mu set so that
`--pass-rate` of the anchors clear valid_thresh = 0.01 (0.05: what a trained network leaves; 1.0: an untrained one, every anchor
of an image in ONE list).  The two forms alternate block by block (`--blocks` blocks of `--reps` launches, events around each
block) and the minimum block is reported, per kernel and for the pair.  For the agnostic decode the bytes are stated three
ways: the 4 bytes per anchor it uses, the 20 bytes per anchor of the box + objectness channels, and the distinct 128-byte lines
its gather touches (what must come through L2), each with the rate the time corresponds to.  One JSON line per measurement.

  python tools/agnostic_probe.py [--batch 32] [--size 608] [--classes 80] [--heads fp32|bf16] [--pass-rate 0.05]
                                 [--tail both|per_class|agnostic] [--reps 20] [--blocks 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ANCHORS = [[116, 90, 156, 198, 373, 326], [30, 61, 62, 45, 59, 119], [10, 13, 16, 30, 33, 23]]
STRIDES = [32, 16, 8]


def _block(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--heads", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--pass-rate", type=float, default=0.05)
    ap.add_argument("--tail", default="both", choices=["both", "per_class", "agnostic"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    a = ap.parse_args()
    from viddet_amd import ops
    B, C_, size = a.batch, a.classes, a.size
    bf16 = a.heads == "bf16"
    if bf16 and a.tail != "agnostic":
        print(json.dumps(dict(note="the per-class kernels read fp32 heads only: --heads bf16 times the agnostic tail alone")), flush=True)
        a.tail = "agnostic"
    grids = [size // s for s in STRIDES]
    npred, ldh = 5 + C_, ops.round_up(3 * (5 + C_), 32)
    P = 3 * sum(g * g for g in grids)
    # objectness logit N(mu, 2) clears logit(0.01) = -4.595 with probability pass_rate
    if a.pass_rate >= 1.0:
        mu = 4.0
    else:
        z = float(torch.distributions.Normal(0.0, 1.0).icdf(torch.tensor(1.0 - a.pass_rate)))
        mu = -4.595 - 2.0 * z
    g_ = torch.Generator(device="cuda").manual_seed(1)
    heads = []
    for g in grids:
        t = torch.zeros(B, g, g, ldh, device="cuda")
        v = t[..., :3 * npred].view(B, g, g, 3, npred)
        v.normal_(generator=g_)
        v[..., 2:4] *= 0.5
        v[..., 4] = v[..., 4] * 2.0 + mu
        v[..., 5:] = v[..., 5:] * 2.0 - 2.0
        heads.append(t.bfloat16() if bf16 else t)
    hd = ops.make_head_desc(heads, grids, ldh, STRIDES, ANCHORS, B, C_)
    esz = 2 if bf16 else 4
    head_bytes = sum(t.numel() for t in heads) * esz
    # distinct 128-byte lines the objectness gather touches (tensors are 256-byte aligned; the same count for every image)
    lines = 0
    for g in grids:
        off = (np.arange(g * g)[:, None] * ldh + np.arange(3)[None, :] * npred + 4) * esz
        lines += len(np.unique(off // 128))
    line_bytes = lines * 128 * B
    out = dict(ids=torch.empty(B, 100, device="cuda"), sc=torch.empty(B, 100, device="cuda"), bx=torch.empty(B, 100, 4, device="cuda"),
               rows=torch.empty(B, 100, dtype=torch.int32, device="cuda"), ws=torch.zeros(4 * B, dtype=torch.uint8, device="cuda"),
               cnt=torch.zeros(B, dtype=torch.int32, device="cuda"))
    forms = {}
    if a.tail in ("both", "per_class"):
        cap = C_ * P
        cs, cr = torch.empty(B, cap, device="cuda"), torch.empty(B, cap, dtype=torch.int32, device="cuda")
        dec = lambda: ops.yolo_decode_filter(hd, 0.01, cs, cr, cap, out["cnt"])
        nms = lambda: ops.nms_topk(hd, cs, cr, cap, out["cnt"], 0.45, 400, 100, out["ids"], out["sc"], out["bx"], out["rows"], out["ws"])
        forms["per_class"] = (dec, nms)
    if a.tail in ("both", "agnostic"):
        cs2, cr2 = torch.empty(B, P, device="cuda"), torch.empty(B, P, dtype=torch.int32, device="cuda")
        dec2 = lambda: ops.yolo_decode_filter_agnostic(hd, 0.01, cs2, cr2, P, out["cnt"], head_bf16=bf16)
        nms2 = lambda: ops.nms_agnostic(hd, cs2, cr2, P, out["cnt"], 0.45, 400, 100, out["ids"], out["sc"], out["bx"], out["rows"],
                                        out["ws"], head_bf16=bf16)
        forms["agnostic"] = (dec2, nms2)
    best, counts, kept = {}, {}, {}
    for name, (dec, nms) in forms.items():                     # warm-up; the list lengths each form's NMS sees
        dec(); nms()
        torch.cuda.synchronize()
        counts[name] = out["cnt"].cpu().numpy().copy()
        kept[name] = int((out["rows"] >= 0).sum())
    for _ in range(a.blocks):
        for name, (dec, nms) in forms.items():
            dec()                                                # (the NMS blocks run on this form's own candidates)
            for kind, fn in (("decode", dec), ("nms", nms), ("pair", lambda: (dec(), nms()))):
                ms = _block(fn, a.reps)
                best[(name, kind)] = min(best.get((name, kind), 1e9), ms)
    base = dict(batch=B, size=size, classes=C_, heads=a.heads, pass_rate=a.pass_rate, anchors_per_image=P, head_mb=round(head_bytes / 1e6, 1))
    for name in forms:
        r = dict(base, tail=name, decode_ms=round(best[(name, "decode")], 4), nms_ms=round(best[(name, "nms")], 4),
                 pair_ms=round(best[(name, "pair")], 4), list_mean=float(counts[name].mean()), list_max=int(counts[name].max()),
                 kept_rows=kept[name])
        if name == "agnostic":
            t = best[(name, "decode")] * 1e-3
            r.update(useful_bytes_per_anchor=esz, ideal_bytes_per_anchor=5 * esz, line_bytes_per_anchor=round(line_bytes / (B * P), 1),
                     line_share_of_head=round(line_bytes / head_bytes, 3), gbs_on_ideal=round(5 * esz * B * P / t / 1e9, 1),
                     gbs_on_lines=round(line_bytes / t / 1e9, 1))
        else:
            r.update(gbs_on_head=round(head_bytes / (best[(name, "decode")] * 1e-3) / 1e9, 1))
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
