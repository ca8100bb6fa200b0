#!/usr/bin/env python
"""The launch records of one plan as canonical JSON, to show that a change to a plan builder (training: YOLOV3._build_train,
train_plan.TrainPlan; inference: _build_infer / _build_infer_bf16 / _build_stream / extract_features, infer_plan.InferPlan)
leaves every launch as it was: build with one revision, then with the other, compare the files.

usage: python tools/plan_dump.py ROOT OUT.json [--plan train|infer|stream|features] [--storage bf16 | --precision bf16]
                                               [--k 3 --join max --pos late] [--conv-types 21,21,2,2,2,2] [--device cpu] [...]

ROOT is the directory that holds the `viddet_amd` package to import: this tree, or another revision's package staged
beside it (VD_LIB names the kernel library when that copy has none).  The training plan needs the GPU: its builder makes
streams and the autotuner times launch records the tuning table does not hold.  The inference plans also build with
`--device cpu` under VD_AUTOTUNE=0, where the builders only allocate and append records (`--plan features` then goes
through extract_features with the launches themselves left out).

Every record of every segment is written with its entry point, its arguments (scalars as they are, descriptor structs
field by field), its `meta` and the stream it runs on (main, side or parity i); a python record as `py` or `collective`
in one form for every revision's closures: record / wait with the event (by first appearance) and the stream's role, a
gradient bucket with its lo / hi and stream, a collective with the tensor it reduces.  Which arguments are pointers comes
from lib.SIGNATURES.  A pointer is written as a named tensor plus a byte offset (the plan's buffers and outputs, the weight
and gradient arenas, the nodes' tensors, the bf16 weight images), any other pointer as a label given at its first
appearance.  Run both revisions under one copy of the tuning table (VD_TUNE_CACHE): `--expect-tuned 0` on the second run
fails when its build added table entries, i.e. timed a descriptor the first run did not have."""
import argparse
import ctypes as C
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("root")
    ap.add_argument("out")
    ap.add_argument("--plan", default="train", choices=["train", "infer", "stream", "features"])
    ap.add_argument("--storage", default="fp32", choices=["fp32", "bf16"], help="training storage (set_storage)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"], help="inference precision (set_precision)")
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    ap.add_argument("--chunk", type=int, default=4, help="--plan stream: output frames per suffix run")
    ap.add_argument("--ring", type=int, default=None, help="--plan stream: ring slots (default: ring_size at step 1)")
    ap.add_argument("--agnostic", action="store_true")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--join", default=None, help="k_join_type")
    ap.add_argument("--pos", default=None, help="k_join_pos")
    ap.add_argument("--block", default="2", help="block_conv_type")
    ap.add_argument("--corr-pos", default=None)
    ap.add_argument("--corr-d", type=int, default=None)
    ap.add_argument("--rnn-pos", default=None, choices=["late", "out"], help="bidirectional ConvGRU over the window")
    ap.add_argument("--t-out", action="store_true", help="per-frame outputs (k = 5)")
    ap.add_argument("--conv-types", default=None, help="e.g. 21,21,2,2,2,2 with --k 3: yolo3_3ddarknet (the TdwNode passes)")
    ap.add_argument("--noback", action="store_true")
    ap.add_argument("--freeze-base", action="store_true")
    ap.add_argument("--range-exact", action="store_true",
                    help="two tensors in net._range_exact, closed over the tensors derived from them (concat, pool, select, add)")
    ap.add_argument("--range-exact-also", default=None, metavar="TENSOR",
                    help="with --range-exact: one more tensor by name, e.g. n0.tr - the records behind n0.cat then leave the fp16 split")
    ap.add_argument("--syncbn", default=None, choices=["all", "reference"],
                    help="SyncBN on a one-rank gloo group (VD_FORCE_DIST=1 puts the exchanges in the plan)")
    ap.add_argument("--expect-tuned", type=int, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from viddet_amd import lib as L
    from viddet_amd import model as M

    if a.syncbn:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29563")
        torch.distributed.init_process_group("gloo", rank=0, world_size=1)
    classes = ["c%d" % i for i in range(a.classes)]
    norm = dict(norm_layer="syncbn", norm_kwargs=dict(scope=a.syncbn)) if a.syncbn else {}
    if a.device != "cuda":
        norm["device"] = a.device
    if a.agnostic:
        norm["agnostic"] = True
    if a.noback:
        net = M.yolo3_no_backbone(classes, **norm)
    elif a.conv_types:
        net = M.yolo3_3ddarknet(classes, freeze_base=a.freeze_base, k=a.k, conv_types=[int(c) for c in a.conv_types.split(",")],
                                **norm)
    else:
        net = M.yolo3_darknet53(classes, freeze_base=a.freeze_base, k=a.k, k_join_type=a.join, k_join_pos=a.pos,
                                block_conv_type=a.block, t_out=a.t_out, corr_pos=a.corr_pos, corr_d=a.corr_d,
                                **(dict(rnn_pos=a.rnn_pos) if a.rnn_pos else {}), **norm)   # (only when asked: older revisions have no such argument)
    if a.range_exact:
        bn = [n for n in net.conv_nodes if n.bn]
        net._range_exact.update([bn[3].dst, "dz:" + bn[6].name] + ([a.range_exact_also] if a.range_exact_also else []))
        if hasattr(net, "_close_range_exact"):     # the rule covers what is derived from a flagged tensor: the outputs of
            net._close_range_exact()               # concatenations, temporal pools, frame selections and adds behind it
    B, H = a.batch, a.size
    cuda = net.device.type == "cuda"
    extra = {}                      # further named tensors of the plan
    if a.plan == "train":
        if a.storage == "bf16":
            net.set_storage("bf16")
        # (revisions before the two storages shared one builder have _build_train_bf16)
        build = getattr(net, "_build_train_bf16", None) if a.storage == "bf16" else None
        tp = (build or net._build_train)(B, H, H)
        segments = [(phase, seg) for phase in ("fwd", "bwd") for seg in tp[phase]]
        bufs, slots, packs = dict(tp["bufs"]), tp["slots"], []
        extra = {k: tp[k] for k in ("ws", "losses")}
    else:
        net.set_precision(a.precision)
        bf16, slots, packs = a.precision == "bf16", {}, []
        if a.plan == "infer":
            built = (net._build_infer_bf16 if bf16 else net._build_infer)(B, H, H)
            progs, bufs, o = [("infer", built[0])], dict(built[1]), built[2]
            packs = built[3] if bf16 else []
        elif a.plan == "stream":
            from viddet_amd.stream import ring_size
            sp = net._build_stream(a.chunk, H, H, a.ring or ring_size(net._k, 1, a.chunk))
            progs, o, packs = [("pre", sp["pre"]), ("suf", sp["suf"])], sp["o"], sp["packs"]
            bufs = {"pre:" + k: t for k, t in sp["pb"].items()}
            bufs.update(("suf:" + k, t) for k, t in sp["sb"].items())
            extra["slots"] = sp["slots"]
        else:
            # the features plan is built inside extract_features; without a GPU the call keeps everything but its launches
            if not cuda:
                M.Program.run = lambda self: None
                net._refresh_fold = net._refresh_wamax = lambda: None
                net._stage_inputs = lambda bufs, x: None
            net.extract_features(torch.zeros(B, 3, H, H, device=net.device))
            prog, bufs = net._programs[("features", B, H, H)]
            progs, bufs, o = [("features", prog)], dict(bufs), {}
        if bf16 and cuda:           # the bf16 records are tuned once their weight images exist (_forward_infer, detect_video)
            net._refresh_bf16(packs)
            for _, prog in progs:
                net._tune_bf16(prog)
        segments = progs
        extra.update(("o." + k, t) for k, t in o.items())
    if cuda:
        torch.cuda.synchronize()

    named = []                      # (base, bytes, name)
    def name(label, t):
        if torch.is_tensor(t) and t.device.type == net.device.type and t.numel():
            named.append((t.data_ptr(), t.numel() * t.element_size(), label))
    for k, t in list(bufs.items()) + list(extra.items()):
        name(k, t)
    for k in ("weights", "grads"):
        name(k, getattr(net, k))
    for i, t in getattr(net, "_sk_ws", {}).items():     # the stream-K hand-off workspaces, by stream index
        name("sk_ws%d" % i, t)
    # (the nodes of a streaming prefix are copies of the net's: the bf16 fold vectors live on the copy the pack names)
    for n in list(net.nodes) + list(net.conv_nodes) + [pk[0] for pk in packs]:
        for k, t in vars(n).items():
            name(n.name + "." + k, t)
    for pk in packs:
        name(pk[0].name + ".wb", pk[1])
    labels = {}

    def ptr(p):
        if not p:
            return None
        hits = [(-base, nb, label) for base, nb, label in named if base <= p < base + nb]
        if hits:                    # the innermost view: the highest base, then the smallest extent
            nbase, _, label = min(hits)
            return "%s+%d" % (label, p + nbase)
        return labels.setdefault(("ptr", p), "ptr%d" % len(labels))

    par = list(getattr(net, "_par_streams", None) or [])

    def role(st):
        if st is None:
            return "main"
        return next(("parity%d" % (i + 1) for i, s in enumerate(par) if s is st), "side")

    def val(v, ty):
        if isinstance(v, M.Slot):
            return "slot:" + slot_of[id(v)]
        if ty is C.c_void_p:
            return ptr(v)
        if hasattr(v, "_obj"):      # C.byref(...)
            return val(v._obj, type(v._obj))
        if isinstance(ty, type) and issubclass(ty, C.Array):
            return [val(x, ty._type_) for x in v]
        if isinstance(ty, type) and issubclass(ty, C.Structure):
            return {f: val(getattr(v, f), t) for f, t in ty._fields_}
        return v

    def py(fn, kind):
        """One description of a python record, whichever revision made its closure: an event record / wait as the event
        (by first appearance) and the role of the stream it is recorded on / of the stream that waits; a gradient bucket as
        its arena range and the stream its all-reduce is queued behind; anything else (a collective) as what it holds."""
        code = fn.__code__
        held = dict(zip(code.co_freevars, [c.cell_contents for c in fn.__closure__ or ()]))
        if fn.__defaults__:
            held.update(zip(code.co_varnames[code.co_argcount - len(fn.__defaults__):code.co_argcount], fn.__defaults__))
        events = [v for v in held.values() if isinstance(v, torch.cuda.Event)]
        streams = [v for v in held.values() if isinstance(v, torch.cuda.Stream)]
        assert len(events) <= 1 and len(streams) <= 1, sorted(held)
        # (closures of older revisions hold the side stream and a flag `on_side` that says whether it is the one meant)
        st = role(streams[0]) if streams and held.get("on_side", True) else "main"
        if events:
            what = "record" if "record" in code.co_names else "wait" if "wait_event" in code.co_names else None
            assert what, code.co_names
            return {kind: what, "event": labels.setdefault(("event", id(events[0])), "event%d" % len(labels)), "stream": st}
        if "lo" in held and "hi" in held:
            return {kind: "bucket", "lo": held["lo"], "hi": held["hi"], "stream": st}
        out = {kind: "call", "stream": st}
        for k in sorted(held):
            v = held[k]
            if torch.is_tensor(v):
                out[k] = ptr(v.data_ptr())
            elif isinstance(v, (bool, int, float)):
                out[k] = v
        return out

    slot_of = {id(s): k for k, s in slots.items()}
    doc, nrec = [], 0
    for phase, seg in segments:
        if not isinstance(seg, M.Program):
            doc.append({"phase": phase, "segment": py(seg, "py")})
            continue
        recs = []
        for (fname, fn, args), meta, st in zip(seg.recs, seg.meta, seg.streams):
            if fname is None:
                recs.append(py(fn, "collective" if (meta or {}).get("kind") == "collective" else "py"))
            else:
                fname = fn.__name__          # the entry point (a record may be listed under a family label: Program.add)
                sig = L.SIGNATURES[fname][1]
                recs.append({"fn": fname,"args": [val(v, t) for v, t in zip(args, sig)], "meta": meta, "stream": role(st)})
        nrec += len(recs)
        doc.append({"phase": phase, "records": recs})
    with open(a.out, "w") as f:
        json.dump(doc, f, sort_keys=True, indent=0)
    tuned = M._TUNE_CACHE.tuned
    print("%s: %d records, %d new tuning-table entries" % (a.out, nrec, tuned))
    if a.expect_tuned is not None and tuned != a.expect_tuned:
        sys.exit("expected %d new tuning-table entries" % a.expect_tuned)


if __name__ == "__main__":
    main()
