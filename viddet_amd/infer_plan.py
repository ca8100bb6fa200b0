"""The builder of the inference programs (YOLOV3._build_infer, _build_infer_bf16, _build_stream, extract_features): one
object, one method per node type, written once for fp32 and bf16 storage."""
import ctypes as C
import os

import torch

from . import lib as L
from . import ops
from .consts import ANCHORS, STRIDES, LEAKY_SLOPE
from .lib import ConvDesc, EPI_AFFINE, EPI_LEAKY, EPI_RESIDUAL
from .model import (Program, ROUTE_TENSORS, ConvNode, UpcatNode, PoolNode, CorrNode, GruNode, SelNode, AddNode, TdwNode,
                    autotune_program, node_inputs)
from .ops import round_up


def bf16_channels(c):
    """channels of a bf16 activation tensor: runs of 64 (one 128-byte K-step); a 32-channel map stays unpadded (two taps per
    K-step, vd_conv_bf16.hip)"""
    return 32 if c == 32 else round_up(c, 64)


class InferPlan:
    """The inference records of `net` at one input size.  The storage changes the leaves only: bf16 runs the `_bf16` twins
    of the elementwise kernels on tensors of bf16_channels() channels (the copy kernels move 4-byte words, two channels
    each), has no max-abs records (they feed fp32's fp16-split arithmetic), and its convolutions are vd_conv_igemm_bf16 on
    padded bf16 weight images (`packs`, filled by _refresh_bf16); the prediction heads are fp32 in both."""

    NODE = {UpcatNode: 'upcat', PoolNode: 'pool', CorrNode: 'corr', SelNode: 'sel_add', AddNode: 'sel_add', GruNode: 'gru',
            TdwNode: 'tdw', ConvNode: 'conv'}

    def __init__(self, net, H, W, bf16):
        self.net, self.H, self.W, self.bf16 = net, H, W, bf16
        self.sfx, self.esz, self.cw = ('_bf16', 2, 2) if bf16 else ('', 4, 1)
        self.cp = bf16_channels if bf16 else (lambda c: c)
        self.packs = []                    # bf16: (node, weight image, its padded Co, its padded Ci)
        self.fuse_stem = None              # bf16: (stem, the stride-2 conv that computes it inside its own launch)

    # ------------------------------------------------------------------ the programs
    def build(self, B):
        """the whole network on B samples -> (prog, bufs, outputs), bf16: + packs"""
        net, prog = self.net, Program()
        bufs = self.buffers(net.tensors, B) if self.bf16 else net._buffers('infer', B, self.H, self.W, False)
        self.input_stage(prog, bufs, B)
        self.add_nodes(prog, net.nodes, bufs, B)
        o = self.detect_tail(prog, bufs, B)
        if self.bf16:                      # (tuned once the weight images exist: _bf16_current)
            return prog, bufs, o, self.packs
        autotune_program(prog)
        return prog, bufs, o

    def build_features(self, B):
        """the fp32 trunk up to the last route tensor (extract_features) -> (prog, bufs)"""
        net, prog = self.net, Program()
        bufs = net._buffers('infer', B, self.H, self.W, False)
        last = max(i for i, n in enumerate(net.nodes) if isinstance(n, ConvNode) and n.dst == ROUTE_TENSORS[-1][0])
        self.input_stage(prog, bufs, B)
        self.add_nodes(prog, net.nodes[:last + 1], bufs, B)
        autotune_program(prog)
        return prog, bufs

    def build_stream(self, Bc, S):
        """The two programs of detect_video: the per-frame prefix on Bc frames, and the joins off the ring of S slots + the
        suffix + decode / NMS on Bc windows."""
        net, dev = self.net, self.net.device
        prefix, suffix = net._stream_split()
        srcs = [n.src for n in suffix if isinstance(n, PoolNode)]
        pb = self.buffers(['in'] + [n.dst for n in prefix], Bc, stream=True)
        sb = self.buffers([n.dst for n in suffix], Bc, stream=True)
        for t in srcs:                                           # slot = frame index mod S
            sb['ring:' + t] = torch.zeros((S,) + tuple(pb[t].shape[1:]), dtype=pb[t].dtype, device=dev)
        slots = torch.zeros(Bc, net._k, dtype=torch.int32, device=dev)
        pre, suf = Program(), Program()
        self.input_stage(pre, pb, Bc)
        self.add_nodes(pre, prefix, pb, Bc)
        self.input_stage(suf, sb, Bc)
        self.add_nodes(suf, suffix, sb, Bc, ring=(slots, S))
        o = self.detect_tail(suf, sb, Bc)
        if not self.bf16:
            autotune_program(pre)
            autotune_program(suf)
        return dict(pre=pre, suf=suf, pb=pb, sb=sb, o=o, packs=self.packs, slots=slots, srcs=srcs, S=S)

    def buffers(self, names, B, stream=False):
        """Activation tensors `names` of an inference plan on B samples: bf16 tensors of bf16_channels() channels, zeroed
        (pad channels are never written), beside fp32 heads, or fp32 tensors with their max-abs slots (the whole-network
        fp32 plan takes net._buffers instead).  stream: the tensors hold B frames, not B windows of `fr` frames."""
        net, dev, bufs = self.net, self.net.device, {}
        for name in names:
            c, div, ld, fr = net.tensors[name]
            rows = B if stream else B * fr
            if name == 'in':
                bufs['in'] = (torch.zeros if stream else torch.empty)(rows, 3, self.H, self.W, device=dev)
            elif self.bf16 and name not in net.head_names:
                bufs[name] = torch.zeros(rows, self.H // div, self.W // div, self.cp(c), dtype=torch.bfloat16, device=dev)
            else:
                bufs[name] = torch.empty(rows, self.H // div, self.W // div, ld, device=dev)
                if not self.bf16:
                    bufs[name].normal_()                       # the autotuner times on these: noise, not zero pages (_buffers)
        if not self.bf16:
            act = [nm for nm in names if nm != 'in']
            bufs['amax'] = torch.zeros(max(1, len(act)) * L.AMAX_FLOATS, device=dev)
            for i, nm in enumerate(act):
                bufs['amax:' + nm] = bufs['amax'][i * L.AMAX_FLOATS:(i + 1) * L.AMAX_FLOATS]
        return bufs

    def input_stage(self, prog, bufs, B):
        """fp32: the max-abs reset (and the no-backbone maps NCHW -> NHWC, _add_input_stage).  bf16: only the no-backbone
        net has one - its three cached feature maps arrive as fp32 NCHW: NHWC, then one conversion each."""
        net, H, W = self.net, self.H, self.W
        if not self.bf16:
            net._add_input_stage(prog, bufs, B, H, W)
        elif net.noback:
            for nm, c_, d_ in ROUTE_TENSORS:
                bufs['in:' + nm] = torch.empty(B, c_, H // d_, W // d_, device=net.device)
                bufs['f32:' + nm] = torch.empty(B, H // d_, W // d_, c_, device=net.device)
                assert self.cp(c_) == c_
                prog.add('vd_nchw_to_nhwc', bufs['in:' + nm].data_ptr(), bufs['f32:' + nm].data_ptr(), B, c_, H // d_, W // d_)
                n_el = bufs[nm].numel()
                prog.add('vd_pack_weight_bf16', bufs['f32:' + nm].data_ptr(), bufs[nm].data_ptr(), 1, 1, n_el, n_el, 1)

    def detect_tail(self, prog, bufs, B):
        """decode + NMS over the (fp32) heads in `bufs`; returns the output tensors"""
        net, dev = self.net, self.net.device
        grids = net._grid(self.H, self.W)
        Bh = B * net._head_frames            # images the decode / NMS see (B*t with per-frame predictions)
        hd = ops.make_head_desc([bufs[h] for h in net.head_names], grids, round_up(3 * (5 + net.num_class), 32),
                                STRIDES[::-1], ANCHORS[::-1], Bh, net.num_class)
        P = 3 * sum(g * g for g in grids)
        # Class-agnostic: one candidate per anchor at the most, so the lists hold P entries per image and cannot overflow.
        # Per class: one candidate slot per row of the reference's (B, C*P, 6) tensor - box_nms (yolo3.py:1197-1202) has no
        # cap, and an untrained net (validation after epoch 0) passes valid_thresh on every row.  8 bytes x C*P per image
        # (14.6 MB at 608x608 / 80 classes) is address space, not traffic: only the rows that pass are ever written or read.
        cap = P if net.agnostic else net.num_class * P
        o = dict(cand_score=torch.empty(Bh, cap, device=dev), cand_row=torch.empty(Bh, cap, dtype=torch.int32, device=dev),
                 counts=torch.zeros(Bh, dtype=torch.int32, device=dev), ids=torch.empty(Bh, net.post_nms, 1, device=dev),
                 scores=torch.empty(Bh, net.post_nms, 1, device=dev), bboxes=torch.empty(Bh, net.post_nms, 4, device=dev),
                 rows=torch.empty(Bh, net.post_nms, dtype=torch.int32, device=dev),
                 overflow=torch.zeros(Bh, dtype=torch.int32, device=dev))
        prog.hold(hd, o)
        cand = (o['cand_score'].data_ptr(), o['cand_row'].data_ptr(), cap, o['counts'].data_ptr())
        nms = (float(net.nms_thresh), int(net.nms_topk), int(net.post_nms), o['ids'].data_ptr(), o['scores'].data_ptr(),
               o['bboxes'].data_ptr(), o['rows'].data_ptr(), o['overflow'].data_ptr(), 4 * Bh)
        if net.agnostic:
            prog.add('vd_yolo_decode_filter_agnostic', C.byref(hd), 0, 0.01, *cand)
            prog.add('vd_nms_agnostic', C.byref(hd), 0, *cand, *nms)
        else:
            prog.add('vd_yolo_decode_filter', C.byref(hd), 0.01, *cand)
            prog.add('vd_nms_topk', C.byref(hd), *cand, *nms)
        return o

    def add_nodes(self, prog, nodes, bufs, B, ring=None):
        """The records of `nodes` on B samples.  ring = (slot table [B][K] int32, S): the joins read their K frames from the
        ring of cached per-frame features `bufs['ring:' + source]` (detect_video, vd_stream.hip)."""
        self.prog, self.nodes, self.bufs, self.B, self.ring = prog, nodes, bufs, B, ring
        for n in nodes:
            getattr(self, self.NODE[type(n)])(n)

    # ------------------------------------------------------------------ leaves
    def amax(self, t):
        """fp32: the max-abs of tensor t, the operand scale of the fp16-split arithmetic of its readers"""
        if not self.bf16:
            self.prog.add('vd_amax', self.bufs[t].data_ptr(), self.bufs[t].numel(), self.bufs['amax:' + t].data_ptr())

    def amax_merge(self, a, b, dst):
        """fp32: the max-abs of dst as the larger of those of a and b (b None: a's)"""
        if not self.bf16:
            am = lambda t: None if t is None else self.bufs['amax:' + t].data_ptr()
            self.prog.add('vd_amax_merge', am(a), am(b), am(dst))

    def fp32_only(self, n):
        assert not self.bf16, "bf16 inference: %s %s has fp32 kernels only" % (type(n).__name__, n.name)

    def conv_desc(self, n, out, epilogue=True):
        """The conv record of node n into `out`, with its BatchNorm fold, LeakyReLU and residual (a head: its bias);
        epilogue=False (fp32): the raw conv."""
        net, bufs, B, H, W = self.net, self.bufs, self.B, self.H, self.W
        if not self.bf16:
            if n.head:
                d = net._conv_desc(n, bufs, B, H, W, out, shift=n.bias)
            elif not epilogue:
                d = net._conv_desc(n, bufs, B, H, W, out)
            else:
                d = net._conv_desc(n, bufs, B, H, W, out, scale=n.fold_scale, shift=n.fold_shift,
                                   residual=bufs[n.residual] if n.residual else None, leaky=True, amax_out=True)
            self.prog.hold(d)
            return d
        assert epilogue
        ci_p = self.cp(n.cin)
        co_p = n.co_pad if n.head else self.cp(n.cout)
        wb = torch.empty(co_p * n.T * ci_p, dtype=torch.bfloat16, device=net.device)
        self.packs.append((n, wb, co_p, ci_p))
        Ho, Wo = H // n.div_out, W // n.div_out
        d = ConvDesc()
        net._set_streamk(d, 0)
        d.in_, d.wp, d.out = bufs[n.src].data_ptr(), wb.data_ptr(), out.data_ptr()
        d.N, d.Hi, d.Wi, d.Ci = B * n.fr, H // n.div_in, W // n.div_in, ci_p
        d.Hg, d.Wg, d.in_stride = Ho, Wo, n.stride
        ops._set_taps(d, n.taps())
        d.Kfr, d.Ho, d.Wo, d.Co = (n.fr if n.kd > 1 else 1), Ho, Wo, co_p
        d.out_stride, d.out_oy, d.out_ox, d.slope = 1, 0, 0, LEAKY_SLOPE
        d.ldo = d.ldr = out.shape[-1]
        if n.head:
            d.flags, d.shift = EPI_AFFINE, n.bias.data_ptr()
        else:
            # padded fp32 fold vectors: one pair per NODE, shared by the plans of every input shape (a per-plan pair
            # would go stale in all plans but the one that last refreshed it)
            if getattr(n, 'bf_scale', None) is None or n.bf_scale.numel() != co_p:
                n.bf_scale, n.bf_shift = torch.zeros(co_p, device=net.device), torch.zeros(co_p, device=net.device)
            d.flags = EPI_AFFINE | EPI_LEAKY | (EPI_RESIDUAL if n.residual else 0)
            d.scale, d.shift = n.bf_scale.data_ptr(), n.bf_shift.data_ptr()
            if n.residual:
                d.residual = bufs[n.residual].data_ptr()
        self.prog.hold(d, wb)
        return d

    def add_conv(self, d, n, meta):
        if self.bf16:
            self.prog.add('vd_conv_igemm_bf16', C.byref(d), 1 if n.head else 0, meta=meta)
        else:
            self.prog.add('vd_conv_igemm', C.byref(d), meta=meta)

    # ------------------------------------------------------------------ per node type
    def upcat(self, n):
        bufs, o = self.bufs, self.bufs[n.dst]
        # a copy of 16-byte units: bf16 channels go as 4-byte words, two channels each
        self.prog.add('vd_upsample2x_concat', bufs[n.up].data_ptr(), bufs[n.route].data_ptr(), o.data_ptr(), self.B * n.fr,
                      o.shape[1], o.shape[2], self.cp(n.cu) // self.cw, self.cp(n.cr) // self.cw)
        self.amax_merge(n.up, n.route, n.dst)                   # a concatenation: max of the two

    def pool(self, n):
        prog, B, ring = self.prog, self.B, self.ring
        o, xs = self.bufs[n.dst], self.bufs[n.src if ring is None else 'ring:' + n.src]
        assert xs.shape[3] % (4 * self.cw) == 0, "join: C = %d must keep 16-byte units" % xs.shape[3]
        px, words = xs.shape[1] * xs.shape[2], xs.shape[3] // self.cw
        if ring is not None:
            slots, S = ring
            if n.type == 2:
                prog.add('vd_temporal_cat_idx', xs.data_ptr(), slots.data_ptr(), o.data_ptr(), S, B, n.K, px, words)
            else:
                prog.add('vd_temporal_pool_idx' + self.sfx, xs.data_ptr(), slots.data_ptr(), o.data_ptr(), S, B, n.K, o[0].numel(),
                         n.type, meta=dict(kind='pool_idx', bytes=float(self.esz) * o.numel() * (n.K + 1)))
            # the ring's frames went through the prefix in other launches: the operand scale is the join's own max-abs
            self.amax(n.dst)
            return
        if n.type == 2:                                         # stacking the K frames' channels: a copy
            prog.add('vd_temporal_cat', xs.data_ptr(), o.data_ptr(), B, n.K, px, words, 0)
        elif self.bf16:
            prog.add('vd_temporal_pool_bf16', xs.data_ptr(), o.data_ptr(), B, n.K, o[0].numel(), n.type)
        else:                                                   # (None: no record of the winning frame, training's)
            prog.add('vd_temporal_pool', xs.data_ptr(), o.data_ptr(), None, B, n.K, o[0].numel(), n.type)
        self.amax_merge(n.src, None, n.dst)                     # max / mean / stacking: bounded by the source's

    def corr(self, n):
        """(no max-abs record: the readers of a correlation join are range-exact, YOLOV3._build)"""
        xs = self.bufs[n.src]
        assert xs.shape[3] == n.C and self.bufs[n.dst].shape[3] == n.ldy
        self.prog.add('vd_corr_fwd' + self.sfx, xs.data_ptr(), self.bufs[n.dst].data_ptr(), self.B, n.K, xs.shape[1], xs.shape[2],
                      n.C, n.d, n.ldy, meta=self.net._corr_meta(n, self.B, xs, 'fwd'))

    def sel_add(self, n):
        self.net._add_sel_add_fwd(self.prog, n, self.bufs, self.B, bf16=self.bf16)

    def gru(self, n):
        self.fp32_only(n)
        self.net._add_gru_fwd(self.prog, n, self.bufs, self.B, self.H, self.W, False)

    def tdw(self, n):
        self.fp32_only(n)
        self.net._add_tdw_fwd(self.prog, n, self.bufs, self.B, self.H, self.W)

    def stem(self, n):
        net, prog, bufs = self.net, self.prog, self.bufs
        if self.bf16:
            # the stem and the stride-2 conv behind it as ONE launch (vd_stem_conv_c32_bf16: the stem's 32-channel map is
            # computed inside the first-stage patch kernel and never stored; same bits) where that conv is the stem's only
            # reader; VD_STEM_FUSED=0: two launches
            users = [m for m in self.nodes if n.dst in node_inputs(m)]
            u = users[0] if len(users) == 1 else None
            self.fuse_stem = None
            if (os.environ.get("VD_STEM_FUSED", "1") != "0" and isinstance(u, ConvNode) and u.src == n.dst and u.k == 3
                    and u.kd == 1 and u.stride == 2 and u.cin == 32 and u.cout == 64 and u.bn and not u.residual
                    and not getattr(u, 'tvalid', False)):
                self.fuse_stem = (n, u)
                return
        # fp32 master weights and BN fold on the fp32 VALU, output in the plan's storage (vd_stem.hip)
        net._add_stem(prog, n, bufs, self.B, self.H, self.W, bufs[n.dst], scale=n.fold_scale, shift=n.fold_shift, leaky=True,
                      bf16=self.bf16)
        self.amax(n.dst)

    def conv(self, n):
        if n.stem:
            return self.stem(n)
        net, prog, bufs, B, H, W = self.net, self.prog, self.bufs, self.B, self.H, self.W
        meta = net._flops(n, B, H, W, 'fwd')
        o = bufs[n.dst]
        if getattr(n, 'tvalid', False):
            # (3,1,1) conv without temporal padding = frames [1, K-1) of the 'same'-padded one: all frames go through the
            # conv, the valid ones are sliced out.  fp32 folds BatchNorm on those; bf16 has the (per-channel, batch-
            # independent) fold in the conv's epilogue
            if self.bf16 and ('zf:' + n.dst) not in bufs:
                bufs['zf:' + n.dst] = torch.zeros(B * n.fr, o.shape[1], o.shape[2], self.cp(n.cout), dtype=torch.bfloat16,
                                                  device=net.device)
            zf = bufs['zf:' + n.dst]
            valid = o if self.bf16 else bufs['zs:' + n.dst]
            self.add_conv(self.conv_desc(n, zf, epilogue=self.bf16), n, meta)
            prog.add('vd_frame_slice', zf.data_ptr(), valid.data_ptr(), B, n.fr, 1, n.fr - 2, zf[0].numel() // self.cw, 0)
            if not self.bf16:
                prog.add('vd_bn_apply_leaky', valid.data_ptr(), n.fold_scale.data_ptr(), n.fold_shift.data_ptr(), None,
                         o.data_ptr(), o.numel() // n.cout, n.cout, LEAKY_SLOPE, bufs['amax:' + n.dst].data_ptr())
            return
        d = self.conv_desc(n, o)
        if self.fuse_stem is not None and self.fuse_stem[1] is n:
            st = self.fuse_stem[0]
            meta['flops'] += net._flops(st, B, H, W, 'fwd')['flops']
            meta['fused_stem'] = True
            d.tile = 16
            prog.add('vd_stem_conv_c32_bf16', bufs['in'].data_ptr(), st.wp.data_ptr(), st.fold_scale.data_ptr(),
                     st.fold_shift.data_ptr(), LEAKY_SLOPE, C.byref(d), meta=meta)
            return
        self.add_conv(d, n, meta)
