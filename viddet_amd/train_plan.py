"""The builder of a training plan (YOLOV3._build_train): one object that holds the schedule state, one method per node type
and pass, and one copy of every block the passes share."""
import ctypes as C
import math
import os

import torch

from . import lib as L
from . import ops
from .consts import ANCHORS, STRIDES, BN_EPS, BN_MOMENTUM, LEAKY_SLOPE
from .lib import ConvDesc, WgradDesc, EPI_AFFINE, EPI_RESIDUAL
from .model import (Program, Slot, ConvNode, UpcatNode, PoolNode, CorrNode, GruNode, SelNode, AddNode, TdwNode,
                    autotune_desc, autotune_program, autotune_wgrad, autotune_wgrad_bf16, consumers_of, ev_record, ev_wait,
                    fp32_math, grad_required, _bf16_pitch, _TUNE_CACHE)
from .ops import dgrad_plans


class Switches:
    """The build-time A/B switches of the training plan, read from the environment when a plan is built (so a test can
    build both forms in one process)."""

    def __init__(self, env=os.environ):
        self.side_prio = int(env.get('VD_SIDE_PRIO', '0'))                   # priority of the weight-gradient side stream
        self.fuse_bwd_bf16 = env.get('VD_FUSE_BWD_BF16', '0') == '1'         # bf16 storage: BN-backward reductions in the data gradients
        self.s2_fused = env.get('VD_S2_FUSED', '1') == '1'                   # 3x3 / stride-2 data gradient as one PARITY4 launch
        self.s2_fused_max_cin = int(env.get('VD_S2_FUSED_MAX_CIN', '64'))    # ... up to this many input channels
        self.s2_chunk_mb = float(env.get('VD_S2_CHUNK_MB', '0'))             # frame chunks of a stride-2 data gradient (0 = off)
        # the four parity launches of a stride-2 data gradient on four streams (+1 % in same-box A/B)
        self.parity_streams = env.get('VD_PARITY_STREAMS', '1') == '1'
        self.fuse_bwd_s2 = env.get('VD_FUSE_BWD_S2', '1') == '1'             # fused BN-backward reductions in stride-2 data gradients
        self.autotune = env.get('VD_AUTOTUNE', '1') != '0'                   # (fused_s2: 'auto' arithmetic needs the autotuner)
        self.stem_fuse_bwd = stem_fuse_bwd(env)                              # stem dz computed inside its weight gradient


def stem_fuse_bwd(env=os.environ):
    """VD_STEM_FUSE_BWD (default 1): the stem's BatchNorm-backward apply pass runs inside its weight-gradient kernel
    (vd_stem_wgrad_bn) and its dz is never stored; also sizes the dz scratch (YOLOV3._buffers)"""
    return env.get('VD_STEM_FUSE_BWD', '1') == '1'


class TrainPlan:
    """The training plan of `net` at one shape: forward with the BatchNorm statistics, the loss, then the fixed reverse pass
    with the weight-gradient GEMMs on a side stream and the bucketed gradient all-reduce queued behind them.  The storage of
    the activations and their gradients (set_storage) changes the leaves of the schedule only: bf16 storage runs the `_bf16`
    twins of the elementwise kernels, has no max-abs slots (the fp16-split arithmetic is fp32's) and runs every
    convolution as vd_conv_igemm_bf16 on bf16 weight images (packed by _refresh_dgrad)."""

    FWD = {UpcatNode: 'fwd_upcat', PoolNode: 'fwd_pool', CorrNode: 'fwd_corr', SelNode: 'fwd_sel_add', AddNode: 'fwd_sel_add',
           GruNode: 'fwd_gru', TdwNode: 'fwd_tdw', ConvNode: 'fwd_conv'}
    BWD = {UpcatNode: 'bwd_upcat', PoolNode: 'bwd_pool', CorrNode: 'bwd_corr', SelNode: 'bwd_sel', AddNode: 'bwd_add',
           GruNode: 'bwd_gru', TdwNode: 'bwd_tdw', ConvNode: 'bwd_conv'}

    def __init__(self, net, B, H, W):
        self.net, self.B, self.H, self.W = net, B, H, W
        self.sw = Switches()
        bf16 = self.bf16 = getattr(net, 'storage', 'fp32') == 'bf16'
        self.sfx, self.esz = ('_bf16', 2) if bf16 else ('', 4)
        self.dt = torch.bfloat16 if bf16 else torch.float32
        self.cw = 2 if bf16 else 1                         # bf16: the copy kernels move 4-byte words, two channels each
        self.bufs = net._buffers('train', B, H, W, True, bf16=bf16)
        self.dev, self.lib = net.device, L.load()
        self.mtiles = self.lib.vd_conv_igemm_bf16_mtiles if bf16 else self.lib.vd_conv_igemm_mtiles
        self.size_workspaces()
        self.side = torch.cuda.Stream(priority=self.sw.side_prio) if net.overlap_wgrad else None
        self.seg = None                                    # the Program the pass in progress appends to

    # ------------------------------------------------------------------ leaves
    def amx(self, t):
        return self.bufs['amax:' + t].data_ptr()

    def amx_arg(self, t):
        """the fp32 kernels' trailing max-abs slots"""
        return () if self.bf16 else (None if t is None else self.amx(t),)

    def size_workspaces(self):
        net, bf16, lib, B, H, W = self.net, self.bf16, self.lib, self.B, self.H, self.W
        ws_bytes = 1 << 20
        for n in net.conv_nodes:
            Hi, Wi = H // n.div_in, W // n.div_in
            Ho, Wo = H // n.div_out, W // n.div_out
            if n.stem:
                ws_bytes = max(ws_bytes, int(lib.vd_stem_wgrad_ws_bytes(B * n.fr, Hi, Wi)))
            elif bf16:
                wd_ = WgradDesc()
                wd_.N, wd_.Hi, wd_.Wi, wd_.Ci, wd_.Hg, wd_.Wg, wd_.Co, wd_.ldd = B * n.fr, Hi, Wi, n.cin, Ho, Wo, n.co_pad, n.co_pad
                ops._set_taps(wd_, n.taps())
                for fl_ in (0, L.WGRAD_HALO):          # the halo-ring kernel picks its own split count
                    wd_.in_stride, wd_.Kfr, wd_.flags = n.stride, (n.fr if n.kd > 1 else 1), L.STORE_BF16 | L.MATH_BF16 | fl_
                    ws_bytes = max(ws_bytes, int(lib.vd_conv_wgrad_ws_bytes(C.byref(wd_))))
            else:
                ws_bytes = max(ws_bytes, ops.wgrad_ws_bytes(B * n.fr, Hi, Wi, n.cin, Ho, Wo, n.co_pad, n.k, n.stride,
                                                            n.pad, n.kd, n.pad_d))
            ws_bytes = max(ws_bytes, ops.bn_stats_ws_bytes(B * n.fr * Ho * Wo, _bf16_pitch(n.co_pad) if bf16 else n.co_pad))
        for n in net.tdw_nodes:
            ws_bytes = max(ws_bytes, int(lib.vd_tdw_bwd_ws_bytes(B, n.K, (H // n.div) * (W // n.div), n.C)))
        self.ws_bytes = ws_bytes
        self.ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.dev)
        self.world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.world = torch.distributed.get_world_size(net.process_group)
            # With SyncBN the statistics all-reduces sit on the critical path of backward; on one communicator they
            # would queue behind a gradient bucket in flight (one RCCL stream per communicator).  The buckets get
            # their own communicator (new_group is collective: every rank builds its training plan at the same point).
            if (self.world > 1 and net.syncbn_scope and net.bucketed_allreduce and net._bucket_group is None
                    and net.process_group is None):
                net._bucket_group = torch.distributed.new_group()
        # partial-sum table of the fused BN statistics: rows = M tiles (>= 64 rows each), 2*Cout floats per row
        smax = 16
        for n in net.conv_nodes:
            if n.bn:
                # (+ 8 rows: the four parity launches of a stride-2 data gradient round their tile counts up separately)
                # (+ 8 + 4 x 64 rows: every parity launch of every frame chunk rounds its tile count up separately)
                smax = max(smax, ((B * n.fr * (H // n.div_out) * (W // n.div_out) + 63) // 64 + 8 + 256) * 2 * n.cout)
        self.stats_ws = torch.empty(smax, device=self.dev)
        # bf16 storage: the forward weight images.  The conv weights live fwd-packed [co_pad][T * Ci] in the arena and need
        # no padding here (every Ci is 32 or a multiple of 64), so ONE conversion of the arena's weight range makes all of them
        self.wb_arena = torch.empty(net.n_weight, dtype=self.dt, device=self.dev) if bf16 else None

    def stats_rows_fit(self, rows, cout):
        assert rows * 2 * cout <= self.stats_ws.numel(), "stats workspace too small"

    def tune(self, d, of32=0):
        """fix the tile (and arithmetic) of a conv record, hence its number of M tiles"""
        if self.bf16:
            self.net._tune_bf16_desc(d, of32)
        else:
            autotune_desc(d)

    def add_conv(self, d, of32=0, **kw):
        if self.bf16:
            self.seg.add('vd_conv_igemm_bf16', C.byref(d), of32, **kw)
        else:
            self.seg.add('vd_conv_igemm', C.byref(d), **kw)

    def fwd_desc(self, n, out):
        """the forward conv record of node n into `out`"""
        net, bufs, B, H, W = self.net, self.bufs, self.B, self.H, self.W
        if not self.bf16:
            d = net._conv_desc(n, bufs, B, H, W, out, shift=n.bias if n.head else None)
            self.seg.hold(d)
            return d
        wb = self.wb_arena[n.w_off:n.w_off + n.w_numel]
        assert n.w_numel == n.co_pad * n.T * n.cin and n.w_off % 8 == 0
        Ho, Wo = H // n.div_out, W // n.div_out
        d = ConvDesc()
        net._set_streamk(d, 0)
        d.in_, d.wp, d.out = bufs[n.src].data_ptr(), wb.data_ptr(), out.data_ptr()
        d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.in_stride = B * n.fr, H // n.div_in, W // n.div_in, n.cin, Ho, Wo, n.stride
        ops._set_taps(d, n.taps())
        d.Kfr, d.Ho, d.Wo, d.Co = (n.fr if n.kd > 1 else 1), Ho, Wo, n.co_pad
        d.out_stride, d.out_oy, d.out_ox, d.slope = 1, 0, 0, LEAKY_SLOPE
        d.ldo = d.ldr = out.shape[-1]                  # (the head: its bf16 pitch)
        if n.head:
            d.flags, d.shift = EPI_AFFINE, n.bias.data_ptr()
        self.seg.hold(d, wb)
        return d

    # ------------------------------------------------------------------ the plan
    def build(self):
        net = self.net
        # ---- forward: list of segments; a segment is a Program or a python callable (collectives)
        self.seg = Program()
        if not self.bf16:
            net._add_input_stage(self.seg, self.bufs, self.B, self.H, self.W)
        for n in net.nodes:
            getattr(self, self.FWD[type(n)])(n)
        slots, losses = self.add_loss()
        fwd = [self.seg]
        self.seg = Program()
        self.begin_backward()
        for n in reversed(net.nodes):
            getattr(self, self.BWD[type(n)])(n)
        if self.side is not None and self.last_side is not None:
            self.seg.add_py(ev_wait(self.last_side))          # join: the optimiser / all-reduce see every gradient
        self.seg.hold(self.ws_w, self.side, self.stats_ws)
        bwd = [self.seg]
        for sg in fwd + bwd:
            if isinstance(sg, Program):
                autotune_program(sg)
        _TUNE_CACHE.save()
        return dict(fwd=fwd, bwd=bwd, bufs=self.bufs, slots=slots, losses=losses, dgrad_packs=self.dgrad_packs, ws=self.ws,
                    wb_arena=self.wb_arena, storage='bf16' if self.bf16 else 'fp32')

    # ------------------------------------------------------------------ forward, per node type
    def fwd_upcat(self, n):
        seg, bufs = self.seg, self.bufs
        o = bufs[n.dst]
        seg.add('vd_upsample2x_concat', bufs[n.up].data_ptr(), bufs[n.route].data_ptr(), o.data_ptr(), self.B * n.fr,
                o.shape[1], o.shape[2], n.cu // self.cw, n.cr // self.cw)
        if not self.bf16:
            seg.add('vd_amax_merge', self.amx(n.up), self.amx(n.route), self.amx(n.dst))

    def fwd_pool(self, n):
        seg, bufs, B, cw = self.seg, self.bufs, self.B, self.cw
        o, xs = bufs[n.dst], bufs[n.src]
        if n.type == 2:
            # a copy of 16-byte units: bf16 channels go as 4-byte words, two channels each
            assert xs.shape[3] % (4 * cw) == 0, "cat join: C = %d must keep 16-byte units" % xs.shape[3]
            seg.add('vd_temporal_cat', xs.data_ptr(), o.data_ptr(), B, n.K, xs.shape[1] * xs.shape[2], xs.shape[3] // cw, 0)
        else:
            am = bufs['am:' + n.dst].data_ptr() if n.type == 0 else None
            seg.add('vd_temporal_pool_train_bf16' if self.bf16 else 'vd_temporal_pool', xs.data_ptr(), o.data_ptr(), am, B, n.K,
                    o[0].numel(), n.type)
        if not self.bf16:
            seg.add('vd_amax_merge', self.amx(n.src), None, self.amx(n.dst))

    def fwd_corr(self, n):
        bufs = self.bufs
        xs = bufs[n.src]
        assert xs.shape[3] == n.C and bufs[n.dst].shape[3] == n.ldy
        self.seg.add('vd_corr_fwd' + self.sfx, xs.data_ptr(), bufs[n.dst].data_ptr(), self.B, n.K, xs.shape[1], xs.shape[2], n.C,
                     n.d, n.ldy, meta=self.net._corr_meta(n, self.B, xs, 'fwd', self.esz))

    def fwd_sel_add(self, n):
        if self.bf16:                                      # (they occur in the temporal_out / temporal_side nets only)
            raise NotImplementedError("bf16-storage training: node type %s" % type(n).__name__)
        self.net._add_sel_add_fwd(self.seg, n, self.bufs, self.B)

    def fwd_gru(self, n):
        self.net._add_gru_fwd(self.seg, n, self.bufs, self.B, self.H, self.W, True, self.side)

    def fwd_tdw(self, n):
        self.net._add_tdw_fwd(self.seg, n, self.bufs, self.B, self.H, self.W)

    def fwd_conv(self, n):
        net, seg, bufs, B, H, W = self.net, self.seg, self.bufs, self.B, self.H, self.W
        Ho, Wo = H // n.div_out, W // n.div_out
        tvalid = getattr(n, 'tvalid', False)
        M = B * (n.fr - 2 if tvalid else n.fr) * Ho * Wo
        meta = net._flops(n, B, H, W, 'fwd', self.esz)
        if n.head:
            d = self.fwd_desc(n, bufs[n.dst])
            if self.bf16:
                self.tune(d, 1)
            self.add_conv(d, 1, meta=meta)
            return
        z = bufs['z:' + n.dst]
        ws, ws_bytes, stats_ws = self.ws, self.ws_bytes, self.stats_ws
        table_rows = None                                  # rows of the partial-sum table; None: n.sums holds the sums
        if n.stem:
            # raw conv output + one row of BatchNorm partial sums per 256-pixel block (vd_stem.hip)
            table_rows = self.lib.vd_stem_conv_blocks(B * n.fr, H, W)
            self.stats_rows_fit(table_rows, n.cout)
            net._add_stem(seg, n, bufs, B, H, W, z, bf16=self.bf16, stats=stats_ws.data_ptr())
        elif tvalid:
            # 'same'-padded temporal conv on all frames, the valid ones sliced out, statistics over those
            zf = bufs['zf:' + n.dst]
            self.add_conv(self.fwd_desc(n, zf), meta=meta)
            seg.add('vd_frame_slice', zf.data_ptr(), z.data_ptr(), B, n.fr, 1, n.fr - 2, zf[0].numel(), 0)
            seg.add('vd_bn_stats', z.data_ptr(), M, n.cout, n.sums.data_ptr(), ws.data_ptr(), ws_bytes)
        elif self.bf16 or net.fuse_bn_stats:
            # BN statistics ride in the conv epilogue: one row of partial sums per M tile, reduced in fp64
            d = self.fwd_desc(n, z)
            d.stats_part = stats_ws.data_ptr()
            self.tune(d)
            table_rows = self.mtiles(C.byref(d))
            self.stats_rows_fit(table_rows, n.cout)
            self.add_conv(d, meta=meta)
        else:
            self.add_conv(self.fwd_desc(n, z), meta=meta)
            seg.add('vd_bn_stats', z.data_ptr(), M, n.cout, n.sums.data_ptr(), ws.data_ptr(), ws_bytes)
        count = float(M)
        fin = (n.gamma.data_ptr(), n.beta.data_ptr(), BN_EPS, BN_MOMENTUM, n.rmean.data_ptr(), n.rvar.data_ptr(),
               n.b_scale.data_ptr(), n.b_shift.data_ptr(), n.b_mean.data_ptr(), n.b_invstd.data_ptr())
        if table_rows is not None and not net._syncbn(n):
            # partial table -> fp64 sums -> scale / shift / running statistics in ONE launch (short tables)
            seg.add('vd_bn_sum_finalize', stats_ws.data_ptr(), table_rows, n.cout, n.sums.data_ptr(), count, *fin,
                    ws.data_ptr(), ws_bytes)
        else:
            if table_rows is not None:
                seg.add('vd_bn_sum_partials', stats_ws.data_ptr(), table_rows, n.cout, n.sums.data_ptr(), ws.data_ptr(),
                        ws_bytes)
            if net._syncbn(n):
                # SyncBN (train_yolov3.py:347-354): the fp64 [sum x, sum x^2] summed over the ranks, then one finalize
                # on the global count
                seg.add_coll(net._syncbn_exchange(n.sums))
                count = float(M * self.world)
            seg.add('vd_bn_finalize', n.sums.data_ptr(), count, n.cout, *fin)
        res = bufs[n.residual].data_ptr() if n.residual else None
        seg.add('vd_bn_apply_leaky' + self.sfx, z.data_ptr(), n.b_scale.data_ptr(), n.b_shift.data_ptr(), res,
                bufs[n.dst].data_ptr(), M, n.cout, LEAKY_SLOPE, *self.amx_arg(n.dst),
                meta=dict(node=n.name, bytes=float(self.esz) * M * n.cout * (3 if n.residual else 2),
                          single_conv_consumer=not self.bf16 and n.dst in net.single_conv_consumer_tensors()))

    def add_loss(self):
        """the loss records (targets are late-bound) -> (slots, losses)"""
        net, seg, bufs, bf16 = self.net, self.seg, self.bufs, self.bf16
        frames = self.B * net._head_frames
        grids = net._grid(self.H, self.W)
        hd = ops.make_head_desc([bufs[h] for h in net.head_names], grids, bufs[net.head_names[0]].shape[-1],
                                STRIDES[::-1], ANCHORS[::-1], frames, net.num_class)
        slots = dict(gt=Slot(), M=Slot(), obj=Slot(), ctr=Slot(), scl=Slot(), wgt=Slot(), cls=Slot(), smooth=Slot())
        losses = torch.zeros(frames, 4, device=self.dev)
        dh = (C.c_void_p * 3)(*[bufs['d:' + h].data_ptr() for h in net.head_names])
        head_node = {m.dst: m for m in net.conv_nodes if m.head}
        # (an rnn_pos='out' network has no prediction convs: nothing reads the loss gradient as a conv operand)
        dha = None if (bf16 or not head_node) else \
            (C.c_void_p * 3)(*[self.amx('dz:' + head_node[h].name) for h in net.head_names])   # max-abs of the three dhead
        lws = torch.empty(max(16, ops.yolo_loss_ws_bytes(hd)), dtype=torch.uint8, device=self.dev)
        seg.hold(hd, dh, dha, lws)
        seg.add('vd_yolo_loss_fwd_bwd' + self.sfx, C.byref(hd), slots['gt'], slots['M'], slots['obj'], slots['ctr'], slots['scl'],
                slots['wgt'], slots['cls'], float(net._ignore_iou_thresh), slots['smooth'], losses.data_ptr(),
                C.byref(dh), None, *([] if bf16 else [C.byref(dha) if dha is not None else None]), lws.data_ptr(), lws.numel())
        return slots, losses

    # ------------------------------------------------------------------ backward: schedule state and shared steps
    def begin_backward(self):
        """The weight-gradient GEMMs (MFMA-bound) run on a side stream beside the main-stream chain
        [BN backward (HBM-bound) -> data gradient]: nothing in the backward pass consumes a weight gradient,
        so the only edges are  dz ready -> wgrad  (event) and  wgrad done -> dz scratch reuse  (event; the dz
        scratch is double-buffered), plus one join before the optimiser.  Tails of one GEMM fill with the other."""
        net, bufs = self.net, self.bufs
        self.ws_w = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.dev) if self.side is not None else self.ws
        self.dz_bufs = [bufs['dz'], bufs['dz2']]
        self.dz_free = [None, None]        # event after which dz_bufs[i] may be overwritten
        self.n_dz = 0
        self.last_side = None
        self.bucket_hi, self.bucket_acc = net.n_wconv, 0     # (the temporal depthwise weights behind n_wconv: allreduce_grads)
        self.written = set(net.head_names)     # gradients already produced (the loss kernel wrote d:head*)
        self.dgrad_packs = []              # (node, plan, packed weight buffer) re-packed when weights change
        # d:x of a residual block input x is  dy_block (skip)  +  dgrad(first conv of the block).  The skip term is not
        # copied: it stays an alias of the block's dy until the dgrad, which reads it as its epilogue residual and
        # writes d:x out of place (saves a read + write of every block output per step).
        self.alias = {}
        # BatchNorm backward reductions (sum g, sum g*xhat over dy and z) ride in the epilogue of the data-gradient conv
        # that writes the FINAL dy of a BatchNorm output - the earliest forward consumer, processed last here - when
        # that conv is a single stride-1 launch; the standalone two-tensor reduction pass is then skipped.
        self.producers = {m.dst: m for m in net.conv_nodes if m.bn}
        self.consumers = consumers_of(net.nodes)
        self.fused_bwd = set()
        self.tgrad = grad_required(net.nodes, self.trainable, lambda t: t in net.input_tensors)
        wtrain = [m for m in net.conv_nodes if net._node_trainable(m)[0]]
        self.first_wtrain = wtrain[0] if wtrain else None       # its weight gradient is the last one backward produces

    def trainable(self, m):
        if isinstance(m, TdwNode):
            return self.net._params[m.pname].grad_req != 'null'
        return any(self.net._node_trainable(m))

    def copy_grad(self, src, dst):
        """dst = src (the identity form of the BatchNorm apply kernel)"""
        c = src.shape[-1]
        self.seg.add('vd_bn_apply_leaky' + self.sfx, src.data_ptr(), self.net._ones(c).data_ptr(), self.net._zeros(c).data_ptr(),
                     None, dst.data_ptr(), src.numel() // c, c, 1.0, *self.amx_arg(None))

    def materialize(self, name):
        if name in self.alias:
            self.copy_grad(self.alias.pop(name), self.bufs['d:' + name])

    def grad_into(self, name, can_alias=False):
        """Return (dst_ptr, accumulate?) for a producer of d:name."""
        if name in self.written:
            if not can_alias:
                self.materialize(name)
            return self.bufs['d:' + name], True
        self.written.add(name)
        return self.bufs['d:' + name], False

    def add_grad(self, dsrc, acc, launch):
        """launch(ptr) writes a gradient contribution to d:src: straight into dsrc, or into tmp then added to dsrc"""
        target = self.bufs['tmp'][:dsrc.numel()] if acc else dsrc
        launch(target.data_ptr())
        if acc:
            self.seg.add('vd_add' + self.sfx, dsrc.data_ptr(), target.data_ptr(), dsrc.data_ptr(), dsrc.numel())

    def incoming(self, n):
        """the finished gradient of node n's output"""
        assert n.dst in self.written, n.name
        self.materialize(n.dst)
        return self.bufs['d:' + n.dst]

    def skip_grad(self, n, dy):
        """the skip term of a residual block closed by node n (a conv cell or a temporal conv): the first producer of
        d:residual aliases dy (no copy, see alias), a later one adds dy"""
        if not (n.residual and self.tgrad[n.residual]):
            return
        dres, acc = self.grad_into(n.residual)
        if acc:
            self.seg.add('vd_add' + self.sfx, dres.data_ptr(), dy.data_ptr(), dres.data_ptr(), dy.numel())
        else:
            self.alias[n.residual] = dy
            if not self.net.alias_skip_grad:
                self.materialize(n.residual)

    def side_launch(self, *wargs, meta, label=None):
        """A weight-gradient launch (`wargs`: entry point and arguments up to the workspace) on the side stream, between
        an event pair: main records `ready`, the side stream waits for it, runs the launch on its own workspace and records
        `done`.  Returns `done` (None without a side stream: the launch is on the main stream)."""
        seg, side = self.seg, self.side
        if side is None:
            seg.add(*wargs, self.ws.data_ptr(), self.ws_bytes, meta=meta, label=label)
            return None
        e_ready, e_done = torch.cuda.Event(), torch.cuda.Event()
        seg.add_py(ev_record(e_ready))
        seg.add_py(ev_wait(e_ready, side))
        seg.add(*wargs, self.ws_w.data_ptr(), self.ws_bytes, meta=meta, stream=side, label=label)
        seg.add_py(ev_record(e_done, side))
        seg.hold(e_ready, e_done)
        self.last_side = e_done
        return e_done

    def close_bucket(self, cn, last):
        """Bucketed gradient all-reduce, overlapped with the rest of the backward pass: weight gradients complete
        in reverse arena order on the stream that runs the wgrad GEMMs, so every time a bucket (~32 MB) of the arena tail
        is final an async all-reduce of that contiguous range is queued behind them (RCCL syncs with that
        stream); allreduce_grads() later waits for the handles and reduces the small gamma/beta/bias range.
        `last`: cn's bucket closes whatever its size (the first trainable conv; the stem, the first conv, closes the arena)."""
        net = self.net
        self.bucket_acc += cn.w_numel
        if net.bucketed_allreduce and (self.bucket_acc >= net.bucket_elems or last):
            lo, hi = cn.w_off, self.bucket_hi
            self.seg.add_py(net._bucket_launcher(lo, hi, self.side))
            self.bucket_hi, self.bucket_acc = lo, 0

    def dgrad_desc(self, cn, src, Hd, Wd, Kd, N, wpk, plan, dst, res):
        """The fields every data-gradient record of conv cn shares: N frames of the incoming gradient at pointer `src`
        (Hd x Wd x Kd) through the packed weights `wpk` over the plan's grid and taps into cn's input map at pointer `dst`,
        plus the rows at `res` when that is not None.  The caller sets what differs: output stride and offsets, Kfr, a
        wider Co, `par_*`, more flags, the max-abs slots and the stream-K workspace."""
        d = ConvDesc()
        d.in_, d.wp, d.out = src, wpk.data_ptr(), dst
        d.N, d.Hi, d.Wi, d.Ci = N, Hd, Wd, Kd
        d.Hg, d.Wg, d.in_stride = plan['Hg'], plan['Wg'], 1
        ops._set_taps(d, plan['taps'])
        d.Kfr, d.Ho, d.Wo, d.Co = 1, self.H // cn.div_in, self.W // cn.div_in, cn.cin
        d.out_stride, d.out_oy, d.out_ox = 1, 0, 0
        d.ldo = d.ldr = cn.cin
        d.flags, d.slope = (EPI_RESIDUAL if res is not None else 0), LEAKY_SLOPE
        if res is not None:
            d.residual = res
        self.seg.hold(d, wpk)
        return d

    def fuse_bn_bwd(self, d, m, z_off, part_off):
        """the BatchNorm-backward reductions of node m in the epilogue of data-gradient record d"""
        d.bs_z = self.bufs['z:' + m.dst].data_ptr() + z_off
        d.bs_scale, d.bs_shift = m.b_scale.data_ptr(), m.b_shift.data_ptr()
        d.bs_mean, d.bs_invstd = m.b_mean.data_ptr(), m.b_invstd.data_ptr()
        d.bs_part, d.bs_slope = self.stats_ws.data_ptr() + part_off, LEAKY_SLOPE

    def fused_param_grads(self, m, rows):
        """close the fused reductions of node m: `rows` rows of the partial table -> sums, gamma / beta gradients"""
        self.seg.add('vd_bn_sum_param_grads', self.stats_ws.data_ptr(), rows, m.cout, m.sums2.data_ptr(),
                     m.ggamma.data_ptr(), m.gbeta.data_ptr(), self.ws.data_ptr(), self.ws_bytes)
        self.fused_bwd.add(m.name)

    # ------------------------------------------------------------------ backward, per node type
    def bwd_tdw(self, n):
        """backward of the temporal conv, in front of its spatial cell's BatchNorm backward: the skip gradient of a
        block is dy itself (alias, as for a 2-D block); ONE launch then writes dx = d:src and the weight
        gradient's partial rows, a second folds them (vd_tdw.hip).  dx is left out when nothing upstream needs a
        gradient, dw under grad_req 'null'.  It runs on the main stream: its dx is on the critical path and the
        weight gradient falls out of the same read of dy."""
        if not self.tgrad[n.dst]:
            return
        B = self.B
        dy = self.incoming(n)
        self.skip_grad(n, dy)
        t_train = self.trainable(n)
        dxp = None
        if self.tgrad[n.src]:
            dsrc, acc = self.grad_into(n.src)
            assert not acc, n.name           # the temporal conv is the only reader of its spatial cell
            dxp = dsrc.data_ptr()
        if dxp is not None or t_train:
            hw = (self.H // n.div) * (self.W // n.div)
            self.seg.add('vd_tdw_bwd', dy.data_ptr(), self.bufs[n.src].data_ptr(), n.w.data_ptr(), dxp,
                         n.gw.data_ptr() if t_train else None, B, n.K, hw, n.C, self.ws.data_ptr(), self.ws_bytes,
                         meta=dict(kind='tdw_bwd', node=n.name, flops=(12.0 if t_train else 6.0) * B * n.K * hw * n.C,
                                   bytes=4.0 * B * n.K * hw * n.C * (1 + (dxp is not None) + t_train)))

    def bwd_upcat(self, n):
        tgrad, seg = self.tgrad, self.seg
        if not tgrad[n.dst]:
            return
        dout = self.bufs['d:' + n.dst]
        dup_p = None                               # NULL = that half is not needed (frozen upstream)
        if tgrad[n.up]:
            dup, acc_u = self.grad_into(n.up)
            assert not acc_u
            dup_p = dup.data_ptr()
        launch = lambda p: seg.add('vd_upsample2x_concat_bwd' + self.sfx, dout.data_ptr(), dup_p, p, self.B * n.fr,
                                   dout.shape[1], dout.shape[2], n.cu, n.cr)
        if tgrad[n.route]:
            self.add_grad(*self.grad_into(n.route), launch)
        elif dup_p:
            launch(None)

    def bwd_sel(self, n):
        if not self.tgrad[n.src]:
            return
        dout = self.incoming(n)
        dsrc, acc = self.grad_into(n.src)
        self.add_grad(dsrc, acc, lambda p: self.seg.add('vd_frame_slice', dout.data_ptr(), p, self.B, n.K, n.k0, n.kc,
                                                        dsrc[0].numel(), 1))

    def bwd_add(self, n):
        if not self.tgrad[n.dst]:
            return
        dout = self.incoming(n)
        for t_ in (n.a, n.b):
            if not self.tgrad[t_]:
                continue
            dsrc, acc = self.grad_into(t_)
            if acc:
                self.seg.add('vd_add', dsrc.data_ptr(), dout.data_ptr(), dsrc.data_ptr(), dsrc.numel())
            else:
                self.copy_grad(dout, dsrc)

    def bwd_pool(self, n):
        if not self.tgrad[n.src]:
            return
        seg, B = self.seg, self.B
        dout = self.bufs['d:' + n.dst]
        assert n.dst in self.written, n.name
        dsrc, acc = self.grad_into(n.src)
        am = self.bufs['am:' + n.dst].data_ptr() if n.type == 0 else None
        if n.type == 2:
            launch = lambda p: seg.add('vd_temporal_cat', dout.data_ptr(), p, B, n.K, dsrc.shape[1] * dsrc.shape[2],
                                       dsrc.shape[3] // self.cw, 1)
        else:
            launch = lambda p: seg.add('vd_temporal_pool_bwd' + self.sfx, dout.data_ptr(), am, p, B, n.K, dout[0].numel(), n.type)
        self.add_grad(dsrc, acc, launch)

    def bwd_corr(self, n):
        if not self.tgrad[n.src]:
            return
        dout, xs = self.incoming(n), self.bufs[n.src]
        dsrc, acc = self.grad_into(n.src)
        # columns [Cc, ldy) of d:dst are never read (vd_corr.hip), and what writes them is an exact zero: the consumers'
        # pad weight rows are exact zeros in fp32, so in their bf16 images, so in the data gradient made from those
        self.add_grad(dsrc, acc, lambda p: self.seg.add(
            'vd_corr_bwd' + self.sfx, dout.data_ptr(), xs.data_ptr(), p, self.B, n.K, xs.shape[1], xs.shape[2], n.C, n.d, n.ldy,
            meta=self.net._corr_meta(n, self.B, xs, 'bwd', self.esz)))

    # ---- ConvGRU
    def gru_dgrad(self, cn, din, nfr, dout, acc, sidx, st, packs):
        """data gradient of a GRU conv over nfr frames: din [nfr, h, w, 3 chp] -> dout [nfr, h, w, cn.cin] (+= when acc)"""
        Hc, Wc = self.H // cn.div_in, self.W // cn.div_in
        if cn not in packs:
            plan = dgrad_plans(cn.k, cn.pad, 1, Hc, Wc)[0]
            wpk = torch.empty(cn.cin * len(plan['taps']) * cn.co_pad, device=self.dev)
            self.dgrad_packs.append((cn, plan, wpk))
            packs[cn] = (plan, wpk)
        plan, wpk = packs[cn]
        d = self.dgrad_desc(cn, din.data_ptr(), Hc, Wc, cn.co_pad, nfr, wpk, plan, dout.data_ptr(),
                            dout.data_ptr() if acc else None)
        d.out_oy, d.out_ox = plan['py'], plan['px']
        # gate gradients are saturated like the loss gradient: no max-abs slots, so autotune_program (end of the build)
        # can only choose the fp32 MFMA or the 3-way bf16 split for this record, never the fp16 split
        d.amax_in, d.amax_w = None, cn.wamax.data_ptr()
        self.net._set_streamk(d, sidx)
        self.seg.add('vd_conv_igemm', C.byref(d), meta=self.net._gru_meta(cn, nfr, self.H, self.W, 'dgrad'), stream=st)

    def gru_wgrad(self, cn, xin, dout, nfr, amax_in):
        """weight gradient of a GRU conv over nfr frames, on the side stream like every weight gradient"""
        Hc, Wc = self.H // cn.div_in, self.W // cn.div_in
        wd_ = WgradDesc()
        wd_.in_, wd_.dout, wd_.dwp = xin.data_ptr(), dout.data_ptr(), cn.gwp.data_ptr()
        wd_.N, wd_.Hi, wd_.Wi, wd_.Ci = nfr, Hc, Wc, cn.cin
        wd_.Hg, wd_.Wg, wd_.Co, wd_.ldd = Hc, Wc, cn.co_pad, cn.co_pad
        wd_.in_stride = 1
        ops._set_taps(wd_, cn.taps())
        wd_.Kfr, wd_.splits = 1, 0
        wd_.amax_in, wd_.amax_dout = amax_in, None
        autotune_wgrad(wd_, self.ws.data_ptr(), self.ws_bytes)
        self.seg.hold(wd_)
        self.side_launch('vd_conv_wgrad', C.byref(wd_), meta=self.net._gru_meta(cn, nfr, self.H, self.W, 'wgrad'))
        self.close_bucket(cn, cn is self.first_wtrain)

    def bwd_gru(self, g):
        """Backward through time of a GruNode: per direction, steps in reverse - gate backward (dI, dH in place, the
        state gradient scaled by z), then the h2h data gradient ADDED into that state gradient by its residual epilogue;
        the reverse direction's chain on the side stream.  Then, batched over time: one i2h data gradient and one i2h
        weight gradient per direction over the B*K frames, one h2h weight gradient over the B*(K-1) frames that had a
        state, and the bias gradients as column sums of dI / dH (the head bias's path)."""
        if not self.tgrad[g.dst]:
            return
        net, seg, bufs, B, side = self.net, self.seg, self.bufs, self.B, self.side
        dy = self.incoming(g)
        K, hw = g.K, (self.H // g.div) * (self.W // g.div)
        packs = {}
        if side is not None:
            e_dy, e_r = torch.cuda.Event(), torch.cuda.Event()
            seg.add_py(ev_record(e_dy))
            seg.add_py(ev_wait(e_dy, side))
            seg.hold(e_dy, e_r)
        for di, (cname, i2h, h2h) in reversed(list(enumerate(g.cells))):
            st = side if (side is not None and di == 1) else None
            sidx = 4 if st is not None else 0
            I, Hb, hs, dh = bufs[i2h.dst], bufs[h2h.dst], bufs[g.key(cname, 'h')], bufs[g.key(cname, 'dh')]
            for s_ in reversed(range(K)):
                t = s_ if di == 0 else K - 1 - s_
                Hs = Hb[s_ * B:(s_ + 1) * B]
                seg.add('vd_gru_gate_bwd', I.data_ptr(), Hs.data_ptr(), 1 if s_ > 0 else 0, h2h.bias.data_ptr(),
                        hs[(s_ - 1) * B:].data_ptr() if s_ > 0 else None, dy.data_ptr(), 0.5, dh.data_ptr(),
                        1 if s_ < K - 1 else 0, B, K, t, hw, g.chp,
                        meta=dict(kind='gru_gate_bwd', node=g.name, flops=30.0 * B * hw * g.chp,
                                  bytes=4.0 * B * hw * g.chp * (16 if s_ > 0 else 11)), stream=st)
                if s_ > 0:
                    self.gru_dgrad(h2h, Hs, B, dh, True, sidx, st, packs)
            if st is not None:
                seg.add_py(ev_record(e_r, side))
        if side is not None:
            seg.add_py(ev_wait(e_r))
        if self.tgrad[g.src]:
            dsrc, acc = self.grad_into(g.src)
            for di, (cname, i2h, h2h) in enumerate(g.cells):
                self.gru_dgrad(i2h, bufs[i2h.dst], B * K, dsrc, acc or di > 0, 0, None, packs)
        for cname, i2h, h2h in g.cells:
            for cn in (i2h, h2h):
                if net._node_trainable(cn)[1]:
                    dz_ = bufs[cn.dst]
                    seg.add('vd_bn_stats', dz_.data_ptr(), B * K * hw, cn.co_pad, cn.sums.data_ptr(), self.ws.data_ptr(),
                            self.ws_bytes)
                    seg.add('vd_bn_param_grads', cn.sums.data_ptr(), cn.co_pad, bufs['tmp'].data_ptr(), cn.gbias.data_ptr())
        for cname, i2h, h2h in reversed(g.cells):                # reverse arena order (the gradient buckets)
            hs, Hb = bufs[g.key(cname, 'h')], bufs[h2h.dst]
            if net._node_trainable(h2h)[0]:
                self.gru_wgrad(h2h, hs, Hb[B:], B * (K - 1), None)
            if net._node_trainable(i2h)[0]:
                self.gru_wgrad(i2h, bufs[g.src], bufs[i2h.dst], B * K, net._amax_or_none(bufs, g.src))

    # ---- convolution cells
    def bwd_conv(self, n):
        if not self.tgrad[n.dst]:
            return                         # frozen, and nothing trainable upstream: no gradient is needed here
        net = self.net
        w_train, v_train = net._node_trainable(n)
        dy = self.incoming(n)
        if n.head:
            dz, slot = self.head_bias_grad(n, dy), None
        else:
            self.skip_grad(n, dy)
            dz, slot = self.bn_backward(n, dy)
        if w_train:
            self.conv_wgrad(n, dz, slot)
        if n.stem or n.src in net.input_tensors or not self.tgrad[n.src]:     # no gradient flows into the network inputs,
            return                                                             # nor below the last trainable parameter
        self.conv_dgrad(n, dz)

    def out_rows(self, n):
        """rows (frames x pixels) of node n's BatchNorm input"""
        frames = n.fr - 2 if getattr(n, 'tvalid', False) else n.fr
        return self.B * frames * (self.H // n.div_out) * (self.W // n.div_out)

    def head_bias_grad(self, n, dz):
        """bias gradient = per-channel sum of dz over its row pitch (reuses the BN column-sum kernels); the dgamma
        slot of the parameter-gradient kernel is scratch.  Returns dz, the loss gradient itself."""
        sums = n.sums
        if self.bf16:                  # (the bf16 pitch may be wider than n.sums)
            if getattr(n, 'sums_b', None) is None or n.sums_b.numel() != 2 * dz.shape[-1]:
                n.sums_b = torch.zeros(2 * dz.shape[-1], dtype=torch.float64, device=self.dev)
            sums = n.sums_b
        self.seg.add('vd_bn_stats' + self.sfx, dz.data_ptr(), self.out_rows(n), dz.shape[-1], sums.data_ptr(),
                     self.ws.data_ptr(), self.ws_bytes)
        self.seg.add('vd_bn_param_grads', sums.data_ptr(), n.co_pad, self.bufs['tmp'].data_ptr(), n.gbias.data_ptr())
        return dz

    def stem_fused(self, n):
        """the stem cell whose apply pass is left to its weight-gradient kernel (VD_STEM_FUSE_BWD; a `tvalid` stem keeps
        the stored dz: its frame slice reads it)"""
        return self.sw.stem_fuse_bwd and n.stem and n.bn and not getattr(n, 'tvalid', False)

    def bn_backward(self, n, dy):
        """BatchNorm (+ LeakyReLU) backward of conv cell n: reduce, SyncBN exchange, apply into one of the two dz scratch
        buffers, frame slice.  Returns (dz, its scratch slot); (None, None) for the fused stem."""
        seg, bufs, sfx, M = self.seg, self.bufs, self.sfx, self.out_rows(n)
        z = bufs['z:' + n.dst]
        bn = (n.b_scale.data_ptr(), n.b_shift.data_ptr(), n.b_mean.data_ptr(), n.b_invstd.data_ptr())
        if n.name not in self.fused_bwd:      # (fused: sums and gamma / beta gradients came with the table reduction)
            seg.add('vd_bn_bwd_reduce' + sfx, z.data_ptr(), dy.data_ptr(), *bn, M, n.cout, LEAKY_SLOPE, n.sums2.data_ptr(),
                    self.ws.data_ptr(), self.ws_bytes)
            seg.add('vd_bn_param_grads', n.sums2.data_ptr(), n.cout, n.ggamma.data_ptr(), n.gbeta.data_ptr())
        count = float(M)
        if self.net._syncbn(n):          # [sum g, sum g xhat] over the ranks (the local gamma / beta gradients came first)
            seg.add_coll(self.net._syncbn_exchange(n.sums2))
            count = float(M * self.world)
        if self.stem_fused(n):
            # dz has one consumer, the stem's weight gradient (no gradient flows into the frames), which computes it from z
            # and dy itself (conv_wgrad): no apply pass, no dz, no scratch slot.  With the stem weight frozen nothing reads it.
            self.stem_bn = (z, dy, bn, count)
            return None, None
        slot = self.n_dz % 2
        self.n_dz += 1
        assert M * n.cout <= self.dz_bufs[slot].numel(), "dz scratch too small for " + n.name
        dz = self.dz_bufs[slot][:M * n.cout].view(-1, self.H // n.div_out, self.W // n.div_out, n.cout)
        if self.side is not None and self.dz_free[slot] is not None:
            seg.add_py(ev_wait(self.dz_free[slot]))           # the wgrad that read this scratch has finished
        seg.add('vd_bn_bwd_apply' + sfx, z.data_ptr(), dy.data_ptr(), *bn, n.sums2.data_ptr(), count, M, n.cout, LEAKY_SLOPE,
                dz.data_ptr(), *self.amx_arg('dz:' + n.name))
        if getattr(n, 'tvalid', False):
            # the gradient of the frame slice: dz of the valid frames, zeros on the two border frames; the conv's
            # weight / data gradients then are those of the 'same'-padded conv
            dzf = bufs['dzf:' + n.dst]
            seg.add('vd_frame_slice', dz.data_ptr(), dzf.data_ptr(), self.B, n.fr, 1, n.fr - 2, dzf[0].numel(), 1)
            dz = dzf
        return dz, slot

    def conv_wgrad(self, n, dz, slot):
        """weight gradient straight into the gradient arena (same fwd-packed layout as the weights)"""
        net, bufs, B, H, W = self.net, self.bufs, self.B, self.H, self.W
        Hi, Wi = H // n.div_in, W // n.div_in
        label = None
        if n.stem and dz is None:
            # the fused stem (bn_backward): dz computed per element from z and dy inside the kernel; the `ready` event of
            # side_launch follows the reductions and the SyncBN exchange of sums2 on the main stream.  Listed under the
            # family name of the weight gradient it replaces.
            z, dy, bn, count = self.stem_bn
            label = 'vd_stem_wgrad' + self.sfx
            wargs = ('vd_stem_wgrad_bn' + self.sfx, bufs['in'].data_ptr(), z.data_ptr(), z.shape[-1], dy.data_ptr(), dy.shape[-1],
                     *bn, n.sums2.data_ptr(), count, LEAKY_SLOPE, n.gwp.data_ptr(), B * n.fr, Hi, Wi)
        elif n.stem:
            # both operands straight from global memory: the NCHW batch and dz (vd_stem.hip)
            wargs = ('vd_stem_wgrad' + self.sfx, bufs['in'].data_ptr(), dz.data_ptr(), n.co_pad, n.gwp.data_ptr(),
                     B * n.fr, Hi, Wi)
        else:
            wd_ = WgradDesc()
            wd_.in_, wd_.dout, wd_.dwp = bufs[n.src].data_ptr(), dz.data_ptr(), n.gwp.data_ptr()
            wd_.N, wd_.Hi, wd_.Wi, wd_.Ci = B * n.fr, Hi, Wi, n.ci_eff
            wd_.Hg, wd_.Wg, wd_.Co, wd_.ldd = H // n.div_out, W // n.div_out, n.co_pad, dz.shape[-1]
            wd_.in_stride = n.stride
            ops._set_taps(wd_, n.taps())
            wd_.Kfr, wd_.splits = (n.fr if n.kd > 1 else 1), 0
            if self.bf16:
                wd_.flags = L.STORE_BF16 | L.MATH_BF16
                autotune_wgrad_bf16(wd_, self.ws.data_ptr(), self.ws_bytes)
            else:
                wd_.amax_in, wd_.amax_dout = net._amax_or_none(bufs, n.src), net._amax_or_none(bufs, 'dz:' + n.name)
                autotune_wgrad(wd_, self.ws.data_ptr(), self.ws_bytes)
            self.seg.hold(wd_)
            wargs = ('vd_conv_wgrad', C.byref(wd_))
        meta = net._flops(n, B, H, W, 'wgrad', self.esz)
        if label is not None:
            meta['bytes'] += float(self.esz) * self.stem_bn[0].numel()       # the fused stem reads z and dy where it read dz
        e_done = self.side_launch(*wargs, meta=meta, label=label)
        if e_done is not None and slot is not None:
            self.dz_free[slot] = e_done
        self.close_bucket(n, n is self.first_wtrain or n.stem)

    def conv_dgrad(self, n, dz):
        """data gradient of conv cell n into d:src"""
        net, H, W = self.net, self.H, self.W
        dsrc, acc = self.grad_into(n.src, can_alias=True)
        res_src = self.alias.pop(n.src) if n.src in self.alias else dsrc      # the skip gradient, still living in the block's dy
        res = res_src if acc else None
        plans = dgrad_plans(n.k, n.pad, n.stride, H // n.div_in, W // n.div_in, n.kd, n.pad_d)
        pm = self.producers.get(n.src)
        # the producer's BatchNorm-backward reductions ride in this data gradient's epilogue when it is the launch (or, for a
        # stride-2 conv, the four parity launches) that completes dy of the producer's output.  (bf16 storage: off by
        # default, VD_FUSE_BWD_BF16=1: measured on one box, 416 / batch 64, 1992 frames/s with the stand-alone reduction
        # passes against 1958 fused - the HBM-bound pass runs beside the side stream's MFMA-bound weight gradients, the
        # fused epilogue lengthens the data gradients on the critical path)
        fuse_m = pm if (pm is not None and self.consumers[n.src][0] is n and
                        (self.sw.fuse_bwd_bf16 if self.bf16 else
                         net.fuse_bn_bwd and (len(plans) == 1 or (n.kd == 1 and self.sw.fuse_bwd_s2)) and pm.fr == n.fr)) else None
        if self.fused_s2(n, plans):
            self.dgrad_parity4(n, dz, dsrc, res, fuse_m)
        else:
            self.dgrad_parity_loop(n, dz, dsrc, res, fuse_m, plans)

    def fused_s2(self, n, plans):
        """Whether a 3x3 / stride-2 data gradient runs as ONE launch (VD_CONV_PARITY4, vd_conv_par.hip) instead of four parity
        launches that each gather and stage the whole dz: rows = positions of dz's grid, columns = (parity class,
        channel), taps = the four offsets of a 2x2 window, zero (offset, class) weight blocks skipped.
        VD_S2_FUSED=0 keeps the four launches (also: odd maps, other arithmetics, range-exact operands, pinned kernels)."""
        Hi, Wi = self.H // n.div_in, self.W // n.div_in
        return (not self.bf16 and len(plans) == 4 and n.k == 3 and n.stride == 2 and n.pad == 1 and n.kd == 1 and
                Hi % 2 == 0 and Wi % 2 == 0 and self.sw.s2_fused and n.cin % 32 == 0 and
                # (measured per layer, batch 64 / 416x416, four launches -> one: 32 channels 1.51 -> 1.12 ms, 64: 0.80 ->
                # 0.80, 128: 0.55 -> 0.66, 256: 0.53 -> 0.59, 512: 0.47 -> 0.53 - the one launch stages all sixteen
                # (offset, class) weight blocks for nine useful ones, which only pays where a parity launch has too few
                # output channels to fill a tile; VD_S2_FUSED_MAX_CIN moves the limit)
                n.cin <= self.sw.s2_fused_max_cin and
                self.net._amax_or_none(self.bufs, 'dz:' + n.name) is not None and
                (fp32_math() == 'split2' or (fp32_math() == 'auto' and self.sw.autotune)))

    def dgrad_parity4(self, n, dz, dsrc, res, fuse_m):
        """the one-launch form of a 3x3 / stride-2 data gradient (fused_s2)"""
        net, seg, B, H, W = self.net, self.seg, self.B, self.H, self.W
        Ho, Wo = H // n.div_out, W // n.div_out
        wp4 = torch.empty(16 * n.cin * n.co_pad, device=self.dev)
        self.dgrad_packs.append((n, dict(fused_s2=True), wp4))
        d = self.dgrad_desc(n, dz.data_ptr(), Ho, Wo, n.co_pad, B * n.fr, wp4, dict(Hg=Ho, Wg=Wo, taps=ops.PARITY4_TAPS),
                            dsrc.data_ptr(), None if res is None else res.data_ptr())
        d.Co, d.out_stride = 4 * n.cin, 2
        d.par_cin, d.par_mask = n.cin, ops.PARITY4_MASK   # (offset, class) blocks that hold a kernel tap
        d.flags |= L.MATH_F16X2 | L.CONV_PARITY4
        d.amax_in, d.amax_w = net._amax_or_none(self.bufs, 'dz:' + n.name), n.wamax.data_ptr()
        if fuse_m is not None:
            self.fuse_bn_bwd(d, fuse_m, 0, 0)
        autotune_desc(d)                                   # fixes the tile, hence the rows of the partial table
        if fuse_m is not None:
            mt = self.lib.vd_conv_igemm_mtiles(C.byref(d))
            self.stats_rows_fit(mt, fuse_m.cout)
            seg.add('vd_fill', self.stats_ws.data_ptr(), 0.0, mt * 2 * fuse_m.cout)     # column tiles narrower than Cin fill part of a row
        seg.add('vd_conv_igemm', C.byref(d), meta=dict(
            kind='dgrad', node=n.name, k=n.k, stride=n.stride, fused_s2=True,
            flops=2.0 * n.cin * n.cout * 9 * Ho * Wo * B * n.fr, bytes=net._flops(n, B, H, W, 'dgrad')['bytes']))
        if fuse_m is not None:
            self.fused_param_grads(fuse_m, mt)

    def frame_chunks(self, n, plans, NF):
        """Frame chunks of a stride-2 data gradient (VD_S2_CHUNK_MB > 0; default 0 = one launch per parity class): each of
        the four parity launches streams the WHOLE incoming gradient dz - 709 MB at 208 x 208 x 64 channels, batch 64 - and
        is HBM-bound on it (isolated: 5.9 TB/s on the one-tap class).  Cut into chunks of frames whose dz fits the 256 MB
        Infinity Cache beside the outputs, the second to fourth class of a chunk find dz there: one HBM read instead of four.
        Returns (frames per chunk, chunks)."""
        nchunks = 1
        # (measured, same box, batch 64 / 416x416: off 1022.0 frames/s, 192 MB 1021.9, 96 MB 1018.6, 48 MB 991.5 - the
        # four launches already share most of dz through the L2s / Infinity Cache when they run side by side on their
        # four streams; the default stays off, the switch and its parity test stay as the record of the experiment)
        chunk_mb = self.sw.s2_chunk_mb
        if not self.bf16 and len(plans) == 4 and n.kd == 1 and chunk_mb > 0:
            dz_mb = 4.0 * NF * (self.H // n.div_out) * (self.W // n.div_out) * n.co_pad / 1e6
            nchunks = max(1, min(NF, int(math.ceil(dz_mb / chunk_mb))))
        fchunk = (NF + nchunks - 1) // nchunks
        return fchunk, (NF + fchunk - 1) // fchunk

    def fork_parity(self):
        """the main stream's position as an event the three parity streams wait for; returns the streams"""
        net, seg = self.net, self.seg
        if getattr(net, '_par_streams', None) is None:
            net._par_streams = [torch.cuda.Stream() for _ in range(3)]
        e_fork = torch.cuda.Event()
        seg.add_py(ev_record(e_fork))
        for st in net._par_streams:
            seg.add_py(ev_wait(e_fork, st))
        return net._par_streams

    def dgrad_parity_loop(self, n, dz, dsrc, res, fuse_m, plans):
        """a data gradient as one launch per parity class of its stride (one class at stride 1) and frame chunk"""
        net, seg, bf16, esz, B, H, W = self.net, self.seg, self.bf16, self.esz, self.B, self.H, self.W
        Hi, Wi = H // n.div_in, W // n.div_in
        Ho, Wo = H // n.div_out, W // n.div_out
        NF = B * n.fr
        fchunk, nchunks = self.frame_chunks(n, plans, NF)
        kp = dz.shape[-1]                                   # K dimension of the data gradient (the bf16 head: its pitch)
        wpks = []
        for plan in plans:
            assert plan['taps'], "a parity class without taps would leave its gradient unwritten"
            wpk = torch.empty(n.cin * len(plan['taps']) * kp, dtype=self.dt, device=self.dev)
            self.dgrad_packs.append((n, plan, wpk))
            wpks.append(wpk)
        in_img, out_img = Ho * Wo * kp * esz, Hi * Wi * n.cin * esz        # bytes per frame of dz / of d:src
        nplans = n.stride * n.stride
        bs_rows = 0
        for ch in range(nchunks):
            f0 = ch * fchunk
            fn_ = min(NF, f0 + fchunk) - f0
            # the four parity launches of a stride-2 data gradient write disjoint pixels and read the same dz: run them
            # side by side on their own streams (VD_PARITY_STREAMS=1) so that they share dz in the L2s and fill each other's tails
            par = None
            if not bf16 and self.sw.parity_streams and len(plans) == 4 and net.overlap_wgrad:
                par = self.fork_parity()
            for pi, plan in enumerate(plans):
                d = self.dgrad_desc(n, dz.data_ptr() + f0 * in_img, Ho, Wo, kp, fn_, wpks[pi], plan,
                                    dsrc.data_ptr() + f0 * out_img, None if res is None else res.data_ptr() + f0 * out_img)
                d.Kfr = n.fr if n.kd > 1 else 1
                d.out_stride, d.out_oy, d.out_ox = n.stride, plan['py'], plan['px']
                if not bf16:
                    d.amax_in, d.amax_w = net._amax_or_none(self.bufs, 'dz:' + n.name), n.wamax.data_ptr()
                net._set_streamk(d, pi if (par is not None) else 0)
                if fuse_m is not None:
                    self.fuse_bn_bwd(d, fuse_m, f0 * out_img, bs_rows * 2 * fuse_m.cout * 4)
                if bf16 or fuse_m is not None:
                    self.tune(d)
                if fuse_m is not None:
                    bs_rows += self.mtiles(C.byref(d))
                    self.stats_rows_fit(bs_rows, fuse_m.cout)
                self.add_conv(d, meta=dict(
                    kind='dgrad', node=n.name, k=n.k, stride=n.stride,
                    flops=2.0 * n.cin * n.cout * len(plan['taps']) * plan['Hg'] * plan['Wg'] * fn_,
                    bytes=net._flops(n, B, H, W, 'dgrad', esz)['bytes'] / nplans * fn_ / NF),
                    stream=(par[pi - 1] if (par is not None and pi > 0) else None))
            if par is not None:
                for st in par:                                  # join before anything reads d:src or the partial table
                    e_join = torch.cuda.Event()
                    seg.add_py(ev_record(e_join, st))
                    seg.add_py(ev_wait(e_join))
        if fuse_m is not None:
            self.fused_param_grads(fuse_m, bs_rows)
