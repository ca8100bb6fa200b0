"""Thin operator layer over the C-ABI: builds descriptors (tap lists, geometry) for torch tensors
used as device storage and launches the HIP kernels on torch's current stream.

No arithmetic happens in Python/torch here; every function ends in a `lib.vd_*` call.
Reference call sites are cited in include/viddet_hip.h next to each entry point.
"""
import ctypes as C

import torch

from . import lib as L
from .lib import (ConvDesc, WgradDesc, HeadDesc, EPI_AFFINE, EPI_LEAKY, EPI_RESIDUAL, MATH_SPLIT, MATH_BF16, MATH_F16X2,
                  MATH_NOHALO, AMAX_FLOATS, check, ptr)


def round_up(v, m):
    return (v + m - 1) // m * m


def _lib():
    return L.load()


def _s():
    return L.stream_ptr()


# --------------------------------------------------------------------------------------------
# tap lists
# --------------------------------------------------------------------------------------------
def fwd_taps(k, pad, kd=1, pad_d=0):
    """Taps of a (kd,k,k) kernel in OI[D]HW order t = (kz*k + ky)*k + kx."""
    taps = []
    for kz in range(kd):
        for ky in range(k):
            for kx in range(k):
                taps.append((ky - pad, kx - pad, kz - pad_d))
    return taps


def dgrad_plans(k, pad, stride, Hi, Wi, kd=1, pad_d=0):
    """Data-gradient launches of a conv with kernel (kd,k,k), spatial `stride`, temporal stride 1.

    Returns a list of plans; each plan = dict(py, px, Hg, Wg, taps=[(dy,dx,dz)], tap_ids=[t]) meaning:
    dX[n, q_y*stride+py, q_x*stride+px, :] = sum_j dZ[n, q_y+dy_j, q_x+dx_j, frame+dz_j, :] . W[:, :, tap_ids[j]]
    """
    plans = []
    for py in range(stride):
        for px in range(stride):
            Hg = (Hi - py + stride - 1) // stride
            Wg = (Wi - px + stride - 1) // stride
            if Hg <= 0 or Wg <= 0:
                continue
            taps, ids = [], []
            for kz in range(kd):
                for ky in range(k):
                    if (py + pad - ky) % stride:
                        continue
                    for kx in range(k):
                        if (px + pad - kx) % stride:
                            continue
                        taps.append(((py + pad - ky) // stride, (px + pad - kx) // stride, pad_d - kz))
                        ids.append((kz * k + ky) * k + kx)
            plans.append(dict(py=py, px=px, Hg=Hg, Wg=Wg, taps=taps, tap_ids=ids))
    return plans


def _set_taps(d, taps):
    d.T = len(taps)
    for i, (dy, dx, dz) in enumerate(taps):
        d.dy[i], d.dx[i], d.dz[i] = dy, dx, dz


# --------------------------------------------------------------------------------------------
# convolution
# --------------------------------------------------------------------------------------------
def conv_igemm(x, wp, out, *, N, Hi, Wi, Ci, Hg, Wg, in_stride, taps, Ho, Wo, Co, ldo,
               out_stride=1, out_oy=0, out_ox=0, scale=None, shift=None, residual=None, ldr=0,
               leaky=False, slope=0.1, kfr=1, in_scale=None, in_shift=None, in_slope=0.1, tile=0, split=False,
               amax_in=None, amax_w=None, amax_out=None, streamk_ws=None, desc_out=None):
    """streamk_ws: a workspace from streamk_workspace() - the launch runs as a persistent stream-K grid where that form
    applies (VD_CONV_STREAMK; bit-identical results).
    split: False = fp32 MFMA; True / 'split' = exact 3-plane bf16 split; 'bf16' = one plane (bf16-rounded operands);
    'f16x2' = two fp16 planes with per-tensor scales - the max-abs slots of x and wp (amax_in / amax_w, see amax())
    are computed here when not given."""
    d = ConvDesc()
    d.tile = tile
    d.in_, d.wp, d.out = ptr(x), ptr(wp), ptr(out)
    d.scale, d.shift, d.residual = ptr(scale), ptr(shift), ptr(residual)
    d.N, d.Hi, d.Wi, d.Ci = N, Hi, Wi, Ci
    d.Hg, d.Wg, d.in_stride = Hg, Wg, in_stride
    _set_taps(d, taps)
    d.Kfr = kfr
    d.Ho, d.Wo, d.Co = Ho, Wo, Co
    d.out_stride, d.out_oy, d.out_ox = out_stride, out_oy, out_ox
    d.ldo, d.ldr = ldo, ldr
    flags = 0
    if scale is not None or shift is not None:
        flags |= EPI_AFFINE
    if leaky:
        flags |= EPI_LEAKY
    if residual is not None:
        flags |= EPI_RESIDUAL
    if split in ('f16x2', 'f16x2nh'):           # 'f16x2nh': without the halo-staged loop of the 3x3 stride-1 convs
        flags |= MATH_F16X2 | (MATH_NOHALO if split == 'f16x2nh' else 0)
        amax_in = amax(x) if amax_in is None else amax_in
        amax_w = amax(wp) if amax_w is None else amax_w
        d.amax_in, d.amax_w = ptr(amax_in), ptr(amax_w)
    elif split:
        flags |= MATH_BF16 if split == 'bf16' else MATH_SPLIT
    d.amax_out = ptr(amax_out)
    if streamk_ws is not None:
        flags |= L.CONV_STREAMK
        d.sk_ws, d.sk_ws_bytes = ptr(streamk_ws), streamk_ws.numel() * streamk_ws.element_size()
    d.flags, d.slope = flags, slope
    d.in_scale, d.in_shift, d.in_slope = ptr(in_scale), ptr(in_shift), in_slope
    if desc_out is not None:
        desc_out.append(d)
    check(_lib().vd_conv_igemm(C.byref(d), _s()), "vd_conv_igemm")


def streamk_workspace(device=None):
    """A stream-K hand-off workspace (vd_conv_desc.sk_ws): its counter header zeroed once, here; one per stream that may
    run such launches at the same time."""
    n = int(_lib().vd_conv_igemm_streamk_ws_bytes())
    ws = torch.empty(n, dtype=torch.uint8, device=device or torch.device("cuda", torch.cuda.current_device()))
    ws[:L.SK_HEADER_BYTES].zero_()
    return ws


def conv_fwd(x, wp, out, *, k, stride, pad, Co, ldo=None, scale=None, shift=None, residual=None,
             leaky=False, slope=0.1, kd=1, pad_d=0, kfr=1, tile=0, split=False, amax_in=None, amax_w=None,
             amax_out=None, in_scale=None, in_shift=None, in_slope=0.1, streamk_ws=None, desc_out=None):
    """Forward conv on NHWC x [N,Hi,Wi,Ci] with fwd-packed weights wp [>=Co][T*Ci] -> out [N,Ho,Wo,ldo].
    in_scale / in_shift: per-input-channel transform leaky(x * s + b) applied in the operand gather (the padding stays zero)."""
    N, Hi, Wi, Ci = x.shape
    Ho = (Hi + 2 * pad - k) // stride + 1
    Wo = (Wi + 2 * pad - k) // stride + 1
    ldo = Co if ldo is None else ldo
    conv_igemm(x, wp, out, N=N, Hi=Hi, Wi=Wi, Ci=Ci, Hg=Ho, Wg=Wo, in_stride=stride,
               taps=fwd_taps(k, pad, kd, pad_d), Ho=Ho, Wo=Wo, Co=Co, ldo=ldo, scale=scale, shift=shift,
               residual=residual, ldr=ldo, leaky=leaky, slope=slope, kfr=kfr, tile=tile, split=split,
               amax_in=amax_in, amax_w=amax_w, amax_out=amax_out, in_scale=in_scale, in_shift=in_shift, in_slope=in_slope,
               streamk_ws=streamk_ws, desc_out=desc_out)
    return Ho, Wo


def conv_igemm_bf16(x, wb, out, *, N, Hi, Wi, Ci, Hg, Wg, in_stride, taps, Ho, Wo, Co, ldo, out_stride=1, out_oy=0, out_ox=0,
                    scale=None, shift=None, residual=None, ldr=0, leaky=False, slope=0.1, kfr=1, tile=0, stats_part=None, nohalo=False,
                    streamk_ws=None, splitk=False):
    """vd_conv_igemm_bf16: x / wb / residual bf16, out bf16 or fp32 (by its dtype); any output geometry; stats_part =
    fused BatchNorm statistics table [mtiles][2 * Co] (conv_bf16_mtiles).  streamk_ws: VD_CONV_STREAMK (bit-identical);
    splitk=True with it: VD_CONV_SPLITK too (launches with too few tiles for the chip are cut along K).  kfr: frames per
    window of a conv with frame taps (dz != 0); a tap that leaves its window reads zeros."""
    d = ConvDesc()
    d.tile = tile
    d.in_, d.wp, d.out = ptr(x), ptr(wb), ptr(out)
    d.scale, d.shift, d.residual = ptr(scale), ptr(shift), ptr(residual)
    d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.in_stride = N, Hi, Wi, Ci, Hg, Wg, in_stride
    _set_taps(d, taps)
    d.Kfr, d.Ho, d.Wo, d.Co = kfr, Ho, Wo, Co
    d.out_stride, d.out_oy, d.out_ox, d.ldo, d.ldr = out_stride, out_oy, out_ox, ldo, ldr
    d.flags = (EPI_AFFINE if (scale is not None or shift is not None) else 0) | (EPI_LEAKY if leaky else 0) | \
              (EPI_RESIDUAL if residual is not None else 0) | (MATH_NOHALO if nohalo else 0)
    d.slope, d.stats_part = slope, ptr(stats_part)
    if streamk_ws is not None:
        d.flags |= L.CONV_STREAMK | (L.CONV_SPLITK if splitk else 0)
        d.sk_ws, d.sk_ws_bytes = ptr(streamk_ws), streamk_ws.numel() * streamk_ws.element_size()
    check(_lib().vd_conv_igemm_bf16(C.byref(d), 1 if out.dtype == torch.float32 else 0, _s()), "vd_conv_igemm_bf16")
    return d


def conv_bf16_mtiles(N, Hg, Wg, Ci, Co, tile=0):
    d = ConvDesc()
    d.N, d.Hg, d.Wg, d.Ci, d.Co, d.tile = N, Hg, Wg, Ci, Co, tile
    return _lib().vd_conv_igemm_bf16_mtiles(C.byref(d))


def pack_weight_bf16(wp32, wb, *, Co, Co_pad, Ci, Ci_pad, T):
    """fp32 packed [>=Co][T*Ci] -> bf16 [Co_pad][T*Ci_pad] (zero-padded rows / channels)."""
    check(_lib().vd_pack_weight_bf16(ptr(wp32), ptr(wb), Co, Co_pad, Ci, Ci_pad, T, _s()), "vd_pack_weight_bf16")


def conv_wgrad(x, dout, dwp, ws, *, k, stride, pad, Co, kd=1, pad_d=0, kfr=1, splits=0, split=False, amax_in=None,
               amax_dout=None, in_scale=None, in_shift=None, in_slope=0.1):
    """dwp [Co][T*Ci] (fwd-packed layout) = wgrad(x [N,Hi,Wi,Ci], dout [N,Ho,Wo,Co])."""
    N, Hi, Wi, Ci = x.shape
    _, Ho, Wo, ldd = dout.shape
    d = WgradDesc()
    d.in_, d.dout, d.dwp = ptr(x), ptr(dout), ptr(dwp)
    d.N, d.Hi, d.Wi, d.Ci = N, Hi, Wi, Ci
    d.Hg, d.Wg, d.Co, d.ldd = Ho, Wo, Co, ldd
    d.in_stride = stride
    _set_taps(d, fwd_taps(k, pad, kd, pad_d))
    d.Kfr, d.splits = kfr, splits
    d.in_scale, d.in_shift, d.in_slope = ptr(in_scale), ptr(in_shift), in_slope
    if split in ('f16x2', 'f16x2nh', 'f16x2h'):
        d.flags = MATH_F16X2 | (L.WGRAD_HALO if split == 'f16x2h' else 0)     # 'f16x2h': the halo-ring kernel where it applies
        amax_in = amax(x) if amax_in is None else amax_in
        amax_dout = amax(dout) if amax_dout is None else amax_dout
        d.amax_in, d.amax_dout = ptr(amax_in), ptr(amax_dout)
    else:
        d.flags = (MATH_BF16 if split == 'bf16' else MATH_SPLIT) if split else 0
    if x.dtype == torch.bfloat16:               # bf16-storage training: both operands bf16, the gradient fp32
        assert dout.dtype == torch.bfloat16 and dwp.dtype == torch.float32
        assert Ci % 8 == 0 and Co % 8 == 0 and ldd % 8 == 0 and x.data_ptr() % 16 == 0 and dout.data_ptr() % 16 == 0, \
            "bf16-stored operands: Ci, Co and the gradient pitch multiples of 8, 16-byte aligned tensors"
        d.flags = L.STORE_BF16 | MATH_BF16 | (L.WGRAD_HALO if split == 'halo' else 0)
    lib = _lib()
    need = lib.vd_conv_wgrad_ws_bytes(C.byref(d))
    if need > ws.numel() * ws.element_size():
        raise L.VidDetHipError("conv_wgrad: workspace %d < %d bytes" % (ws.numel() * ws.element_size(), need))
    check(lib.vd_conv_wgrad(C.byref(d), ptr(ws), ws.numel() * ws.element_size(), _s()), "vd_conv_wgrad")


def wgrad_ws_bytes(N, Hi, Wi, Ci, Ho, Wo, Co, k, stride, pad, kd=1, pad_d=0):
    d = WgradDesc()
    d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.Co, d.ldd = N, Hi, Wi, Ci, Ho, Wo, Co, Co
    d.in_stride = stride
    _set_taps(d, fwd_taps(k, pad, kd, pad_d))
    d.Kfr, d.splits = 1, 0
    need = 0
    # the product arithmetics pick different split counts (every split form: the same); the halo-ring kernel its own.  The
    # library only looks at shapes and flags here, so a non-null placeholder stands for the max-abs pointers of MATH_F16X2
    for fl in (0, MATH_SPLIT, MATH_F16X2 | L.WGRAD_HALO, L.STORE_BF16 | L.WGRAD_HALO):
        d.flags = fl
        d.amax_in = d.amax_dout = 1 if fl & MATH_F16X2 else None
        need = max(need, _lib().vd_conv_wgrad_ws_bytes(C.byref(d)))
    return need


def pack_weight_fwd(w_oihw, wp, Co_pad):
    Co, Ci = w_oihw.shape[0], w_oihw.shape[1]
    if w_oihw.dim() == 4:
        kd, kh, kw = 1, w_oihw.shape[2], w_oihw.shape[3]
    else:
        kd, kh, kw = w_oihw.shape[2:]
    check(_lib().vd_pack_weight_fwd(ptr(w_oihw), ptr(wp), Co, Co_pad, Ci, kd, kh, kw, _s()), "vd_pack_weight_fwd")


def pack_weight_dgrad(w, wp, *, Co, Co_pad, Ci, kd, kh, kw, tap_ids, src_packed):
    arr = (C.c_int32 * len(tap_ids))(*tap_ids)
    check(_lib().vd_pack_weight_dgrad(ptr(w), ptr(wp), Co, Co_pad, Ci, kd, kh, kw, arr, len(tap_ids),
                                      1 if src_packed else 0, _s()), "vd_pack_weight_dgrad")


PARITY4_TAPS = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0)]


def _parity4_mask():
    """bit (4 * offset + class) set where a 3x3 / stride-2 / pad-1 kernel has a tap for output parity class c = 2 py + px at
    gradient offset o = 2 dy + dx (vd_conv_par.hip par_tap: parity 0 -> k = 1 at offset 0; parity 1 -> k = 2 at 0, k = 0 at 1)"""
    tap = lambda parity, off: (1 if off == 0 else -1) if parity == 0 else (2 if off == 0 else 0)
    m = 0
    for o in range(4):
        for c in range(4):
            if tap(c >> 1, o >> 1) >= 0 and tap(c & 1, o & 1) >= 0:
                m |= 1 << (4 * o + c)
    return m


PARITY4_MASK = _parity4_mask()          # 0x8caf: nine of the sixteen blocks


def pack_weight_dgrad_s2(wp_fwd, wp4, *, Co, Co_pad, Ci):
    """weight image of the parity-fused stride-2 data gradient (VD_CONV_PARITY4): fwd-packed [Co][9 * Ci] ->
    [4 * Ci][4 * Co_pad]; returns the 16-bit mask of its nonzero (offset, class) blocks"""
    m = C.c_int32(0)
    check(_lib().vd_pack_weight_dgrad_s2(ptr(wp_fwd), ptr(wp4), Co, Co_pad, Ci, C.byref(m), _s()), "vd_pack_weight_dgrad_s2")
    return int(m.value)


def conv_dgrad_s2_fused(dz, wp4, dx, *, Cin, par_mask, residual=None, tile=0, amax_in=None, amax_w=None, desc_out=None):
    """dx [N, 2 Ho, 2 Wo, Cin] = data gradient of a 3x3 / stride-2 / pad-1 conv from dz [N, Ho, Wo, Cout] in ONE launch"""
    N, Ho, Wo, Cout = dz.shape
    d = ConvDesc()
    d.tile = tile
    d.in_, d.wp, d.out, d.residual = ptr(dz), ptr(wp4), ptr(dx), ptr(residual)
    d.N, d.Hi, d.Wi, d.Ci, d.Hg, d.Wg, d.in_stride = N, Ho, Wo, Cout, Ho, Wo, 1
    _set_taps(d, PARITY4_TAPS)
    d.Kfr, d.Ho, d.Wo, d.Co = 1, 2 * Ho, 2 * Wo, 4 * Cin
    d.out_stride, d.out_oy, d.out_ox, d.ldo, d.ldr = 2, 0, 0, dx.shape[-1], dx.shape[-1]
    d.flags = MATH_F16X2 | L.CONV_PARITY4 | (EPI_RESIDUAL if residual is not None else 0)
    d.par_cin, d.par_mask, d.slope = Cin, par_mask, 0.1
    amax_in = amax(dz) if amax_in is None else amax_in
    amax_w = amax(wp4) if amax_w is None else amax_w
    d.amax_in, d.amax_w = ptr(amax_in), ptr(amax_w)
    if desc_out is not None:
        desc_out.append((d, amax_in, amax_w))
    check(_lib().vd_conv_igemm(C.byref(d), _s()), "vd_conv_igemm/parity4")


def unpack_weight(wp, w_oihw):
    """fwd-packed [>=Co][T*Ci] -> OIHW (also used for gradients)."""
    Co, Ci = w_oihw.shape[0], w_oihw.shape[1]
    if w_oihw.dim() == 4:
        kd, kh, kw = 1, w_oihw.shape[2], w_oihw.shape[3]
    else:
        kd, kh, kw = w_oihw.shape[2:]
    check(_lib().vd_unpack_wgrad(ptr(wp), ptr(w_oihw), Co, Ci, kd, kh, kw, _s()), "vd_unpack_wgrad")


def stem_im2col(x, col, nchw):
    if nchw:
        N, _, H, W = x.shape
    else:
        N, H, W, _ = x.shape
    check(_lib().vd_stem_im2col(ptr(x), ptr(col), N, H, W, 1 if nchw else 0, _s()), "vd_stem_im2col")


# --------------------------------------------------------------------------------------------
# batch norm
# --------------------------------------------------------------------------------------------
def stem_conv(x_nchw, wp, out, *, scale=None, shift=None, leaky=False, slope=0.1, stats_part=None):
    """Direct stem conv (3x3, 3->32) from the NCHW fp32 batch; out NHWC fp32 or bf16 [N,H,W,32]."""
    N, _, H, W = x_nchw.shape
    flags = (EPI_AFFINE if scale is not None else 0) | (EPI_LEAKY if leaky else 0)
    check(_lib().vd_stem_conv(ptr(x_nchw), ptr(wp), ptr(out), out.shape[-1], N, H, W, ptr(scale), ptr(shift), slope, flags,
                              1 if out.dtype == torch.bfloat16 else 0, ptr(stats_part), _s()), "vd_stem_conv")


def stem_wgrad(x_nchw, dz, dwp, ws):
    """Weight gradient of the stem: dwp [32][32] fwd-packed from x (N,3,H,W) and dz [N,H,W,ldd]."""
    N, _, H, W = x_nchw.shape
    fn = _lib().vd_stem_wgrad_bf16 if dz.dtype == torch.bfloat16 else _lib().vd_stem_wgrad
    check(fn(ptr(x_nchw), ptr(dz), dz.shape[-1], ptr(dwp), N, H, W, ptr(ws), ws.numel() * ws.element_size(), _s()), "vd_stem_wgrad")


def stem_wgrad_bn(x_nchw, z, dy, scale, shift, smean, sinv, sums2, count, dwp, ws, slope=0.1):
    """The stem's weight gradient with dz = BatchNorm (+ LeakyReLU) backward of (z, dy) computed inside the kernel; z and dy
    [N,H,W,ld] with their own row pitches (ld = shape[-1] of the tensor passed; channels 0..31 are read)."""
    N, _, H, W = x_nchw.shape
    fn = _lib().vd_stem_wgrad_bn_bf16 if z.dtype == torch.bfloat16 else _lib().vd_stem_wgrad_bn
    check(fn(ptr(x_nchw), ptr(z), z.shape[-1], ptr(dy), dy.shape[-1], ptr(scale), ptr(shift), ptr(smean), ptr(sinv), ptr(sums2),
             float(count), slope, ptr(dwp), N, H, W, ptr(ws), ws.numel() * ws.element_size(), _s()), "vd_stem_wgrad_bn")


def bn_stats(x2d_rows, C_, x, sums, ws):
    fn = _lib().vd_bn_stats_bf16 if x.dtype == torch.bfloat16 else _lib().vd_bn_stats
    check(fn(ptr(x), x2d_rows, C_, ptr(sums), ptr(ws), ws.numel() * ws.element_size(), _s()), "vd_bn_stats")


def bn_stats_ws_bytes(M, C_):
    return _lib().vd_bn_stats_ws_bytes(M, C_)


def bn_finalize(sums, count, C_, gamma, beta, eps, momentum, rmean, rvar, scale, shift, smean, sinv):
    check(_lib().vd_bn_finalize(ptr(sums), float(count), C_, ptr(gamma), ptr(beta), eps, momentum, ptr(rmean),
                                ptr(rvar), ptr(scale), ptr(shift), ptr(smean), ptr(sinv), _s()), "vd_bn_finalize")


def _nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def bn_sum_partials_ws_bytes(nblk, C_):
    return int(_lib().vd_bn_sum_partials_ws_bytes(nblk, C_))


def bn_sum_partials(part, nblk, C_, sums, ws=None):
    check(_lib().vd_bn_sum_partials(ptr(part), nblk, C_, ptr(sums), ptr(ws), _nbytes(ws), _s()), "vd_bn_sum_partials")


def bn_sum_finalize(part, nblk, C_, sums, count, gamma, beta, eps, momentum, rmean, rvar, scale, shift, smean, sinv, ws=None):
    """vd_bn_sum_partials + vd_bn_finalize of a partial table part[nblk][2C] (one launch up to 1024 rows; ws beyond)"""
    check(_lib().vd_bn_sum_finalize(ptr(part), nblk, C_, ptr(sums), float(count), ptr(gamma), ptr(beta), eps, momentum,
                                    ptr(rmean), ptr(rvar), ptr(scale), ptr(shift), ptr(smean), ptr(sinv), ptr(ws), _nbytes(ws),
                                    _s()), "vd_bn_sum_finalize")


def bn_sum_param_grads(part, nblk, C_, sums2, dgamma, dbeta, ws=None):
    """vd_bn_sum_partials + vd_bn_param_grads of a partial table part[nblk][2C]"""
    check(_lib().vd_bn_sum_param_grads(ptr(part), nblk, C_, ptr(sums2), ptr(dgamma), ptr(dbeta), ptr(ws), _nbytes(ws), _s()),
          "vd_bn_sum_param_grads")


def bn_fold_eval(gamma, beta, rmean, rvar, eps, scale, shift):
    check(_lib().vd_bn_fold_eval(ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), eps, gamma.numel(), ptr(scale),
                                 ptr(shift), _s()), "vd_bn_fold_eval")


def bn_apply_leaky(x, scale, shift, residual, y, M, C_, slope=0.1, amax_out=None):
    if x.dtype == torch.bfloat16:
        check(_lib().vd_bn_apply_leaky_bf16(ptr(x), ptr(scale), ptr(shift), ptr(residual), ptr(y), M, C_, slope, _s()),
              "vd_bn_apply_leaky_bf16")
        return
    check(_lib().vd_bn_apply_leaky(ptr(x), ptr(scale), ptr(shift), ptr(residual), ptr(y), M, C_, slope, ptr(amax_out),
                                   _s()), "vd_bn_apply_leaky")


def bn_bwd_reduce(x, dy, scale, shift, smean, sinv, M, C_, sums2, ws, slope=0.1):
    if x.dtype == torch.bfloat16:
        check(_lib().vd_bn_bwd_reduce_bf16(ptr(x), ptr(dy), ptr(scale), ptr(shift), ptr(smean), ptr(sinv), M, C_, slope,
                                           ptr(sums2), ptr(ws), ws.numel() * ws.element_size(), _s()), "vd_bn_bwd_reduce_bf16")
        return
    check(_lib().vd_bn_bwd_reduce(ptr(x), ptr(dy), ptr(scale), ptr(shift), ptr(smean), ptr(sinv), M, C_, slope,
                                  ptr(sums2), ptr(ws), ws.numel() * ws.element_size(), _s()), "vd_bn_bwd_reduce")


def bn_param_grads(sums2, C_, dgamma, dbeta):
    check(_lib().vd_bn_param_grads(ptr(sums2), C_, ptr(dgamma), ptr(dbeta), _s()), "vd_bn_param_grads")


def bn_bwd_apply(x, dy, scale, shift, smean, sinv, sums2, count, M, C_, dx, slope=0.1, amax_out=None):
    if x.dtype == torch.bfloat16:
        check(_lib().vd_bn_bwd_apply_bf16(ptr(x), ptr(dy), ptr(scale), ptr(shift), ptr(smean), ptr(sinv), ptr(sums2),
                                          float(count), M, C_, slope, ptr(dx), _s()), "vd_bn_bwd_apply_bf16")
        return
    check(_lib().vd_bn_bwd_apply(ptr(x), ptr(dy), ptr(scale), ptr(shift), ptr(smean), ptr(sinv), ptr(sums2),
                                 float(count), M, C_, slope, ptr(dx), ptr(amax_out), _s()), "vd_bn_bwd_apply")


# --------------------------------------------------------------------------------------------
# pointwise
# --------------------------------------------------------------------------------------------
def amax(x, out=None):
    """Max-abs slots (AMAX_FLOATS floats) of a tensor: the operand-scale input of the VD_MATH_F16X2 arithmetic."""
    out = torch.empty(AMAX_FLOATS, device=x.device) if out is None else out
    check(_lib().vd_amax(ptr(x), x.numel(), ptr(out), _s()), "vd_amax")
    return out


def amax_value(slots):
    """The tensor's max-abs as a Python float (tests / diagnostics; synchronises)."""
    return float(slots.view(-1)[::L.AMAX_STRIDE][:L.AMAX_SLOTS].max())


def add(a, b, out):
    if out.dtype == torch.bfloat16:
        check(_lib().vd_add_bf16(ptr(a), ptr(b), ptr(out), out.numel(), _s()), "vd_add_bf16")
        return
    check(_lib().vd_add(ptr(a), ptr(b), ptr(out), out.numel(), _s()), "vd_add")


def fill(t, v):
    check(_lib().vd_fill(ptr(t), float(v), t.numel(), _s()), "vd_fill")


def upsample2x_concat(up, route, out):
    N, Ho, Wo, Cr = route.shape
    Cu = up.shape[3]
    if out.dtype == torch.bfloat16:             # a copy: two bf16 = one 4-byte word
        Cu, Cr = Cu // 2, Cr // 2
    check(_lib().vd_upsample2x_concat(ptr(up), ptr(route), ptr(out), N, Ho, Wo, Cu, Cr, _s()), "vd_upsample2x_concat")


def upsample2x_concat_bwd(dout, dup, droute):
    N, Ho, Wo, Cr = droute.shape
    Cu = dup.shape[3]
    if dout.dtype == torch.bfloat16:
        check(_lib().vd_upsample2x_concat_bwd_bf16(ptr(dout), ptr(dup), ptr(droute), N, Ho, Wo, Cu, Cr, _s()),
              "vd_upsample2x_concat_bwd_bf16")
        return
    check(_lib().vd_upsample2x_concat_bwd(ptr(dout), ptr(dup), ptr(droute), N, Ho, Wo, Cu, Cr, _s()),
          "vd_upsample2x_concat_bwd")


def nchw_to_nhwc(x, out):
    N, Cc, H, W = x.shape
    check(_lib().vd_nchw_to_nhwc(ptr(x), ptr(out), N, Cc, H, W, _s()), "vd_nchw_to_nhwc")


def preprocess_u8(x_u8, out):
    check(_lib().vd_preprocess_u8_nhwc(ptr(x_u8), ptr(out), x_u8.numel() // 3, _s()), "vd_preprocess_u8_nhwc")


def augment_u8_nchw(raw, src_off, src_hw, color, idx_y, w_y, Ty, idx_x, w_x, Tx, fill, out, N, K, H, W):
    """vd_augment_u8_nchw; every array argument is a device tensor (the sections of viddet_amd.augment's packed upload)"""
    check(_lib().vd_augment_u8_nchw(ptr(raw), ptr(src_off), ptr(src_hw), ptr(color), ptr(idx_y), ptr(w_y), Ty, ptr(idx_x), ptr(w_x),
                                    Tx, ptr(fill), ptr(out), N, K, H, W, _s()), "vd_augment_u8_nchw")


def yolo_targets(gt, ids, idw, mix, N, M, C, H, W, obj, ctr, scl, wgt, cls):
    """vd_yolo_targets: gt (N,M,4), ids (N,M,idw) and mix (N,M) or None are device tensors (fp32); the five outputs are written
    whole (they may be uninitialised)"""
    check(_lib().vd_yolo_targets(ptr(gt), ptr(ids), idw, ptr(mix), N, M, C, H, W, ptr(obj), ptr(ctr), ptr(scl), ptr(wgt),
                                 ptr(cls), _s()), "vd_yolo_targets")


def voc_match(det_ids, det_scores, det_boxes, gt, clip_hi, iou_thresh, rec_cls, rec_score, rec_hit, npos, ndiff=None):
    """vd_voc_match: det_ids (B,N[,1]), det_scores (B,N[,1]), det_boxes (B,N,4) and gt (B,M,5|6) are contiguous fp32 device
    tensors; rec_cls (B,N) int32, rec_score (B,N) fp32 and rec_hit (B,N) int8 are written whole (they may be uninitialised);
    npos (C,) and ndiff (C,) or None are int32 and accumulated.  clip_hi < 0: the detections are not clipped."""
    if det_boxes.dim() != 3 or det_boxes.shape[-1] != 4:
        raise ValueError("voc_match: det_boxes must be (B,N,4), got %r" % (tuple(det_boxes.shape),))
    B, N = int(det_boxes.shape[0]), int(det_boxes.shape[1])
    if gt.dim() != 3 or gt.shape[-1] not in (5, 6):
        raise ValueError("voc_match: gt must be (B,M,5|6) [x1, y1, x2, y2, id(, difficult)], got %r" % (tuple(gt.shape),))
    M, gt_w = int(gt.shape[1]), int(gt.shape[2])
    if N > L.VOC_MATCH_MAX_DET:
        raise ValueError("voc_match: N=%d detections per image, vd_voc_match takes at most %d" % (N, L.VOC_MATCH_MAX_DET))
    if M > L.VOC_MATCH_MAX_GT:
        raise ValueError("voc_match: M=%d label rows per image, vd_voc_match takes at most %d" % (M, L.VOC_MATCH_MAX_GT))
    if int(gt.shape[0]) != B:
        raise ValueError("voc_match: gt holds %d images, det_boxes %d" % (int(gt.shape[0]), B))
    for name, t, n, dt in (("det_ids", det_ids, B * N, torch.float32), ("det_scores", det_scores, B * N, torch.float32),
                           ("det_boxes", det_boxes, B * N * 4, torch.float32), ("gt", gt, B * M * gt_w, torch.float32),
                           ("rec_cls", rec_cls, B * N, torch.int32), ("rec_score", rec_score, B * N, torch.float32),
                           ("rec_hit", rec_hit, B * N, torch.int8), ("npos", npos, npos.numel(), torch.int32),
                           ("ndiff", ndiff, npos.numel(), torch.int32)):
        if t is None and name == "ndiff":
            continue
        if t.dtype != dt or t.numel() != n or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("voc_match: %s must be a contiguous %s device tensor of %d elements, got %s %r"
                             % (name, dt, n, t.dtype, tuple(t.shape)))
    check(_lib().vd_voc_match(ptr(det_ids), ptr(det_scores), ptr(det_boxes), B, N, ptr(gt), M, gt_w, float(clip_hi),
                              float(iou_thresh), ptr(rec_cls), ptr(rec_score), ptr(rec_hit), ptr(npos), ptr(ndiff),
                              int(npos.numel()), _s()), "vd_voc_match")


def vid_match(det, gt, motion_ranges, area_ranges, iou_thresh, pixel_tolerance, rec_gt, rec_tp, rec_fp, img_nig, img_ngt, npos,
              nout):
    """vd_vid_match: det (B,N,6) [label, score, x1, y1, x2, y2], gt (B,M,6) [x1, y1, x2, y2, label, motion_iou], motion_ranges
    (4,2) and area_ranges (4,2) are contiguous fp64 device tensors; rec_gt / rec_tp / rec_fp (B,N), img_nig (B,4) and img_ngt
    (B,) are int32 and written whole (they may be uninitialised); npos (C,) and nout (16,C) are int32 and accumulated."""
    if det.dim() != 3 or det.shape[-1] != 6:
        raise ValueError("vid_match: det must be (B,N,6) [label, score, x1, y1, x2, y2], got %r" % (tuple(det.shape),))
    if gt.dim() != 3 or gt.shape[-1] != 6:
        raise ValueError("vid_match: gt must be (B,M,6) [x1, y1, x2, y2, label, motion_iou], got %r" % (tuple(gt.shape),))
    B, N, M, C = int(det.shape[0]), int(det.shape[1]), int(gt.shape[1]), int(npos.numel())
    if N > L.VID_MATCH_MAX_DET:
        raise ValueError("vid_match: det holds N=%d detection rows per image, vd_vid_match takes at most %d" % (N, L.VID_MATCH_MAX_DET))
    if M > L.VID_MATCH_MAX_GT:
        raise ValueError("vid_match: gt holds M=%d label rows per image, vd_vid_match takes at most %d" % (M, L.VID_MATCH_MAX_GT))
    if int(gt.shape[0]) != B:
        raise ValueError("vid_match: gt holds %d images, det %d" % (int(gt.shape[0]), B))
    f64, i32 = torch.float64, torch.int32
    for name, t, n, dt in (("det", det, B * N * 6, f64), ("gt", gt, B * M * 6, f64), ("motion_ranges", motion_ranges, 8, f64),
                           ("area_ranges", area_ranges, 8, f64), ("rec_gt", rec_gt, B * N, i32), ("rec_tp", rec_tp, B * N, i32),
                           ("rec_fp", rec_fp, B * N, i32), ("img_nig", img_nig, B * 4, i32), ("img_ngt", img_ngt, B, i32),
                           ("npos", npos, C, i32), ("nout", nout, 16 * C, i32)):
        if t.dtype != dt or t.numel() != n or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("vid_match: %s must be a contiguous %s device tensor of %d elements, got %s %r"
                             % (name, dt, n, t.dtype, tuple(t.shape)))
    check(_lib().vd_vid_match(ptr(det), B, N, ptr(gt), M, ptr(motion_ranges), ptr(area_ranges), float(iou_thresh),
                              float(pixel_tolerance), ptr(rec_gt), ptr(rec_tp), ptr(rec_fp), ptr(img_nig), ptr(img_ngt), ptr(npos),
                              ptr(nout), C, _s()), "vd_vid_match")


def coco_match(det, gt, iou_thrs, area_rng, rec_rank, rec_bits, npig):
    """vd_coco_match: det (B,N,6) [x, y, w, h, score, category], gt (B,M,8) [x, y, w, h, area, category, annotation id, iscrowd],
    iou_thrs (10,) and area_rng (4,2) are contiguous fp64 device tensors; rec_rank (B,N) and rec_bits (B,N,4) are int32 and
    written whole (they may be uninitialised); npig (K,4) is int32 and accumulated."""
    if det.dim() != 3 or det.shape[-1] != 6:
        raise ValueError("coco_match: det must be (B,N,6) [x, y, w, h, score, category], got %r" % (tuple(det.shape),))
    if gt.dim() != 3 or gt.shape[-1] != 8:
        raise ValueError("coco_match: gt must be (B,M,8) [x, y, w, h, area, category, annotation id, iscrowd], got %r"
                         % (tuple(gt.shape),))
    if npig.dim() != 2 or npig.shape[-1] != 4:
        raise ValueError("coco_match: npig must be (K,4), got %r" % (tuple(npig.shape),))
    B, N, M, K = int(det.shape[0]), int(det.shape[1]), int(gt.shape[1]), int(npig.shape[0])
    if N > L.COCO_MATCH_MAX_DET:
        raise ValueError("coco_match: det holds N=%d detection rows per image, vd_coco_match takes at most %d" % (N, L.COCO_MATCH_MAX_DET))
    if M > L.COCO_MATCH_MAX_GT:
        raise ValueError("coco_match: gt holds M=%d label rows per image, vd_coco_match takes at most %d" % (M, L.COCO_MATCH_MAX_GT))
    if int(gt.shape[0]) != B:
        raise ValueError("coco_match: gt holds %d images, det %d" % (int(gt.shape[0]), B))
    f64, i32 = torch.float64, torch.int32
    for name, t, n, dt in (("det", det, B * N * 6, f64), ("gt", gt, B * M * 8, f64), ("iou_thrs", iou_thrs, 10, f64),
                           ("area_rng", area_rng, 8, f64), ("rec_rank", rec_rank, B * N, i32), ("rec_bits", rec_bits, B * N * 4, i32),
                           ("npig", npig, K * 4, i32)):
        if t.dtype != dt or t.numel() != n or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("coco_match: %s must be a contiguous %s device tensor of %d elements, got %s %r"
                             % (name, dt, n, t.dtype, tuple(t.shape)))
    check(_lib().vd_coco_match(ptr(det), B, N, ptr(gt), M, ptr(iou_thrs), ptr(area_rng), ptr(rec_rank), ptr(rec_bits), ptr(npig),
                               K, _s()), "vd_coco_match")


# --------------------------------------------------------------------------------------------
# the clip-row contract: what every binding that takes the rows of a clip asks of ids, scores, bboxes, track,
# clip_start and ws, stated once.  `who` is the binding's name, the front of every message.
# --------------------------------------------------------------------------------------------
def _int_arg(who, name, v, lo, hi=None):
    """v as an int in [lo, hi] (hi None: unbounded); a bool or anything without __index__ is no integer"""
    if isinstance(v, bool) or not hasattr(v, "__index__") or int(v) < lo or (hi is not None and int(v) > hi):
        if hi is None:
            raise ValueError("%s: %s must be an integer >= %d, got %r" % (who, name, lo, v))
        raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (who, name, lo, hi, v))
    return int(v)


def _rows_shape(who, vd, bboxes, max_rows):
    """(F, N) of bboxes (F,N,4); the entry point `vd` takes at most max_rows rows per frame"""
    if not torch.is_tensor(bboxes) or bboxes.dim() != 3 or bboxes.shape[-1] != 4:
        raise ValueError("%s: bboxes must be (F,N,4), got %r" % (who, tuple(getattr(bboxes, "shape", ()))))
    F, N = int(bboxes.shape[0]), int(bboxes.shape[1])
    if N > max_rows:
        raise ValueError("%s: N=%d rows per frame, %s takes at most %d" % (who, N, vd, max_rows))
    return F, N


def _match_shape(who, gt_boxes, bboxes, max_frames=None):
    """(F, G, N) of a matcher's gt_boxes (F,G,4) and bboxes (F,N,4): the same frames, 1 to MOT_MAX_ROWS rows of either"""
    for name, t, axis in (("gt_boxes", gt_boxes, "G"), ("bboxes", bboxes, "N")):
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[-1] != 4:
            raise ValueError("%s: %s must be (F,%s,4), got %r" % (who, name, axis, tuple(getattr(t, "shape", ()))))
    F, G, N = int(gt_boxes.shape[0]), int(gt_boxes.shape[1]), int(bboxes.shape[1])
    if int(bboxes.shape[0]) != F:
        raise ValueError("%s: gt_boxes holds %d frames, bboxes %d" % (who, F, int(bboxes.shape[0])))
    if max_frames is not None and F > max_frames:
        raise ValueError("%s: gt_boxes holds F=%d frames, vd_%s takes at most %d" % (who, F, who, max_frames))
    if not 1 <= G <= L.MOT_MAX_ROWS:
        raise ValueError("%s: gt_boxes holds G=%d label rows per frame, vd_%s takes 1 to %d" % (who, G, who, L.MOT_MAX_ROWS))
    if not 1 <= N <= L.MOT_MAX_ROWS:
        raise ValueError("%s: bboxes holds N=%d prediction rows per frame, vd_%s takes 1 to %d" % (who, N, who, L.MOT_MAX_ROWS))
    return F, G, N


def _row_specs(ids, scores, bboxes, n, *track):
    """the (name, tensor, numel, dtype) of n rows for _row_tensors; track: the (n,) int32 track table where the binding has one"""
    f32 = torch.float32
    return (("ids", ids, n, f32), ("scores", scores, n, f32), ("bboxes", bboxes, n * 4, f32)) + \
        tuple(("track", t, n, torch.int32) for t in track)


def _row_tensors(who, specs):
    """every (name, tensor, numel, dtype) of specs is a contiguous device tensor of that many elements of that type"""
    for name, t, n, dt in specs:
        if not torch.is_tensor(t) or t.dtype != dt or t.numel() != n or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("%s: %s must be a contiguous %s device tensor of %d elements, got %s %r"
                             % (who, name, str(dt).split(".")[-1], n, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))


def _tracked_rows(who, vd, ids, scores, bboxes, track, clip_start, num_class):
    """the checks of a pass along tracks (tubelet, smooth, stitch), in their order -> (F, N, num_class, clip_start, V)"""
    F, N = _rows_shape(who, vd, bboxes, L.TUBELET_MAX_ROWS)
    num_class = _int_arg(who, "num_class", num_class, 1)
    _row_tensors(who, _row_specs(ids, scores, bboxes, F * N, track))
    if tuple(track.shape) != (F, N):
        raise ValueError("%s: track must be (F,N) = (%d,%d), got %r" % (who, F, N, tuple(track.shape)))
    return (F, N, num_class) + _clip_offsets(who, clip_start, F, bboxes.device)


def _match_rows(who, gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, F, G, N, clip_start):
    """a matcher's label rows and prediction rows, then its clip offsets -> (clip_start, V)"""
    f32, i32 = torch.float32, torch.int32
    _row_tensors(who, (("gt_boxes", gt_boxes, F * G * 4, f32), ("gt_cls", gt_cls, F * G, i32), ("gt_id", gt_id, F * G, i32))
                 + _row_specs(ids, scores, bboxes, F * N, track))
    for name, t, shape in (("gt_cls", gt_cls, (F, G)), ("gt_id", gt_id, (F, G)), ("track", track, (F, N))):
        if tuple(t.shape) != shape:
            raise ValueError("%s: %s must be %r, got %r" % (who, name, shape, tuple(t.shape)))
    return _clip_offsets(who, clip_start, F, bboxes.device)


def _clip_offsets(who, clip_start, F, device):
    """-> (clip_start on the device or None, V): None is one clip of the F frames; V+1 ascending host offsets from 0 to F are
    checked here, then uploaded; an int32 device vector of them is taken as it is"""
    if clip_start is None:
        return None, 1
    if torch.is_tensor(clip_start) and clip_start.is_cuda:
        if clip_start.dtype != torch.int32 or clip_start.dim() != 1 or clip_start.numel() < 2 or not clip_start.is_contiguous():
            raise ValueError("%s: a device clip_start must be a contiguous int32 vector of V+1 offsets, got %s %r"
                             % (who, clip_start.dtype, tuple(clip_start.shape)))
    else:
        cs = [int(v) for v in (clip_start.tolist() if hasattr(clip_start, "tolist") else clip_start)]
        if len(cs) < 2 or cs[0] != 0 or cs[-1] != F or any(b < a for a, b in zip(cs, cs[1:])):
            raise ValueError("%s: clip_start must be V+1 ascending offsets from 0 to F=%d, got %r" % (who, F, cs))
        clip_start = torch.tensor(cs, dtype=torch.int32).to(device, non_blocking=True)
    return clip_start, int(clip_start.numel()) - 1


def _workspace(who, ws, need, device, align=1, at_least=0):
    """ws None: a new workspace of max(need, at_least) bytes on `device`; else ws itself, checked to hold need bytes"""
    if ws is None:
        return torch.empty(max(need, at_least), dtype=torch.uint8, device=device)
    if not torch.is_tensor(ws) or ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous() or not ws.is_cuda \
            or ws.data_ptr() % align:
        raise ValueError("%s: ws must be a contiguous%s uint8 device tensor of >= %d bytes"
                         % (who, ", %d-byte aligned" % align if align > 1 else "", need))
    return ws


def seq_nms(ids, scores, bboxes, clip_start=None, num_class=1, link_thresh=0.5, nms_thresh=0.3, rescore="avg", ws=None, stages=None):
    """vd_seq_nms (viddet_amd/seq_nms.py::seq_nms_host on the device, bit for bit): ids (F,N[,1]), scores (F,N[,1]) and bboxes
    (F,N,4) are contiguous fp32 device tensors, N <= 128; clip_start: None (one clip), V+1 ascending host offsets from 0 to F
    (checked here, then uploaded) or an int32 device tensor of them (taken as it is).  Returns (ids, scores, bboxes, perm) as new
    device tensors of the inputs' shapes, perm (F,N) int32.  Launches on the current stream; nothing is downloaded and nothing
    waits.  ws: a uint8 device tensor of >= 48*F*N bytes to reuse, else one is allocated.  stages (1 or 3; tools/seq_nms_probe.py):
    only the first one or two of the three launches are made (vd_seq_nms_stages) and the outputs stay unwritten."""
    from .seq_nms import RESCORE
    if rescore not in RESCORE:
        raise ValueError("seq_nms: rescore must be 'avg' or 'max', got %r" % (rescore,))
    F, N = _rows_shape("seq_nms", "vd_seq_nms", bboxes, L.SEQ_NMS_MAX_ROWS)
    _row_tensors("seq_nms", _row_specs(ids, scores, bboxes, F * N))
    clip_start, V = _clip_offsets("seq_nms", clip_start, F, bboxes.device)
    ws = _workspace("seq_nms", ws, L.SEQ_NMS_WS_PER_ROW * F * N, bboxes.device)
    out_ids, out_scores, out_bboxes = torch.empty_like(ids), torch.empty_like(scores), torch.empty_like(bboxes)
    perm = torch.empty(F, N, dtype=torch.int32, device=bboxes.device)
    if F == 0 or N == 0:
        return out_ids, out_scores, out_bboxes, perm
    args = (ptr(ids), ptr(scores), ptr(bboxes), ptr(clip_start), V, F, N, int(num_class), float(link_thresh), float(nms_thresh),
            RESCORE[rescore], ptr(out_ids), ptr(out_scores), ptr(out_bboxes), ptr(perm), ptr(ws), int(ws.numel()))
    if stages is None:
        check(_lib().vd_seq_nms(*args, _s()), "vd_seq_nms")
    else:
        check(_lib().vd_seq_nms_stages(*args, int(stages), _s()), "vd_seq_nms_stages")
    return out_ids, out_scores, out_bboxes, perm


def track(ids, scores, bboxes, clip_start=None, num_class=1, sigma_l=0.0, sigma_h=0.5, sigma_iou=0.5, t_min=2, max_age=0, ws=None):
    """vd_track (viddet_amd/track.py::track_host on the device, bit for bit): ids (F,N[,1]), scores (F,N[,1]) and bboxes (F,N,4)
    are contiguous fp32 device tensors, N <= 128; clip_start as ops.seq_nms takes it.  Returns (track, tlen, tscore), new device
    tensors (F,N): int32 track ids (-1: no candidate, or a dropped track), int32 track lengths, fp32 track maxima.  Launches on
    the current stream; nothing is downloaded and nothing waits.  ws: a uint8 device tensor of >= 8*F*N bytes to reuse, else
    one is allocated."""
    from .track import check_params
    sl, sh, si, t_min, max_age = check_params(sigma_l, sigma_h, sigma_iou, t_min, max_age, "track")
    F, N = _rows_shape("track", "vd_track", bboxes, L.TRACK_MAX_ROWS)
    _row_tensors("track", _row_specs(ids, scores, bboxes, F * N))
    clip_start, V = _clip_offsets("track", clip_start, F, bboxes.device)
    ws = _workspace("track", ws, L.TRACK_WS_PER_ROW * F * N, bboxes.device)
    out_track = torch.empty(F, N, dtype=torch.int32, device=bboxes.device)
    out_len = torch.empty(F, N, dtype=torch.int32, device=bboxes.device)
    out_score = torch.empty(F, N, dtype=torch.float32, device=bboxes.device)
    if F == 0 or N == 0:
        return out_track, out_len, out_score
    check(_lib().vd_track(ptr(ids), ptr(scores), ptr(bboxes), ptr(clip_start), V, F, N, int(num_class), float(sl), float(sh),
                          float(si), t_min, max_age, ptr(out_track), ptr(out_len), ptr(out_score), ptr(ws), int(ws.numel()),
                          _s()), "vd_track")
    return out_track, out_len, out_score


def _kalman_link_args(who, ids, scores, bboxes, clip_start, ws):
    """The tensor checks, clip offsets, workspace and outputs that ops.track_sort and ops.track_byte share ->
    (V, F, N, clip_start on the device or None, ws, (out_track, out_len, out_score, out_tbox))"""
    F, N = _rows_shape(who, "vd_" + who, bboxes, L.TRACK_MAX_ROWS)
    _row_tensors(who, _row_specs(ids, scores, bboxes, F * N))
    clip_start, V = _clip_offsets(who, clip_start, F, bboxes.device)
    ws = _workspace(who, ws, L.TRACK_SORT_WS_PER_ROW * F * N + L.TRACK_SORT_WS_PER_CLIP * V, bboxes.device)
    outs = (torch.empty(F, N, dtype=torch.int32, device=bboxes.device), torch.empty(F, N, dtype=torch.int32, device=bboxes.device),
            torch.empty(F, N, dtype=torch.float32, device=bboxes.device), torch.empty(F, N, 4, dtype=torch.float32, device=bboxes.device))
    return V, F, N, clip_start, ws, outs


def track_sort(ids, scores, bboxes, clip_start=None, num_class=1, sigma_l=0.0, sigma_h=0.5, sigma_iou=0.3, t_min=2, max_age=1,
               ws=None):
    """vd_track_sort (viddet_amd/sort.py::sort_host on the device, bit for bit): SORT - Kalman prediction, optimal
    assignment.  The inputs are ops.track's.  Returns (track, tlen, tscore, tbox), new device tensors: ops.track's three (F,N)
    and tbox (F,N,4) fp32, the filtered box of the row's track after this row's update (-1 beside a track of -1).  Launches on
    the current stream; nothing is downloaded and nothing waits.  ws: a uint8 device tensor of >= 8*F*N + 139264*V bytes to
    reuse, else one is allocated."""
    from .track import check_params
    sl, sh, si, t_min, max_age = check_params(sigma_l, sigma_h, sigma_iou, t_min, max_age, "track_sort")
    V, F, N, clip_start, ws, outs = _kalman_link_args("track_sort", ids, scores, bboxes, clip_start, ws)
    if F == 0 or N == 0:
        return outs
    check(_lib().vd_track_sort(ptr(ids), ptr(scores), ptr(bboxes), ptr(clip_start), V, F, N, int(num_class), float(sl), float(sh),
                               float(si), t_min, max_age, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(ws),
                               int(ws.numel()), _s()), "vd_track_sort")
    return outs


def roi_embed(fmap, ids, bboxes, stride, map_index=None, out=None):
    """vd_roi_embed (viddet_amd/appearance.py::embed_host on the device, bit for bit): the int8 appearance
    descriptor of every row, pooled from a route tensor under the row's box.  fmap: a fp32 or bf16 device tensor (S,Hf,Wf,C) whose
    last axis is dense and whose other axes are dense over a pixel pitch of ld >= C elements (a view [..., :C] of a padded plan
    buffer is taken as it is); ids (B,N[,1]) and bboxes (B,N,4) contiguous fp32 device tensors, N <= 128; map_index: None (image
    b reads map b) or an int32 device vector of B entries; out: an int8 device tensor (B,N,C) to write, else one is allocated.
    Returns emb (B,N,C) int8.  Launches on the current stream; nothing is downloaded and nothing waits."""
    from .appearance import check_embed_shape
    if not torch.is_tensor(fmap) or fmap.dim() != 4 or not fmap.is_cuda or fmap.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("roi_embed: fmap must be a fp32 or bf16 device tensor (S,Hf,Wf,C), got %s %r"
                         % (getattr(fmap, "dtype", type(fmap)), tuple(getattr(fmap, "shape", ()))))
    S, Hf, Wf, Cn = (int(v) for v in fmap.shape)
    Cn, stride = check_embed_shape(Cn, stride, "roi_embed")
    if S < 1 or Hf < 1 or Wf < 1:
        raise ValueError("roi_embed: fmap must hold at least one map of one cell, got %r" % (tuple(fmap.shape),))
    # the pitch of a pixel: what the innermost axis of more than one entry says; a single pixel has none to say
    ld = int(fmap.stride(2)) if Wf > 1 else int(fmap.stride(1)) if Hf > 1 else int(fmap.stride(0)) if S > 1 else Cn
    if fmap.stride(3) != 1 or ld < Cn or (Hf > 1 and fmap.stride(1) != Wf * ld) or (S > 1 and fmap.stride(0) != Hf * Wf * ld):
        raise ValueError("roi_embed: fmap must be NHWC, dense over a pixel pitch >= C, got shape %r strides %r"
                         % (tuple(fmap.shape), tuple(fmap.stride())))
    F, N = _rows_shape("roi_embed", "vd_roi_embed", bboxes, L.EMBED_MAX_ROWS)
    f32 = torch.float32
    _row_tensors("roi_embed", (("ids", ids, F * N, f32), ("bboxes", bboxes, F * N * 4, f32)))
    if map_index is not None:
        _row_tensors("roi_embed", (("map_index", map_index, F, torch.int32),))
    elif F > S:
        raise ValueError("roi_embed: %d images and %d maps: map_index must say which map an image reads" % (F, S))
    if out is None:
        out = torch.empty(F, N, Cn, dtype=torch.int8, device=bboxes.device)
    else:
        _row_tensors("roi_embed", (("out", out, F * N * Cn, torch.int8),))
    if F == 0 or N == 0:
        return out
    check(_lib().vd_roi_embed(ptr(fmap), int(fmap.dtype == torch.bfloat16), S, Hf, Wf, Cn, ld, ptr(ids), ptr(bboxes), ptr(map_index),
                              F, N, stride, ptr(out), _s()), "vd_roi_embed")
    return out


def track_sort_app(ids, scores, bboxes, emb, clip_start=None, num_class=1, sigma_l=0.0, sigma_h=0.5, sigma_iou=0.3, t_min=2,
                   max_age=1, sigma_app=0.8, sigma_prox=0.1, ws=None):
    """vd_track_sort_app (viddet_amd/appearance.py::app_sort_host on the device, bit for bit): SORT with the fused
    cost of geometry and appearance.  The inputs are ops.track_sort's and emb (F,N,C), a contiguous int8 device tensor,
    ops.roi_embed's; the returned (track, tlen, tscore, tbox) are ops.track_sort's.  Launches on the current stream; nothing is
    downloaded and nothing waits.  ws: a uint8 device tensor of >= 8*F*N + 663552*V bytes to reuse, else one is allocated."""
    from .appearance import check_app_params, check_embed_shape
    from .track import check_params
    sl, sh, si, t_min, max_age = check_params(sigma_l, sigma_h, sigma_iou, t_min, max_age, "track_sort_app")
    sa, sp = check_app_params(sigma_app, sigma_prox, "track_sort_app")
    F, N = _rows_shape("track_sort_app", "vd_track_sort_app", bboxes, L.TRACK_MAX_ROWS)
    _row_tensors("track_sort_app", _row_specs(ids, scores, bboxes, F * N))
    if not torch.is_tensor(emb) or emb.dim() != 3 or tuple(emb.shape[:2]) != (F, N):
        raise ValueError("track_sort_app: emb must be (F,N,C) = (%d,%d,C), got %r" % (F, N, tuple(getattr(emb, "shape", ()))))
    Cn, _ = check_embed_shape(int(emb.shape[2]), 8, "track_sort_app")
    _row_tensors("track_sort_app", (("emb", emb, F * N * Cn, torch.int8),))
    clip_start, V = _clip_offsets("track_sort_app", clip_start, F, bboxes.device)
    ws = _workspace("track_sort_app", ws, L.TRACK_SORT_WS_PER_ROW * F * N + L.TRACK_SORT_APP_WS_PER_CLIP * V, bboxes.device)
    dev = bboxes.device
    outs = (torch.empty(F, N, dtype=torch.int32, device=dev), torch.empty(F, N, dtype=torch.int32, device=dev),
            torch.empty(F, N, dtype=torch.float32, device=dev), torch.empty(F, N, 4, dtype=torch.float32, device=dev))
    if F == 0 or N == 0:
        return outs
    check(_lib().vd_track_sort_app(ptr(ids), ptr(scores), ptr(bboxes), ptr(emb), Cn, ptr(clip_start), V, F, N, int(num_class),
                                   float(sl), float(sh), float(si), t_min, max_age, float(sa), float(sp), ptr(outs[0]),
                                   ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(ws), int(ws.numel()), _s()), "vd_track_sort_app")
    return outs


def track_byte(ids, scores, bboxes, clip_start=None, num_class=1, sigma_l=0.1, sigma_d=0.5, sigma_new=0.6, sigma_iou=0.2,
               sigma_iou2=0.5, sigma_h=0.5, t_min=2, max_age=7, ws=None):
    """vd_track_byte (viddet_amd/byte.py::byte_host on the device, bit for bit): BYTE - SORT's filter and
    assignment, made twice a frame: the rows scored >= sigma_d against every track, then the other candidates against the tracks
    that are left and were seen in the last frame; only a row scored >= sigma_new starts a track.  The inputs, the checks and
    the returned (track, tlen, tscore, tbox) are ops.track_sort's.  Launches on the current stream; nothing is downloaded and
    nothing waits.  ws: a uint8 device tensor of >= 8*F*N + 139264*V bytes to reuse, else one is allocated."""
    from .byte import check_byte_params
    sl, sd, sn, si, si2, sh, t_min, max_age = check_byte_params(sigma_l, sigma_d, sigma_new, sigma_iou, sigma_iou2, sigma_h, t_min,
                                                                max_age, "track_byte")
    V, F, N, clip_start, ws, outs = _kalman_link_args("track_byte", ids, scores, bboxes, clip_start, ws)
    if F == 0 or N == 0:
        return outs
    check(_lib().vd_track_byte(ptr(ids), ptr(scores), ptr(bboxes), ptr(clip_start), V, F, N, int(num_class), float(sl), float(sd),
                               float(sn), float(sh), float(si), float(si2), t_min, max_age, ptr(outs[0]), ptr(outs[1]),
                               ptr(outs[2]), ptr(outs[3]), ptr(ws), int(ws.numel()), _s()), "vd_track_byte")
    return outs


def tubelet(ids, scores, bboxes, track, clip_start=None, num_class=1, rescore="avg", max_gap=7, drop_untracked=False, ws=None,
            stages=None):
    """vd_tubelet (viddet_amd/tubelet.py::tubelet_host on the device, bit for bit): ids (F,N[,1]), scores (F,N[,1])
    and bboxes (F,N,4) are contiguous fp32 device tensors, N <= 128; track (F,N) a contiguous int32 device tensor, ops.track's
    first result; clip_start as ops.seq_nms takes it.  Returns (ids, scores, bboxes, perm, track_out, dropped), new device
    tensors: the first three of the inputs' shapes, perm and track_out (F,N) int32, dropped (F,) int32.  Launches on the current
    stream; nothing is downloaded and nothing waits.  ws: a uint8 device tensor of >= 24*F*N bytes to reuse, else one is
    allocated.  stages (a mask of 1, 2, 4, 8; tools/tubelet_probe.py): only those of the four launches are made
    (vd_tubelet_stages) and the outputs may stay unwritten."""
    from .tubelet import RESCORE, check_params
    rescore, max_gap, drop_untracked = check_params(rescore, max_gap, drop_untracked, "tubelet")
    F, N, num_class, clip_start, V = _tracked_rows("tubelet", "vd_tubelet", ids, scores, bboxes, track, clip_start, num_class)
    ws = _workspace("tubelet", ws, L.TUBELET_WS_PER_ROW * F * N, bboxes.device)
    dev = bboxes.device
    out_ids, out_scores, out_bboxes = torch.empty_like(ids), torch.empty_like(scores), torch.empty_like(bboxes)
    perm = torch.empty(F, N, dtype=torch.int32, device=dev)
    track_out = torch.empty(F, N, dtype=torch.int32, device=dev)
    dropped = torch.empty(F, dtype=torch.int32, device=dev)
    if F == 0 or N == 0:
        return out_ids, out_scores, out_bboxes, perm, track_out, dropped
    args = (ptr(ids), ptr(scores), ptr(bboxes), ptr(track), ptr(clip_start), V, F, N, int(num_class), RESCORE[rescore], max_gap,
            int(drop_untracked), ptr(out_ids), ptr(out_scores), ptr(out_bboxes), ptr(perm), ptr(track_out), ptr(dropped), ptr(ws),
            int(ws.numel()))
    if stages is None:
        check(_lib().vd_tubelet(*args, _s()), "vd_tubelet")
    else:
        check(_lib().vd_tubelet_stages(*args, int(stages), _s()), "vd_tubelet_stages")
    return out_ids, out_scores, out_bboxes, perm, track_out, dropped


def smooth(ids, scores, bboxes, track, clip_start=None, num_class=1, max_gap=7, ws=None, stages=None):
    """vd_track_smooth (viddet_amd/smooth.py::smooth_host on the device, bit for bit): ids (F,N[,1]), scores
    (F,N[,1]) and bboxes (F,N,4) are contiguous fp32 device tensors, N <= 128; track (F,N) a contiguous int32 device tensor, the
    first result of ops.track / ops.track_sort / ops.track_byte; clip_start as ops.seq_nms takes it.  Returns (sbox, slen), new
    device tensors: sbox (F,N,4) fp32, the Rauch-Tung-Striebel smoothed box of every member of a segment of two or more members
    and the input box elsewhere; slen (F,N) int32, the members of the row's segment.  Launches on the current stream; nothing is
    downloaded and nothing waits.  ws: a uint8 device tensor of >= 80*F*N bytes to reuse, else one is allocated.  stages (a mask
    of 1, 2, 4, 8; tools/smooth_probe.py): only those of the four launches are made (vd_track_smooth_stages) and the outputs may
    stay unwritten."""
    from .smooth import check_params
    max_gap = check_params(max_gap, "smooth")
    F, N, num_class, clip_start, V = _tracked_rows("smooth", "vd_track_smooth", ids, scores, bboxes, track, clip_start, num_class)
    ws = _workspace("smooth", ws, L.TRACK_SMOOTH_WS_PER_ROW * F * N, bboxes.device)
    sbox = torch.empty_like(bboxes)
    slen = torch.empty(F, N, dtype=torch.int32, device=bboxes.device)
    if F == 0 or N == 0:
        return sbox, slen
    args = (ptr(ids), ptr(scores), ptr(bboxes), ptr(track), ptr(clip_start), V, F, N, int(num_class), max_gap, ptr(sbox), ptr(slen),
            ptr(ws), int(ws.numel()))
    if stages is None:
        check(_lib().vd_track_smooth(*args, _s()), "vd_track_smooth")
    else:
        check(_lib().vd_track_smooth_stages(*args, int(stages), _s()), "vd_track_smooth_stages")
    return sbox, slen


def stitch(ids, scores, bboxes, track, clip_start=None, num_class=1, max_gap=30, sigma_iou=0.3, ws=None):
    """vd_track_stitch (viddet_amd/stitch.py::stitch_host on the device, bit for bit): ids (F,N[,1]), scores
    (F,N[,1]) and bboxes (F,N,4) are contiguous fp32 device tensors, N <= 128; track (F,N) a contiguous int32 device tensor, the
    first result of ops.track / ops.track_sort / ops.track_byte; clip_start as ops.seq_nms takes it.  Returns (strack, tlen,
    tscore, stitches, overflow), new device tensors: (F,N) int32, int32 and fp32 - the id of the first track of the row's chain
    of re-linked fragments, the chain's members and its maximum score, -1 / 0 / -1 for a row in no track - and (V,) int32 twice,
    the links of every clip and its tracks beyond the first 512, which enter no link.  Launches on the current stream; nothing
    is downloaded and nothing waits.  ws: a uint8 device tensor of >= 100*F*N bytes to reuse, else one is allocated."""
    from .stitch import check_params
    max_gap, sigma_iou = check_params(max_gap, sigma_iou, "stitch")
    F, N, num_class, clip_start, V = _tracked_rows("stitch", "vd_track_stitch", ids, scores, bboxes, track, clip_start, num_class)
    ws = _workspace("stitch", ws, L.TRACK_STITCH_WS_PER_ROW * F * N, bboxes.device)
    dev = bboxes.device
    strack = torch.empty(F, N, dtype=torch.int32, device=dev)
    tlen = torch.empty(F, N, dtype=torch.int32, device=dev)
    tscore = torch.empty(F, N, dtype=torch.float32, device=dev)
    stitches = torch.empty(V, dtype=torch.int32, device=dev)
    overflow = torch.empty(V, dtype=torch.int32, device=dev)
    if F == 0 or N == 0:
        return strack, tlen, tscore, stitches.zero_(), overflow.zero_()
    check(_lib().vd_track_stitch(ptr(ids), ptr(scores), ptr(bboxes), ptr(track), ptr(clip_start), V, F, N, int(num_class), max_gap,
                                 float(sigma_iou), ptr(strack), ptr(tlen), ptr(tscore), ptr(stitches), ptr(overflow), ptr(ws),
                                 int(ws.numel()), _s()), "vd_track_stitch")
    return strack, tlen, tscore, stitches, overflow


def mot_match(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, clip_start=None, num_class=1, iou_thresh=0.5, agnostic=False,
              ws=None):
    """vd_mot_match (viddet_amd/mot_metric.py::mot_match_host on the device, bit for bit): gt_boxes (F,G,4) fp32,
    gt_cls and gt_id (F,G) int32 - the label rows -, ids (F,N[,1]), scores (F,N[,1]) and bboxes (F,N,4) fp32, track (F,N) int32
    (ops.track's first result, ops.tubelet's fifth), all contiguous device tensors, G and N <= 128; clip_start as ops.seq_nms
    takes it.  Returns (match (F,G) int32, miou (F,G) fp32, flags (F,G) int32, adm (F,G,4) int32 - the bits of the definition's
    uint32 words), new device tensors.  Launches on the current stream; nothing is downloaded and nothing waits.  ws: a uint8
    device tensor of >= 4*F*(G+N) bytes to reuse, else one is allocated."""
    from .mot_metric import check_iou_thresh
    thr = check_iou_thresh(iou_thresh, "mot_match")
    if type(agnostic).__name__ not in ("bool", "bool_"):
        raise ValueError("mot_match: agnostic must be a bool, got %r" % (agnostic,))
    F, G, N = _match_shape("mot_match", gt_boxes, bboxes)
    num_class = _int_arg("mot_match", "num_class", num_class, 1)
    clip_start, V = _match_rows("mot_match", gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, F, G, N, clip_start)
    ws = _workspace("mot_match", ws, L.MOT_WS_PER_ROW * F * (G + N), bboxes.device, at_least=1)
    dev, f32, i32 = bboxes.device, torch.float32, torch.int32
    match = torch.empty(F, G, dtype=i32, device=dev)
    miou = torch.empty(F, G, dtype=f32, device=dev)
    flags = torch.empty(F, G, dtype=i32, device=dev)
    adm = torch.empty(F, G, 4, dtype=i32, device=dev)
    if F == 0:
        return match, miou, flags, adm
    check(_lib().vd_mot_match(ptr(gt_boxes), ptr(gt_cls), ptr(gt_id), ptr(ids), ptr(scores), ptr(bboxes), ptr(track), ptr(clip_start),
                              V, F, G, N, int(num_class), float(thr), int(bool(agnostic)), ptr(match), ptr(miou), ptr(flags), ptr(adm),
                              ptr(ws), int(ws.numel()), _s()), "vd_mot_match")
    return match, miou, flags, adm


def hota_match(gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, num_gt_id, num_track, clip_start=None, num_class=1,
               agnostic=False, ws=None):
    """vd_hota_match (viddet_amd/hota_metric.py::hota_match_host on the device, bit for bit): the tensors and
    clip_start as ops.mot_match takes them, with dense ids: a label row takes part iff 0 <= gt_id < num_gt_id (A, at most 1024),
    a prediction row iff 0 <= track < num_track (P); rows outside are no candidates, as rows with the id -1 are for the host
    definition.  Returns (match (F,G) int32, msim (F,G) fp32, mscore (F,G) int32), new device tensors.  Launches on the current
    stream; nothing is downloaded and nothing waits.  ws: a uint8 device tensor of >= hota_ws_bytes(V, A, P) bytes to reuse
    (whatever it holds), else one is allocated."""
    if type(agnostic).__name__ not in ("bool", "bool_"):
        raise ValueError("hota_match: agnostic must be a bool, got %r" % (agnostic,))
    F, G, N = _match_shape("hota_match", gt_boxes, bboxes, L.HOTA_MAX_FRAMES)
    A = _int_arg("hota_match", "num_gt_id", num_gt_id, 1, L.HOTA_MAX_GT_IDS)
    P = _int_arg("hota_match", "num_track", num_track, 1, 2 ** 31 - 1)
    num_class = _int_arg("hota_match", "num_class", num_class, 1, 2 ** 31 - 1)
    clip_start, V = _match_rows("hota_match", gt_boxes, gt_cls, gt_id, ids, scores, bboxes, track, F, G, N, clip_start)
    ws = _workspace("hota_match", ws, hota_ws_bytes(V, A, P), bboxes.device, align=8)
    dev, f32, i32 = bboxes.device, torch.float32, torch.int32
    match = torch.empty(F, G, dtype=i32, device=dev)
    msim = torch.empty(F, G, dtype=f32, device=dev)
    mscore = torch.empty(F, G, dtype=i32, device=dev)
    if F == 0:
        return match, msim, mscore
    check(_lib().vd_hota_match(ptr(gt_boxes), ptr(gt_cls), ptr(gt_id), ptr(ids), ptr(scores), ptr(bboxes), ptr(track), ptr(clip_start),
                               V, F, G, N, A, P, int(num_class), int(bool(agnostic)), ptr(match), ptr(msim), ptr(mscore), ptr(ws),
                               int(ws.numel()), _s()), "vd_hota_match")
    return match, msim, mscore


def hota_ws_bytes(V, num_gt_id, num_track):
    """the bytes of vd_hota_match's workspace for V clips: V * (8 * A * P + 4 * A + 4 * P); ValueError beyond what is taken"""
    V, A, P = int(V), int(num_gt_id), int(num_track)
    if V < 1 or not 1 <= A <= L.HOTA_MAX_GT_IDS or not 1 <= P <= 2 ** 31 - 1 or V > 2 ** 31 - 1 or V * (8 * A * P + 4 * A + 4 * P) >= 2 ** 47:
        raise ValueError("hota_match: a workspace for V=%d clips, num_gt_id=%d and num_track=%d is beyond what is taken" % (V, A, P))
    return V * (8 * A * P + 4 * A + 4 * P)


_OVERLAY_TABLES = {}     # (kind, device, value) -> the device tensor: the font, and every distinct palette and class-name table


def _overlay_table(kind, device, value, make):
    """a constant table of vd_overlay on `device`, uploaded once per distinct value"""
    key = (kind, str(device), value)
    if key not in _OVERLAY_TABLES:
        _OVERLAY_TABLES[key] = torch.from_numpy(make()).to(device, non_blocking=True)
    return _OVERLAY_TABLES[key]


def overlay(frames, ids, scores, bboxes, track=None, gt=None, clip_start=None, out=None, ws=None, stages=None, H0=None, W0=None,
            pitch=None, uv_offset=None, frame_stride=None, **params):
    """vd_overlay (viddet_amd/overlay.py::overlay_host on the device, bit for bit): detections, tracks and ground
    truth drawn onto video frames.  frames: a uint8 device tensor (F,H0,W0,3), contiguous; with fmt='nv12' (F,H0*3/2,W0) whose
    last stride is 1 (a contiguous tensor, or the view [..., :W0] of a pitched surface: its strides are the pitch and the frame
    stride), or a 1-D surface with H0, W0 and pitch given (uv_offset: the chroma plane's byte offset in a frame, pitch * H0
    where it is not given; frame_stride: uv_offset + pitch * H0 / 2).  ids, scores (F,N[,1]) and bboxes (F,N,4): contiguous fp32
    device tensors in net_size coordinates, N <= 128; track (F,N) int32 or None; gt (F,G,>=5) fp32 or None, G <= 128;
    clip_start as ops.seq_nms takes it.  out: None (a new tensor of the frames' layout: every pixel is written, bytes between
    rows and planes are not), or `frames` itself (in place: only painted pixels are written), or a tensor of the frames' layout
    that does not overlap them.  params: those of overlay.check_params.  Returns (out, painted (F,) int32).  Launches on the
    current stream; nothing is downloaded and nothing waits.  The font, the palette and the class-name table are uploaded once
    per distinct value.  ws: a uint8 device tensor of >= 128*F*(N+G) bytes to reuse.  stages (a mask of 1, 2;
    tools/overlay_probe.py): only those launches are made (vd_overlay_stages)."""
    from . import overlay as O
    p = O.check_params(tracked=track is not None, who="overlay", **params)
    nv12 = p["fmt"] == "nv12"
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise ValueError("overlay: frames must be a uint8 tensor, got %s" % (getattr(frames, "dtype", type(frames)),))
    F, N = _rows_shape("overlay", "vd_overlay", bboxes, L.OVERLAY_MAX_ROWS)
    if nv12 and frames.dim() == 1:
        if H0 is None or W0 is None or pitch is None:
            raise ValueError("overlay: a 1-D NV12 surface needs H0, W0 and pitch")
        h0, w0, pitch = int(H0), int(W0), int(pitch)
        if h0 < 2 or w0 < 2 or h0 % 2 or w0 % 2 or h0 > O.MAX_SIZE or w0 > O.MAX_SIZE:
            raise ValueError("overlay: NV12 needs an even frame size of at most %d pixels a side, got H0=%d W0=%d"
                             % (O.MAX_SIZE, h0, w0))
        uv_offset = pitch * h0 if uv_offset is None else int(uv_offset)
        span = uv_offset + pitch * (h0 // 2 - 1) + w0
        frame_stride = uv_offset + pitch * (h0 // 2) if frame_stride is None else int(frame_stride)
        if pitch < w0 or uv_offset < pitch * h0 or frame_stride < span or frames.numel() < (F - 1) * frame_stride + span \
                or not frames.is_contiguous():
            raise ValueError("overlay: a surface of %d bytes does not hold F=%d NV12 frames of %dx%d with pitch=%d uv_offset=%d "
                             "frame_stride=%d" % (frames.numel(), F, h0, w0, pitch, uv_offset, frame_stride))
    else:
        if (H0, W0, pitch, uv_offset, frame_stride) != (None,) * 5:
            raise ValueError("overlay: H0, W0, pitch, uv_offset and frame_stride describe a 1-D NV12 surface, got frames %r"
                             % (tuple(frames.shape),))
        f_, h0, w0 = O.frame_size(tuple(frames.shape), p["fmt"])
        if f_ != F:
            raise ValueError("overlay: %d frames but rows of %d" % (f_, F))
        if nv12:
            pitch, frame_stride = int(frames.stride(1)), int(frames.stride(0))
            uv_offset = pitch * h0
            if frames.stride(2) != 1 or pitch < w0 or (F > 1 and frame_stride < uv_offset + pitch * (h0 // 2 - 1) + w0):
                raise ValueError("overlay: NV12 frames need a last stride of 1, rows at least W0 and frames at least a frame "
                                 "apart, got strides %r" % (tuple(frames.stride()),))
            frame_stride = max(frame_stride, uv_offset + pitch * (h0 // 2 - 1) + w0)
        else:
            if not frames.is_contiguous():
                raise ValueError("overlay: RGB frames must be contiguous, got strides %r" % (tuple(frames.stride()),))
            pitch, uv_offset = 3 * w0, 0
            frame_stride = h0 * pitch
    if not frames.is_cuda:
        raise ValueError("overlay: frames must be a device tensor")
    dev = frames.device
    _row_tensors("overlay", _row_specs(ids, scores, bboxes, F * N, *(() if track is None else (track,))))
    G, gt_stride = 0, 0
    if gt is not None:
        if not torch.is_tensor(gt) or gt.dtype != torch.float32 or gt.dim() != 3 or gt.shape[0] != F or gt.shape[2] < 5 \
                or not gt.is_contiguous() or not gt.is_cuda:
            raise ValueError("overlay: gt must be a contiguous fp32 device tensor (F,G,>=5) with F=%d, got %s %r"
                             % (F, getattr(gt, "dtype", type(gt)), tuple(getattr(gt, "shape", ()))))
        G, gt_stride = int(gt.shape[1]), int(gt.shape[2])
        if G > L.OVERLAY_MAX_ROWS:
            raise ValueError("overlay: G=%d ground-truth rows per frame, vd_overlay takes at most %d" % (G, L.OVERLAY_MAX_ROWS))
        if G == 0:
            gt = None
    clip_start, V = _clip_offsets("overlay", clip_start, F, dev)
    if out is None:
        out = torch.empty_strided(tuple(frames.shape), tuple(frames.stride()), dtype=torch.uint8, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != tuple(frames.shape) \
            or tuple(out.stride()) != tuple(frames.stride()):
        raise ValueError("overlay: out must be a uint8 tensor of the frames' shape and strides on their device (or `frames` itself)")
    ws = _workspace("overlay", ws, L.OVERLAY_WS_PER_ROW * F * (N + G), dev)
    # (the primitives launch resets the count; the paint launch alone adds to it)
    painted = (torch.empty if stages is None or int(stages) & 1 else torch.zeros)(F, dtype=torch.int32, device=dev)
    if F == 0 or N == 0:
        if out.data_ptr() != frames.data_ptr():
            out.copy_(frames)
        return out, painted.zero_()
    net = p["net_size"] or (h0, w0)
    font = _overlay_table("font", dev, None, lambda: O.font_table())
    pal = _overlay_table("palette", dev, (p["palette"].tobytes(), p["fmt"], p["matrix"], p["range"]),
                         lambda: O.palette_words(p["palette"], p["fmt"], p["matrix"], p["range"]).view("int32"))
    names = None
    if p["class_names"]:
        names = _overlay_table("names", dev, p["class_names"], lambda: O.names_table(p["class_names"]))
    args = (ptr(frames), ptr(out), frame_stride, pitch, uv_offset, 1 if nv12 else 0, F, h0, w0, ptr(ids), ptr(scores), ptr(bboxes),
            ptr(track), ptr(gt), gt_stride, ptr(clip_start), V, N, G, net[0], net[1], p["thresh"], p["thickness"], p["scale"],
            p["trail"], 1 if p["color_by"] == "track" else 0, ptr(names), 0 if names is None else int(names.shape[0]), ptr(pal),
            ptr(font), ptr(painted), ptr(ws), int(ws.numel()))
    if stages is None:
        check(_lib().vd_overlay(*args, _s()), "vd_overlay")
    else:
        check(_lib().vd_overlay_stages(*args, int(stages), _s()), "vd_overlay_stages")
    return out, painted


def motion_signature(frames, cell=4, fmt="rgb", H0=None, W0=None, pitch=None, frame_stride=None, out=None):
    """vd_motion_sig (viddet_amd/motion.py::signature_host on the device, bit for bit): the luma of every frame
    summed over cell x cell blocks.  frames: a uint8 device tensor with ops.overlay's surface conventions - (F,H0,W0,3)
    contiguous; with fmt='nv12' (F,H0*3/2,W0) whose last stride is 1 (a contiguous tensor, or the view [..., :W0] of a pitched
    surface), or a 1-D surface with H0, W0 and pitch given (frame_stride: pitch * H0 * 3 / 2 where it is not given; the frames it
    holds are counted from its size).  out: a contiguous uint16 device tensor (F,Gh,Gw) to write, else one is allocated.  Returns
    sig (F,Gh,Gw) uint16.  The frames are never written.  Launches on the current stream; nothing is downloaded and nothing
    waits."""
    from . import motion as M
    cell, _, _ = M.check_params(cell=cell, who="motion_signature")
    if fmt not in M.FORMATS:
        raise ValueError("motion_signature: fmt must be 'rgb' or 'nv12', got %r" % (fmt,))
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise ValueError("motion_signature: frames must be a uint8 tensor, got %s" % (getattr(frames, "dtype", type(frames)),))
    nv12 = fmt == "nv12"
    if nv12 and frames.dim() == 1:
        if H0 is None or W0 is None or pitch is None:
            raise ValueError("motion_signature: a 1-D NV12 surface needs H0, W0 and pitch")
        h0, w0, pitch = int(H0), int(W0), int(pitch)
        if h0 < 2 or w0 < 2 or h0 % 2 or w0 % 2:
            raise ValueError("motion_signature: NV12 needs an even frame size, got H0=%d W0=%d" % (h0, w0))
        span = pitch * (h0 + h0 // 2 - 1) + w0
        frame_stride = pitch * (h0 + h0 // 2) if frame_stride is None else int(frame_stride)
        if pitch < w0 or frame_stride < span or frames.numel() < span or not frames.is_contiguous():
            raise ValueError("motion_signature: a surface of %d bytes holds no NV12 frame of %dx%d with pitch=%d frame_stride=%d"
                             % (frames.numel(), h0, w0, pitch, frame_stride))
        F = (int(frames.numel()) - span) // frame_stride + 1
    else:
        if (H0, W0, pitch, frame_stride) != (None,) * 4:
            raise ValueError("motion_signature: H0, W0, pitch and frame_stride describe a 1-D NV12 surface, got frames %r"
                             % (tuple(frames.shape),))
        F, h0, w0 = M.frame_size(tuple(frames.shape), fmt)
        if nv12:
            pitch, frame_stride = int(frames.stride(1)), int(frames.stride(0))
            span = pitch * (h0 + h0 // 2 - 1) + w0
            if frames.stride(2) != 1 or pitch < w0 or (F > 1 and frame_stride < span):
                raise ValueError("motion_signature: NV12 frames need a last stride of 1, rows at least W0 and frames at least a "
                                 "frame apart, got strides %r" % (tuple(frames.stride()),))
            frame_stride = max(frame_stride, span)
        else:
            if not frames.is_contiguous():
                raise ValueError("motion_signature: RGB frames must be contiguous, got strides %r" % (tuple(frames.stride()),))
            pitch = 3 * w0
            frame_stride = h0 * pitch
    if not frames.is_cuda:
        raise ValueError("motion_signature: frames must be a device tensor")
    Gh, Gw = M.grid_size(h0, w0, cell)
    if Gh < 1 or Gw < 1:
        raise ValueError("motion_signature: frames of %d x %d hold no cell of %d pixels" % (h0, w0, cell))
    if out is None:
        out = torch.empty(F, Gh, Gw, dtype=torch.uint16, device=frames.device)
    else:
        _row_tensors("motion_signature", (("out", out, F * Gh * Gw, torch.uint16),))
        if out.device != frames.device:
            raise ValueError("motion_signature: out must be on the frames' device")
    if F == 0:
        return out
    check(_lib().vd_motion_sig(ptr(frames), frame_stride, pitch, 1 if nv12 else 0, F, h0, w0, cell, ptr(out), _s()), "vd_motion_sig")
    return out


def motion_match(sig, clip_start=None, radius=8, gate=0.75, ws=None, cell=4):
    """vd_motion_match (viddet_amd/motion.py::match_host on the device, bit for bit): the translation between
    consecutive frames by block matching on their signatures.  sig: a contiguous uint16 device tensor (F,Gh,Gw),
    ops.motion_signature's; clip_start as ops.seq_nms takes it; cell: the signature's, the unit of the result.  Returns device
    tensors (motion (F,2) int32 in source pixels, sad (F,2) int64, cum (F,2) int32: the running sum of motion inside every clip).
    Launches on the current stream; nothing is downloaded and nothing waits.  ws: a uint8 device tensor of >= 8 * F *
    (2 * radius + 1)**2 bytes, 8-byte aligned, to reuse, else one is allocated."""
    from . import motion as M
    cell, radius, g = M.check_params(cell, radius, gate, "motion_match")
    if not torch.is_tensor(sig) or sig.dtype != torch.uint16 or sig.dim() != 3 or not sig.is_contiguous() or not sig.is_cuda:
        raise ValueError("motion_match: sig must be a contiguous uint16 device tensor (F,Gh,Gw), got %s %r"
                         % (getattr(sig, "dtype", type(sig)), tuple(getattr(sig, "shape", ()))))
    F, Gh, Gw = (int(v) for v in sig.shape)
    M.check_grid(Gh, Gw, radius, "motion_match")
    dev = sig.device
    clip_start, V = _clip_offsets("motion_match", clip_start, F, dev)
    motion = torch.empty(F, 2, dtype=torch.int32, device=dev)
    sad = torch.empty(F, 2, dtype=torch.int64, device=dev)
    cum = torch.empty(F, 2, dtype=torch.int32, device=dev)
    if F == 0:
        return motion, sad, cum
    need = int(_lib().vd_motion_match_ws_bytes(F, radius))
    if need < 0:
        raise ValueError("motion_match: F=%d frames at radius=%d: vd_motion_match takes at most 2^31 - 1 table entries" % (F, radius))
    ws = _workspace("motion_match", ws, need, dev, align=8)
    check(_lib().vd_motion_match(ptr(sig), ptr(clip_start), V, F, Gh, Gw, cell, radius, float(g), ptr(motion), ptr(sad), ptr(cum),
                                 ptr(ws), int(ws.numel()), _s()), "vd_motion_match")
    return motion, sad, cum


def motion_shift(ids_or_track, boxes, cum, sx, sy, sign):
    """vd_motion_shift (viddet_amd/motion.py::stabilise_host with sign -1, restore_host with sign +1, on the device, bit for bit,
    DESIGN.md 44).  ids_or_track: contiguous fp32 ids (F,N[,1]) - the rows with id >= 0 move - or an int32 track table (F,N) -
    those with track >= 0 do; boxes (F,N,4) contiguous fp32; cum (F,2) int32, ops.motion_match's; sx, sy: the network's size over
    the source's.  Returns a new tensor; the input is never written.  Launches on the current stream; nothing is downloaded and
    nothing waits."""
    if isinstance(sign, bool) or sign not in (1, -1):
        raise ValueError("motion_shift: sign must be +1 (restore) or -1 (stabilise), got %r" % (sign,))
    if not torch.is_tensor(boxes) or boxes.dim() != 3 or boxes.shape[-1] != 4:
        raise ValueError("motion_shift: boxes must be (F,N,4), got %r" % (tuple(getattr(boxes, "shape", ())),))
    F, N = int(boxes.shape[0]), int(boxes.shape[1])
    if not torch.is_tensor(ids_or_track) or ids_or_track.dtype not in (torch.float32, torch.int32):
        raise ValueError("motion_shift: ids_or_track must be fp32 ids or an int32 track table, got %s"
                         % (getattr(ids_or_track, "dtype", type(ids_or_track)),))
    is_track = ids_or_track.dtype == torch.int32
    _row_tensors("motion_shift", (("track" if is_track else "ids", ids_or_track, F * N, ids_or_track.dtype),
                                  ("boxes", boxes, F * N * 4, torch.float32), ("cum", cum, F * 2, torch.int32)))
    out = torch.empty_like(boxes)
    if F == 0 or N == 0:
        return out
    check(_lib().vd_motion_shift(ptr(ids_or_track), int(is_track), ptr(boxes), ptr(cum), F, N, float(sx), float(sy), int(sign), ptr(out),
                                 _s()), "vd_motion_shift")
    return out


class _StreamState:
    """What the live-state classes share: V streams of N rows per frame, a zeroed uint8 state tensor (V, bytes) - all zero is
    a fresh stream -, the frames pushed since the last reset, and the checks of a push."""

    _IDS = "hand out"                                 # what a push does with track ids, in the refusal of too many frames

    def _open(self, V, N, num_class, state_bytes, device):
        who = type(self).__name__
        self.V = _int_arg(who, "V", V, 1, 2 ** 31 - 1)
        self.N = _int_arg(who, "N", N, 1, L.TRACK_MAX_ROWS)
        self.num_class = _int_arg(who, "num_class", num_class, 1, 2 ** 31 - 1)
        self.state = torch.zeros(self.V, state_bytes, dtype=torch.uint8, device=device)
        self.frames = 0                               # pushed to every stream since the last reset

    def reset(self):
        self.state.zero_()
        self.frames = 0

    def _push_rows(self, ids, scores, bboxes, *track):
        """the checks of push(ids, scores, bboxes[, track]) -> (lead, F): the outputs' leading shape (V,F) or (F,), the frames"""
        who, V, N = type(self).__name__ + ".push", self.V, self.N
        lead = tuple(getattr(bboxes, "shape", ())[:-2])
        if not torch.is_tensor(bboxes) or bboxes.dim() not in (3, 4) or bboxes.shape[-1] != 4 or bboxes.shape[-2] != N \
                or (lead[:-1] or (1,)) != (V,):
            raise ValueError("%s: bboxes must be (%d,F,%d,4)%s, got %r"
                             % (who, V, N, " or (F,%d,4)" % N if V == 1 else "", tuple(getattr(bboxes, "shape", ()))))
        F = int(lead[-1])
        _row_tensors(who, _row_specs(ids, scores, bboxes, V * F * N))
        for t in track:
            if not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != lead + (N,) or not t.is_contiguous() \
                    or not t.is_cuda:
                raise ValueError("%s: track must be a contiguous int32 device tensor %r, got %s %r"
                                 % (who, lead + (N,), getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
        if (self.frames + F) * N > 2 ** 31 - 1:
            raise ValueError("%s: %d + %d frames of %d rows could %s more than 2**31 - 1 track ids; reset() the state (a new clip) "
                             "first" % (who, self.frames, F, N, self._IDS))
        return lead, F


class TrackState(_StreamState):
    """The tracker on V streams that never say where they end (vd_track_push; viddet_amd/track.py::track_online_host on the
    device, bit for bit): owns the state tensor (V, VD_TRACK_STATE_BYTES) uint8 - all zero is a fresh stream -
    and the fixed parameters.  push(ids, scores, bboxes) runs the next F frames of every stream: ids (V,F,N[,1]), scores
    (V,F,N[,1]) and bboxes (V,F,N,4), contiguous fp32 device tensors (V == 1: the leading axis may be left out), ->
    (track, tlen, tscore), new device tensors of the leading shape: the row's track id counted over the whole stream (-1: no
    candidate), its track's length so far and maximum so far.  Launches on the current stream; nothing is downloaded and
    nothing waits.  A stream hands out at most N ids per frame, so a push that could take frames * N past 2**31 - 1 is
    refused (counted on the host).  reset() starts every stream afresh."""

    def __init__(self, V=1, N=100, num_class=1, sigma_l=0.0, sigma_iou=0.5, max_age=0, device="cuda"):
        from .track import check_params
        self.sigma_l, _, self.sigma_iou, _, self.max_age = check_params(sigma_l, 0.5, sigma_iou, 1, max_age, "TrackState")
        self._open(V, N, num_class, L.TRACK_STATE_BYTES, device)

    def push(self, ids, scores, bboxes):
        V, N = self.V, self.N
        lead, F = self._push_rows(ids, scores, bboxes)
        dev = bboxes.device
        out_track = torch.empty(lead + (N,), dtype=torch.int32, device=dev)
        out_len = torch.empty(lead + (N,), dtype=torch.int32, device=dev)
        out_score = torch.empty(lead + (N,), dtype=torch.float32, device=dev)
        if F == 0:
            return out_track, out_len, out_score
        check(_lib().vd_track_push(ptr(ids), ptr(scores), ptr(bboxes), V, F, N, self.num_class, float(self.sigma_l),
                                   float(self.sigma_iou), self.max_age, ptr(self.state), int(self.state.numel()), ptr(out_track),
                                   ptr(out_len), ptr(out_score), _s()), "vd_track_push")
        self.frames += F
        return out_track, out_len, out_score


class KalmanTrackState(_StreamState):
    """SORT or BYTE on V streams that never say where they end (vd_track_kf_push; viddet_amd/sort.py::sort_online_host and
    viddet_amd/byte.py::byte_online_host on the device, bit for bit): owns the state tensor
    (V, VD_TRACK_KF_STATE_BYTES) uint8 - the tracks' words and their filter states; all zero is a fresh stream - and the fixed
    parameters: method 'sort' (sigma_l, sigma_iou, max_age; sort.DEFAULTS where left out) or 'byte' (sigma_l, sigma_d,
    sigma_new, sigma_iou, sigma_iou2, max_age; byte.DEFAULTS), without sigma_h and t_min, since nothing is decided online.
    push(ids, scores, bboxes) runs the next F frames of every stream, the tensors as TrackState.push takes them, ->
    (track, tlen, tscore, tbox), new device tensors: TrackState's three and tbox of the leading shape + (N,4), the posterior
    box of the row's track after this row's update (-1 beside a track of -1).  Launches on the current stream; nothing is
    downloaded and nothing waits.  A push that could take frames * N past 2**31 - 1 is refused (counted on the host).  reset()
    starts every stream afresh."""

    def __init__(self, V=1, N=100, num_class=1, method="sort", device="cuda", **params):
        who = "KalmanTrackState"
        if method == "iou":
            raise ValueError("%s: method 'iou' has no filter to carry: ops.TrackState is its resumable form" % who)
        if method not in ("sort", "byte"):
            raise ValueError("%s: method must be 'sort' or 'byte', got %r" % (who, method))
        if method == "sort":
            from .sort import DEFAULTS
        else:
            from .byte import DEFAULTS
        names = [k for k in DEFAULTS if k not in ("sigma_h", "t_min")]
        unknown = sorted(set(params) - set(names))
        if unknown:
            raise ValueError("%s: method %r takes %s, got %s" % (who, method, ", ".join(names), ", ".join(unknown)))
        kw = dict({k: DEFAULTS[k] for k in names}, **params)
        if method == "sort":
            # SORT on BYTE's frame body: every candidate is a high row that may start a track, the second association never runs
            from .track import check_params
            sl, _, si, _, age = check_params(sigma_h=0.5, t_min=1, who=who, **kw)
            sd, sn, si2 = sl, sl, si
        else:
            from .byte import check_byte_params
            sl, sd, sn, si, si2, _, _, age = check_byte_params(sigma_h=0.5, t_min=1, who=who, **kw)
        self._open(V, N, num_class, L.TRACK_KF_STATE_BYTES, device)
        self.method, self.params = method, kw
        self.sigma_l, self.sigma_d, self.sigma_new, self.sigma_iou, self.sigma_iou2 = (float(v) for v in (sl, sd, sn, si, si2))
        self.max_age = age

    def push(self, ids, scores, bboxes):
        V, N = self.V, self.N
        lead, F = self._push_rows(ids, scores, bboxes)
        dev = bboxes.device
        out_track = torch.empty(lead + (N,), dtype=torch.int32, device=dev)
        out_len = torch.empty(lead + (N,), dtype=torch.int32, device=dev)
        out_score = torch.empty(lead + (N,), dtype=torch.float32, device=dev)
        out_tbox = torch.empty(lead + (N, 4), dtype=torch.float32, device=dev)
        if F == 0:
            return out_track, out_len, out_score, out_tbox
        check(_lib().vd_track_kf_push(ptr(ids), ptr(scores), ptr(bboxes), V, F, N, self.num_class, self.sigma_l, self.sigma_d,
                                      self.sigma_new, self.sigma_iou, self.sigma_iou2, self.max_age, ptr(self.state),
                                      int(self.state.numel()), ptr(out_track), ptr(out_len), ptr(out_score), ptr(out_tbox), _s()),
              "vd_track_kf_push")
        self.frames += F
        return out_track, out_len, out_score, out_tbox


class SmoothLagState(_StreamState):
    """Fixed-lag smoothing of the boxes of V streams along their tracks (vd_track_smooth_push;
    viddet_amd/smooth_lag.py::smooth_lag_host on the device, bit for bit): owns the state tensor
    (V, VD_TRACK_SMOOTH_LIVE_STATE_BYTES) uint8 - the last 16 frames' members, boxes, posterior states and links; all zero is a
    fresh stream - and the fixed parameters lag (0..15, no default: a latency must be chosen) and max_gap (0..7).
    push(ids, scores, bboxes, track) takes the next F frames of every stream - the tensors as KalmanTrackState.push takes
    them, and track (V,F,N) or (F,N) int32, the per-row ids of an online tracker counted over the stream - and returns
    (t0, sbox, slen), new device tensors for the m frames [t0, t0 + m) that became final: frame u is final once frame u + lag
    has been taken; sbox of the leading shape (m,N,4) fp32 (with V: (V,m,N,4)) and slen (m,N) int32.  m == 0 gives empty
    tensors.  flush() emits the frames still waiting and leaves the state fresh; reset() zeroes the state and the count.
    Every stream takes the same frames, so m is one number, counted on the host: launches on the current stream, nothing is
    downloaded and nothing waits.  A push that could take frames * N past 2**31 - 1 is refused."""

    _IDS = "meet"                                     # this pass is handed the ids of a tracker

    def __init__(self, V=1, N=100, num_class=1, lag=None, max_gap=7, device="cuda"):
        from .smooth_lag import check_params
        who = "SmoothLagState"
        if lag is None:
            raise ValueError("%s: lag must be given: a frame comes out `lag` frames late, an integer in [0, 15]" % who)
        self.lag, self.max_gap = check_params(lag, max_gap, who)
        self._open(V, N, num_class, L.TRACK_SMOOTH_LIVE_STATE_BYTES, device)
        self._lead = (self.V,) if self.V > 1 else ()  # the outputs' leading shape: the last push's

    @property
    def emitted(self):
        """the frames given out since the last reset"""
        return max(0, self.frames - self.lag)

    def _launch(self, ids, scores, bboxes, track, lead, F, flush):
        V, N = self.V, self.N
        t0 = self.emitted
        m = (self.frames + F if flush else max(0, self.frames + F - self.lag)) - t0
        dev = self.state.device
        sbox = torch.empty(lead + (m, N, 4), dtype=torch.float32, device=dev)
        slen = torch.empty(lead + (m, N), dtype=torch.int32, device=dev)
        if F or flush:
            args = (0, 0, 0, 0) if F == 0 else (ptr(ids), ptr(scores), ptr(bboxes), ptr(track))
            check(_lib().vd_track_smooth_push(*args, V, F, N, self.num_class, self.lag, self.max_gap, 1 if flush else 0,
                                              ptr(self.state), int(self.state.numel()), m, ptr(sbox) if m else 0,
                                              ptr(slen) if m else 0, _s()), "vd_track_smooth_push")
        self.frames += F
        return t0, sbox, slen

    def push(self, ids, scores, bboxes, track):
        lead, F = self._push_rows(ids, scores, bboxes, track)
        self._lead = lead[:-1]
        return self._launch(ids, scores, bboxes, track, lead[:-1], F, False)

    def flush(self):
        """-> (t0, sbox, slen) of the frames still waiting, smoothed against the last frame taken; the state is fresh afterwards"""
        out = self._launch(None, None, None, None, self._lead, 0, True)
        self.reset()                                  # the kernel zeroed the header; the bytes are a fresh stream's too
        return out


def temporal_pool(x, y, argmax, B, K, inner, type_):
    check(_lib().vd_temporal_pool(ptr(x), ptr(y), ptr(argmax), B, K, inner, type_, _s()), "vd_temporal_pool")


def temporal_pool_bwd(dy, argmax, dx, B, K, inner, type_):
    check(_lib().vd_temporal_pool_bwd(ptr(dy), ptr(argmax), ptr(dx), B, K, inner, type_, _s()), "vd_temporal_pool_bwd")


def frame_slice(x, y, B, K, k0, kc, inner, backward=False):
    """frames [k0, k0 + kc) of every K-frame window: x [B*K, inner] -> y [B*kc, inner]; backward: x = dy, y = dx (written whole)"""
    check(_lib().vd_frame_slice(ptr(x), ptr(y), B, K, k0, kc, inner, 1 if backward else 0, _s()), "vd_frame_slice")


def temporal_cat(x, y, B, K, hw, C_, backward=False):
    """'cat' join: x [B*K, hw, C] -> y [B, hw, K*C]; backward: x = the stacked gradient, y = the per-frame one"""
    check(_lib().vd_temporal_cat(ptr(x), ptr(y), B, K, hw, C_, 1 if backward else 0, _s()), "vd_temporal_cat")


def tdw_fwd(x, w, res, y, B, K, HW, C_, amax_out=None):
    """y = depthwise (3,1,1) conv of x over the K frames of each window, repeat padding (tail pad = frame K-2) [+ res]"""
    check(_lib().vd_tdw_fwd(ptr(x), ptr(w), ptr(res), ptr(y), B, K, HW, C_, ptr(amax_out), _s()), "vd_tdw_fwd")


def tdw_bwd_ws_bytes(B, K, HW, C_):
    return int(_lib().vd_tdw_bwd_ws_bytes(B, K, HW, C_))


def tdw_bwd(dy, x, w, dx, dw, B, K, HW, C_, ws=None):
    """dx (None: skipped) and dw [C][3] (None: skipped) of tdw_fwd; ws = the partial-sum rows of the weight gradient"""
    check(_lib().vd_tdw_bwd(ptr(dy), ptr(x), ptr(w), ptr(dx), ptr(dw), B, K, HW, C_, ptr(ws),
                            0 if ws is None else ws.numel() * ws.element_size(), _s()), "vd_tdw_bwd")


def sgd_momentum(w, g, m, lr, momentum, wd, rescale):
    check(_lib().vd_sgd_momentum(ptr(w), ptr(g), ptr(m), w.numel(), lr, momentum, wd, rescale, _s()), "vd_sgd_momentum")


# --------------------------------------------------------------------------------------------
# yolo head
# --------------------------------------------------------------------------------------------
def make_head_desc(heads, grids, ldh, strides, anchors, B, num_class):
    h = HeadDesc()
    for s in range(3):
        h.head[s] = heads[s].data_ptr()
        h.g[s] = grids[s]
        h.stride[s] = float(strides[s])
        for j in range(6):
            h.anchors[s][j] = float(anchors[s][j])
    h.ldh, h.B, h.C = ldh, B, num_class
    return h


def yolo_decode_filter(h, valid_thresh, cand_score, cand_row, cap, counts):
    check(_lib().vd_yolo_decode_filter(C.byref(h), valid_thresh, ptr(cand_score), ptr(cand_row), cap, ptr(counts), _s()),
          "vd_yolo_decode_filter")


def nms_topk(h, cand_score, cand_row, cap, counts, nms_thresh, topk, post_nms, ids, scores, boxes, rows, ws):
    check(_lib().vd_nms_topk(C.byref(h), ptr(cand_score), ptr(cand_row), cap, ptr(counts), nms_thresh, topk, post_nms,
                             ptr(ids), ptr(scores), ptr(boxes), ptr(rows), ptr(ws), ws.numel() * ws.element_size(),
                             _s()), "vd_nms_topk")


def yolo_decode_filter_agnostic(h, valid_thresh, cand_score, cand_row, cap, counts, head_bf16=False):
    """class-agnostic candidates (one per anchor, score = sigmoid(objectness)); head_bf16: h.head point to bf16 tensors"""
    check(_lib().vd_yolo_decode_filter_agnostic(C.byref(h), 1 if head_bf16 else 0, valid_thresh, ptr(cand_score), ptr(cand_row),
                                                cap, ptr(counts), _s()), "vd_yolo_decode_filter_agnostic")


def nms_agnostic(h, cand_score, cand_row, cap, counts, nms_thresh, topk, post_nms, ids, scores, boxes, rows, ws, head_bf16=False):
    check(_lib().vd_nms_agnostic(C.byref(h), 1 if head_bf16 else 0, ptr(cand_score), ptr(cand_row), cap, ptr(counts), nms_thresh,
                                 topk, post_nms, ptr(ids), ptr(scores), ptr(boxes), ptr(rows), ptr(ws),
                                 ws.numel() * ws.element_size(), _s()), "vd_nms_agnostic")


def yolo_loss_fwd_bwd(h, gt, M, obj_t, center_t, scale_t, weight_t, class_t, ignore_thresh, label_smooth, losses,
                      dheads, box_out, ws, dhead_amax=None):
    arr = (C.c_void_p * 3)(*[t.data_ptr() for t in dheads])
    if dheads[0].dtype == torch.bfloat16:       # bf16-storage training: bf16 gradient rows (fp32 logits)
        check(_lib().vd_yolo_loss_fwd_bwd_bf16(C.byref(h), ptr(gt), M, ptr(obj_t), ptr(center_t), ptr(scale_t), ptr(weight_t),
                                               ptr(class_t), ignore_thresh, 1 if label_smooth else 0, ptr(losses),
                                               C.byref(arr), ptr(box_out), ptr(ws), ws.numel() * ws.element_size(), _s()),
              "vd_yolo_loss_fwd_bwd_bf16")
        return
    am = None if dhead_amax is None else C.byref((C.c_void_p * 3)(*[t.data_ptr() for t in dhead_amax]))
    check(_lib().vd_yolo_loss_fwd_bwd(C.byref(h), ptr(gt), M, ptr(obj_t), ptr(center_t), ptr(scale_t), ptr(weight_t),
                                      ptr(class_t), ignore_thresh, 1 if label_smooth else 0, ptr(losses),
                                      C.byref(arr), ptr(box_out), am, ptr(ws), ws.numel() * ws.element_size(), _s()),
          "vd_yolo_loss_fwd_bwd")


def yolo_loss_ws_bytes(h):
    return _lib().vd_yolo_loss_ws_bytes(C.byref(h))
