/*
 * viddet_hip.h — C-ABI of libviddet_hip.so, the MI355X (gfx950) kernel library behind the
 * yolo3_darknet53 train / detect hot path.
 *
 * The reference (HaydenFaulkner/VidDet) has no FFI: its hot path is a Gluon HybridBlock that
 * composes MXNet/GluonCV operators.  Each entry point below therefore names the reference
 * *operator call site* (file:line under /root/reference) whose arithmetic it replaces.  The
 * Python host (viddet_amd/) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - every function returns int: 0 = ok, <0 = VD_E* ; vd_last_error() gives a thread-local text.
 *  - the library never allocates or frees device memory: every buffer (incl. workspaces) is
 *    owned by the caller; pointers are raw device addresses.
 *  - `stream` is a hipStream_t passed as void*; ordering is by stream only; calls are
 *    asynchronous and re-entrant.
 *  - ONE device per process (the design is one process per GPU): the library caches the device
 *    address of its resident zero pages and its kernels' dynamic-LDS attributes in process-wide statics the first time
 *    an entry point runs; a process that drove a second device through it would read the first device's addresses.
 *  - activations are NHWC fp32 (bf16 where stated); conv weights arrive in the reference's OIHW
 *    layout and are re-packed by vd_pack_* into the K-contiguous layouts the kernels read.
 */
#ifndef VIDDET_HIP_H
#define VIDDET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VD_OK            0
#define VD_EINVAL       -1   /* bad argument / unsupported shape */
#define VD_ELAUNCH      -2   /* hip launch error */
#define VD_EWORKSPACE   -3   /* workspace too small */

#define VD_MAX_TAPS 27

/* epilogue flags of vd_conv_igemm */
#define VD_EPI_AFFINE    1   /* v = v*scale[c] + shift[c]   (BN-eval fold, or bias with scale==NULL) */
#define VD_EPI_LEAKY     2   /* v = v>0 ? v : slope*v */
#define VD_EPI_RESIDUAL  4   /* v += residual[m][c]  (after the activation) */
/* Arithmetic of the fp32 products (vd_conv_desc.flags / vd_wgrad_desc.flags).  Default: v_mfma_f32_32x32x2_f32, an
 * exact fp32 fma chain.  VD_MATH_SPLIT: each fp32 operand is split exactly into three bf16 pieces (24 significand
 * bits) and six of the nine partial products are accumulated in fp32 on the bf16 matrix pipe; the dropped terms are
 * below 2^-23 of the product (one fp32 rounding).  Storage, accumulation and the epilogue stay fp32. */
#define VD_MATH_SPLIT    16
/* VD_MATH_BF16: products on bf16-ROUNDED operands (only the leading piece of the split: one bf16 MFMA per product
 * block), fp32 tensors / accumulation / epilogues unchanged - the mixed-precision training arithmetic of BASELINE
 * configs[4]; results are bf16-accurate (2^-8 per operand), NOT fp32-accurate.  Same kernels and tiles as VD_MATH_SPLIT. */
#define VD_MATH_BF16     32

/* VD_MATH_F16X2: each fp32 operand x is scaled by a per-tensor power of two s (exact) and split into two fp16 pieces,
 * h = fp16(x*s), l = fp16(x*s - h) (round-to-nearest): 22-23 significand bits, |x*s - h - l| <= 2^-23 |x*s|.  A product is
 * accumulated in fp32 from THREE partial products al*bh, ah*bl, ah*bh on the f16 matrix pipe (the dropped al*bl is below
 * 2^-22 of the product) - half the matrix-pipe work of VD_MATH_SPLIT - and the epilogue multiplies by the inverse powers
 * of two (exact).  The scale puts the tensor's max-abs in [2^14, 2^15): every element within 2^19 of it keeps full
 * precision, smaller ones degrade gracefully towards an absolute floor of 2^-40 of the max.  The max-abs values are
 * read from device memory (vd_conv_desc.amax_in / amax_w, vd_wgrad_desc.amax_in / amax_dout): VD_AMAX_SLOTS sub-slots,
 * VD_AMAX_STRIDE floats apart, written by the producing kernels (atomic max; the caller zeroes them before the producer
 * runs) or by vd_amax / vd_amax_segments.  Measured against fp64 the error is not above the fp32 MFMA's. */
#define VD_MATH_F16X2    64
/* with VD_MATH_F16X2: keep the generic K loop where the library would stage the activation operand as a pixel halo tile
 * (3x3 stride-1 convs and their data gradients; vd_conv.hip, HALO) - for A/B timing by the host autotuner */
#define VD_MATH_NOHALO   128
/* VD_STORE_BF16 (vd_wgrad_desc.flags): `in` and `dout` are bf16 tensors (bf16-storage training, BASELINE configs[4]): the
 * products are the one-term bf16 MFMA of VD_MATH_BF16 on operands that are ALREADY bf16, the weight gradient stays fp32.
 * The forward / data-gradient convs of that mode are vd_conv_igemm_bf16. */
#define VD_STORE_BF16    256
/* VD_WGRAD_HALO (vd_wgrad_desc.flags, with VD_MATH_F16X2 or VD_STORE_BF16): where the launch is a 3x3 / stride-1 / 'same'
 * weight gradient with Co >= 128, a workgroup owns BM output channels x (9 taps x 32 input channels) and stages the
 * activation rows ONCE per pixel in a sliding LDS ring that the nine taps read at shifted rows (vd_wgrad_halo.hip), instead
 * of gathering the activation tile once per tap.  Same arithmetic, slabs and reduction; other geometries ignore the flag. */
#define VD_WGRAD_HALO    512
/* VD_CONV_STREAMK (vd_conv_desc.flags, with VD_MATH_F16X2): run the launch as a PERSISTENT stream-K grid - one workgroup
 * per CU slot, each owning an equal contiguous run of (tile, K-unit) units instead of whole tiles, so the launch ends
 * together on every CU whatever the tile count (vd_conv_sk.hip).  A tile cut by a run boundary is finished by the next
 * workgroup FROM the first one's accumulators (handed over through sk_ws), i.e. the same MFMA chain in the same order:
 * results are bit-identical to the launch without the flag.  Needs vd_conv_desc.sk_ws / sk_ws_bytes; where the form does
 * not apply (too few tiles, workspace too small, another arithmetic) the flag is ignored.  vd_conv_igemm_streamk(d) tells. */
#define VD_CONV_STREAMK  1024
/* VD_CONV_PARITY4 (vd_conv_desc.flags, with VD_MATH_F16X2): the data gradient of a 3x3 / stride-2 / pad-1 convolution as
 * ONE launch instead of four parity launches.  `in` = the incoming gradient dz [N, Hi, Wi, Ci = Cout], Hg = Hi, Wg = Wi,
 * in_stride 1, T = 4 taps with (dy, dx) = (0,0), (0,1), (1,0), (1,1); Co = 4 * par_cin GEMM columns = (parity class c,
 * channel), `wp` packed by vd_pack_weight_dgrad_s2; out = dx [N, Ho = 2 Hi, Wo = 2 Wi, ldo >= par_cin], out_stride 2: row q,
 * class c goes to pixel (2 qy + (c >> 1), 2 qx + (c & 1)).  Epilogue: residual (accumulate) and the fused BatchNorm-backward
 * reductions (bs_*: one table row [2 par_cin] per (M tile, column tile): vd_conv_igemm_mtiles() rows, the caller zeroes
 * the table first); no affine / LeakyReLU / statistics.  par_mask: bit (4 * tap + class) set where that weight block is
 * nonzero (vd_pack_weight_dgrad_s2 returns it).  Replaces autograd's backward of nn.Conv2D(strides=2),
 * three_darknet.py:182-183. */
#define VD_CONV_PARITY4  2048
/* vd_conv_igemm_bf16 only: SPLIT-K for launches whose tiles cannot fill the chip (batch-1 detection: 24 tiles of 128 x 128
 * at 19 x 19).  Each tile is cut along K into 2..8 parts run by as many workgroups; every part publishes its raw
 * accumulators in `sk_ws` (the stream-K workspace and hand-off protocol) and the part that arrives LAST sums them in part
 * order and runs the epilogue - nobody waits.  Deterministic, but another association than the one-tile launch (stream-K
 * proper is bit-identical to it), so it is its own flag: the host sets it for inference plans only.  Ignored where the
 * launch has tiles enough, where fewer than 4 K-steps per part would be left, or with the fused backward reductions. */
#define VD_CONV_SPLITK   4096
#define VD_SK_MAX_WG        2048     /* seam counters per workspace (the last one counts the polls that gave up: diagnostics) */
#define VD_SK_HEADER_BYTES  32768    /* [VD_SK_MAX_WG] u32 hand-off counters + [VD_SK_MAX_WG] u32 consumed counts + [VD_SK_SPLIT_MAX_TILES] u32 arrivals */
#define VD_SK_SPLIT_CNT_OFF   4096   /* (u32 words) the split-K form's per-tile arrival counters: zero between launches */
#define VD_SK_SPLIT_MAX_TILES 4096
#define VD_SK_TIMEOUT_TICKS 4000     /* bound of the hand-off poll in 10 ns ticks, after which the consumer recomputes */
#define VD_AMAX_SLOTS    32
#define VD_AMAX_STRIDE   64   /* floats between sub-slots (256 B) */
#define VD_AMAX_FLOATS   (VD_AMAX_SLOTS * VD_AMAX_STRIDE)   /* floats per tensor */

const char* vd_last_error(void);
int vd_version(void);
/* The ABI's revision: bumped whenever an entry point's argument list or a descriptor's layout changes (round 2 added the
 * amax_out / dhead_amax pointers in front of ws / stream and grew both descriptors: a caller built against the older
 * header would have passed its stream handle as amax_out).  A binding checks vd_abi_version() == VD_ABI_VERSION and
 * vd_sizeof_desc(i) == sizeof(its mirror of the descriptor) at load, before the first compute call: viddet_amd/lib.py
 * does, INTEGRATION.md shows it.  i: 0 = vd_conv_desc, 1 = vd_wgrad_desc, 2 = vd_head_desc; unknown i -> -1. */
#define VD_ABI_VERSION 8
int vd_abi_version(void);
int64_t vd_sizeof_desc(int which);

/* ---------------------------------------------------------------------------------------
 * Generic tap-list implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 *
 *   out[n, gy*os+oy, gx*os+ox, co] = epi( sum_{t<T} sum_{ci<Ci}
 *          in[n, gy*is+dy[t], gx*is+dx[t], ci] * wp[co][t*Ci + ci] )        (zero outside the image)
 *
 * One kernel serves: forward 1x1/3x3 s1/s2 (layers.py:66-67 nn.Conv2D inside _conv2d;
 * yolo3.py:62 prediction conv), the 3-tap / 27-tap temporal convs (layers.py:73-89), and the
 * data gradient of all of them (autograd.backward, train_yolov3.py:631) through flipped /
 * parity-split tap lists built by the host.
 * Requirements: Ci % 32 == 0; in/out 16-byte aligned; ldo >= Co (output pixel pitch in floats).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* in;        /* [N, Hi, Wi, Ci] */
    const float* wp;        /* [Co][T*Ci] packed, k contiguous */
    float*       out;       /* [N, Ho, Wo, ldo] */
    const float* scale;     /* [Co] or NULL */
    const float* shift;     /* [Co] or NULL */
    const float* residual;  /* same geometry as out, pitch ldr, or NULL */
    int32_t N, Hi, Wi, Ci;
    int32_t Hg, Wg;         /* GEMM row grid per image */
    int32_t in_stride;      /* is */
    int32_t T;
    int32_t dy[VD_MAX_TAPS], dx[VD_MAX_TAPS];
    int32_t dz[VD_MAX_TAPS];/* temporal tap offset (frames); 0 for 2-D convs */
    int32_t Kfr;            /* frames per window for temporal convs (N = windows*Kfr); 1 otherwise */
    int32_t Ho, Wo, Co;
    int32_t out_stride, out_oy, out_ox;
    int32_t ldo, ldr;
    int32_t flags;
    float   slope;
    /* in-load transform: the A operand is leaky(in*in_scale[ci]+in_shift[ci]) when in_scale!=NULL
     * (fuses the producer's BatchNorm+LeakyReLU into this conv's gather; padding stays 0) */
    const float* in_scale;
    const float* in_shift;
    float   in_slope;
    int32_t tile;           /* 0 = library heuristic; 1..8 (fp32 MFMA) / 1..16 (split arithmetics) = explicit tile variant (host autotuner) */
    /* fused BatchNorm statistics (training forward, flags must be 0): per-M-tile partial sums
     * stats_part[tile_m][0..Co) = sum, [Co..2Co) = sum of squares; vd_conv_igemm_mtiles() rows;
     * finish with vd_bn_sum_partials().  NULL = off. */
    float*  stats_part;
    /* fused BatchNorm BACKWARD reductions (training; this launch is the data-gradient conv that writes the final
     * gradient dy of a BatchNorm+LeakyReLU output, direct geometry: out_stride 1, Ho==Hg, Wo==Wg).  With
     * g = dy * leaky'(z*bs_scale+bs_shift) and xhat = (z - bs_mean)*bs_invstd, the epilogue adds the per-M-tile
     * partial sums  bs_part[tile_m][0..Co) = sum g,  [Co..2Co) = sum g*xhat  (rows as vd_conv_igemm_mtiles());
     * bs_z is that layer's pre-BN conv output, laid out like `out` (pitch ldo).  Finish with
     * vd_bn_sum_partials(); replaces vd_bn_bwd_reduce.  bs_part NULL = off. */
    const float* bs_z;
    const float* bs_scale;
    const float* bs_shift;
    const float* bs_mean;
    const float* bs_invstd;
    float*  bs_part;
    float   bs_slope;
    /* VD_MATH_F16X2: max-abs slots (VD_AMAX_FLOATS floats each) of `in` and of `wp`; required with that flag */
    const float* amax_in;
    const float* amax_w;
    /* optional, any arithmetic: the epilogue publishes the max-abs of what it stores (zeroed by the caller) */
    float*  amax_out;
    /* VD_CONV_STREAMK: hand-off workspace, vd_conv_igemm_streamk_ws_bytes() bytes.  The caller zeroes its first
     * VD_SK_HEADER_BYTES ONCE, when it allocates it (the counters are monotonic across launches), and never shares one
     * workspace between launches that may run at the same time (one per stream).  VD_CONV_SPLITK uses the same workspace
     * (its per-tile arrival counters are zero between launches). */
    void*   sk_ws;
    int64_t sk_ws_bytes;
    /* VD_CONV_PARITY4: channels per parity class, nonzero (tap, class) weight blocks */
    int32_t par_cin;
    int32_t par_mask;
} vd_conv_desc;

int vd_conv_igemm(const vd_conv_desc* d, void* stream);
/* 1 when vd_conv_igemm(d) would run as a persistent stream-K grid (flag set, arithmetic / tile / tile count it serves and
 * a large enough workspace), else 0: for host autotuners and tests. */
int vd_conv_igemm_streamk(const vd_conv_desc* d);
/* bytes of a stream-K workspace that serves every launch shape (header + one fp32 accumulator tile per CU slot) */
int64_t vd_conv_igemm_streamk_ws_bytes(void);
/* number of M tiles (rows of stats_part) the launch described by d will use */
int vd_conv_igemm_mtiles(const vd_conv_desc* d);

/* bf16 variant of vd_conv_igemm for inference (BASELINE configs[1] asks for bf16; the reference is fp32-only):
 * in / wp / residual are bf16 (NHWC with Ci % 64 == 0, or Ci == 32 unpadded: a K-step then holds two taps;
 * weights [Co][T*Ci]), accumulation and epilogue fp32,
 * out is bf16 (out_f32 = 0) or fp32 (out_f32 = 1: prediction heads, shared decode / NMS kernels).
 * Any output geometry of vd_conv_igemm (the strided / offset outputs of the stride-2 data gradients included) and, for
 * bf16-storage training, d->stats_part: the fused BatchNorm statistics of the raw outputs, taken from the fp32
 * accumulators before they are rounded to bf16 - [vd_conv_igemm_bf16_mtiles(d)][2 * Co] floats, as vd_conv_igemm writes
 * them.  d->tile: 0 = default, 1..13 = tile variant (256x256 .. 128x64; the host autotunes it). */
int vd_conv_igemm_bf16(const vd_conv_desc* d, int out_f32, void* stream);
/* VD_CONV_STREAMK in d->flags (with sk_ws / sk_ws_bytes) runs the launch as a persistent stream-K grid where that form
 * applies (bf16 outputs, Ci % 64 == 0, enough tiles: as vd_conv_igemm), VD_CONV_SPLITK as a split-K grid where THAT
 * applies (too few tiles for the chip).  Returns 1 when vd_conv_igemm_bf16(d, out_f32) would run the stream-K form, 2 when
 * it would run the split-K form, 0 when it would launch one workgroup per tile. */
int vd_conv_igemm_bf16_streamk(const vd_conv_desc* d, int out_f32);
int vd_conv_igemm_bf16_mtiles(const vd_conv_desc* d);
/* fp32 fwd-packed [>=Co][T*Ci] -> bf16 [Co_pad][T*Ci_pad] (zero padded rows / channels) */
int vd_pack_weight_bf16(const float* wp_f32, void* wp_bf16, int Co, int Co_pad, int Ci, int Ci_pad, int T,
                        void* stream);
/* stem im2col into 64 bf16 columns per pixel (27 real), from [N,H,W,3] (nchw=0) or [N,3,H,W] (nchw=1) fp32.
 * Off the product path since vd_stem_conv (direct stem kernel): kept as the explicit lowering the tests compare with. */
int vd_stem_im2col_bf16(const float* in, void* col, int N, int H, int W, int nchw, void* stream);

/* Weight gradient (autograd.backward wrt nn.Conv2D weight, train_yolov3.py:631):
 *   dwp[co][t*Ci+ci] = sum_{n,gy,gx} dout[n,gy,gx,co] * in[n, gy*is+dy[t], gx*is+dx[t], ci]
 * split over `splits` pixel ranges into workspace slabs, then reduced deterministically.
 * ws must hold vd_conv_wgrad_ws_bytes() bytes. */
typedef struct {
    const float* in;        /* [N, Hi, Wi, Ci] */
    const float* dout;      /* [N, Hg, Wg, ldd] */
    float*       dwp;       /* [Co][T*Ci] */
    int32_t N, Hi, Wi, Ci;
    int32_t Hg, Wg, Co, ldd;
    int32_t in_stride;
    int32_t T;
    int32_t dy[VD_MAX_TAPS], dx[VD_MAX_TAPS];
    int32_t dz[VD_MAX_TAPS];
    int32_t Kfr;
    int32_t splits;         /* 0 = choose */
    const float* in_scale;  /* optional in-load transform as in vd_conv_desc */
    const float* in_shift;
    float   in_slope;
    int32_t flags;          /* VD_MATH_SPLIT / VD_MATH_F16X2: split-operand products (Co >= 64; narrower layers stay on the fp32 MFMA) */
    const float* amax_in;   /* VD_MATH_F16X2: max-abs slots of `in` and of `dout` */
    const float* amax_dout;
} vd_wgrad_desc;

int64_t vd_conv_wgrad_ws_bytes(const vd_wgrad_desc* d);
int vd_conv_wgrad(const vd_wgrad_desc* d, void* ws, int64_t ws_bytes, void* stream);
/* 1 when vd_conv_wgrad(d) would run the halo-ring kernel (VD_WGRAD_HALO set and the geometry / arithmetic is one it
 * serves), else 0: for host autotuners (no point timing the flag where it is ignored) and tests. */
int vd_conv_wgrad_uses_halo(const vd_wgrad_desc* d);

/* Direct stem convolution (3x3, 3 -> 32 channels, stride 1, pad 1; three_darknet.py:163-164) straight from the NCHW
 * fp32 frame batch (transforms.py:239-245): no im2col round trip.  wp is the fwd-packed stem weight [32][32]
 * (k = (ky*3+kx)*3 + c, k >= 27 zero).  out: NHWC [N,H,W,ldo >= 32] (32 channels written per pixel; a wider pitch
 * leaves the pad channels alone) fp32, or bf16 when out_bf16; flags = VD_EPI_AFFINE /
 * VD_EPI_LEAKY (BN-eval fold + LeakyReLU); stats_part (flags 0, fp32 out): per-block BatchNorm partial sums
 * [vd_stem_conv_blocks()][2*32], finish with vd_bn_sum_partials(). */
/* bf16 inference: the stem and the stride-2 conv behind it (three_darknet.py:163-164 + :182-183) in ONE launch of the
 * first-stage patch kernel (vd_conv_c32_bf16.hip): `d` describes the 3x3 / stride-2 / 32 -> 64 channel conv as for
 * vd_conv_igemm_bf16 (N, Hi = H, Wi = W of the frames; folded BatchNorm + LeakyReLU epilogue, bf16 output; d->in is not
 * read), the stem's 32-channel map is computed inside the kernel from the fp32 NCHW frames and never stored.  Outputs are
 * bit-identical to vd_stem_conv(..., VD_EPI_AFFINE | VD_EPI_LEAKY, out_bf16 = 1) followed by vd_conv_igemm_bf16 with tile
 * 16.  VD_EINVAL where the descriptor is not that conv. */
int vd_stem_conv_c32_bf16(const float* x_nchw, const float* stem_wp, const float* stem_scale, const float* stem_shift,
                          float stem_slope, const vd_conv_desc* d, void* stream);
int vd_stem_conv_blocks(int N, int H, int W);
int vd_stem_conv(const float* x_nchw, const float* wp, void* out, int ldo, int N, int H, int W, const float* scale,
                 const float* shift, float slope, int flags, int out_bf16, float* stats_part, void* stream);
/* Weight gradient of the stem from the same NCHW batch and the gradient dz [N*H*W][ldd >= 32] of its output:
 * dwp [32][32] in the fwd-packed layout (columns >= 27 come out zero). */
int64_t vd_stem_wgrad_ws_bytes(int N, int H, int W);
int vd_stem_wgrad(const float* x_nchw, const float* dz, int ldd, float* dwp, int N, int H, int W, void* ws,
                  int64_t ws_bytes, void* stream);
/* The same weight gradient without a stored dz: every element of dz is computed where vd_stem_wgrad loads it, from the
 * stem's conv output z [N*H*W][ldz >= 32], the gradient dy [N*H*W][ldy >= 32] of its cell's output and the per-channel
 * operands of vd_bn_bwd_apply (scale, shift, save_mean, save_invstd [32], sums2 fp64 [64], count, slope), in that
 * kernel's arithmetic.  dwp is bit-identical to vd_bn_bwd_apply into a buffer followed by vd_stem_wgrad on it; same
 * workspace (vd_stem_wgrad_ws_bytes). */
int vd_stem_wgrad_bn(const float* x_nchw, const float* z, int ldz, const float* dy, int ldy, const float* scale,
                     const float* shift, const float* save_mean, const float* save_invstd, const double* sums2, double count,
                     float slope, float* dwp, int N, int H, int W, void* ws, int64_t ws_bytes, void* stream);
/* Stem conv 3->32 3x3 s1 p1 (three_darknet.py:163-164): Ci=3 is too thin for the GEMM path, so
 * the stem is lowered to an explicit 32-wide im2col ( col[n,y,x,(ky*3+kx)*3+c], entries 27..31
 * zero ) followed by vd_conv_igemm / vd_conv_wgrad with T=1, Ci=32.  `in` is [N,H,W,3] (nchw=0)
 * or the reference's [N,3,H,W] batch layout (nchw=1, transforms.py:239-245). */
int vd_stem_im2col(const float* in, float* col, int N, int H, int W, int nchw, void* stream);

/* OIHW -> packed [Co_pad][T*Ci] (forward) ; rows >= Co are zero.  kd = temporal kernel depth (1 for 2-D). */
int vd_pack_weight_fwd(const float* w_oihw, float* wp, int Co, int Co_pad, int Ci,
                       int kd, int kh, int kw, void* stream);
/* OIHW -> dgrad pack [Ci][T'*Co_pad] for the tap subset `taps` (indices into kd*kh*kw, already
 * in the order the dgrad tap list uses; HOST pointer).  src_packed=1: w is already in the
 * forward-packed layout [Co][T*Ci] (the layout the parameter arena keeps) instead of OIHW. */
int vd_pack_weight_dgrad(const float* w_oihw, float* wp, int Co, int Co_pad, int Ci,
                         int kd, int kh, int kw, const int32_t* taps, int ntaps, int src_packed,
                         void* stream);
/* VD_CONV_PARITY4 weight image from the fwd-packed weights [Co][9 * Ci] of a 3x3 conv: wp4 [4 * Ci][4 * Co_pad],
 * wp4[(c * Ci + ci)][o * Co_pad + co] = w[co][ci][ky][kx] for the kernel tap (ky, kx) that output parity class c = 2 py + px
 * reaches at gradient offset o = 2 dy + dx (py = 0: ky = 1 at dy = 0; py = 1: ky = 2 at dy = 0, ky = 0 at dy = 1; likewise
 * px / kx / dx), zero where there is none.  Returns the 16-bit block mask through *par_mask (host pointer; a constant). */
int vd_pack_weight_dgrad_s2(const float* wp_fwd, float* wp4, int Co, int Co_pad, int Ci, int32_t* par_mask, void* stream);
/* packed gradient [Co_pad][T*Ci] -> OIHW [Co][Ci][kd][kh][kw] (accumulate=0 overwrites) */
int vd_unpack_wgrad(const float* dwp, float* dw_oihw, int Co, int Ci, int kd, int kh, int kw,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * BatchNorm (layers.py:68 norm_layer(epsilon=1e-5, momentum=0.9)) + LeakyReLU(0.1) (layers.py:69)
 * on NHWC [M, C] (M = N*H*W).
 * ------------------------------------------------------------------------------------- */
/* partial sums: sums[0..C) = sum x, sums[C..2C) = sum x^2 (fp64 accumulators, deterministic) */
int64_t vd_bn_stats_ws_bytes(int64_t M, int C);
int vd_bn_stats(const float* x, int64_t M, int C, double* sums, void* ws, int64_t ws_bytes,
                void* stream);
/* fp64 reduction of a partial table part[nblk][2C] (vd_conv_igemm stats_part) into sums[2C] */
int64_t vd_bn_sum_partials_ws_bytes(int nblk, int C);
int vd_bn_sum_partials(const float* part, int nblk, int C, double* sums, void* ws, int64_t ws_bytes, void* stream);
/* The same reduction fused with what follows it (one launch for tables of up to 1024 rows, else the calls above):
 * forward  = vd_bn_sum_partials + vd_bn_finalize;  backward = vd_bn_sum_partials + vd_bn_param_grads.  The fp64 sums
 * are written as well.  (With SyncBN the unfused calls are used: the all-reduce sits between the two halves.) */
int vd_bn_sum_finalize(const float* part, int nblk, int C, double* sums, double count, const float* gamma,
                       const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                       float* scale, float* shift, float* save_mean, float* save_invstd, void* ws, int64_t ws_bytes,
                       void* stream);
int vd_bn_sum_param_grads(const float* part, int nblk, int C, double* sums2, float* dgamma, float* dbeta, void* ws,
                          int64_t ws_bytes, void* stream);
/* from (possibly all-reduced) sums and total count: mean, biased var -> scale/shift for the
 * apply, saved mean/invstd for backward, running-stat update run = mom*run + (1-mom)*batch */
int vd_bn_finalize(const double* sums, double count, int C, const float* gamma, const float* beta,
                   float eps, float momentum, float* running_mean, float* running_var,
                   float* scale, float* shift, float* save_mean, float* save_invstd, void* stream);
/* eval: scale/shift from running stats */
int vd_bn_fold_eval(const float* gamma, const float* beta, const float* running_mean,
                    const float* running_var, float eps, int C, float* scale, float* shift,
                    void* stream);
/* y = leaky(x*scale+shift) (+ residual); amax_out (optional): max-abs slots of y (VD_AMAX_FLOATS floats, zeroed by the
 * caller) for the fp16 operand scale of the convs that read y (VD_MATH_F16X2) */
int vd_bn_apply_leaky(const float* x, const float* scale, const float* shift, const float* residual,
                      float* y, int64_t M, int C, float slope, float* amax_out, void* stream);
/* Launch geometry of vd_bn_apply_leaky / vd_bn_bwd_apply (and their _bf16 forms) over n_vec vectors of 4 (or, for 16-byte
 * aligned bf16 tensors with C % 8 == 0, 8) channels in cvec vector columns: the number of 256-thread blocks, and in *unroll
 * (optional) the vectors U a thread handles.  A group of cvec / gcd(256, cvec) blocks owns one contiguous run of U * 256
 * vectors per block; the grid is one group per run.  For tests and tools: results never depend on it. */
int vd_bn_stream_grid(int64_t n_vec, int cvec, int* unroll);
/* backward, pass 1: partial sums of g=dy*leaky'(.) and g*xhat -> sums2[0..C)=sum g, [C..2C)=sum g*xhat */
int vd_bn_bwd_reduce(const float* x, const float* dy, const float* scale, const float* shift,
                     const float* save_mean, const float* save_invstd, int64_t M, int C, float slope,
                     double* sums2, void* ws, int64_t ws_bytes, void* stream);
/* dgamma[c] = sum g*xhat, dbeta[c] = sum g from the LOCAL sums2 (before any SyncBN all-reduce) */
int vd_bn_param_grads(const double* sums2, int C, float* dgamma, float* dbeta, void* stream);
/* backward, pass 2: dx = scale*(g - mean_g - xhat*mean_gx), means from (all-reduced) sums2 / count */
int vd_bn_bwd_apply(const float* x, const float* dy, const float* scale, const float* shift,
                    const float* save_mean, const float* save_invstd,
                    const double* sums2, double count, int64_t M, int C, float slope,
                    float* dx, float* amax_out /* optional, as in vd_bn_apply_leaky */, void* stream);

/* Operand-range guard of VD_MATH_F16X2.  That arithmetic scales a whole tensor by ONE power of two; elements more than
 * ~2^18 below the tensor's max-abs are staged with fewer than 22 significant bits.  Dense tensors (activations, gradients
 * behind a BatchNorm backward) only get there through their per-channel scales, which are known from the layer's vectors:
 * per BatchNorm layer i, ratios[2i] = min_c / max_c of (|gamma_c| + |beta_c|) (the cell's output y), ratios[2i+1] the same
 * of |scale_c| (= gamma_c * invstd_c: the gradient dz the layer's backward writes; scale may be NULL: ratio 1), and
 * flags[2i+k] = ratios[2i+k] < thresh.  `items` is a DEVICE array.  The host reads the flags when it synchronises anyway
 * and rebuilds the plans of flagged tensors' consumers in VD_MATH_SPLIT, whose bf16 pieces have fp32's exponent range
 * (viddet_amd/model.py check_operand_ranges).  Sparse saturated tensors - the loss gradient - never run in VD_MATH_F16X2. */
typedef struct {
    const float* gamma;
    const float* beta;
    const float* scale;     /* gamma * invstd of the last training forward, or NULL */
    int32_t C;
    int32_t pad_;
} vd_guard_item;
int vd_range_guard(const vd_guard_item* items, int n, float thresh, float* ratios, int32_t* flags, void* stream);

/* out[slot] = max(a[slot], b[slot]) over the sub-slots (b may be NULL: copy): the max-abs of a tensor assembled from, or
 * bounded by, other tensors (upsample+concat, temporal pooling / stacking) without another pass over it */
int vd_amax_merge(const float* a, const float* b, float* out, void* stream);
/* max-abs of a tensor into its slots (zeroes them first): amax[VD_AMAX_FLOATS] */
int vd_amax(const float* x, int64_t n, float* amax, void* stream);
/* the same for `nseg` ranges of one buffer in ONE launch (the conv weights of the parameter arena, once per optimiser
 * step): seg is a DEVICE array [nseg][2] = (element offset, element count); amax [nseg][VD_AMAX_FLOATS] */
int vd_amax_segments(const float* base, const int64_t* seg, int nseg, float* amax, void* stream);

/* ---------------------------------------------------------------------------------------
 * Pointwise helpers
 * ------------------------------------------------------------------------------------- */
/* out = a + b (residual backward fan-in etc.) */
int vd_add(const float* a, const float* b, float* out, int64_t n, void* stream);
int vd_fill(float* out, float v, int64_t n, void* stream);
/* layers.py:11-20 _upsample (nearest x2) + yolo3.py:1170-1177 slice_like + concat(dim=1):
 * out[n, y, x, 0:Cu) = up[n, y/2, x/2, :], out[..., Cu:Cu+Cr) = route[n, y, x, :] */
int vd_upsample2x_concat(const float* up, const float* route, float* out,
                         int N, int Ho, int Wo, int Cu, int Cr, void* stream);
/* backward: dup[n,y2,x2,:] = sum of the 4 children of dout[..., 0:Cu); droute = dout[..., Cu:).  Either output may be
 * NULL (that gradient is not needed: every parameter upstream of it has grad_req 'null', wrappers.py:55-57). */
int vd_upsample2x_concat_bwd(const float* dout, float* dup, float* droute,
                             int N, int Ho, int Wo, int Cu, int Cr, void* stream);
/* NCHW fp32 -> NHWC fp32 (the reference feeds NCHW, transforms.py:239-245) */
int vd_nchw_to_nhwc(const float* in, float* out, int N, int C, int H, int W, void* stream);
/* transforms.py:229-245: uint8 HWC -> /255 -> (x-mean)/std, NHWC fp32 */
int vd_preprocess_u8_nhwc(const uint8_t* in, float* out, int64_t npix, void* stream);
/* the same arithmetic from uint8 NHWC frames [N,H,W,3] into the planar fp32 batch [N,3,H,W] the network takes
 * (transforms.py:239-245 to_tensor + normalize): loaders ship uint8, a quarter of the bytes */
int vd_preprocess_u8_nchw(const uint8_t* in, float* out, int N, int H, int W, void* stream);
/* layers.py:161-205 TemporalPooling over K frames: x [B,K,HW*C] -> y [B,HW*C]; type 0=max 1=mean */
int vd_temporal_pool(const float* x, float* y, int32_t* argmax, int B, int K, int64_t inner, int type,
                     void* stream);
int vd_temporal_pool_bwd(const float* dy, const int32_t* argmax, float* dx, int B, int K,
                         int64_t inner, int type, void* stream);
/* x.slice_axis(axis=1, begin=k0, end=k0+kc) on folded frames (yolo3_temporal.py:437-446): x [B*K, inner] -> y [B*kc, inner];
 * backward=1 is its gradient (x = dy [B*kc, inner], y = dx [B*K, inner], zero outside the range).  Also how the un-padded
 * temporal convs of _conv21d(padding=[1,0]) (:329-332) are taken out of the 'same'-padded ones: frames [1, K-1). */
int vd_frame_slice(const float* x, float* y, int B, int K, int k0, int kc, int64_t inner, int backward, void* stream);
/* 'cat' join (yolo3.py:1108,1136 reshape (B,K,C,h,w)->(B,K*C,h,w)): NHWC [B*K,hw,C] -> [B,hw,K*C];
 * backward=1 runs the inverse (x = stacked gradient, y = per-frame gradient) */
int vd_temporal_cat(const float* x, float* y, int B, int K, int64_t hw, int C, int backward, void* stream);
/* Correlation join (Corr(d, K, kernal_size=1, stride=1, keep='all'), layers.py:93-132): x [B*K, H, W, C] fp32 NHWC
 * (frame b*K + k) -> y [B, H, W, ldy], mid = K/2, D = 2d+1, Cc = K*C + (K-1)*D*D:
 *   y[b, p, k*C + c]                          = x[b*K + k, p, c]                              (the 'cat' join)
 *   y[b, p, K*C + tt*D*D + (dy+d)*D + (dx+d)] = (1/C) sum_c x[b*K+t, p, c] * x[b*K+mid, p + (dy, dx), c]
 *                                               for every t != mid (tt = t - (t > mid)); 0 where p + (dy, dx) leaves the map
 *   y[b, p, Cc .. ldy)                        = 0
 * i.e. mx.sym.Correlation(x_t, x_mid, kernel_size=1, max_displacement=d, pad_size=d, stride1=stride2=1, is_multiply=1),
 * whose divisor is kernel_size^2 * C.  Requires C % 32 == 0, 0 <= d <= 5, ldy >= Cc, ldy % 8 == 0.  One launch.
 * vd_corr_bwd: dx [B*K, H, W, C] from dy [B, H, W, ldy] and x, two gathers in a fixed order (bit-reproducible):
 *   dx[t != mid][p] = dy_cat[t][p] + (1/C) sum_disp dy_t[p, disp] * x_mid[p + disp]
 *   dx[mid][q]      = dy_cat[mid][q] + (1/C) sum_{t != mid} sum_disp dy_t[q - disp, disp] * x_t[q - disp]
 * vd_corr_fwd_bf16: the forward on bf16 tensors (fp32 sums, bf16 output). */
int vd_corr_fwd(const float* x, float* y, int B, int K, int H, int W, int C, int d, int ldy, void* stream);
int vd_corr_bwd(const float* dy, const float* x, float* dx, int B, int K, int H, int W, int C, int d, int ldy, void* stream);
int vd_corr_fwd_bf16(const void* x, void* y, int B, int K, int H, int W, int C, int d, int ldy, void* stream);

/* Bidirectional convolutional GRU over the K frames of a window (RNN(k, type='gru', bi=True), layers.py:267-306; the cell
 * restated from MXNet's Conv2DGRUCell): the gate arithmetic between the cell's convolutions, which are
 * vd_conv_igemm launches (i2h over all B*K folded frames, h2h on the B frames of one step, biases in the epilogue).
 * The 3*Ch channels of I and H are three blocks of Ch in the order r, z, o; fp32, Ch % 4 == 0, 16-byte aligned pointers.
 *   I      [B*K, HW, 3*Ch]  i2h output of the folded frames (frame b*K + t); the step reads frame t of every window
 *   H      [B*HW, 3*Ch]     h2h output of this step, or NULL: the state is zero and H is `hbias` [3*Ch] alone
 *   hprev  [B*HW, Ch]       the previous state, or NULL (zero)
 *   h      [B*HW, Ch]       r = sigmoid(I_r + H_r), z = sigmoid(I_z + H_z), n = tanh(I_o + r * H_o), h = (1 - z) n + z hprev
 * Nothing else is kept for backward: vd_gru_gate_bwd recomputes r, z, n from I and H (h_valid = 0: from hbias) and
 * overwrites them IN PLACE with  dI = [dr', dz', da]  and  dH = [dr', dz', da * r]  (H is written at a first step too: its
 * column sums are the h2h bias gradient), where  dh = dy_scale * dy[frame t] + (carry ? dh : 0),  dn = dh (1 - z),
 * dz = dh (hprev - n), da = dn (1 - n^2), dr = da H_o, dr' = dr r (1 - r), dz' = dz z (1 - z); with a previous state it
 * also writes  dh <- dh * z, to which the h2h data gradient is then added (VD_EPI_RESIDUAL).  dy [B*K, HW, Ch] is the folded
 * gradient of the layer output y; dy_scale = 1/2 is the backward of the bidirectional average.
 * vd_gru_avg: y[b*K + t] = (hl[t][b] + hr[K-1-t][b]) / 2 from the two directions' STEP-major states [K][B][inner] (step s
 * of the reverse direction is frame K-1-s) into the folded output; amax_out (optional) as in vd_bn_apply_leaky. */
int vd_gru_gate_fwd(const float* I, const float* H, const float* hbias, const float* hprev, float* h, int B, int K, int t,
                    int64_t HW, int Ch, void* stream);
int vd_gru_gate_bwd(float* I, float* H, int h_valid, const float* hbias, const float* hprev, const float* dy, float dy_scale,
                    float* dh, int carry, int B, int K, int t, int64_t HW, int Ch, void* stream);
int vd_gru_avg(const float* hl, const float* hr, float* y, int B, int K, int64_t inner, float* amax_out, void* stream);

/* Temporal half of the BACKBONE's R(2+1)D cell (--conv_types 21; Conv3DRepPad, darknet/three_darknet.py:19-70):
 * a depthwise (3,1,1) convolution over the K frames of a window with repeat padding, no bias, nothing behind it.
 *   x, y, res, dy, dx  [B*K, HW, C] fp32 NHWC rows, frames folded (frame b*K + t);  w, dw [C][3] = the reference's (C,1,3,1,1)
 *   y_t = w0 x_{max(t-1,0)} + w1 x_t + w2 x_{t+1 < K ? t+1 : K-2}  [+ res_t]
 * The tail pad is frame K-2 (slice_axis(begin=-2, end=-1), :62), not the last frame; hence K >= 2.  C % 4 == 0, 16-byte
 * aligned pointers.  res (optional) is the residual of DarknetBasicBlockV3 added in the same pass; amax_out (optional) as in
 * vd_bn_apply_leaky: the max-abs of y for the convolutions that read it.
 * vd_tdw_bwd: one launch reads dy (and x) once and writes dx (NULL = skipped) and one row of weight-gradient partial sums
 * per workgroup into ws; a second launch adds the rows in a fixed order in fp64 into dw (NULL = skipped, ws not needed).
 * Frame 0 of dx also collects w0 dy_0 and frame K-2 also collects w2 dy_{K-1}.  No atomics: bit-reproducible. */
int vd_tdw_fwd(const float* x, const float* w, const float* res, float* y, int B, int K, int64_t HW, int C, float* amax_out,
               void* stream);
int64_t vd_tdw_bwd_ws_bytes(int B, int K, int64_t HW, int C);
int vd_tdw_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, int B, int K, int64_t HW, int C, void* ws,
               int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * YOLO head: decode / filter / NMS / targets / loss
 * Head tensors are the raw prediction-conv outputs, NHWC [B, g, g, ldh], channel = a*(5+C)+j,
 * j: 0,1 = raw xy, 2,3 = raw wh, 4 = objectness, 5.. = classes (yolo3.py:158-165).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* head[3];   /* scale order = reference output order: stride 32, 16, 8 (yolo3.py:1013) */
    int32_t g[3];           /* grid side per scale */
    int32_t ldh;            /* channel pitch of head tensors */
    float   stride[3];
    float   anchors[3][6];  /* (w,h) x3 per scale, in reference output order */
    int32_t B, C;
} vd_head_desc;

/* Inference (yolo3.py:167-199 + 1195-1206): fused decode + valid_thresh filter.
 * Emits per image a candidate list of (score, row) where row is the row index into the
 * (B, C*P, 6) tensor the reference would materialise.  counts[b] = number emitted (may exceed
 * cap: then only the first cap are stored and vd_nms_topk reports overflow). */
int vd_yolo_decode_filter(const vd_head_desc* h, float valid_thresh,
                          float* cand_score, int32_t* cand_row, int32_t cap, int32_t* counts,
                          void* stream);
/* F.contrib.box_nms(overlap_thresh, topk, id_index=0, score_index=1, coord_start=2,
 * force_suppress=False) + slice_axis(0:post_nms)  (yolo3.py:1197-1202).
 * out_ids/out_scores [B,post_nms], out_boxes [B,post_nms,4], out_rows [B,post_nms] (original
 * row index of each kept detection, -1 padded).  ws >= vd_nms_ws_bytes. */
int64_t vd_nms_ws_bytes(int B, int cap, int topk);
int vd_nms_topk(const vd_head_desc* h, const float* cand_score, const int32_t* cand_row,
                int32_t cap, const int32_t* counts, float nms_thresh, int topk, int post_nms,
                float* out_ids, float* out_scores, float* out_boxes, int32_t* out_rows,
                void* ws, int64_t ws_bytes, void* stream);
/* Class-agnostic tail (YOLOOutputV3(agnostic=True), yolo3.py:184-188, + the same box_nms / slice_axis): ONE candidate per
 * (pixel, anchor), id 0, score = sigmoid(objectness) - the class channels are never read.  row indexes the (B, P, 6) tensor
 * the reference concatenates: [head][pixel][anchor], P = 3 * sum g[s]^2.  cap >= P cannot overflow (counts / the overflow
 * flags are kept for symmetry with the per-class pair).  head_bf16 != 0: h->head[s] point to bf16 tensors of the same
 * geometry (ldh counted in elements).  With a single id the NMS is plain NMS over the image: the set and the sweep order are
 * those of "sort by (score desc, row asc), take topk, greedy sweep"; out_ids are 0 for kept rows, -1 fill as vd_nms_topk.
 * No floating-point atomics; bit-identical from run to run. */
int vd_yolo_decode_filter_agnostic(const vd_head_desc* h, int head_bf16, float valid_thresh,
                                   float* cand_score, int32_t* cand_row, int32_t cap, int32_t* counts,
                                   void* stream);
int vd_nms_agnostic(const vd_head_desc* h, int head_bf16, const float* cand_score, const int32_t* cand_row,
                    int32_t cap, const int32_t* counts, float nms_thresh, int topk, int post_nms,
                    float* out_ids, float* out_scores, float* out_boxes, int32_t* out_rows,
                    void* ws, int64_t ws_bytes, void* stream);

/* Training (yolo3.py:1140-1187 + yolo_target.py:173-281 + gluoncv YOLOV3Loss):
 * fused decode -> dynamic ignore mask (IoU>thr vs gt) -> target merge -> 4 losses and their
 * gradient wrt the raw head outputs.  targets are the prefetched ones, (B,P,.) in reference row
 * order; gt [B,M,4] corner boxes padded with -1.  losses [B,4] = obj, center, scale, cls.
 * dhead[s] has the geometry of head[s] (pad channels get 0).  box_out (optional) [B,P,4]. */
int vd_yolo_loss_fwd_bwd(const vd_head_desc* h, const float* gt, int M,
                         const float* obj_t, const float* center_t, const float* scale_t,
                         const float* weight_t, const float* class_t,
                         float ignore_thresh, int label_smooth,
                         float* losses, float* const dhead[3], float* box_out,
                         float* const dhead_amax[3] /* optional: max-abs slots of the three gradients, zeroed by the caller */,
                         void* ws, int64_t ws_bytes, void* stream);
int64_t vd_yolo_loss_ws_bytes(const vd_head_desc* h);

/* ---------------------------------------------------------------------------------------
 * Optimiser (gluon.Trainer('sgd'), train_yolov3.py:527-530,634):
 *   g = rescale*grad ; mom = momentum*mom - lr*(g + wd*w) ; w += mom
 * over a flat parameter arena.
 * ------------------------------------------------------------------------------------- */
int vd_sgd_momentum(float* w, const float* grad, float* mom, int64_t n,
                    float lr, float momentum, float wd, float rescale, void* stream);

/* ---------------------------------------------------------------------------------------
 * bf16-STORAGE training (BASELINE configs[4]: "combined-dataset training ... bf16"; the reference is fp32-only,
 * train_yolov3.py:623-636, so this mode is judged against the fp32 oracle at a stated bf16 tolerance).
 * Activations (conv outputs z, cell outputs y) and their gradients (dy, dz) are bf16 NHWC tensors; weights (fp32 master +
 * bf16 images), weight gradients, BatchNorm vectors / statistics, the head logits, the losses and the optimiser stay fp32.
 *   convs fwd / dgrad      vd_conv_igemm_bf16 (stats_part; strided outputs)
 *   weight gradients       vd_conv_wgrad with VD_STORE_BF16 in vd_wgrad_desc.flags; vd_stem_wgrad_bf16
 *   BatchNorm passes       the entry points below: the fp32 kernels instantiated on bf16 tensors (fp32 arithmetic)
 *   concat                 vd_upsample2x_concat on half the channel counts (a copy); vd_upsample2x_concat_bwd_bf16
 *   loss                   vd_yolo_loss_fwd_bwd_bf16: fp32 logits in, bf16 gradient rows out
 * ------------------------------------------------------------------------------------- */
int vd_bn_stats_bf16(const void* x, int64_t M, int C, double* sums, void* ws, int64_t ws_bytes, void* stream);
int vd_bn_apply_leaky_bf16(const void* x, const float* scale, const float* shift, const void* residual, void* y,
                           int64_t M, int C, float slope, void* stream);
int vd_bn_bwd_reduce_bf16(const void* x, const void* dy, const float* scale, const float* shift, const float* save_mean,
                          const float* save_invstd, int64_t M, int C, float slope, double* sums2, void* ws, int64_t ws_bytes,
                          void* stream);
int vd_bn_bwd_apply_bf16(const void* x, const void* dy, const float* scale, const float* shift, const float* save_mean,
                         const float* save_invstd, const double* sums2, double count, int64_t M, int C, float slope,
                         void* dx, void* stream);
int vd_pack_weight_dgrad_bf16(const float* w, void* wp_bf16, int Co, int Co_pad, int Ci, int kd, int kh, int kw,
                              const int32_t* taps, int ntaps, int src_packed, void* stream);
int vd_add_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);
/* TemporalPooling (layers.py:161-205; type 0 = max, 1 = mean) over the K frames of a window on bf16 tensors: the bf16
 * inference of the k > 1 networks.  vd_frame_slice / vd_temporal_cat are copies: they take bf16 tensors with the inner /
 * channel counts halved (two bf16 = one 4-byte word). */
int vd_temporal_pool_bf16(const void* x, void* y, int B, int K, int64_t inner, int type, void* stream);
int vd_upsample2x_concat_bwd_bf16(const void* dout, void* dup, void* droute, int N, int Ho, int Wo, int Cu, int Cr, void* stream);
/* bf16-storage training of the k > 1 networks: the joins' training forward and backward on bf16 tensors.
 * vd_temporal_pool_train_bf16: the values of vd_temporal_pool_bf16; type 0 also records the winning frame in argmax_u8, ONE
 * byte per element (K < 128; NULL allowed for type 1).  Ties go to the lowest frame index (t > v, strictly: vd_temporal_pool's
 * rule).  vd_temporal_pool_bwd_bf16: max: dx[b,k] = dy[b] where argmax == k, else 0; mean: dy / K rounded to bf16 once; every
 * element of dx is written.  inner % 8 == 0.  The 'cat' join and the frame slice stay vd_temporal_cat / vd_frame_slice with
 * the channel / inner count halved, in both directions (C % 8 == 0 keeps their 16-byte units). */
int vd_temporal_pool_train_bf16(const void* x, void* y, uint8_t* argmax_u8, int B, int K, int64_t inner, int type, void* stream);
int vd_temporal_pool_bwd_bf16(const void* dy, const uint8_t* argmax_u8, void* dx, int B, int K, int64_t inner, int type,
                              void* stream);
/* The gradient of the correlation join (vd_corr_bwd) on bf16 dy [B,H,W,ldy], x and dx [B*K,H,W,C]: the same definition and
 * fixed summation order, fp32 accumulation, one rounding to bf16 at the store; no atomics, bit-reproducible; every element of
 * dx is written.  Columns [Cc, ldy) of dy are never read.  The dy slice of a workgroup is staged in LDS (vd_corr.hip). */
int vd_corr_bwd_bf16(const void* dy, const void* x, void* dx, int B, int K, int H, int W, int C, int d, int ldy, void* stream);
int vd_stem_wgrad_bf16(const float* x_nchw, const void* dz, int ldd, float* dwp, int N, int H, int W, void* ws, int64_t ws_bytes,
                       void* stream);
/* vd_stem_wgrad_bn on bf16 z and dy: each dz element is rounded to bf16 before use, as vd_bn_bwd_apply_bf16 stores it */
int vd_stem_wgrad_bn_bf16(const float* x_nchw, const void* z, int ldz, const void* dy, int ldy, const float* scale,
                          const float* shift, const float* save_mean, const float* save_invstd, const double* sums2, double count,
                          float slope, float* dwp, int N, int H, int W, void* ws, int64_t ws_bytes, void* stream);
int vd_yolo_loss_fwd_bwd_bf16(const vd_head_desc* h, const float* gt, int M, const float* obj_t, const float* center_t,
                              const float* scale_t, const float* weight_t, const float* class_t, float ignore_thresh,
                              int label_smooth, float* losses, void* const dhead[3], float* box_out, void* ws, int64_t ws_bytes,
                              void* stream);

/* ---- the joins of streaming video detection (vd_stream.hip): vd_temporal_pool / vd_temporal_pool_bf16 /
 * vd_temporal_cat (forward) read in place from a ring of cached per-frame features.  ring [S][inner] = [S][hw][C]; slots
 * [B][K] int32 in device memory, values in [0, S), any order, repeats allowed (a value outside the range is clamped into it:
 * a bad table never reads outside the ring).  pool: y [B][inner], type 0 = max, 1 = mean; cat: y [B][hw][K*C].  The same
 * arithmetic in the same order as the windowed kernels: the results are bit-equal to those kernels on the gathered copy
 * [B][K][inner].  1 <= K < 128, S >= 1, inner % 4 == 0 (fp32) / % 8 (bf16), C % 4 == 0 (bf16 tensors go through the cat with
 * C halved, as through vd_temporal_cat), ring / y 16-byte aligned.  Inference only: there is no backward. */
int vd_temporal_pool_idx(const float* ring, const int32_t* slots, float* y, int S, int B, int K, int64_t inner, int type,
                         void* stream);
int vd_temporal_pool_idx_bf16(const void* ring, const int32_t* slots, void* y, int S, int B, int K, int64_t inner, int type,
                              void* stream);
int vd_temporal_cat_idx(const float* ring, const int32_t* slots, float* y, int S, int B, int K, int64_t hw, int C, void* stream);

/* ---- resize of raw uint8 frames on the device, fused with the input normalisation (vd_resize.hip).
 * in [N,H0,W0,3] uint8 -> out [N,3,H,W] fp32, normalised as vd_preprocess_u8_nchw normalises; out_u8 (may be NULL) receives
 * the resized frame [N,H,W,3] uint8.  The resample is separable and given by tables in device memory, per axis T taps per
 * output index: idx_y [H][Ty] int32 / w_y [H][Ty] fp32, idx_x [W][Tx] / w_x [W][Tx] - what viddet_amd/video.py _axis_taps
 * returns (area, bilinear, bicubic, Lanczos), cast; an index outside the axis is clamped into it (a bad table reads a wrong
 * pixel, never memory outside the frame).  fp32 arithmetic in a fixed order (horizontal taps 0 .. Tx-1, then vertical taps
 * 0 .. Ty-1, fmaf from 0), rintf, clamp to [0, 255]: `out` is bit-equal to vd_preprocess_u8_nchw applied to `out_u8`.
 * 1 <= Ty, Tx <= 16; all sizes >= 1; out and the tables 4-byte aligned; VD_EINVAL where the source rows one tile needs do not
 * fit in LDS (a shrink beyond what 16 taps cover).  No atomics, bit-reproducible. */
int vd_resize_u8_nchw(const uint8_t* in, float* out, uint8_t* out_u8, int N, int H0, int W0, int H, int W, const int32_t* idx_y,
                      const float* w_y, int Ty, const int32_t* idx_x, const float* w_x, int Tx, void* stream);

/* ---- the same resize on NV12 frames (vd_resize.hip): what video decoders hand out.  A frame starts every
 * `frame_stride` bytes of `in`: H0 rows of luma Y, and from `uv_offset` bytes into the frame H0/2 rows of interleaved chroma
 * pairs U V (one pair per 2 x 2 block), `pitch` bytes from row to row in both planes.  Pixel (y, x) takes the pair (y >> 1,
 * x >> 1) (nearest chroma); C = Y - off, D = U - 128, E = V - 128 and in int32
 *   R = clip((gain*C + ru*D + rv*E + 128) >> 8, 0, 255), G with (gu, gv), B with (bu, 0)
 * - an arithmetic (floor) shift, then the clip: viddet_amd/video.py nv12_to_rgb with the seven integers of its NV12_MATRICES
 * entry.  Everything behind the conversion is vd_resize_u8_nchw: out / out_u8 are bit-equal to that entry point on
 * nv12_to_rgb of the frames.  H0, W0 even; W0 <= pitch < 2^31; uv_offset >= pitch * H0; uv_offset + pitch * H0 / 2 <=
 * frame_stride < 2^40; in_bytes >= (N - 1) * frame_stride + uv_offset + pitch * (H0 / 2 - 1) + W0 (the last chroma byte of the
 * last frame: no slack, padding or whole last pitch need exist behind it).  No byte outside [in, in + in_bytes) is read,
 * whatever the tables hold; `in` needs no alignment.  Otherwise as vd_resize_u8_nchw.  No atomics, bit-reproducible. */
int vd_resize_nv12_nchw(const uint8_t* in, int64_t in_bytes, int64_t frame_stride, int64_t pitch, int64_t uv_offset, float* out,
                        uint8_t* out_u8, int N, int H0, int W0, int H, int W, const int32_t* idx_y, const float* w_y, int Ty,
                        const int32_t* idx_x, const float* w_x, int Tx, int off, int gain, int ru, int rv, int gu, int gv, int bu,
                        void* stream);

/* ---- training augmentation on the device (vd_augment.hip): the pixels of colour distortion, expansion,
 * crop, resize and flip in one launch, from decisions taken on the host.  raw: the uint8 frames of N samples, K frames
 * [h0,w0,3] each, sample n at byte src_off[n] with (h0, w0) = src_hw[n]; frames n*K .. n*K+K-1 share record n.
 * color [N][12] fp32: M (3x3 row-major) and b, level_c = sum_i x_i M[i][c] + b[c].  idx_y [N][H][Ty] int32 / w_y [N][H][Ty] fp32,
 * idx_x [N][W][Tx] / w_x [N][W][Tx]: per-axis taps in SOURCE coordinates; an index < 0 is a tap on the canvas fill `fill[3]`,
 * one >= the source's size is clamped into it (a bad table reads a wrong pixel of the sample's own frames, never memory outside
 * them).  out [N*K,3,H,W] fp32, normalised as vd_preprocess_u8_nchw normalises, no rounding to uint8.  fp32 in a fixed order:
 * horizontal taps 0 .. Tx-1 per source row then vertical taps 0 .. Ty-1 (fmaf from 0, fill taps skipped) give S[i]; per axis
 * Wsrc = sum of source-tap weights, Wall = sum of all weights (adds from 0 in tap order), multiplied across the axes; then
 * t = S[0]*M[0][c]; t = fmaf(S[1], M[1][c], t); t = fmaf(S[2], M[2][c], t); t = fmaf(b[c], Wsrc, t);
 * t = fmaf(fill[c], Wall - Wsrc, t) - the colour affine once per output pixel.  1 <= Ty, Tx <= 32; all sizes >= 1; src_off
 * 8-byte aligned, every other table and out 4-byte aligned.  No atomics, bit-reproducible. */
int vd_augment_u8_nchw(const uint8_t* raw, const int64_t* src_off, const int32_t* src_hw, const float* color, const int32_t* idx_y,
                       const float* w_y, int Ty, const int32_t* idx_x, const float* w_x, int Tx, const float* fill, float* out, int N,
                       int K, int H, int W, void* stream);

/* ---- YOLO training targets on the device (vd_targets.hip): viddet_amd/targets.py::prefetch_targets in two
 * launches, from the label rows alone.  gt [N][M][4] fp32 corner boxes, rows padded with -1; ids [N][M][idw] fp32, idw = 1 a
 * class index, idw = C a multi-hot row; mix [N][M] mixup ratios (the objectness target) or NULL (1).  Outputs, fp32, EVERY
 * element written on every call: obj [N][P][1], ctr [N][P][2], scl [N][P][2], wgt [N][P][2] (default 0) and cls [N][P][C]
 * (default -1), P = 3 * sum over strides 32, 16, 8 of (H/s)(W/s), row = the stride-32 layer first, (y*w + x)*3 + a inside a
 * layer.  Per gt: width, height and centre x0 + w/2 in fp32, then fp64 without FMA contraction - shape IoU against the nine
 * anchors (inter / union, 0 where union <= 0, first maximum wins), fx = gx / W * w_layer, lx = (int)fx, ctr = fx - lx,
 * scl = log(max(gw, 1) / anchor), wgt = 2 - gw*gh / W / H; bit-equal to the host except log().  A row is valid if all four
 * coordinates are >= 0 (NaN is not); an image's rows END at its first invalid row; of two gts on one row p the later one wins
 * every column, its whole class row included; a gt whose p lies outside [0, P) is dropped (fx, fy are clamped before the cast:
 * no input stores out of bounds); a class index outside [0, C) writes no 1.  N, M, C >= 1; M <= 512; H, W multiples of 32;
 * idw in {1, C}; every pointer 4-byte aligned.  No atomics, bit-reproducible. */
int vd_yolo_targets(const float* gt, const float* ids, int idw, const float* mix, int N, int M, int C, int H, int W, float* obj,
                    float* ctr, float* scl, float* wgt, float* cls, void* stream);

/* ---- VOC mAP matching on the device (vd_eval.hip): what viddet_amd.metrics.VOCMApMetric.update decides for one
 * image, one workgroup per image.  det_ids [B][N], det_scores [B][N], det_boxes [B][N][4] fp32 (the network's outputs); gt
 * [B][M][gt_w] fp32 label rows x1, y1, x2, y2, id (gt_w = 5) + difficult (gt_w = 6).  A detection row with id < 0 is no detection
 * (rec_cls -1, rec_hit -2); a label row with id < 0 is padding wherever it sits; ids are truncated like astype(int).  clip_hi >= 0:
 * every DETECTION coordinate is clipped to [0, clip_hi] first (numpy.clip; train_yolov3.py validate() clips the detections, not
 * the labels); < 0: no clip.  Best ground truth of a detection of class c: among the label rows of class c in row order, the
 * highest bbox_iou in fp32 without FMA contraction and with correctly rounded division - lo = max, hi = min, overlap = lo < hi
 * on both axes, inter = ((hi.x-lo.x)*(hi.y-lo.y)) * overlap, iou = inter / ((area_a + area_b) - inter) - chosen as numpy.argmax
 * chooses (first maximum; the first NaN beats everything) and dropped only where max < iou_thresh is true (a NaN keeps its
 * match).  rec_hit: -1 for every detection whose best row is difficult; otherwise 1 for the first detection on that row in the
 * host's visiting order (score descending, then row index) and 0 for every later one; 0 without a best row.  rec_cls [B][N]
 * int32, rec_score [B][N] fp32 (the scores, copied), rec_hit [B][N] int8: written in full.  npos [C] += the non-difficult and
 * ndiff [C] (may be NULL) += the difficult label rows per class, by integer atomics; a label id outside [0, C) is counted in
 * neither and a detection id outside [0, C) is only recorded: no id indexes memory.  0 <= N <= 1024, 0 <= M <= 512, B >= 0,
 * C >= 1; every pointer but rec_hit 4-byte aligned.  Bit-reproducible. */
int vd_voc_match(const float* det_ids, const float* det_scores, const float* det_boxes, int B, int N, const float* gt, int M,
                 int gt_w, float clip_hi, float iou_thresh, int32_t* rec_cls, float* rec_score, int8_t* rec_hit, int32_t* npos,
                 int32_t* ndiff, int C, void* stream);

/* ---- ImageNet VID motion metric, matching on the device (vd_vid_eval.hip): what viddet_amd.vid_metric.match_image
 * decides for one image, one workgroup per image.  All inputs are float64: det [B][N][6] rows label, score, x1, y1, x2, y2 in
 * source pixels (label < 0: a padded row, wherever it sits); gt [B][M][6] rows x1, y1, x2, y2, label, motion_iou (label < 0:
 * padded); motion_ranges [4][2], area_ranges [4][2] (lo, hi), on the device too.  Per label row thr = (w*h) / ((w+tol)*(h+tol))
 * with w = x2-x1+1, h = y2-y1+1, capped at iou_thresh; it is ignored by motion range r where miou < lo | miou > hi (a NaN is
 * inside every range) and by area range r where (y2-y1+1)*(x2-x1+1) < lo | > hi.  The detections are visited by score
 * descending (numpy's stable argsort of -score: NaN last, ties by row); each takes the not yet taken label row of its class
 * (labels truncated like astype(int)) with ov >= thr and the largest ov, the lowest row on ties - ov = iw*ih / ((area_det +
 * area_gt) - iw*ih) where iw = min(x2) - max(x1) + 1 > 0 and ih > 0, else 0; fp64 without FMA contraction, correctly rounded
 * division.  Outputs, int32, cell c = 4 * motion + area:
 *   rec_gt [B][N]   the matched label row, -1 unmatched, -2 a padded row
 *   rec_tp [B][N]   bit c: matched, and the row is ignored by neither range of the cell
 *   rec_fp [B][N]   bits 2c, 2c+1, of an unmatched detection: 0 (its own area is outside the area range, or its largest ov over
 *                   all label rows the motion range ignores exceeds that over those it does not), 1 (the reverse), 2 (the two
 *                   are equal and the image has no label row: the host's empty_weight), 3 (equal otherwise: the image's ignored
 *                   fraction img_nig / img_ngt)
 *   img_nig [B][4]  label rows ignored by motion range r;  img_ngt [B] valid label rows       - these five are written in full
 *   npos [C] += label rows per class;  nout [16][C] += label rows per class ignored by cell c - integer atomics, the caller zeroes
 * A label id outside [0, C) is counted in neither; a detection id outside [0, C) is only recorded: no id indexes memory.
 * 0 <= N <= 1024, 0 <= M <= 512, B >= 0, C >= 1; double pointers 8-byte, int pointers 4-byte aligned.  Bit-reproducible. */
int vd_vid_match(const double* det, int B, int N, const double* gt, int M, const double* motion_ranges, const double* area_ranges,
                 double iou_thresh, double pixel_tolerance, int32_t* rec_gt, int32_t* rec_tp, int32_t* rec_fp, int32_t* img_nig,
                 int32_t* img_ngt, int32_t* npos, int32_t* nout, int C, void* stream);

/* ---- COCO detection metric, matching on the device (vd_coco_eval.hip): what viddet_amd.coco_metric.match_image
 * decides for one image - COCOeval's computeIoU and evaluateImg for every category, 4 area ranges and 10 IoU thresholds - one
 * workgroup per image.  All inputs are float64 and on the device: det [B][N][6] rows x, y, w, h, score, category; gt [B][M][8]
 * rows x, y, w, h, area, category, annotation id, iscrowd; iou_thrs [10]; area_rng [4][2] (lo, hi, both inclusive).  A row
 * whose category is not in [0, K) (-1: a padded row, wherever it sits; NaN) takes no part; categories are truncated like a C
 * cast.  iou = 0 where w <= 0 or h <= 0 with w = min(dx+dw, gx+gw) - max(dx, gx), h likewise, else w*h / u, u = dw*dh for a
 * crowd, (dw*dh + gw*gh) - w*h otherwise; fp64 without FMA contraction, correctly rounded division.  A ground truth is ignored
 * by range r where it is a crowd or area < lo | area > hi.  The detections of a category are ranked by score descending
 * (numpy's stable argsort of -score: NaN last, ties by row) and the first 100 take part; per range and threshold t each, in
 * rank order, starts from iou = min(t, 1 - 1e-10) and walks the category's ground truths, the not-ignored ones first, in row
 * order: one matched at t that is no crowd is skipped, the walk ends before the ignored ones once a not-ignored one is held,
 * one with ious < iou is skipped, any other is taken and raises iou (on equal IoUs the later one wins).  Outputs, int32:
 *   rec_rank [B][N]     the rank inside (image, category), -1 for a row beyond the first 100 or one that takes no part
 *   rec_bits [B][N][4]  per area range: bit t = matched at threshold t to an annotation whose id is not 0 (COCOeval's
 *                       `dtm != 0`), bit 10 + t = ignored: the match's ground truth is ignored, or the matched bit is clear and
 *                       the detection's own area dw*dh is outside the range; 0 where rec_rank is -1   - both written in full
 *   npig [K][4] += the ground truths of category k that range r does not ignore - integer atomics, the caller zeroes
 * Boxes are finite: a NaN IoU passes `ious < iou` here, which the host's vectorised form does not restate.
 * 0 <= N <= 1024, 0 <= M <= 512, B >= 0, 1 <= K <= 32767; double pointers 8-byte, int pointers 4-byte aligned.  Bit-reproducible. */
int vd_coco_match(const double* det, int B, int N, const double* gt, int M, const double* iou_thrs, const double* area_rng,
                  int32_t* rec_rank, int32_t* rec_bits, int32_t* npig, int K, void* stream);

/* ---- Seq-NMS over the detections of video clips (vd_seq_nms.hip): what viddet_amd.seq_nms.seq_nms_host computes,
 * bit for bit.  ids [F][N], scores [F][N], bboxes [F][N][4] fp32 (the network's outputs over F frames, corner boxes; a row with
 * id < 0 is padding); clip_start [V + 1] int32 ON THE DEVICE, ascending offsets into the frame axis from 0 to F (NULL with V = 1:
 * one clip [0, F)); nothing links across a clip boundary, and an offset outside [0, F] is clamped into it (a frame that no clip
 * covers comes out as -1 rows): no offset indexes memory.  A row is a candidate iff id >= 0 (NaN is not), its score is finite and
 * its class - the id truncated like astype(int) - is below num_class; classes are independent.  iou = iw*ih / ((a1 + a2) - iw*ih)
 * where iw = min(x2) - max(x1) > 0 and ih > 0, else 0 (no +1; min / max propagate a NaN); fp32 without FMA contraction, correctly
 * rounded division; `iou > thresh` is strict.  Per clip and class, every candidate alive, rounds repeat while a row is alive:
 * frames t from last to first, alive rows i in row order: b = 0, p = none; over the alive rows j of frame t + 1 in row order with
 * iou(i, j) > link_thresh and best[t+1][j] > b: b = best[t+1][j], p = j; best[t][i] = score + b (one add), next[t][i] = p.  The
 * start is the alive row with the largest best, ties to the lowest frame, then the lowest row; the sequence follows next; its
 * score is (rescore 0, avg) the sum of its rows' scores in frame order, from 0, divided by their number, or (rescore 1, max)
 * their maximum; its rows are final with that score, and in each of its frames every alive row of the class with
 * iou > nms_thresh to the sequence's row is dead.  Outputs, written in full: per frame the final rows by new score descending,
 * stably by old row - out_ids [F][N] (the row's id), out_scores [F][N] (the new score), out_bboxes [F][N][4], out_perm [F][N]
 * int32 (the old row) - then rows of -1 in all four.  Three launches: the link table (a 128-bit mask per row and threshold), one
 * wavefront per (clip, class) for the rounds, a stable rank sort per frame.  1 <= N <= 128, F >= 1, V >= 1, 1 <= num_class <=
 * 65535; ws_bytes >= 48 * F * N; bboxes, out_bboxes and ws 16-byte, every other pointer 4-byte aligned.  The inputs are never
 * written.  No atomics, bit-reproducible. */
int vd_seq_nms(const float* ids, const float* scores, const float* bboxes, const int32_t* clip_start, int V, int F, int N,
               int num_class, float link_thresh, float nms_thresh, int rescore, float* out_ids, float* out_scores,
               float* out_bboxes, int32_t* out_perm, void* ws, int64_t ws_bytes, void* stream);
/* For timing the launches apart (tools/seq_nms_probe.py): vd_seq_nms with the same checks (their messages name vd_seq_nms), making
 * only the first one (stages 1), two (3) or all three (7) launches; with fewer than three the outputs are not written. */
int vd_seq_nms_stages(const float* ids, const float* scores, const float* bboxes, const int32_t* clip_start, int V, int F, int N,
                      int num_class, float link_thresh, float nms_thresh, int rescore, float* out_ids, float* out_scores,
                      float* out_bboxes, int32_t* out_perm, void* ws, int64_t ws_bytes, int stages, void* stream);

/* ---- The detections of video clips linked into tracks (vd_track.hip): what viddet_amd.track.track_host computes,
 * bit for bit - the IOU tracker of Bochinski, Eiselein and Sikora (AVSS 2017) with a max_age extension (0 is the paper).  ids,
 * scores, bboxes, clip_start, V, F, N, num_class: as vd_seq_nms takes them, and a row is a candidate iff it is one there and
 * score >= sigma_l.  Per clip, frames in order.  Extend: the active tracks in order of creation; a track of class c takes, among
 * the candidates of class c of the frame that no track has taken, the one with the largest IoU (vd_seq_nms's arithmetic) to the
 * track's last matched box, ties to the lowest row (a NaN IoU ranks first and matches nothing); where that IoU >= sigma_iou the
 * row joins, the track's last box is the row's, its miss count 0, its maximum score max(maximum, score); otherwise, or with no
 * candidate left, the miss count grows by one and the track is closed once it exceeds max_age.  Start: every candidate not taken
 * starts a track, in row order; a track's id is its creation number within the clip, from 0, one counter for all classes.
 * Decide, at the clip's end: a track is kept iff its maximum score >= sigma_h and it holds at least t_min rows; ids are not
 * renumbered.  Outputs, written in full: out_track [F][N] int32 (the row's track id; -1 for a row that is no candidate, of a
 * dropped track or of a frame that no clip covers), out_len [F][N] int32 (the rows of its track, 0 beside -1), out_score [F][N]
 * (the track's maximum score, -1 beside -1).  One workgroup per clip, the active tracks (at most N * (max_age + 1) <= 1024) in
 * LDS; ws holds the length and the maximum of every track made, VD_TRACK_WS_PER_ROW bytes per (frame, row).  1 <= N <= 128,
 * F >= 1, V >= 1, num_class >= 1, t_min >= 1, 0 <= max_age <= 7, no threshold NaN; bboxes 16-byte, every other pointer 4-byte
 * aligned.  The inputs are never written.  No atomics, bit-reproducible. */
#define VD_TRACK_WS_PER_ROW 8
int vd_track(const float* ids, const float* scores, const float* bboxes, const int32_t* clip_start, int V, int F, int N,
             int num_class, float sigma_l, float sigma_h, float sigma_iou, int t_min, int max_age, int32_t* out_track,
             int32_t* out_len, float* out_score, void* ws, int64_t ws_bytes, void* stream);

/* ---- The same tracker in resumable form, for a stream of frames that never says where it ends (vd_track_live.hip, DESIGN.md
 * 31): what viddet_amd.track.track_online_host computes, bit for bit.  One launch runs the extend and start steps above, with the
 * same arithmetic and tie rules, on the F frames of V streams - ids, scores [V][F][N], bboxes [V][F][N][4] - starting from each
 * stream's state and leaving the new state behind; nothing is decided on the device, so sigma_h and t_min are no arguments
 * (track.finalize_tracks decides on the host, once a clip has ended).  state: V blocks of VD_TRACK_STATE_BYTES, each
 *   int32 n_active, int32 next_id, 8 bytes unused, then float4 box[1024], int32 class[1024], id[1024], misses[1024],
 *   length[1024], float maximum[1024] - the active tracks in order of creation, the first n_active entries live.
 * A block of all zero bytes is a fresh stream; n_active is clamped into [0, 1024] before it indexes anything; the live entries
 * and the header are written back with ordinary stores.  Outputs, written in full, [V][F][N]: out_track int32 (the row's track
 * id, a creation number counted over the whole stream from 0, one counter for all classes; -1 for a row that is no candidate),
 * out_len int32 (the rows of its track so far, this one included; 0 beside -1), out_score (the track's maximum score so far; -1
 * beside -1).  A stream hands out at most N ids per frame: the caller keeps frames * N below 2^31.  One workgroup per stream, no
 * workspace, no atomics, bit-reproducible; the inputs are never written.  1 <= N <= 128, F >= 1, V >= 1, num_class >= 1,
 * 0 <= max_age <= 7, no threshold NaN; bboxes and state 16-byte, every other pointer 4-byte aligned. */
#define VD_TRACK_STATE_BYTES 36880
int vd_track_push(const float* ids, const float* scores, const float* bboxes, int V, int F, int N, int num_class, float sigma_l,
                  float sigma_iou, int max_age, void* state, int64_t state_bytes, int32_t* out_track, int32_t* out_len,
                  float* out_score, void* stream);

/* ---- Tubelet rescoring and gap filling over the tracks of video clips (vd_tubelet.hip): what
 * viddet_amd.tubelet.tubelet_host computes, bit for bit, on all six outputs.  ids, scores, bboxes, clip_start, V, F, N,
 * num_class: as vd_seq_nms takes them; track [F][N] int32: vd_track's out_track (any table is safe).  Per clip [t0, t1):
 *   1. a row is present iff it is a candidate of vd_seq_nms (id >= 0, a finite score, a class below num_class); a present row is
 *      a member of track u = track[t][i] iff 0 <= u < (t1 - t0) * N and no lower row of its frame is a member of u already; a
 *      track's members are ordered by frame.
 *   2. rescore 1 (avg): s_u = the fp32 sum of the members' scores in frame order, from 0, one rounding per add, divided by
 *      (float)len, correctly rounded; 2 (max): the first member's score, replaced by a later one's where that is greater; every
 *      member's new score is s_u; 0: the scores stay.  A row that is no member keeps its score.
 *   3. consecutive members at frames f0 < f1, g = f1 - f0, 1 < g <= max_gap + 1, give every frame f0 + j, 0 < j < g, a candidate
 *      fill row: the id of the member at f0, track u, w = (float)j / (float)g, every coordinate a + (b - a) * w (a at f0, b at
 *      f1; every operation rounded, no FMA), score s_u, with rescore 0 the same formula on the two scores.
 *   4. per frame: the kept rows - the present rows in row order, with drop_untracked only the members - then the fills in
 *      ascending track id while kept + admitted < N (dropped[t] counts the others), sorted by new score descending, stably, by
 *      float comparison (-0.0 and 0.0 tie; no score is a NaN: the members' scores are finite); rows of -1 follow.
 * Outputs, written in full: out_ids, out_scores [F][N], out_bboxes [F][N][4]; perm [F][N] int32 (the old row of an output row,
 * -2 a filled row, -1 an empty one); track_out [F][N] int32 (the output row's track, -1 where it has none or the row is empty);
 * dropped [F] int32.  A frame that no clip covers comes out empty.  A track id is checked against [0, (t1 - t0) * N) before it
 * indexes the per-track tables (sum, count, maximum, last member), which live in ws, VD_TUBELET_WS_PER_ROW bytes per (frame,
 * row), at the clip's first row + the id.  Four launches (one fewer without clip_start): clear, members per (clip, frame), ONE
 * workgroup per clip accumulating in frame order, assembly per (clip, frame).  1 <= N <= 128, F >= 1, F * N < 2^31, V >= 1,
 * num_class >= 1, 0 <= max_gap <= 7; bboxes and out_bboxes 16-byte, every other pointer 4-byte aligned.  The inputs are never
 * written.  No atomics, bit-reproducible.  vd_tubelet_ws_bytes: the bytes ws must hold, -1 for sizes that are not taken. */
#define VD_TUBELET_WS_PER_ROW 24
int64_t vd_tubelet_ws_bytes(int F, int N);
int vd_tubelet(const float* ids, const float* scores, const float* bboxes, const int32_t* track, const int32_t* clip_start, int V,
               int F, int N, int num_class, int rescore, int max_gap, int drop_untracked, float* out_ids, float* out_scores,
               float* out_bboxes, int32_t* perm, int32_t* track_out, int32_t* dropped, void* ws, int64_t ws_bytes, void* stream);
/* the same, for timing the launches one by one (tools/tubelet_probe.py): stages is a mask of 1 (clear), 2 (members), 4 (chain),
 * 8 (frames); vd_tubelet is stages 15.  With fewer the outputs may stay unwritten; an id read back from the workspace is checked
 * against the clip's range again, so a launch that meets a workspace no earlier launch filled stays inside it. */
int vd_tubelet_stages(const float* ids, const float* scores, const float* bboxes, const int32_t* track, const int32_t* clip_start,
                      int V, int F, int N, int num_class, int rescore, int max_gap, int drop_untracked, float* out_ids,
                      float* out_scores, float* out_bboxes, int32_t* perm, int32_t* track_out, int32_t* dropped, void* ws,
                      int64_t ws_bytes, int stages, void* stream);

/* ---- Fixed-interval (Rauch-Tung-Striebel) smoothing of the boxes of video clips along their tracks (vd_track_smooth.hip,
 * DESIGN.md 37): what viddet_amd.smooth.smooth_host computes, bit for bit, on both outputs.  ids, scores, bboxes, clip_start, V,
 * F, N, num_class: as vd_seq_nms takes them; track [F][N] int32: the out_track of vd_track / vd_track_sort / vd_track_byte (any
 * table is safe).  Per clip [t0, t1):
 *   1. members: vd_tubelet's step 1 - a present row is a member of track u = track[t][i] iff 0 <= u < (t1 - t0) * N and no lower
 *      row of its frame is a member of u already;
 *   2. segments: a track's members in frame order, cut where two consecutive members lie more than max_gap + 1 frames apart;
 *   3. forward, for a segment of n >= 2 members: the Kalman filter of vd_track_sort (start at the first member's box, predict
 *      once per frame of a gap, update with every member's box);
 *   4. backward: from the last member's posterior state, one Rauch-Tung-Striebel step per frame of every gap, the gap's
 *      predicted states recomputed from the earlier member's posterior (smooth.py states every operation and its order);
 *   5. out_sbox [F][N][4]: the box of a member's smoothed state; a member whose smoothed box is not finite, the member of a
 *      segment of one, a row that is no member and every row of a frame that no clip covers keep the bits of their input box.
 *      out_slen [F][N] int32: the members of the row's segment, 0 for a row that is no member.
 * Both outputs are written in full.  A row index read back from the workspace is checked against the clip's rows before it
 * indexes anything and a walk only ever moves to a strictly later (forward) or earlier (backward) frame.  ws holds
 * VD_TRACK_SMOOTH_WS_PER_ROW bytes per (frame, row): the member id, the predecessor, the successor and the 17-float posterior
 * state.  Four launches (one fewer without clip_start): clear, members per (clip, frame), links per (clip, frame), segments (a
 * thread per row, a segment's first member does the work).  1 <= N <= 128, F >= 1, F * N < 2^31, V >= 1, num_class >= 1,
 * 0 <= max_gap <= 7; bboxes and out_sbox 16-byte, every other pointer 4-byte aligned.  The inputs are never written.  No atomics,
 * bit-reproducible.  vd_track_smooth_ws_bytes: the bytes ws must hold, -1 for sizes that are not taken. */
#define VD_TRACK_SMOOTH_WS_PER_ROW 80
int64_t vd_track_smooth_ws_bytes(int F, int N);
int vd_track_smooth(const float* ids, const float* scores, const float* bboxes, const int32_t* track, const int32_t* clip_start,
                    int V, int F, int N, int num_class, int max_gap, float* out_sbox, int32_t* out_slen, void* ws, int64_t ws_bytes,
                    void* stream);
/* the same, for timing the launches one by one (tools/smooth_probe.py): stages is a mask of 1 (clear), 2 (members), 4 (links),
 * 8 (segments); vd_track_smooth is stages 15.  With fewer the outputs may stay unwritten; whatever the workspace holds, a row
 * index read from it is checked against the clip's rows and a walk moves to a strictly later or earlier frame only, so a launch
 * that meets a workspace no earlier launch filled stays inside it and ends. */
int vd_track_smooth_stages(const float* ids, const float* scores, const float* bboxes, const int32_t* track,
                           const int32_t* clip_start, int V, int F, int N, int num_class, int max_gap, float* out_sbox,
                           int32_t* out_slen, void* ws, int64_t ws_bytes, int stages, void* stream);

/* ---- The same smoother in fixed-lag form, resumable, for streams of frames that never say where they end
 * (vd_track_smooth_live.hip): what viddet_amd.smooth_lag.smooth_lag_host computes, bit for bit, on both outputs.
 * One launch takes the next F >= 0 frames of V streams - ids, scores, track [V][F][N], bboxes [V][F][N][4]; track the out_track
 * of vd_track_push / vd_track_kf_push, ids counted over the stream (any table is safe) - starting from each stream's state and
 * leaving the new state behind, and emits the frames that became final: frame u once frame u + lag has been taken, every frame
 * taken with flush != 0 (the new frames first, then the rest against the last frame; the state's header is zeroed: a fresh
 * stream).  An emitted frame u is smoothed against the horizon h = min(u + lag, the last frame taken):
 *   members as vd_track_smooth finds them, with the causal bound 0 <= track[t][i] < (t + 1) * N (t the stream's frame); a
 *   member's predecessor is the member of its id in the nearest of the max_gap + 1 frames before it; the forward filter is
 *   vd_track_smooth's; the backward pass starts at the last member of the row's segment at a frame <= h; out_sbox and out_slen
 *   follow vd_track_smooth's step 5 on the segment truncated behind h.
 * state: V blocks of VD_TRACK_SMOOTH_LIVE_STATE_BYTES, each a ring of 16 frame slots (frame t lives in slot t % 16) of 128 rows:
 *   int32 frames (taken so far), emitted (given out so far), two unused words (16 bytes); int32 slot_frame[16], the frame a
 *   slot holds (64 bytes); then, indexed by e = slot * 128 + row, int32 mem[2048] (the id the row is a member of, -1: none),
 *   prev_frame[2048], prev_row[2048] (the segment's member before this one as (stream frame, row), -1: none), next_frame[2048],
 *   next_row[2048] (the one after it), pos[2048] (the member's position in its segment, from 0); float box[2048][4] (the input
 *   box); float post[17][2048] (the member's posterior state, field-major).
 * A block of all zero bytes is a fresh stream.  The contents are never trusted: the counts are clamped before they index, a
 * (frame, row) word is checked - the row against [0, N), the frame against the window of the ring, the slot's stored frame
 * against the frame expected - before it indexes, a walk moves to a strictly later (forward) or earlier (backward) frame only
 * and makes at most 16 steps.  Outputs [V][m][N][4] and [V][m][N], written in full, m the frames that become final in this
 * call: every stream of a launch must have taken the same number of frames, so that m is one number, which the caller knows
 * from its own frame count T: without flush m = max(0, T + F - lag) - max(0, T - lag), with flush m = T + F - max(0, T - lag).
 * m is checked against F, lag and flush; a stream whose state disagrees with it gets the surplus rows zeroed.  ids, scores,
 * bboxes and track may be NULL where F == 0, the outputs where m == 0.  One workgroup of 256 threads per stream, 8,768 bytes of
 * LDS, no workspace, no atomics, bit-reproducible; the inputs are never written.  1 <= N <= 128, F >= 0, V >= 1, num_class >= 1,
 * 0 <= lag <= 15, 0 <= max_gap <= 7; the caller keeps frames * N below 2^31; bboxes, out_sbox and state 16-byte, every other
 * pointer 4-byte aligned. */
#define VD_TRACK_SMOOTH_LIVE_STATE_BYTES 221264
int vd_track_smooth_push(const float* ids, const float* scores, const float* bboxes, const int32_t* track, int V, int F, int N,
                         int num_class, int lag, int max_gap, int flush, void* state, int64_t state_bytes, int m, float* out_sbox,
                         int32_t* out_slen, void* stream);

/* ---- The track fragments of video clips re-linked across long gaps (vd_track_stitch.hip): what
 * viddet_amd.stitch.stitch_host computes, bit for bit, on all five outputs.  ids, scores, bboxes, clip_start, V, F, N,
 * num_class: as vd_seq_nms takes them; track [F][N] int32: the out_track of vd_track / vd_track_sort / vd_track_byte (any table
 * is safe).  Per clip [t0, t1):
 *   1. members: vd_track_smooth's step 1; a track is an id with at least one member;
 *   2. participants: the tracks in ascending id, the first VD_TRACK_STITCH_MAX_TRACKS of them; the others enter no link, keep
 *      their id, length and maximum and are counted in out_overflow[clip];
 *   3. a participant's tail: the Kalman filter of vd_track_sort run over all its members (start at the first member's box,
 *      predict once per frame between two members, update with every member's box), with the last member's frame and class;
 *      its head: the first member's input box, frame and class;
 *   4. tail a and head b are admissible iff a != b, 1 <= g = head frame - tail frame <= max_gap, the classes are equal and
 *      iou(the box of a's state after g predictions, b's box) >= sigma_iou (vd_seq_nms's fp32 IoU, the track side first); the
 *      links are the minimum-cost assignment of vd_track_sort over the admissible pairs at cost 2^20 - int(iou * 2^20), a dummy
 *      column per row at 2^27, rows (tails) and columns (heads) in ascending id; entered only with two or more participants;
 *   5. out_track [F][N] int32: the id of the first track of the row's chain of links, out_len [F][N] int32: the members of the
 *      chain, out_score [F][N]: its maximum score (`if s > m: m = s` over a track's members in frame order, then over the chain's
 *      tracks in chain order); -1 / 0 / -1 for a row that is no member and for every row of a frame that no clip covers.
 *      out_stitches [V] int32: the links of every clip; out_overflow [V] int32: its tracks beyond the participants.
 * All five outputs are written in full.  ws holds VD_TRACK_STITCH_WS_PER_ROW bytes per (frame, row): the member id of the row and
 * 24 words per track id (a clip's ids lie in [0, (t1 - t0) * N)).  Two launches (one without clip_start): fill, then one
 * workgroup per clip.  1 <= N <= 128, F >= 1, F * N < 2^31, V >= 1, num_class >= 1, 1 <= max_gap <= VD_TRACK_STITCH_MAX_GAP,
 * sigma_iou not NaN; bboxes 16-byte, every other pointer 4-byte aligned.  The inputs are never written.  No atomics,
 * bit-reproducible.  vd_track_stitch_ws_bytes: the bytes ws must hold, -1 for sizes that are not taken. */
#define VD_TRACK_STITCH_MAX_TRACKS 512
#define VD_TRACK_STITCH_MAX_GAP 32
#define VD_TRACK_STITCH_WS_PER_ROW 100
int64_t vd_track_stitch_ws_bytes(int F, int N);
int vd_track_stitch(const float* ids, const float* scores, const float* bboxes, const int32_t* track, const int32_t* clip_start,
                    int V, int F, int N, int num_class, int max_gap, float sigma_iou, int32_t* out_track, int32_t* out_len,
                    float* out_score, int32_t* out_stitches, int32_t* out_overflow, void* ws, int64_t ws_bytes, void* stream);

/* ---- The per-frame matching of the MOT tracking metric (vd_mot_eval.hip): what
 * viddet_amd.mot_metric.mot_match_host computes, bit for bit, on all four outputs.  gt_boxes [F][G][4] fp32, gt_cls, gt_id
 * [F][G] int32: the label rows (corner boxes, class, ground-truth track id); ids, scores, bboxes, clip_start, V, F, N, num_class: as
 * vd_seq_nms takes them; track [F][N] int32: vd_track's out_track / vd_tubelet's track_out (any table is safe).  Per clip
 * [t0, t1), frames in order, last[a] (0 <= a < 1024) = the prediction id ground-truth id a was matched to last, none at t0:
 *   1. a prediction row is eligible iff it is a candidate of vd_seq_nms and track >= 0, a ground-truth row iff gt_cls >= 0 and
 *      0 <= gt_id < 1024; an eligible row is a candidate iff no lower eligible row of its frame carries its id;
 *   2. (g, j) is admissible iff both are candidates, iou >= iou_thresh (vd_seq_nms's fp32 IoU) and (agnostic or the classes are
 *      equal): bit j % 32 of adm[t][g][j / 32];
 *   3. carry-over, ground-truth candidates in row order: where last[gt_id] = p, the candidate row j carrying p is free and (g, j)
 *      is admissible, g is matched to j;
 *   4. the rest: the minimum-cost assignment over admissible pairs at cost 2^20 - int(iou * 2^20), a dummy column per row at
 *      2^27 - successive shortest augmenting paths with int64 potentials, rows in row order, among columns of equal least slack
 *      the lowest (prediction rows in row order, then the dummies); entered only when both pools hold a row;
 *   5. match [F][G] int32: the prediction row, -1 an unmatched candidate, -2 no candidate; miou [F][G]: the pair's IoU, else 0;
 *      flags [F][G] int32: bit 0 an id switch (last[a] set and different from the matched id), bit 1 a carry-over match; then
 *      last[a] = the matched id.
 * All four outputs are written in full; the rows of a frame that no clip covers get -2 / 0 / 0 / 0.  ws carries the candidate
 * tables between the launches, VD_MOT_WS_PER_ROW bytes per (frame, row) of either side.  Three launches (one fewer without
 * clip_start): clear, pairs per (clip, frame), ONE workgroup per clip for steps 3 to 5.  1 <= G, N <= 128, F >= 1, V >= 1,
 * num_class >= 1, 0 < iou_thresh <= 1, agnostic 0 or 1; gt_boxes, bboxes and adm 16-byte, every other pointer 4-byte aligned.
 * The inputs are never written.  No atomics, bit-reproducible.  vd_mot_match_ws_bytes: the bytes ws must hold, -1 for sizes
 * that are not taken. */
#define VD_MOT_WS_PER_ROW 4
int64_t vd_mot_match_ws_bytes(int F, int G, int N);
int vd_mot_match(const float* gt_boxes, const int32_t* gt_cls, const int32_t* gt_id, const float* ids, const float* scores,
                 const float* bboxes, const int32_t* track, const int32_t* clip_start, int V, int F, int G, int N, int num_class,
                 float iou_thresh, int agnostic, int32_t* match, float* miou, int32_t* flags, uint32_t* adm, void* ws,
                 int64_t ws_bytes, void* stream);

/* ---- The detections of video clips linked into tracks by SORT (vd_track_sort.hip): what
 * viddet_amd.sort.sort_host computes, bit for bit, on all four outputs - Bewley et al., "Simple Online and Realtime Tracking"
 * (ICIP 2016).  ids, scores, bboxes, clip_start, V, F, N, num_class, sigma_l, sigma_h, t_min, max_age: as vd_track takes them,
 * and a row is a candidate iff it is one there.  The filter of a track is 17 floats, (x, xd, p00, p01, p11) for the centre u,
 * v and the area s and (r, p) for the aspect w / h; every operation is one fp32 operation, nothing is contracted into an FMA,
 * `/` and sqrt are correctly rounded:
 *   measurement of a box  w = x2 - x1, h = y2 - y1, z = (x1 + w/2, y1 + h/2, w*h, w/h)
 *   start                 x = z, xd = 0, (p00, p01, p11) = (10, 0, 1e4); p = 10 for r
 *   predict               first `if s + ds <= 0: ds = 0` (a NaN compares false); per pair, on the old values: x = x + xd,
 *                         p00 = ((p00 + p01) + (p01 + p11)) + 1, p01 = p01 + p11, p11 = p11 + (.01, .01, 1e-4); p = p + 1
 *   box of a state        w = sqrt(s*r), h = s / w, (u - w/2, v - h/2, u + w/2, v + h/2)
 *   update with z         per pair: S = p00 + (1, 1, 10), k0 = p00 / S, k1 = p01 / S, y = z - x, x = x + k0*y, xd = xd + k1*y,
 *                         p11 = p11 - k1*p01, p01 = p01 - k0*p01, p00 = p00 - k0*p00; S = p + 10, k = p / S,
 *                         r = r + k*(z - r), p = p - k*p
 * Per clip, frames in order.  Predict: every active track.  Associate: rows = the frame's candidates in row order, columns = the
 * active tracks in order of creation, then a dummy per row; (row i, track k) is admissible iff the classes are equal and
 * iou(predicted box of k, box of i) >= sigma_iou (vd_seq_nms's arithmetic, the track side first; a NaN is not admissible) and
 * costs 2^20 - int(iou * 2^20); a row's own dummy costs 2^27; the minimum-cost assignment is vd_mot_match's - successive
 * shortest augmenting paths with int64 potentials, rows in row order, among columns of equal least slack the lowest; entered
 * only when the frame has a candidate and a track is active.  Update: a matched track is updated with its row, its miss count
 * 0, its length one more, its maximum max(maximum, score); every other track's miss count grows by one and the track is closed
 * once it exceeds max_age; the survivors keep their order.  Start: every candidate that took its dummy (every candidate where
 * no assignment was made) starts a track, in row order; ids as vd_track's.  Decide, at the clip's end, as vd_track.  Outputs,
 * written in full: out_track, out_len, out_score [F][N] as vd_track's; out_tbox [F][N][4]: the posterior box of the row's
 * track after this row's update (the box of the start state for a track's first row), -1 beside a track of -1.  The rows of a
 * frame that no clip covers get -1 / 0 / -1 / -1.  Degenerate boxes get no special case: the NaNs travel.  One workgroup per
 * clip; the predicted boxes and the tracks' words in LDS; ws holds the length and maximum of every track made,
 * VD_TRACK_SORT_WS_PER_ROW bytes per (frame, row), then two tables of filter states per clip, VD_TRACK_SORT_WS_PER_CLIP bytes.
 * 1 <= N <= 128, F >= 1, F * N < 2^31, V >= 1, num_class >= 1, t_min >= 1, 0 <= max_age <= 7, no threshold NaN; bboxes and
 * out_tbox 16-byte, every other pointer 4-byte aligned.  The inputs are never written.  No atomics, bit-reproducible.
 * vd_track_sort_ws_bytes: the bytes ws must hold, -1 for sizes that are not taken. */
#define VD_TRACK_SORT_WS_PER_ROW 8
#define VD_TRACK_SORT_WS_PER_CLIP 139264
int64_t vd_track_sort_ws_bytes(int V, int F, int N);
int vd_track_sort(const float* ids, const float* scores, const float* bboxes, const int32_t* clip_start, int V, int F, int N,
                  int num_class, float sigma_l, float sigma_h, float sigma_iou, int t_min, int max_age, int32_t* out_track,
                  int32_t* out_len, float* out_score, float* out_tbox, void* ws, int64_t ws_bytes, void* stream);

/* ---- The appearance descriptor of detected rows, pooled from a route tensor of the backbone (vd_appearance.hip, DESIGN.md
 * 43): what viddet_amd.appearance.embed_host computes, bit for bit.  fmap [S][Hf][Wf][ld]: S NHWC maps of C channels at a pixel
 * pitch of ld >= C elements, fp32 or (is_bf16 = 1) bf16, upcast exactly; ids [B][N], bboxes [B][N][4] in network-input pixels;
 * image b reads map map_index[b] (b itself where map_index is NULL), cut to [0, S); stride: the map's, 8, 16 or 32;
 * emb [B][N][C] int8, written in full.  Every step is one fp32 operation, nothing contracted, `/` correctly rounded.  A row
 * whose id is not >= 0 or that holds a coordinate that is not finite has no descriptor: zeros.  Else, with bw = x2 - x1 and
 * k = (.125, .375, .625, .875): cx_i = (x1 + bw * k_i) * (1 / stride) - 0.5, below 0 (or NaN) -> 0, above Wf - 1 -> Wf - 1;
 * x0 = min(floor(cx), max(Wf - 2, 0)), x1i = min(x0 + 1, Wf - 1), ax = cx - x0; y alike; per channel the sample
 * t = f[y0][x0] + ax * (f[y0][x1i] - f[y0][x0]), u alike on row y1i, v = t + ay * (u - t); the 16 samples summed one after the
 * other, y outer and x inner, times 0.0625 = p; m = hsum(p) / C with hsum the halving sum (p[:n/2] + p[n/2:n] until one is
 * left); d = p - m; a = max |d| (a NaN travels); a == 0 or not finite: zeros; else q = int8(rint((d / a) * 127)), ties to even.
 * One workgroup per row, four channels a thread.  C a power of two in [8, 1024], ld a multiple of 4, 1 <= N <= 128, B >= 1;
 * fmap aligned to four of its elements, bboxes to 16 bytes, every other pointer to 4.  The inputs are never written. */
int vd_roi_embed(const void* fmap, int is_bf16, int S, int Hf, int Wf, int C, int ld, const float* ids, const float* bboxes,
                 const int32_t* map_index, int B, int N, int stride, int8_t* emb, void* stream);

/* ---- SORT with appearance association (vd_track_sort_app.hip): what viddet_amd.appearance.app_sort_host
 * computes, bit for bit, on all four outputs.  Everything is vd_track_sort's - the arguments, the candidates, the filter, the
 * assignment, the update, the decision, the outputs, the limits and the alignment - but the cost of a cell.  emb [F][N][C] int8
 * (vd_roi_embed's, C a power of two in [8, 1024], 4-byte aligned): the descriptor of every row, zeros: none.  A track's
 * descriptor is that of its most recent matched row that had one (the row that started it counts).  For row i and track k of
 * equal classes, with dot, na, nb the exact dot product and squared norms of the two descriptors: cos_q = 0 when dot <= 0 or a
 * norm is 0, else floor(double(dot) * 2^20 / sqrt(double(na) * double(nb))); adm = iou >= sigma_iou; app = iou >= sigma_prox
 * and both norms > 0 and cos_q >= int(sigma_app * 2^20); the cell is admissible iff adm or app and costs
 * 2^20 - max(int(iou * 2^20) if adm else 0, cos_q if app else 0).  sigma_app and sigma_prox lie in [0, 1].  With emb all zero
 * the outputs are vd_track_sort's.  The cells of a frame are written once into a table of 128 x 1024 int32 per clip and read by
 * the assignment: ws holds vd_track_sort's words, VD_TRACK_SORT_WS_PER_ROW bytes per (frame, row), and
 * VD_TRACK_SORT_APP_WS_PER_CLIP bytes per clip.  vd_track_sort_app_ws_bytes: the bytes ws must hold, -1 for sizes not taken. */
#define VD_TRACK_SORT_APP_WS_PER_CLIP 663552
int64_t vd_track_sort_app_ws_bytes(int V, int F, int N);
int vd_track_sort_app(const float* ids, const float* scores, const float* bboxes, const int8_t* emb, int C, const int32_t* clip_start,
                      int V, int F, int N, int num_class, float sigma_l, float sigma_h, float sigma_iou, int t_min, int max_age,
                      float sigma_app, float sigma_prox, int32_t* out_track, int32_t* out_len, float* out_score, float* out_tbox,
                      void* ws, int64_t ws_bytes, void* stream);

/* ---- The detections of video clips linked into tracks by BYTE (vd_track_byte.hip): what
 * viddet_amd.byte.byte_host computes, bit for bit, on all four outputs - Zhang et al., "ByteTrack: Multi-Object Tracking by
 * Associating Every Detection Box" (ECCV 2022).  Everything is vd_track_sort's - the arguments, the candidates (score >=
 * sigma_l), the filter, the cost of a cell, the assignment, the update, the decision at the clip's end, the outputs, the
 * workspace (vd_track_byte_ws_bytes gives vd_track_sort_ws_bytes' figure: VD_TRACK_SORT_WS_PER_ROW per (frame, row) and
 * VD_TRACK_SORT_WS_PER_CLIP per clip), the limits and the alignment - but the frame's association, which is made twice:
 *   first    rows = the HIGH rows (candidates with score >= sigma_d) in row order, columns = ALL active tracks in order of
 *            creation, then a dummy per row; admissible iff equal classes and iou(predicted box, row box) >= sigma_iou
 *   second   rows = the LOW rows (every other candidate) in row order, the same columns in the same places; a track is eligible
 *            iff the first association did not match it AND its miss count on entry to the frame is 0, every cell of another
 *            track's column is forbidden; admissible iff eligible, equal classes and iou >= sigma_iou2
 * Either is entered only when it has a row and a track is active.  A track matched by either is updated with its row; every
 * other track's miss count grows by one.  Start: the high rows that the first association left without a track and whose score
 * >= sigma_new, in row order; a low row, and a high row below sigma_new, that found no track gets -1 / 0 / -1 / -1.  No order
 * among the thresholds is demanded (sigma_l > sigma_d leaves no low rows); none may be NaN.  One workgroup of 256 threads per
 * clip, 51,344 bytes of LDS; the inputs are never written.  No atomics, bit-reproducible. */
int64_t vd_track_byte_ws_bytes(int V, int F, int N);
int vd_track_byte(const float* ids, const float* scores, const float* bboxes, const int32_t* clip_start, int V, int F, int N,
                  int num_class, float sigma_l, float sigma_d, float sigma_new, float sigma_h, float sigma_iou, float sigma_iou2,
                  int t_min, int max_age, int32_t* out_track, int32_t* out_len, float* out_score, float* out_tbox, void* ws,
                  int64_t ws_bytes, void* stream);

/* ---- The Kalman trackers in resumable form, for streams of frames that never say where they end (vd_track_kf_live.hip, DESIGN.md
 * 39): what viddet_amd.byte.byte_online_host computes, bit for bit, on all four outputs - and, with sigma_d = sigma_new =
 * sigma_l (the low list is then empty, the second association never entered, sigma_iou2 unused: pass sigma_iou), what
 * viddet_amd.sort.sort_online_host computes.  One launch runs vd_track_byte's frame body - predict, the two associations,
 * update, start - with the same arithmetic and tie rules on the F frames of V streams - ids, scores [V][F][N], bboxes
 * [V][F][N][4] - starting from each stream's state and leaving the new state behind; nothing is decided on the device, so
 * sigma_h and t_min are no arguments (track.finalize_tracks decides on the host, once a clip has ended).  state: V blocks of
 * VD_TRACK_KF_STATE_BYTES, each
 *   int32 n_active, next_id, cur, unused (16 bytes); int32 class[1024], id[1024], misses[1024], length[1024], float
 *   maximum[1024] - the active tracks in order of creation, the first n_active entries live; float table[2][17][1024] - their
 *   filter states, field-major, table `cur` current.
 * A block of all zero bytes is a fresh stream; n_active is clamped into [0, 1024] and cur into {0, 1} before either indexes
 * anything; the filter tables are used in place; the live words and the header are written back with ordinary stores.  Outputs,
 * written in full, [V][F][N]: out_track int32 (the row's track id, a creation number counted over the whole stream from 0, one
 * counter for all classes; -1 for a row that is no candidate or that neither found nor started a track), out_len int32 (the rows
 * of its track so far, this one included; 0 beside -1), out_score (the track's maximum score so far; -1 beside -1), out_tbox
 * [V][F][N][4] (the posterior box of the row's track after this row's update; -1 beside -1).  A stream hands out at most N ids
 * per frame: the caller keeps frames * N below 2^31.  One workgroup of 256 threads per stream, 51,344 bytes of LDS, no workspace,
 * no atomics, bit-reproducible; the inputs are never written.  1 <= N <= 128, F >= 1, V >= 1, num_class >= 1, 0 <= max_age <= 7,
 * no threshold NaN; bboxes, out_tbox and state 16-byte, every other pointer 4-byte aligned. */
#define VD_TRACK_KF_STATE_BYTES 159760
int vd_track_kf_push(const float* ids, const float* scores, const float* bboxes, int V, int F, int N, int num_class, float sigma_l,
                     float sigma_d, float sigma_new, float sigma_iou, float sigma_iou2, int max_age, void* state,
                     int64_t state_bytes, int32_t* out_track, int32_t* out_len, float* out_score, float* out_tbox, void* stream);

/* ---- The per-frame matching of the HOTA tracking metric (vd_hota_eval.hip): what
 * viddet_amd.hota_metric.hota_match_host computes, bit for bit, on all three outputs - Luiten et al., "HOTA: A Higher Order
 * Metric for Evaluating Multi-Object Tracking" (IJCV 2021).  The inputs are vd_mot_match's; the ids are dense: a ground-truth row
 * is eligible iff gt_cls >= 0 and 0 <= gt_id < A (A <= 1024), a prediction row iff it is a candidate of vd_seq_nms and
 * 0 <= track < P; an eligible row is a candidate iff no lower eligible row of its frame carries its id.  Per clip [t0, t1):
 *   1. q[g][j] = int(iou * 2^20) (vd_seq_nms's fp32 IoU; a NaN counts as 0) where both rows are candidates and (agnostic or the
 *      classes are equal), else 0; a pair is admissible iff q > 0;
 *   2. over all frames of the clip, in integers: with rq / cq the row and column sums of q in the frame,
 *      pm[a][p] += (q << 20) / (rq[g] + cq[j] - q) per admissible pair of ids (a, p); cg[a], cp[p]: the candidate rows of an id;
 *   3. A[a][p] = (pm << 20) / (((cg[a] + cp[p]) << 20) - pm), 0 where pm is 0;
 *   4. every frame on its own: the score of an admissible pair is s = (A[a][p] * q) >> 20; the minimum-cost assignment of the
 *      ground-truth candidates (row order) to the prediction candidates (row order) at cost 2^20 - s, a dummy column per row at
 *      2^20, is vd_mot_match's - successive shortest augmenting paths with int64 potentials, among columns of equal least
 *      slack the lowest; entered only when both pools hold a row;
 *   5. match [F][G] int32: the prediction row, -1 an unmatched candidate, -2 no candidate; msim [F][G]: the pair's IoU, else 0;
 *      mscore [F][G] int32: the pair's s, else 0.
 * All three outputs are written in full; the rows of a frame that no clip covers get -2 / 0 / 0.  ws holds pm [V][A][P] int64,
 * then cg [V][A] and cp [V][P] int32; it is cleared by the first launch, whatever it held.  Three launches: clear; pass 2 with a
 * workgroup per frame (integer atomicAdd on ws: sums of integers, bit-reproducible); pass 4 with a workgroup per frame.
 * 1 <= G, N <= 128, 1 <= F <= 2^22, V >= 1, 1 <= A <= 1024, P >= 1, num_class >= 1, agnostic 0 or 1; gt_boxes and bboxes 16-byte,
 * ws 8-byte, every other pointer 4-byte aligned.  The inputs are never written.  vd_hota_ws_bytes: the bytes ws must hold,
 * V * (8 * A * P + 4 * A + 4 * P), -1 for sizes that are not taken. */
int64_t vd_hota_ws_bytes(int V, int A, int P);
int vd_hota_match(const float* gt_boxes, const int32_t* gt_cls, const int32_t* gt_id, const float* ids, const float* scores,
                  const float* bboxes, const int32_t* track, const int32_t* clip_start, int V, int F, int G, int N, int A, int P,
                  int num_class, int agnostic, int32_t* match, float* msim, int32_t* mscore, void* ws, int64_t ws_bytes,
                  void* stream);

/* ---- Detections, tracks and ground truth drawn onto video frames (vd_overlay.hip): what
 * viddet_amd.overlay.overlay_host paints, bit for bit, on the frames and on `painted`.  frames / out: F uint8 frames, frame f
 * at byte f * frame_stride, rows `pitch` bytes apart.  fmt 0: packed RGB, H0 rows of W0 pixels (pitch >= 3 * W0; uv_offset is
 * not read).  fmt 1: NV12 as vd_resize_nv12_nchw takes it - H0 rows of luma, from uv_offset bytes into the frame H0 / 2 rows of
 * interleaved chroma pairs, H0 and W0 even, pitch >= W0, uv_offset >= pitch * H0.  frame_stride covers a frame's last byte.
 * out == frames paints in place: only threads with a painted pixel write.  Otherwise every pixel of out is written (the source
 * where nothing is painted; bytes between rows and planes are not touched) and the two ranges must not overlap.
 * ids, scores [F][N] fp32, bboxes [F][N][4] fp32 in the coordinates of a network input of Hn x Wn; track [F][N] int32 (NULL:
 * no row is tracked); gt (NULL with G == 0) [F][G][gt_stride] fp32 rows x1, y1, x2, y2, class, .., a class < 0 padding;
 * clip_start [V + 1] int32 (NULL with V == 1): a trail of frame f reaches back to the largest offset <= f at most.
 * Row (f, i) is drawn iff ids >= 0, scores >= thresh, the four box values are finite, x1 <= x2 and y1 <= y2.  Its pixel box:
 * sx = (float)W0 / (float)Wn, px0 = (int)clamp(floorf(x1 * sx), 0, W0 - 1), and so on, in single fp32 operations.  Its colour:
 * palette word (class & 255), with by_track and track >= 0 (track & 255); ground truth takes word 256.  Its tag: "#<track> "
 * where tracked, the class name (names [n_names][16] uint8, NUL padded; the decimal class id where names is NULL or the class
 * is beyond it), a space, and q / 100 . q % 100 of q = min(999, (int)(score * 100.0f + 0.5f)); ground truth: the name alone;
 * cut to 32 characters, in the 5 x 7 font `font` ([95][8] uint8: seven row bytes, bit 4 the left column, and a pad byte) at
 * `scale` pixels a font pixel, above the box (inside it where there is no room).  Its trail (tracked rows): the centres of
 * the row and of the lowest drawn row of the same track in each of the `trail` frames before it, joined by segments of
 * `thickness` pixels, a thickness x thickness square on every vertex.  Layers, bottom to top: ground truth, trails, rings of
 * `thickness` pixels growing inward, tags; inside a layer the lower row is on top.  palette [259] uint32: c0 | c1 << 8 |
 * c2 << 16 - (R, G, B), or for NV12 (Y, U, V), no colour arithmetic is done on the device - and bit 24: glyphs on this colour
 * are white (word 258), else black (257).  An NV12 chroma pair (cy, cx) is painted iff luma pixel (2 cy, 2 cx) is, with that
 * pixel's colour.  painted [F] int32: the pixels of each frame that took a colour (NV12: luma pixels).
 * Two launches.  Primitives (stage 1): a workgroup per frame writes one record of VD_OVERLAY_WS_PER_ROW bytes per row and
 * per ground-truth row into ws (overlay.REC_DTYPE: rows [F][N], then ground truth [F][G]) and sets painted to 0; no atomics.
 * Paint (stage 2): a workgroup per (frame, tile of 64 x 16 pixels), a thread per 4 pixels, walks the frame's records top
 * layer first in batches through LDS; nothing limits the primitives of a tile; one integer atomicAdd on painted per workgroup
 * (bit-reproducible).  Where W0, pitch, frame_stride (and uv_offset) are multiples of 4 and frames / out are 4-byte aligned the
 * pixels move as dwords, else byte by byte: frames and out need no alignment.  1 <= N <= 128, 0 <= G <= 128, F >= 1,
 * 1 <= thickness <= 8, 1 <= scale <= 4, 0 <= trail <= 16, H0, W0 <= 8192; bboxes and ws 16-byte, every other table 4-byte
 * aligned.  The rows are never written.  vd_overlay_ws_bytes: the bytes ws must hold, -1 for sizes that are not taken. */
#define VD_OVERLAY_WS_PER_ROW 128
int64_t vd_overlay_ws_bytes(int F, int N, int G);
int vd_overlay(const uint8_t* frames, uint8_t* out, int64_t frame_stride, int64_t pitch, int64_t uv_offset, int fmt, int F, int H0,
               int W0, const float* ids, const float* scores, const float* bboxes, const int32_t* track, const float* gt,
               int gt_stride, const int32_t* clip_start, int V, int N, int G, int Hn, int Wn, float thresh, int thickness, int scale,
               int trail, int by_track, const uint8_t* names, int n_names, const uint32_t* palette, const uint8_t* font,
               int32_t* painted, void* ws, int64_t ws_bytes, void* stream);
/* the same with a mask of the launches to make (tests, tools/overlay_probe.py): 1 (primitives), 2 (paint); vd_overlay is stages
 * 3.  Stage 2 alone paints whatever records ws holds: a vertex count is clamped and every pixel address is formed from
 * coordinates checked against the frame, so nothing outside the frames is touched; painted is added to, not reset. */
int vd_overlay_stages(const uint8_t* frames, uint8_t* out, int64_t frame_stride, int64_t pitch, int64_t uv_offset, int fmt, int F,
                      int H0, int W0, const float* ids, const float* scores, const float* bboxes, const int32_t* track,
                      const float* gt, int gt_stride, const int32_t* clip_start, int V, int N, int G, int Hn, int Wn, float thresh,
                      int thickness, int scale, int trail, int by_track, const uint8_t* names, int n_names,
                      const uint32_t* palette, const uint8_t* font, int32_t* painted, void* ws, int64_t ws_bytes, int stages,
                      void* stream);

/* ---- Camera-motion compensation of the clip trackers (vd_motion.hip): what viddet_amd.motion defines, bit for
 * bit.  All three launch on `stream`, download nothing, wait for nothing and never write their inputs.
 * vd_motion_sig: frames as vd_overlay takes them - F uint8 frames, frame f at byte f * frame_stride, rows `pitch` bytes apart;
 * fmt 0: packed RGB (pitch >= 3 * W0), luma (77 R + 150 G + 29 B + 128) >> 8; fmt 1: the luma plane of NV12 (pitch >= W0; the
 * chroma plane is never read, frame_stride only has to cover the luma rows).  sig [F][Gh][Gw] uint16, Gh = H0 / cell, Gw = W0 /
 * cell: the luma summed over every cell x cell block; the pixels right of Gw * cell and below Gh * cell are not read.  cell
 * is 2, 4, 8 or 16; cell <= H0, W0 <= 16384.  Where frames, pitch and frame_stride are multiples of 16 the pixels move as
 * 16-byte loads, else byte by byte, with the same result; frames need no alignment.
 * vd_motion_match: sig [F][Gh][Gw] of F frames in V clips, clip_start [V + 1] int32 (NULL with V == 1; cut to [0, F)).  For
 * every frame t that is not the first of its clip and every (dx, dy) in [-radius, radius]^2, SAD(dx, dy) = the sum over gy in
 * [radius, Gh - radius), gx in [radius, Gw - radius) of |sig[t][gy][gx] - sig[t-1][gy-dy][gx-dx]|; the winner is the least
 * (SAD, dx*dx + dy*dy, dy, dx); sad [F][2] int64 = (SAD(winner), SAD(0,0)); motion [F][2] int32 = (dx * cell, dy * cell) iff
 * SAD(winner) * 256 <= SAD(0,0) * (int)(gate * 256.0f), else (0, 0); cum [F][2] int32 the running sum of motion inside the
 * clip.  First frames of clips and frames that no clip covers get zeros.  1 <= radius <= 16, 0 < gate <= 1, 2 * radius < Gh,
 * Gw <= 4096.  ws: vd_motion_match_ws_bytes(F, radius) = 8 * F * (2 * radius + 1)^2 bytes, 8-byte aligned (-1: sizes that are not
 * taken).  Two launches, no atomics.
 * vd_motion_shift: out [F][N][4] = boxes [F][N][4] with (float)cum[t].x * sx added to x1 and x2 and (float)cum[t].y * sy to
 * y1 and y2 (sign +1) or subtracted (sign -1), one fp32 multiply and one fp32 add or subtract each, on the rows whose key is
 * >= 0 - key [F][N] fp32 ids (a NaN is not >= 0) with key_is_track 0, int32 track ids with 1; the other rows keep their bits.
 * out must not be boxes; both 16-byte aligned. */
int vd_motion_sig(const uint8_t* frames, int64_t frame_stride, int64_t pitch, int fmt, int F, int H0, int W0, int cell, uint16_t* sig,
                  void* stream);
int64_t vd_motion_match_ws_bytes(int F, int radius);
int vd_motion_match(const uint16_t* sig, const int32_t* clip_start, int V, int F, int Gh, int Gw, int cell, int radius, float gate,
                    int32_t* motion, int64_t* sad, int32_t* cum, void* ws, int64_t ws_bytes, void* stream);
int vd_motion_shift(const void* key, int key_is_track, const float* boxes, const int32_t* cum, int F, int N, float sx, float sy, int sign,
                    float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIDDET_HIP_H */
