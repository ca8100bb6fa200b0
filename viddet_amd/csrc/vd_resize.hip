// vd_resize.hip — resize of raw uint8 video frames on the device, fused with the normalisation of the input path
// (YOLOV3.set_device_resize): [N,H0,W0,3] uint8 -> the planar fp32 batch [N,3,H,W] the stem reads, and, on
// request, the resized uint8 frame [N,H,W,3] itself.
//
// The resample is the separable operator of viddet_amd/video.py imresize: per axis a table of T taps per output index,
//   out[d] = sum_k w[d][k] * in[idx[d][k]]      (video.py _axis_taps: area, bilinear, bicubic, Lanczos; indices clipped)
// so one kernel serves every interpolation.  Arithmetic is fp32 in a fixed order: per source row the horizontal sum over
// k = 0 .. Tx-1 with fmaf from 0, then the vertical sum over k = 0 .. Ty-1 with fmaf from 0; then rintf (half to even, as
// np.rint), clamp to [0, 255] and vd_normalize_level of the rounded value (vd_preprocess.h: the function
// vd_preprocess_u8_nchw applies) -> `out` is bit-equal to vd_preprocess_u8_nchw on `out_u8`.
//
// Work shape: a workgroup of 256 threads owns TH x TW output pixels of one frame.
//   1. the tile's slices of the four tables go to LDS (indices clamped into the frame on the way) and a wave reduction
//      gives the tile's source rows [rlo, rhi] and columns [clo, chi];
//   2. in batches of RB source rows: a wave copies one row's bytes [clo*3, (chi+1)*3) to LDS with aligned dword loads
//      (64 lanes = 256 contiguous bytes; a dword that reaches outside the buffer is put together from byte loads), then
//      a wave resamples one row horizontally out of LDS into the float stage [row][col*3 + ch];
//   3. the vertical pass reads the stage (lane stride 3 floats: conflict-free over 32 banks) and stores `out` along W per
//      plane, 64 consecutive floats per wave-instruction.
// Every source byte a tile needs is read from global memory once per tile.  The tile (TH, TW), the stage's rows and the
// batch are chosen on the host from H0/H, W0/W and the tap counts so that everything fits in 64 KB of LDS (two or more
// workgroups per CU).  The kernel does not trust the tables: indices are clamped into the frame and then into the staged
// span, so a bad table reads a wrong pixel, never memory outside the frame or the stage.  Plain loads and stores, no
// atomics: two runs give the same bits.
//
// k_resize_nv12_nchw (below) is the same operator on NV12 frames: the colour conversion sits between the row copy and the
// horizontal pass.
#include "vd_common.h"
#include "vd_preprocess.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kLdsBudget = 64 * 1024;         // all of a workgroup's LDS
constexpr int kRawRowBudget = 16 * 1024;      // one staged source row's bytes at most
constexpr int kMaxTaps = 16;

// launch geometry: TH x (1 << tw_shift) output pixels per tile, RMAX float rows in the stage, CMAX source columns and
// DWROW dwords per raw row, RB raw rows per batch
struct ResizeGeo {
    int TH, tw_shift, RMAX, CMAX, RB, DWROW;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(kThreads) void k_resize_u8_nchw(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                             uint8_t* __restrict__ out_u8, int64_t in_bytes, int H0, int W0, int H,
                                                             int W, const int32_t* __restrict__ idx_y,
                                                             const float* __restrict__ w_y, int Ty,
                                                             const int32_t* __restrict__ idx_x,
                                                             const float* __restrict__ w_x, int Tx, int tiles_x, int tiles_y,
                                                             ResizeGeo g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int TW = 1 << g.tw_shift, TW3 = TW * 3, TH = g.TH;
    float* stage = reinterpret_cast<float*>(smem);                 // [RMAX][TW3]
    float* s_wx = stage + g.RMAX * TW3;                            // [TW][Tx]
    int* s_ix = reinterpret_cast<int*>(s_wx + TW * Tx);
    float* s_wy = reinterpret_cast<float*>(s_ix + TW * Tx);        // [TH][Ty]
    int* s_iy = reinterpret_cast<int*>(s_wy + TH * Ty);
    int* s_red = s_iy + TH * Ty;                                   // [4][kWaves]
    uint32_t* raw = reinterpret_cast<uint32_t*>(s_red + 4 * kWaves);   // [RB][DWROW]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, n = b / tiles_y;
    const int ox0 = tx * TW, oy0 = ty * TH;
    const int ncol_out = min(TW, W - ox0), nrow_out = min(TH, H - oy0);

    // 1. the tile's tables, clamped into the frame; entries of columns / rows past the frame's edge carry weight 0
    int lo_x = W0, hi_x = -1, lo_y = H0, hi_y = -1;
    for (int e = tid; e < TW * Tx; e += kThreads) {
        int i = 0;
        float w = 0.f;
        if (e < ncol_out * Tx) {
            i = clampi(idx_x[(int64_t)ox0 * Tx + e], 0, W0 - 1);
            w = w_x[(int64_t)ox0 * Tx + e];
            lo_x = min(lo_x, i);
            hi_x = max(hi_x, i);
        }
        s_ix[e] = i;
        s_wx[e] = w;
    }
    for (int e = tid; e < TH * Ty; e += kThreads) {
        int i = 0;
        float w = 0.f;
        if (e < nrow_out * Ty) {
            i = clampi(idx_y[(int64_t)oy0 * Ty + e], 0, H0 - 1);
            w = w_y[(int64_t)oy0 * Ty + e];
            lo_y = min(lo_y, i);
            hi_y = max(hi_y, i);
        }
        s_iy[e] = i;
        s_wy[e] = w;
    }
    lo_x = wave_min(lo_x), hi_x = wave_max(hi_x), lo_y = wave_min(lo_y), hi_y = wave_max(hi_y);
    if (lane == 0) {
        s_red[wave] = lo_x, s_red[kWaves + wave] = hi_x, s_red[2 * kWaves + wave] = lo_y, s_red[3 * kWaves + wave] = hi_y;
    }
    __syncthreads();
    int clo = s_red[0], chi = s_red[kWaves], rlo = s_red[2 * kWaves], rhi = s_red[3 * kWaves];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        clo = min(clo, s_red[w]), chi = max(chi, s_red[kWaves + w]);
        rlo = min(rlo, s_red[2 * kWaves + w]), rhi = max(rhi, s_red[3 * kWaves + w]);
    }
    // (a tile has at least one row and one column, so the spans are not empty; tables that span more than the host sized
    // the stage for are cut to it - wrong pixels, no access outside)
    const int nrows = min(rhi - rlo + 1, g.RMAX), ncols = min(chi - clo + 1, g.CMAX);
    const int rowbytes = ncols * 3;
    const uintptr_t buf_lo = reinterpret_cast<uintptr_t>(in), buf_hi = buf_lo + (uintptr_t)in_bytes;

    // 2. source rows -> LDS bytes -> horizontally resampled float rows
    for (int r0 = 0; r0 < nrows; r0 += g.RB) {
        const int rb = min(g.RB, nrows - r0);
        for (int q = wave; q < rb; q += kWaves) {
            const uint8_t* p = in + (((int64_t)n * H0 + (rlo + r0 + q)) * W0 + clo) * 3;
            const int ph = (int)(reinterpret_cast<uintptr_t>(p) & 3);
            const uint8_t* pa = p - ph;                            // 4-byte aligned; LDS keeps the row's phase
            const int ndw = (ph + rowbytes + 3) >> 2;              // <= DWROW
            uint32_t* dst = raw + q * g.DWROW;
            for (int i = lane; i < ndw; i += 64) {
                const uint8_t* a = pa + 4 * i;
                const uintptr_t ua = reinterpret_cast<uintptr_t>(a);
                uint32_t v;
                if (ua >= buf_lo && ua + 4 <= buf_hi) {
                    v = *reinterpret_cast<const uint32_t*>(a);
                } else {                                           // the buffer's first / last bytes
                    v = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (ua + e >= buf_lo && ua + e < buf_hi) v |= (uint32_t)a[e] << (8 * e);
                }
                dst[i] = v;
            }
        }
        __syncthreads();
        for (int q = wave; q < rb; q += kWaves) {
            const uint8_t* p = in + (((int64_t)n * H0 + (rlo + r0 + q)) * W0 + clo) * 3;
            const int ph = (int)(reinterpret_cast<uintptr_t>(p) & 3);
            const uint8_t* src = reinterpret_cast<const uint8_t*>(raw + q * g.DWROW) + ph;
            float* dst = stage + (r0 + q) * TW3;
            for (int e = lane; e < TW3; e += 64) {
                const int col = e / 3, ch = e - col * 3;
                const int* ix = s_ix + col * Tx;
                const float* wx = s_wx + col * Tx;
                float acc = 0.f;
                for (int k = 0; k < Tx; ++k) {
                    const int c = clampi(ix[k] - clo, 0, ncols - 1);
                    acc = fmaf(wx[k], (float)src[c * 3 + ch], acc);
                }
                dst[e] = acc;
            }
        }
        __syncthreads();
    }

    // 3. vertical pass out of the stage, rounding, normalisation
    const int64_t hw = (int64_t)H * W;
    for (int j = tid; j < nrow_out * TW3; j += kThreads) {
        const int ox = j & (TW - 1), t = j >> g.tw_shift;
        const int oyl = t / 3, ch = t - oyl * 3;
        if (ox >= ncol_out) continue;
        const int* iy = s_iy + oyl * Ty;
        const float* wy = s_wy + oyl * Ty;
        float acc = 0.f;
        for (int k = 0; k < Ty; ++k) {
            const int r = clampi(iy[k] - rlo, 0, nrows - 1);
            acc = fmaf(wy[k], stage[r * TW3 + ox * 3 + ch], acc);
        }
        const float v = fminf(fmaxf(rintf(acc), 0.f), 255.f);
        const int64_t pix = (int64_t)(oy0 + oyl) * W + (ox0 + ox);
        out[((int64_t)n * 3 + ch) * hw + pix] = vd_normalize_level(v, ch);
        if (out_u8) out_u8[((int64_t)n * hw + pix) * 3 + ch] = (uint8_t)v;
    }
}

inline size_t lds_bytes(const ResizeGeo& g, int Ty, int Tx) {
    const int TW = 1 << g.tw_shift;
    return (size_t)g.RMAX * TW * 3 * 4 + (size_t)(TW * Tx + g.TH * Ty) * 8 + 4 * kWaves * 4 + (size_t)g.RB * g.DWROW * 4;
}

// The largest tile whose staged rows fit: TH output rows need at most ceil(TH * H0 / H) + Ty + 1 source rows (the taps of
// consecutive outputs advance by H0 / H; _axis_taps), TW columns ceil(TW * W0 / W) + Tx + 1 source columns.
inline bool pick_geo(int H0, int W0, int H, int W, int Ty, int Tx, ResizeGeo* out) {
    for (int tw_shift = 6; tw_shift >= 4; --tw_shift) {
        const int TW = 1 << tw_shift;
        ResizeGeo g;
        g.tw_shift = tw_shift;
        const int64_t cm = vd_cdiv((int64_t)TW * W0, W) + Tx + 1;
        g.CMAX = (int)(cm < W0 ? cm : W0);
        g.DWROW = (g.CMAX * 3 + 6) / 4;                            // a phase of up to 3 bytes in front, rounded up
        if ((int64_t)g.DWROW * 4 > kRawRowBudget) continue;
        for (g.TH = 16; g.TH >= 1; g.TH >>= 1) {
            const int64_t rm = vd_cdiv((int64_t)g.TH * H0, H) + Ty + 1;
            g.RMAX = (int)(rm < H0 ? rm : H0);
            g.RB = 0;
            const int64_t left = (int64_t)kLdsBudget - (int64_t)lds_bytes(g, Ty, Tx);
            if (left < (int64_t)g.DWROW * 4) continue;
            const int64_t rbm = left / ((int64_t)g.DWROW * 4);
            g.RB = (int)(rbm < g.RMAX ? rbm : g.RMAX);
            *out = g;
            return true;
        }
    }
    return false;
}

// ---- NV12 sources (vd_resize_nv12_nchw): the same tile, tables, passes and arithmetic as above on frames that
// arrive as two planes - H0 rows of luma, then H0/2 rows of interleaved U V pairs, `pitch` bytes per row in both, a frame every
// `frame_stride` bytes, its chroma plane `uv_offset` bytes in.  Per batch of source rows a wave stages one Y row's bytes
// [clo, chi] or one UV row's bytes [clo & ~1, chi | 1] (UV row r >> 1 serves Y rows r and r ^ 1: staged once per batch), one
// pass turns each staged Y row into packed RGB bytes in LDS - a lane per source pixel, once per pixel, the integer arithmetic
// of viddet_amd/video.py nv12_to_rgb with the seven integers the host passes - and the horizontal pass reads those bytes as
// k_resize_u8_nchw reads its raw rows: the result is bit-equal to vd_resize_u8_nchw on nv12_to_rgb of the frames.

// off, gain, ru, rv, gu, gv, bu of video.py NV12_MATRICES
struct Nv12Coef {
    int off, gain, ru, rv, gu, gv, bu;
};

// ResizeGeo with the raw row split in three: DWY dwords per staged Y row, DWUV per staged UV row ([RB/2 + 1] of them),
// DWRGB per converted row
struct Nv12Geo {
    int TH, tw_shift, RMAX, CMAX, RB, DWY, DWUV, DWRGB;
};

// bytes [p, p + nbytes) -> dst, keeping p's phase in its dword: aligned dword loads, a dword that reaches outside
// [buf_lo, buf_hi) put together from the bytes inside it (k_resize_u8_nchw's row copy)
__device__ __forceinline__ void stage_row_bytes(const uint8_t* p, int nbytes, uint32_t* dst, int lane, uintptr_t buf_lo,
                                                uintptr_t buf_hi) {
    const int ph = (int)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint8_t* pa = p - ph;
    const int ndw = (ph + nbytes + 3) >> 2;
    for (int i = lane; i < ndw; i += 64) {
        const uint8_t* a = pa + 4 * i;
        const uintptr_t ua = reinterpret_cast<uintptr_t>(a);
        uint32_t v;
        if (ua >= buf_lo && ua + 4 <= buf_hi) {
            v = *reinterpret_cast<const uint32_t*>(a);
        } else {
            v = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (ua + e >= buf_lo && ua + e < buf_hi) v |= (uint32_t)a[e] << (8 * e);
        }
        dst[i] = v;
    }
}

__global__ __launch_bounds__(kThreads) void k_resize_nv12_nchw(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                               uint8_t* __restrict__ out_u8, int64_t in_bytes,
                                                               int64_t frame_stride, int64_t pitch, int64_t uv_offset, int H0,
                                                               int W0, int H, int W, const int32_t* __restrict__ idx_y,
                                                               const float* __restrict__ w_y, int Ty,
                                                               const int32_t* __restrict__ idx_x,
                                                               const float* __restrict__ w_x, int Tx, int tiles_x, int tiles_y,
                                                               Nv12Geo g, Nv12Coef m) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int TW = 1 << g.tw_shift, TW3 = TW * 3, TH = g.TH;
    float* stage = reinterpret_cast<float*>(smem);                 // [RMAX][TW3]
    float* s_wx = stage + g.RMAX * TW3;                            // [TW][Tx]
    int* s_ix = reinterpret_cast<int*>(s_wx + TW * Tx);
    float* s_wy = reinterpret_cast<float*>(s_ix + TW * Tx);        // [TH][Ty]
    int* s_iy = reinterpret_cast<int*>(s_wy + TH * Ty);
    int* s_red = s_iy + TH * Ty;                                   // [4][kWaves]
    uint32_t* raw_y = reinterpret_cast<uint32_t*>(s_red + 4 * kWaves);   // [RB][DWY]
    uint32_t* raw_uv = raw_y + g.RB * g.DWY;                       // [RB / 2 + 1][DWUV]
    uint32_t* rgb = raw_uv + (g.RB / 2 + 1) * g.DWUV;              // [RB][DWRGB]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, n = b / tiles_y;
    const int ox0 = tx * TW, oy0 = ty * TH;
    const int ncol_out = min(TW, W - ox0), nrow_out = min(TH, H - oy0);

    // 1. the tile's tables, clamped into the frame; entries of columns / rows past the frame's edge carry weight 0
    int lo_x = W0, hi_x = -1, lo_y = H0, hi_y = -1;
    for (int e = tid; e < TW * Tx; e += kThreads) {
        int i = 0;
        float w = 0.f;
        if (e < ncol_out * Tx) {
            i = clampi(idx_x[(int64_t)ox0 * Tx + e], 0, W0 - 1);
            w = w_x[(int64_t)ox0 * Tx + e];
            lo_x = min(lo_x, i);
            hi_x = max(hi_x, i);
        }
        s_ix[e] = i;
        s_wx[e] = w;
    }
    for (int e = tid; e < TH * Ty; e += kThreads) {
        int i = 0;
        float w = 0.f;
        if (e < nrow_out * Ty) {
            i = clampi(idx_y[(int64_t)oy0 * Ty + e], 0, H0 - 1);
            w = w_y[(int64_t)oy0 * Ty + e];
            lo_y = min(lo_y, i);
            hi_y = max(hi_y, i);
        }
        s_iy[e] = i;
        s_wy[e] = w;
    }
    lo_x = wave_min(lo_x), hi_x = wave_max(hi_x), lo_y = wave_min(lo_y), hi_y = wave_max(hi_y);
    if (lane == 0) {
        s_red[wave] = lo_x, s_red[kWaves + wave] = hi_x, s_red[2 * kWaves + wave] = lo_y, s_red[3 * kWaves + wave] = hi_y;
    }
    __syncthreads();
    int clo = s_red[0], chi = s_red[kWaves], rlo = s_red[2 * kWaves], rhi = s_red[3 * kWaves];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        clo = min(clo, s_red[w]), chi = max(chi, s_red[kWaves + w]);
        rlo = min(rlo, s_red[2 * kWaves + w]), rhi = max(rhi, s_red[3 * kWaves + w]);
    }
    // (spans cut to what the host sized the stage for, as in k_resize_u8_nchw)
    const int nrows = min(rhi - rlo + 1, g.RMAX), ncols = min(chi - clo + 1, g.CMAX);
    // the chroma pairs of columns [clo, clo + ncols): bytes [ulo, uhi] of a UV row; W0 is even, so uhi <= W0 - 1
    const int ulo = clo & ~1, uhi = (clo + ncols - 1) | 1;
    const uintptr_t buf_lo = reinterpret_cast<uintptr_t>(in), buf_hi = buf_lo + (uintptr_t)in_bytes;
    const uint8_t* frame = in + (int64_t)n * frame_stride;
    const uint8_t* plane_uv = frame + uv_offset;

    // 2. source rows -> LDS bytes -> RGB bytes -> horizontally resampled float rows
    for (int r0 = 0; r0 < nrows; r0 += g.RB) {
        const int rb = min(g.RB, nrows - r0);
        const int uv0 = (rlo + r0) >> 1, nuv = ((rlo + r0 + rb - 1) >> 1) - uv0 + 1;      // <= RB / 2 + 1 chroma rows
        for (int q = wave; q < rb + nuv; q += kWaves) {
            if (q < rb)
                stage_row_bytes(frame + (int64_t)(rlo + r0 + q) * pitch + clo, ncols, raw_y + q * g.DWY, lane, buf_lo, buf_hi);
            else
                stage_row_bytes(plane_uv + (int64_t)(uv0 + q - rb) * pitch + ulo, uhi - ulo + 1, raw_uv + (q - rb) * g.DWUV, lane,
                                buf_lo, buf_hi);
        }
        __syncthreads();
        for (int q = wave; q < rb; q += kWaves) {
            const int r = rlo + r0 + q;
            const uint8_t* py = frame + (int64_t)r * pitch + clo;
            const uint8_t* pu = plane_uv + (int64_t)(r >> 1) * pitch + ulo;
            const uint8_t* sy = reinterpret_cast<const uint8_t*>(raw_y + q * g.DWY) + (reinterpret_cast<uintptr_t>(py) & 3);
            const uint8_t* su =
                reinterpret_cast<const uint8_t*>(raw_uv + ((r >> 1) - uv0) * g.DWUV) + (reinterpret_cast<uintptr_t>(pu) & 3);
            uint8_t* dst = reinterpret_cast<uint8_t*>(rgb + q * g.DWRGB);
            for (int c = lane; c < ncols; c += 64) {
                const int u = ((clo + c) & ~1) - ulo;                                     // the pixel's pair in the staged span
                const int C = (int)sy[c] - m.off, D = (int)su[u] - 128, E = (int)su[u + 1] - 128;
                const int y = m.gain * C + 128;
                dst[c * 3 + 0] = (uint8_t)clampi((y + m.ru * D + m.rv * E) >> 8, 0, 255);
                dst[c * 3 + 1] = (uint8_t)clampi((y + m.gu * D + m.gv * E) >> 8, 0, 255);
                dst[c * 3 + 2] = (uint8_t)clampi((y + m.bu * D) >> 8, 0, 255);
            }
        }
        __syncthreads();
        for (int q = wave; q < rb; q += kWaves) {
            const uint8_t* src = reinterpret_cast<const uint8_t*>(rgb + q * g.DWRGB);
            float* dst = stage + (r0 + q) * TW3;
            for (int e = lane; e < TW3; e += 64) {
                const int col = e / 3, ch = e - col * 3;
                const int* ix = s_ix + col * Tx;
                const float* wx = s_wx + col * Tx;
                float acc = 0.f;
                for (int k = 0; k < Tx; ++k) {
                    const int c = clampi(ix[k] - clo, 0, ncols - 1);
                    acc = fmaf(wx[k], (float)src[c * 3 + ch], acc);
                }
                dst[e] = acc;
            }
        }
        __syncthreads();
    }

    // 3. vertical pass out of the stage, rounding, normalisation
    const int64_t hw = (int64_t)H * W;
    for (int j = tid; j < nrow_out * TW3; j += kThreads) {
        const int ox = j & (TW - 1), t = j >> g.tw_shift;
        const int oyl = t / 3, ch = t - oyl * 3;
        if (ox >= ncol_out) continue;
        const int* iy = s_iy + oyl * Ty;
        const float* wy = s_wy + oyl * Ty;
        float acc = 0.f;
        for (int k = 0; k < Ty; ++k) {
            const int r = clampi(iy[k] - rlo, 0, nrows - 1);
            acc = fmaf(wy[k], stage[r * TW3 + ox * 3 + ch], acc);
        }
        const float v = fminf(fmaxf(rintf(acc), 0.f), 255.f);
        const int64_t pix = (int64_t)(oy0 + oyl) * W + (ox0 + ox);
        out[((int64_t)n * 3 + ch) * hw + pix] = vd_normalize_level(v, ch);
        if (out_u8) out_u8[((int64_t)n * hw + pix) * 3 + ch] = (uint8_t)v;
    }
}

inline size_t lds_bytes_nv12(const Nv12Geo& g, int Ty, int Tx) {
    const int TW = 1 << g.tw_shift;
    return (size_t)g.RMAX * TW * 3 * 4 + (size_t)(TW * Tx + g.TH * Ty) * 8 + 4 * kWaves * 4 +
           ((size_t)g.RB * (g.DWY + g.DWRGB) + (size_t)(g.RB / 2 + 1) * g.DWUV) * 4;
}

// pick_geo with the batch's three row kinds: RB Y rows, their RB / 2 + 1 UV rows and RB converted rows must fit beside the
// stage and the tables; the largest such RB, at least 1
inline bool pick_geo_nv12(int H0, int W0, int H, int W, int Ty, int Tx, Nv12Geo* out) {
    for (int tw_shift = 6; tw_shift >= 4; --tw_shift) {
        const int TW = 1 << tw_shift;
        Nv12Geo g;
        g.tw_shift = tw_shift;
        const int64_t cm = vd_cdiv((int64_t)TW * W0, W) + Tx + 1;
        g.CMAX = (int)(cm < W0 ? cm : W0);
        g.DWY = (g.CMAX + 6) / 4;                                  // a phase of up to 3 bytes in front, rounded up
        g.DWUV = (g.CMAX + 2 + 6) / 4;                             // the span grows by a byte at either end to whole pairs
        g.DWRGB = (g.CMAX * 3 + 3) / 4;
        if ((int64_t)g.DWRGB * 4 > kRawRowBudget) continue;
        for (g.TH = 16; g.TH >= 1; g.TH >>= 1) {
            const int64_t rm = vd_cdiv((int64_t)g.TH * H0, H) + Ty + 1;
            g.RMAX = (int)(rm < H0 ? rm : H0);
            for (g.RB = g.RMAX; g.RB >= 1; --g.RB)
                if (lds_bytes_nv12(g, Ty, Tx) <= (size_t)kLdsBudget) break;
            if (g.RB < 1) continue;
            *out = g;
            return true;
        }
    }
    return false;
}

}  // namespace

extern "C" {

int vd_resize_u8_nchw(const uint8_t* in, float* out, uint8_t* out_u8, int N, int H0, int W0, int H, int W, const int32_t* idx_y,
                      const float* w_y, int Ty, const int32_t* idx_x, const float* w_x, int Tx, void* stream) {
    VD_REQUIRE(in && out && idx_y && w_y && idx_x && w_x,
               "vd_resize_u8_nchw: in, out and the four tap tables (idx_y, w_y, idx_x, w_x) must not be NULL");
    VD_REQUIRE(N >= 1 && H0 >= 1 && W0 >= 1 && H >= 1 && W >= 1,
               "vd_resize_u8_nchw: all sizes must be >= 1, got N=%d H0=%d W0=%d H=%d W=%d", N, H0, W0, H, W);
    VD_REQUIRE(Ty >= 1 && Ty <= kMaxTaps && Tx >= 1 && Tx <= kMaxTaps, "vd_resize_u8_nchw: 1 <= Ty, Tx <= %d needed, got Ty=%d Tx=%d",
               kMaxTaps, Ty, Tx);
    VD_REQUIRE((((uintptr_t)idx_y | (uintptr_t)w_y | (uintptr_t)idx_x | (uintptr_t)w_x | (uintptr_t)out) % 4) == 0,
               "vd_resize_u8_nchw: out and the tap tables must be 4-byte aligned");
    ResizeGeo g;
    VD_REQUIRE(pick_geo(H0, W0, H, W, Ty, Tx, &g),
               "vd_resize_u8_nchw: the staged source rows of a %dx%d -> %dx%d resize with Ty=%d Tx=%d do not fit in %d KB of LDS",
               H0, W0, H, W, Ty, Tx, kLdsBudget / 1024);
    const int TW = 1 << g.tw_shift;
    const int64_t tiles_x = vd_cdiv(W, TW), tiles_y = vd_cdiv(H, g.TH), blocks = tiles_x * tiles_y * N;
    VD_REQUIRE(blocks < ((int64_t)1 << 31), "vd_resize_u8_nchw: %lld tiles are more than one launch takes", (long long)blocks);
    hipLaunchKernelGGL(k_resize_u8_nchw, dim3((unsigned)blocks), dim3(kThreads), lds_bytes(g, Ty, Tx), (hipStream_t)stream, in, out,
                       out_u8, (int64_t)N * H0 * W0 * 3, H0, W0, H, W, idx_y, w_y, Ty, idx_x, w_x, Tx, (int)tiles_x, (int)tiles_y, g);
    VD_CHECK_LAUNCH("vd_resize_u8_nchw");
    return VD_OK;
}

int vd_resize_nv12_nchw(const uint8_t* in, int64_t in_bytes, int64_t frame_stride, int64_t pitch, int64_t uv_offset, float* out,
                        uint8_t* out_u8, int N, int H0, int W0, int H, int W, const int32_t* idx_y, const float* w_y, int Ty,
                        const int32_t* idx_x, const float* w_x, int Tx, int off, int gain, int ru, int rv, int gu, int gv, int bu,
                        void* stream) {
    VD_REQUIRE(in && out && idx_y && w_y && idx_x && w_x,
               "vd_resize_nv12_nchw: in, out and the four tap tables (idx_y, w_y, idx_x, w_x) must not be NULL");
    VD_REQUIRE(N >= 1 && H0 >= 1 && W0 >= 1 && H >= 1 && W >= 1,
               "vd_resize_nv12_nchw: all sizes must be >= 1, got N=%d H0=%d W0=%d H=%d W=%d", N, H0, W0, H, W);
    VD_REQUIRE(H0 % 2 == 0 && W0 % 2 == 0,
               "vd_resize_nv12_nchw: NV12 has one chroma pair per 2 x 2 block, H0 and W0 must be even, got H0=%d W0=%d", H0, W0);
    VD_REQUIRE(pitch >= W0 && pitch < ((int64_t)1 << 31), "vd_resize_nv12_nchw: W0 <= pitch < 2^31 needed, got pitch=%lld W0=%d",
               (long long)pitch, W0);
    VD_REQUIRE(uv_offset >= pitch * H0, "vd_resize_nv12_nchw: the UV plane starts behind the Y plane, uv_offset >= pitch * H0 = %lld "
               "needed, got uv_offset=%lld", (long long)(pitch * H0), (long long)uv_offset);
    VD_REQUIRE(frame_stride >= uv_offset + pitch * (H0 / 2) && frame_stride < ((int64_t)1 << 40),
               "vd_resize_nv12_nchw: a frame holds both planes, uv_offset + pitch * H0 / 2 = %lld <= frame_stride < 2^40 needed, got "
               "frame_stride=%lld", (long long)(uv_offset + pitch * (H0 / 2)), (long long)frame_stride);
    // the last byte a launch may read is the last chroma byte of the last frame's last UV row: nothing behind it need exist
    const int64_t need = (int64_t)(N - 1) * frame_stride + uv_offset + pitch * (H0 / 2 - 1) + W0;
    VD_REQUIRE(in_bytes >= need,
               "vd_resize_nv12_nchw: in_bytes=%lld is less than the %lld bytes N=%d frames reach ((N - 1) * frame_stride + uv_offset + "
               "pitch * (H0 / 2 - 1) + W0)", (long long)in_bytes, (long long)need, N);
    VD_REQUIRE(Ty >= 1 && Ty <= kMaxTaps && Tx >= 1 && Tx <= kMaxTaps, "vd_resize_nv12_nchw: 1 <= Ty, Tx <= %d needed, got Ty=%d Tx=%d",
               kMaxTaps, Ty, Tx);
    VD_REQUIRE((((uintptr_t)idx_y | (uintptr_t)w_y | (uintptr_t)idx_x | (uintptr_t)w_x | (uintptr_t)out) % 4) == 0,
               "vd_resize_nv12_nchw: out and the tap tables must be 4-byte aligned");
    Nv12Geo g;
    VD_REQUIRE(pick_geo_nv12(H0, W0, H, W, Ty, Tx, &g),
               "vd_resize_nv12_nchw: the staged source rows of a %dx%d -> %dx%d resize with Ty=%d Tx=%d do not fit in %d KB of LDS",
               H0, W0, H, W, Ty, Tx, kLdsBudget / 1024);
    const int TW = 1 << g.tw_shift;
    const int64_t tiles_x = vd_cdiv(W, TW), tiles_y = vd_cdiv(H, g.TH), blocks = tiles_x * tiles_y * N;
    VD_REQUIRE(blocks < ((int64_t)1 << 31), "vd_resize_nv12_nchw: %lld tiles are more than one launch takes", (long long)blocks);
    const Nv12Coef m = {off, gain, ru, rv, gu, gv, bu};
    hipLaunchKernelGGL(k_resize_nv12_nchw, dim3((unsigned)blocks), dim3(kThreads), lds_bytes_nv12(g, Ty, Tx), (hipStream_t)stream, in,
                       out, out_u8, in_bytes, frame_stride, pitch, uv_offset, H0, W0, H, W, idx_y, w_y, Ty, idx_x, w_x, Tx,
                       (int)tiles_x, (int)tiles_y, g, m);
    VD_CHECK_LAUNCH("vd_resize_nv12_nchw");
    return VD_OK;
}

}  // extern "C"
