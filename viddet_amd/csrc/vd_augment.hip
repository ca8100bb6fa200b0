// vd_augment.hip — the pixel half of the training augmentation on the device (YOLO3VideoTrainTransform(device_augment=True),
// viddet_amd/augment.py): raw uint8 frames of N samples (K frames each, any source size per sample) -> the
// normalised planar fp32 batch [N*K,3,H,W] the training step reads.  Every decision (colour draws, expansion, constrained
// crop, interpolation, flip) was taken on the host and arrives as a per-sample record:
//   color[12]   M (3x3, row-major, M[i][c]) and b (3): the composed colour distortion  level_c = sum_i x_i M[i][c] + b[c]
//   idx/w y,x   per-axis tap tables of the crop -> (H,W) resize in SOURCE coordinates (video.py _axis_taps, shifted by the crop
//               origin minus the expansion offset; x rows reversed by a flip); index -1 = the tap lies on the canvas fill
//   fill[3]     the expansion canvas' colour (not distorted)
//
// Arithmetic, fp32, per output pixel (oy, ox) of a frame, in this order:
//   1. per source row r = idx_y[oy][ky] >= 0, per input channel i:  h_r[i] = sum over kx = 0 .. Tx-1 with idx_x[ox][kx] >= 0 of
//      w_x[ox][kx] * x[r][idx_x[ox][kx]][i], fmaf from 0;
//   2. S[i] = sum over ky = 0 .. Ty-1 with idx_y[oy][ky] >= 0 of w_y[oy][ky] * h_r[i], fmaf from 0;
//   3. per axis Wsrc_a = sum of the weights of taps with index >= 0, Wall_a = sum of all weights, plain adds from 0 in tap
//      order; Wsrc = Wsrc_y * Wsrc_x, Wall = Wall_y * Wall_x;
//   4. the colour affine ONCE per output pixel (source membership is a rectangle, so it commutes with the resample):
//      t = S[0] * M[0][c]; t = fmaf(S[1], M[1][c], t); t = fmaf(S[2], M[2][c], t); t = fmaf(b[c], Wsrc, t);
//      t = fmaf(fill[c], Wall - Wsrc, t);
//   5. out = vd_normalize_level(t, c) - no rounding to uint8 anywhere.
// tests/augment_oracle.py restates exactly this in NumPy.
//
// Work shape: a workgroup of 256 threads owns an 8 x 32 tile of output pixels of one frame, one thread per pixel in the last
// pass.
//   a. the tile's slices of the sample's four tables go to LDS, transposed to [tap][column] (conflict-free reads), indices
//      clamped into the source on the way; a wave reduction gives the tile's span of source rows [rlo, rhi];
//   b. if the span fits the stage (kRMax rows): every source row of the span is resampled horizontally ONCE into the float
//      stage [row][col*3 + ch] (byte loads of consecutive lanes fall on consecutive addresses of one source row), then each
//      thread sums its pixel's vertical taps out of the stage (lane stride 3 floats: conflict-free);
//   c. otherwise (a tile of a very strong shrink) each thread gathers its own taps from global memory - the same sums in the
//      same order, so both paths give the same bits.
// A tile of an expanded frame that lies in the fill has an empty span and reads no pixel.  The kernel trusts no table: an
// index below 0 is fill, one at or above the source's size is clamped into it, so a bad table reads a wrong pixel of the
// sample's own frames, never anything else (src_off / src_hw are the host's statement of where those frames are).  Plain loads
// and stores, no atomics: two runs give the same bits.
#include "vd_common.h"
#include "vd_preprocess.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTH = 8, kTW = 32, kTW3 = kTW * 3;
constexpr int kMaxTaps = 32;
constexpr int kRMax = 64;                     // staged source rows: 64 * 96 floats = 24 KB of the workgroup's ~35 KB

__global__ __launch_bounds__(kThreads) void k_augment_u8_nchw(const uint8_t* __restrict__ raw, const int64_t* __restrict__ src_off,
                                                              const int32_t* __restrict__ src_hw, const float* __restrict__ color,
                                                              const int32_t* __restrict__ idx_y, const float* __restrict__ w_y,
                                                              int Ty, const int32_t* __restrict__ idx_x,
                                                              const float* __restrict__ w_x, int Tx,
                                                              const float* __restrict__ fill, float* __restrict__ out, int K, int H,
                                                              int W, int tiles_x, int tiles_y) {
    __shared__ float stage[kRMax * kTW3];
    __shared__ float s_wx[kMaxTaps * kTW];    // [k][col]
    __shared__ int s_ix[kMaxTaps * kTW];
    __shared__ float s_wy[kMaxTaps * kTH];    // [k][row]
    __shared__ int s_iy[kMaxTaps * kTH];
    __shared__ float s_sum[2 * (kTW + kTH)];  // Wsrc_x[kTW], Wall_x[kTW], Wsrc_y[kTH], Wall_y[kTH]
    __shared__ int s_red[2 * kWaves];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, f = b / tiles_y;       // f: frame of the batch, n: its sample
    const int n = f / K;
    const int ox0 = tx * kTW, oy0 = ty * kTH;
    const int ncol_out = min(kTW, W - ox0), nrow_out = min(kTH, H - oy0);
    const int h0 = src_hw[2 * n], w0 = src_hw[2 * n + 1];
    const bool has_src = h0 >= 1 && w0 >= 1;           // a sample without a source is all fill
    const uint8_t* frame = raw + src_off[n] + (int64_t)(f - n * K) * (has_src ? (int64_t)h0 * w0 * 3 : 0);

    // a. the tile's tables; entries of columns / rows past the output's edge are fill taps of weight 0
    const int32_t* gix = idx_x + ((int64_t)n * W + ox0) * Tx;
    const float* gwx = w_x + ((int64_t)n * W + ox0) * Tx;
    for (int e = tid; e < kTW * Tx; e += kThreads) {
        const int col = e / Tx, k = e - col * Tx;
        int i = -1;
        float w = 0.f;
        if (col < ncol_out) {
            i = gix[e];
            w = gwx[e];
            i = (i < 0 || !has_src) ? -1 : min(i, w0 - 1);
        }
        s_ix[k * kTW + col] = i;
        s_wx[k * kTW + col] = w;
    }
    const int32_t* giy = idx_y + ((int64_t)n * H + oy0) * Ty;
    const float* gwy = w_y + ((int64_t)n * H + oy0) * Ty;
    int lo_y = 0x7fffffff, hi_y = -1;
    for (int e = tid; e < kTH * Ty; e += kThreads) {
        const int row = e / Ty, k = e - row * Ty;
        int i = -1;
        float w = 0.f;
        if (row < nrow_out) {
            i = giy[e];
            w = gwy[e];
            i = (i < 0 || !has_src) ? -1 : min(i, h0 - 1);
            if (i >= 0) lo_y = min(lo_y, i), hi_y = max(hi_y, i);
        }
        s_iy[k * kTH + row] = i;
        s_wy[k * kTH + row] = w;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo_y = min(lo_y, __shfl_xor(lo_y, off));
        hi_y = max(hi_y, __shfl_xor(hi_y, off));
    }
    if (lane == 0) s_red[wave] = lo_y, s_red[kWaves + wave] = hi_y;
    __syncthreads();
    int rlo = s_red[0], rhi = s_red[kWaves];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) rlo = min(rlo, s_red[w]), rhi = max(rhi, s_red[kWaves + w]);
    const int nrows = rhi >= rlo ? rhi - rlo + 1 : 0;  // 0: no tap of this tile lies on a source row
    const bool staged = nrows <= kRMax;                // uniform over the workgroup

    // the per-axis weight sums (step 3), one thread per column / row
    if (tid < kTW) {
        float ws = 0.f, wa = 0.f;
        for (int k = 0; k < Tx; ++k) {
            const float w = s_wx[k * kTW + tid];
            wa += w;
            if (s_ix[k * kTW + tid] >= 0) ws += w;
        }
        s_sum[tid] = ws, s_sum[kTW + tid] = wa;
    } else if (tid < kTW + kTH) {
        const int r = tid - kTW;
        float ws = 0.f, wa = 0.f;
        for (int k = 0; k < Ty; ++k) {
            const float w = s_wy[k * kTH + r];
            wa += w;
            if (s_iy[k * kTH + r] >= 0) ws += w;
        }
        s_sum[2 * kTW + r] = ws, s_sum[2 * kTW + kTH + r] = wa;
    }

    // b. horizontal pass of the span's rows into the stage (step 1)
    if (staged) {
        for (int j = tid; j < nrows * kTW3; j += kThreads) {
            const int q = j / kTW3, e = j - q * kTW3;
            const int col = e / 3, ch = e - col * 3;
            const uint8_t* src = frame + (int64_t)(rlo + q) * w0 * 3 + ch;
            float acc = 0.f;
            for (int k = 0; k < Tx; ++k) {
                const int c = s_ix[k * kTW + col];
                if (c >= 0) acc = fmaf(s_wx[k * kTW + col], (float)src[c * 3], acc);
            }
            stage[j] = acc;
        }
    }
    __syncthreads();

    // vertical pass (step 2), colour affine, fill and normalisation (steps 4, 5): one thread per output pixel
    const int ox = tid & (kTW - 1), oyl = tid >> 5;
    if (ox >= ncol_out || oyl >= nrow_out) return;
    float S[3] = {0.f, 0.f, 0.f};
    for (int ky = 0; ky < Ty; ++ky) {
        const int r = s_iy[ky * kTH + oyl];
        if (r < 0) continue;
        const float wy = s_wy[ky * kTH + oyl];
        float h[3];
        if (staged) {
            const float* st = stage + (r - rlo) * kTW3 + ox * 3;
            h[0] = st[0], h[1] = st[1], h[2] = st[2];
        } else {                                       // c. the same sums straight from global memory
            const uint8_t* src = frame + (int64_t)r * w0 * 3;
            h[0] = h[1] = h[2] = 0.f;
            for (int k = 0; k < Tx; ++k) {
                const int c = s_ix[k * kTW + ox];
                if (c < 0) continue;
                const float wx = s_wx[k * kTW + ox];
                h[0] = fmaf(wx, (float)src[c * 3 + 0], h[0]);
                h[1] = fmaf(wx, (float)src[c * 3 + 1], h[1]);
                h[2] = fmaf(wx, (float)src[c * 3 + 2], h[2]);
            }
        }
        S[0] = fmaf(wy, h[0], S[0]), S[1] = fmaf(wy, h[1], S[1]), S[2] = fmaf(wy, h[2], S[2]);
    }
    const float wsrc = s_sum[2 * kTW + oyl] * s_sum[ox];
    const float wall = s_sum[2 * kTW + kTH + oyl] * s_sum[kTW + ox];
    const float wfill = wall - wsrc;
    const float* M = color + 12 * n;
    const int64_t hw = (int64_t)H * W;
    const int64_t pix = (int64_t)(oy0 + oyl) * W + (ox0 + ox);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = S[0] * M[c];
        t = fmaf(S[1], M[3 + c], t);
        t = fmaf(S[2], M[6 + c], t);
        t = fmaf(M[9 + c], wsrc, t);
        t = fmaf(fill[c], wfill, t);
        out[((int64_t)f * 3 + c) * hw + pix] = vd_normalize_level(t, c);
    }
}

}  // namespace

extern "C" {

int vd_augment_u8_nchw(const uint8_t* raw, const int64_t* src_off, const int32_t* src_hw, const float* color, const int32_t* idx_y,
                       const float* w_y, int Ty, const int32_t* idx_x, const float* w_x, int Tx, const float* fill, float* out, int N,
                       int K, int H, int W, void* stream) {
    VD_REQUIRE(raw && src_off && src_hw && color && idx_y && w_y && idx_x && w_x && fill && out,
               "vd_augment_u8_nchw: raw, src_off, src_hw, color, the four tap tables (idx_y, w_y, idx_x, w_x), fill and out must "
               "not be NULL");
    VD_REQUIRE(N >= 1 && K >= 1 && H >= 1 && W >= 1, "vd_augment_u8_nchw: all sizes must be >= 1, got N=%d K=%d H=%d W=%d", N, K, H, W);
    VD_REQUIRE(Ty >= 1 && Ty <= kMaxTaps && Tx >= 1 && Tx <= kMaxTaps,
               "vd_augment_u8_nchw: 1 <= Ty, Tx <= %d needed, got Ty=%d Tx=%d", kMaxTaps, Ty, Tx);
    VD_REQUIRE(((uintptr_t)src_off % 8) == 0, "vd_augment_u8_nchw: src_off (int64) must be 8-byte aligned");
    VD_REQUIRE((((uintptr_t)src_hw | (uintptr_t)color | (uintptr_t)idx_y | (uintptr_t)w_y | (uintptr_t)idx_x | (uintptr_t)w_x |
                 (uintptr_t)fill | (uintptr_t)out) % 4) == 0,
               "vd_augment_u8_nchw: src_hw, color, the tap tables, fill and out must be 4-byte aligned");
    const int64_t tiles_x = vd_cdiv(W, kTW), tiles_y = vd_cdiv(H, kTH), blocks = tiles_x * tiles_y * N * K;
    VD_REQUIRE(blocks < ((int64_t)1 << 31), "vd_augment_u8_nchw: %lld tiles are more than one launch takes", (long long)blocks);
    hipLaunchKernelGGL(k_augment_u8_nchw, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, raw, src_off, src_hw, color,
                       idx_y, w_y, Ty, idx_x, w_x, Tx, fill, out, K, H, W, (int)tiles_x, (int)tiles_y);
    VD_CHECK_LAUNCH("vd_augment_u8_nchw");
    return VD_OK;
}

}  // extern "C"
