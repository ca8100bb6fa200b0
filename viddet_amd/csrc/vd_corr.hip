// vd_corr.hip — the correlation join of a temporal window (Corr(d, k, kernal_size=1, stride=1, keep='all')):
// the K frames' channels stacked ('cat' part) followed by one FlowNet-style cost volume per frame t != K/2 against the
// window's centre frame (mx.sym.Correlation, kernel_size 1, max_displacement = pad_size = d, stride1 = stride2 = 1).
//
// Reference call sites (under /root/reference):
//   Corr                           models/definitions/layers.py:93-132
//   early / late positions         models/definitions/yolo/yolo3.py:1105-1124, 1139-1140
//
// Layouts: x [B*K, H, W, C] NHWC (frame b*K + k), y [B, H, W, ldy]:
//   y[.., k*C + c]                                    = x[b*K + k, .., c]
//   y[.., K*C + tt*D2 + (dy+d)*D + (dx+d)]            = (1/C) sum_c x[b*K+t, y, x, c] * x[b*K+mid, y+dy, x+dx, c]
//   y[.., Cc .. ldy)                                  = 0
// with D = 2d+1, D2 = D*D, mid = K/2, tt = t - (t > mid), Cc = K*C + (K-1)*D2; zero where (y+dy, x+dx) leaves the map.
//
// Shape of the work: a workgroup owns an 8x8 pixel tile of one frame of one window.  Channels are staged 32 at a time in
// LDS (the tile of frame t, the (8+2d)^2 halo of the centre frame), and every (pixel, displacement) pair is summed in fp32
// on the vector ALU in increasing channel order, so results are reproducible bit for bit.  The operator is < 1 % of a
// step's FLOPs; nothing here uses MFMA.  The backward is two gathers (no atomics), in a fixed summation order.
// Every store is a plain vector store.
//
// bf16-storage training has its own backward (k_corr_bwd_bf16): same grid, same thread layout and the same summation order
// as k_corr_bwd, but the (pixel, displacement) slice of `dy` a workgroup needs for the side frame at hand is gathered into
// LDS once (64 x D^2 bf16 values, 15.5 KB at d = 5) instead of being loaded per displacement by every channel-quad lane.
#include "vd_common.h"

namespace {

constexpr int TS = 8;             // pixel tile side
constexpr int TP = TS * TS;       // pixels of a tile
constexpr int CC = 32;            // channels per LDS chunk
constexpr int LP = CC + 4;        // LDS row pitch in floats (16-B aligned rows, staggered banks)
constexpr int MAXD = 5;           // largest displacement built (D2 = 121)

template <typename T>
__device__ __forceinline__ void store1(T* p, float v) { *p = (T)v; }

// load CC channels [c0, c0 + CC) of `src` pixel (gy, gx) into an LDS row; zeros outside the map
template <typename T>
__device__ __forceinline__ void stage_row(float* row, const T* __restrict__ src, int gy, int gx, int H, int W, int C, int c0,
                                          int q) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = vd_ld4(src + ((int64_t)gy * W + gx) * C + c0, q);
    *reinterpret_cast<f32x4*>(row + 4 * q) = v;
}

// grid (tiles, K, B); 256 threads.  Frame t != mid: its correlation map and its 'cat' channels over the tile.  Frame mid:
// its 'cat' channels and the zero tail [Cc, ldy).
template <typename T, int DD>
__global__ __launch_bounds__(256) void k_corr_fwd(const T* __restrict__ x, T* __restrict__ y, int K, int H, int W, int C,
                                                  int ldy, int tiles_x) {
    constexpr int D = 2 * DD + 1, D2 = D * D, NACC = (D2 + 3) / 4, HT = TS + 2 * DD;
    __shared__ __attribute__((aligned(16))) float s_t[TP * LP];
    __shared__ __attribute__((aligned(16))) float s_m[HT * HT * LP];
    const int tid = threadIdx.x;
    const int t = blockIdx.y, b = blockIdx.z, mid = K / 2;
    const int ty0 = (blockIdx.x / tiles_x) * TS, tx0 = (blockIdx.x % tiles_x) * TS;
    const int64_t HW = (int64_t)H * W;
    const T* xt = x + ((int64_t)b * K + t) * HW * C;
    const T* xm = x + ((int64_t)b * K + mid) * HW * C;
    T* yb = y + (int64_t)b * HW * ldy;

    // 'cat' part: y[.., t*C + c] = x_t (a copy)
    const int C4 = C / 4;
    for (int i = tid; i < TP * C4; i += 256) {
        const int p = i / C4, q = i % C4;
        const int gy = ty0 + p / TS, gx = tx0 + p % TS;
        if (gy < H && gx < W) {
            const int64_t pix = (int64_t)gy * W + gx;
            vd_st4(yb + pix * ldy + t * C, q, vd_ld4(xt + pix * C, q));
        }
    }
    const int Cc = K * C + (K - 1) * D2;
    if (t == mid) {
        const int npad = ldy - Cc;
        for (int i = tid; i < TP * npad; i += 256) {
            const int p = i / npad, c = Cc + i % npad;
            const int gy = ty0 + p / TS, gx = tx0 + p % TS;
            if (gy < H && gx < W) store1(yb + ((int64_t)gy * W + gx) * ldy + c, 0.f);
        }
        return;                                      // uniform over the workgroup: no barrier follows for it
    }

    // correlation map: thread = (pixel p, displacement group g); displacements j = g + 4 i
    const int p = tid & (TP - 1), g = tid >> 6;      // g is uniform over a wavefront
    const int py = p / TS, px = p % TS;
    int off[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        const int j = g + 4 * i < D2 ? g + 4 * i : 0;
        off[i] = ((py + j / D) * HT + px + j % D) * LP;  // halo pixel (y + dy, x + dx), halo origin (ty0 - d, tx0 - d)
    }
    float acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.f;

    for (int c0 = 0; c0 < C; c0 += CC) {
        __syncthreads();                             // the previous chunk's reads are done
        for (int i = tid; i < TP * (CC / 4); i += 256) {
            const int pp = i / (CC / 4), q = i % (CC / 4);
            stage_row(s_t + pp * LP, xt, ty0 + pp / TS, tx0 + pp % TS, H, W, C, c0, q);
        }
        for (int i = tid; i < HT * HT * (CC / 4); i += 256) {
            const int h = i / (CC / 4), q = i % (CC / 4);
            stage_row(s_m + h * LP, xm, ty0 - DD + h / HT, tx0 - DD + h % HT, H, W, C, c0, q);
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < CC / 4; ++q) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(s_t + p * LP + 4 * q);
#pragma unroll
            for (int i = 0; i < NACC; ++i) {
                if (g + 4 * i < D2) {
                    const f32x4 m = *reinterpret_cast<const f32x4*>(s_m + off[i] + 4 * q);
                    float s = acc[i];
                    s = fmaf(a[0], m[0], s);
                    s = fmaf(a[1], m[1], s);
                    s = fmaf(a[2], m[2], s);
                    s = fmaf(a[3], m[3], s);
                    acc[i] = s;
                }
            }
        }
    }
    const int gy = ty0 + py, gx = tx0 + px;
    if (gy >= H || gx >= W) return;
    const float inv = 1.0f / (float)C;
    T* yo = yb + ((int64_t)gy * W + gx) * ldy + K * C + (t - (t > mid)) * D2;
#pragma unroll
    for (int i = 0; i < NACC; ++i)
        if (g + 4 * i < D2) store1(yo + g + 4 * i, acc[i] * inv);
}

// grid (tiles, K, B * C/CC); 256 threads = 8 channel quads x 32 pixel slots (pixels s and s + 32 of the tile).
//   t != mid: dx_t[p] = dy_cat_t[p] + (1/C) sum_j dy_t[p, j] * x_mid[p + disp_j]
//   t == mid: dx_mid[q] = dy_cat_mid[q] + (1/C) sum_{s != mid, increasing} sum_j dy_s[q - disp_j, j] * x_s[q - disp_j]
template <int DD>
__global__ __launch_bounds__(256) void k_corr_bwd(const float* __restrict__ dy, const float* __restrict__ x,
                                                  float* __restrict__ dx, int K, int H, int W, int C, int ldy, int tiles_x) {
    constexpr int D = 2 * DD + 1, D2 = D * D, HT = TS + 2 * DD;
    __shared__ __attribute__((aligned(16))) float s_h[HT * HT * LP];
    const int tid = threadIdx.x;
    const int nchunk = C / CC;
    const int t = blockIdx.y, b = blockIdx.z / nchunk, c0 = (blockIdx.z % nchunk) * CC, mid = K / 2;
    const int ty0 = (blockIdx.x / tiles_x) * TS, tx0 = (blockIdx.x % tiles_x) * TS;
    const int64_t HW = (int64_t)H * W;
    const float* dyb = dy + (int64_t)b * HW * ldy;
    const int q = tid & 7, slot = tid >> 3;
    const float inv = 1.0f / (float)C;
    const int base0 = K * C;                          // first correlation channel

    f32x4 acc[2];
    acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < K; ++s) {
        // the halo operand: x_mid for a side frame, x_s (every s != mid) for the centre frame
        if (t != mid ? s != mid : s == mid) continue;
        const float* src = x + ((int64_t)b * K + s) * HW * C;
        __syncthreads();
        for (int i = tid; i < HT * HT * (CC / 4); i += 256) {
            const int h = i / (CC / 4), qq = i % (CC / 4);
            stage_row(s_h + h * LP, src, ty0 - DD + h / HT, tx0 - DD + h % HT, H, W, C, c0, qq);
        }
        __syncthreads();
        const int map = t != mid ? t : s;             // whose correlation map's gradient is read
        const int base = base0 + (map - (map > mid)) * D2;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int p = slot + 32 * r, py = p / TS, px = p % TS;
            const int gy = ty0 + py, gx = tx0 + px;
            if (gy >= H || gx >= W) continue;
            f32x4 a = acc[r];
            if (t != mid) {
                const float* dyp = dyb + ((int64_t)gy * W + gx) * ldy + base;
                for (int j = 0; j < D2; ++j) {
                    const float gv = dyp[j];
                    const f32x4 m = *reinterpret_cast<const f32x4*>(s_h + ((py + j / D) * HT + px + j % D) * LP + 4 * q);
                    a[0] = fmaf(gv, m[0], a[0]);
                    a[1] = fmaf(gv, m[1], a[1]);
                    a[2] = fmaf(gv, m[2], a[2]);
                    a[3] = fmaf(gv, m[3], a[3]);
                }
            } else {
                for (int j = 0; j < D2; ++j) {
                    const int oy = j / D - DD, ox = j % D - DD;
                    const int sy = gy - oy, sx = gx - ox;      // the side-frame pixel whose displacement j lands on (gy, gx)
                    if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
                    const float gv = dyb[((int64_t)sy * W + sx) * ldy + base + j];
                    const f32x4 m = *reinterpret_cast<const f32x4*>(s_h + ((py - oy + DD) * HT + px - ox + DD) * LP + 4 * q);
                    a[0] = fmaf(gv, m[0], a[0]);
                    a[1] = fmaf(gv, m[1], a[1]);
                    a[2] = fmaf(gv, m[2], a[2]);
                    a[3] = fmaf(gv, m[3], a[3]);
                }
            }
            acc[r] = a;
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int p = slot + 32 * r;
        const int gy = ty0 + p / TS, gx = tx0 + p % TS;
        if (gy >= H || gx >= W) continue;
        const int64_t pix = (int64_t)gy * W + gx;
        const f32x4 dc = vd_ld4(dyb + pix * ldy + t * C + c0, q);
        vd_st4(dx + ((int64_t)b * K + t) * HW * C + pix * C + c0, q, dc + acc[r] * inv);
    }
}

// bf16 tensors, fp32 accumulation, one rounding at the store.  Grid, thread layout and summation order of k_corr_bwd.
// Per side frame s (one for t != mid, the K - 1 side frames in increasing order for t == mid) the workgroup stages
//   s_h : the 32-channel halo of the x operand, fp32                      (HT^2 x 36 floats: 46.6 KB at d = 5)
//   s_g : dy of that frame's correlation map, bf16 bit patterns, [pixel of the tile][displacement j]
//         t != mid: dy_t[p, j]            t == mid: dy_s[p - disp_j, j]   (64 x D^2 x 2 bytes: 15.5 KB at d = 5)
// so the centre-frame pass never holds more than one side frame's gathered slice (62 KB in all at d = 5: two workgroups per
// CU; 47 KB at d = 4: three).  Out-of-map sources are staged as zeros: their products add an exact zero.
template <int DD>
__global__ __launch_bounds__(256) void k_corr_bwd_bf16(const __bf16* __restrict__ dy, const __bf16* __restrict__ x,
                                                       __bf16* __restrict__ dx, int K, int H, int W, int C, int ldy,
                                                       int tiles_x) {
    constexpr int D = 2 * DD + 1, D2 = D * D, HT = TS + 2 * DD;
    __shared__ __attribute__((aligned(16))) float s_h[HT * HT * LP];
    __shared__ __attribute__((aligned(16))) unsigned short s_g[(TP * D2 + 7) & ~7];
    const int tid = threadIdx.x;
    const int nchunk = C / CC;
    const int t = blockIdx.y, b = blockIdx.z / nchunk, c0 = (blockIdx.z % nchunk) * CC, mid = K / 2;
    const int ty0 = (blockIdx.x / tiles_x) * TS, tx0 = (blockIdx.x % tiles_x) * TS;
    const int64_t HW = (int64_t)H * W;
    const unsigned short* dyb = reinterpret_cast<const unsigned short*>(dy) + (int64_t)b * HW * ldy;
    const int q = tid & 7, slot = tid >> 3;
    const float inv = 1.0f / (float)C;
    const int base0 = K * C;                          // first correlation channel
    const bool centre = t == mid;                     // uniform over the workgroup

    f32x4 acc[2];
    acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < K; ++s) {
        if (centre ? s == mid : s != mid) continue;   // the halo operand: x_mid for a side frame, x_s for the centre frame
        const __bf16* src = x + ((int64_t)b * K + s) * HW * C;
        const int map = centre ? s : t;               // whose correlation map's gradient is read
        const int base = base0 + (map - (map > mid)) * D2;
        __syncthreads();                              // the previous frame's reads are done
        for (int i = tid; i < HT * HT * (CC / 4); i += 256) {
            const int h = i / (CC / 4), qq = i % (CC / 4);
            stage_row(s_h + h * LP, src, ty0 - DD + h / HT, tx0 - DD + h % HT, H, W, C, c0, qq);
        }
        for (int i = tid; i < TP * D2; i += 256) {
            const int p = i / D2, j = i % D2;
            int sy = ty0 + p / TS, sx = tx0 + p % TS;
            if (centre) {                             // the side-frame pixel whose displacement j lands on pixel p
                sy -= j / D - DD;
                sx -= j % D - DD;
            }
            unsigned short v = 0;
            if (sy >= 0 && sy < H && sx >= 0 && sx < W) v = dyb[((int64_t)sy * W + sx) * ldy + base + j];
            s_g[i] = v;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int p = slot + 32 * r, py = p / TS, px = p % TS;
            if (ty0 + py >= H || tx0 + px >= W) continue;
            f32x4 a = acc[r];
            const unsigned short* gp = s_g + p * D2;
            // halo pixel of displacement (jy, jx): (py + jy, px + jx) for a side frame, (py + 2d - jy, px + 2d - jx) for the centre
            const float* hp = s_h + ((centre ? py + 2 * DD : py) * HT + (centre ? px + 2 * DD : px)) * LP + 4 * q;
            const int step = centre ? -LP : LP;
            for (int jy = 0; jy < D; ++jy) {
#pragma unroll
                for (int jx = 0; jx < D; ++jx) {
                    const float gv = __uint_as_float((unsigned)gp[jy * D + jx] << 16);
                    const f32x4 m = *reinterpret_cast<const f32x4*>(hp + (jy * HT + jx) * step);
                    a[0] = fmaf(gv, m[0], a[0]);
                    a[1] = fmaf(gv, m[1], a[1]);
                    a[2] = fmaf(gv, m[2], a[2]);
                    a[3] = fmaf(gv, m[3], a[3]);
                }
            }
            acc[r] = a;
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int p = slot + 32 * r;
        const int gy = ty0 + p / TS, gx = tx0 + p % TS;
        if (gy >= H || gx >= W) continue;
        const int64_t pix = (int64_t)gy * W + gx;
        const f32x4 dc = vd_ld4(dy + (int64_t)b * HW * ldy + pix * ldy + t * C + c0, q);
        vd_st4(dx + ((int64_t)b * K + t) * HW * C + pix * C + c0, q, dc + acc[r] * inv);
    }
}

template <typename T>
int corr_fwd(const T* x, T* y, int B, int K, int H, int W, int C, int d, int ldy, void* stream, const char* name) {
    VD_REQUIRE(x && y && B > 0 && K > 1 && H > 0 && W > 0, "%s: bad args", name);
    VD_REQUIRE(C > 0 && C % 32 == 0, "%s: C = %d must be a multiple of 32", name, C);
    VD_REQUIRE(d >= 0 && d <= MAXD, "%s: max displacement %d outside [0, %d]", name, d, MAXD);
    const int Cc = K * C + (K - 1) * (2 * d + 1) * (2 * d + 1);
    VD_REQUIRE(ldy >= Cc && ldy % 8 == 0, "%s: ldy = %d (needs >= %d, a multiple of 8)", name, ldy, Cc);
    const int tx = (int)vd_cdiv(W, TS), ty = (int)vd_cdiv(H, TS);
    const dim3 grid(tx * ty, K, B);
    hipStream_t s = (hipStream_t)stream;
    switch (d) {
        case 0: hipLaunchKernelGGL((k_corr_fwd<T, 0>), grid, dim3(256), 0, s, x, y, K, H, W, C, ldy, tx); break;
        case 1: hipLaunchKernelGGL((k_corr_fwd<T, 1>), grid, dim3(256), 0, s, x, y, K, H, W, C, ldy, tx); break;
        case 2: hipLaunchKernelGGL((k_corr_fwd<T, 2>), grid, dim3(256), 0, s, x, y, K, H, W, C, ldy, tx); break;
        case 3: hipLaunchKernelGGL((k_corr_fwd<T, 3>), grid, dim3(256), 0, s, x, y, K, H, W, C, ldy, tx); break;
        case 4: hipLaunchKernelGGL((k_corr_fwd<T, 4>), grid, dim3(256), 0, s, x, y, K, H, W, C, ldy, tx); break;
        default: hipLaunchKernelGGL((k_corr_fwd<T, 5>), grid, dim3(256), 0, s, x, y, K, H, W, C, ldy, tx); break;
    }
    VD_CHECK_LAUNCH(name);
    return VD_OK;
}

}  // namespace

extern "C" {

int vd_corr_fwd(const float* x, float* y, int B, int K, int H, int W, int C, int d, int ldy, void* stream) {
    return corr_fwd<float>(x, y, B, K, H, W, C, d, ldy, stream, "vd_corr_fwd");
}

int vd_corr_fwd_bf16(const void* x, void* y, int B, int K, int H, int W, int C, int d, int ldy, void* stream) {
    return corr_fwd<__bf16>((const __bf16*)x, (__bf16*)y, B, K, H, W, C, d, ldy, stream, "vd_corr_fwd_bf16");
}

int vd_corr_bwd(const float* dy, const float* x, float* dx, int B, int K, int H, int W, int C, int d, int ldy, void* stream) {
    VD_REQUIRE(dy && x && dx && B > 0 && K > 1 && H > 0 && W > 0, "vd_corr_bwd: bad args");
    VD_REQUIRE(C > 0 && C % 32 == 0, "vd_corr_bwd: C = %d must be a multiple of 32", C);
    VD_REQUIRE(d >= 0 && d <= MAXD, "vd_corr_bwd: max displacement %d outside [0, %d]", d, MAXD);
    const int Cc = K * C + (K - 1) * (2 * d + 1) * (2 * d + 1);
    VD_REQUIRE(ldy >= Cc && ldy % 8 == 0, "vd_corr_bwd: ldy = %d (needs >= %d, a multiple of 8)", ldy, Cc);
    const int tx = (int)vd_cdiv(W, TS), ty = (int)vd_cdiv(H, TS);
    const dim3 grid(tx * ty, K, B * (C / CC));
    hipStream_t s = (hipStream_t)stream;
    switch (d) {
        case 0: hipLaunchKernelGGL(k_corr_bwd<0>, grid, dim3(256), 0, s, dy, x, dx, K, H, W, C, ldy, tx); break;
        case 1: hipLaunchKernelGGL(k_corr_bwd<1>, grid, dim3(256), 0, s, dy, x, dx, K, H, W, C, ldy, tx); break;
        case 2: hipLaunchKernelGGL(k_corr_bwd<2>, grid, dim3(256), 0, s, dy, x, dx, K, H, W, C, ldy, tx); break;
        case 3: hipLaunchKernelGGL(k_corr_bwd<3>, grid, dim3(256), 0, s, dy, x, dx, K, H, W, C, ldy, tx); break;
        case 4: hipLaunchKernelGGL(k_corr_bwd<4>, grid, dim3(256), 0, s, dy, x, dx, K, H, W, C, ldy, tx); break;
        default: hipLaunchKernelGGL(k_corr_bwd<5>, grid, dim3(256), 0, s, dy, x, dx, K, H, W, C, ldy, tx); break;
    }
    VD_CHECK_LAUNCH("vd_corr_bwd");
    return VD_OK;
}

int vd_corr_bwd_bf16(const void* dy, const void* x, void* dx, int B, int K, int H, int W, int C, int d, int ldy, void* stream) {
    VD_REQUIRE(dy && x && dx && B > 0 && K > 1 && H > 0 && W > 0, "vd_corr_bwd_bf16: bad args");
    VD_REQUIRE(C > 0 && C % 32 == 0, "vd_corr_bwd_bf16: C = %d must be a multiple of 32", C);
    VD_REQUIRE(d >= 0 && d <= MAXD, "vd_corr_bwd_bf16: max displacement %d outside [0, %d]", d, MAXD);
    const int Cc = K * C + (K - 1) * (2 * d + 1) * (2 * d + 1);
    VD_REQUIRE(ldy >= Cc && ldy % 8 == 0, "vd_corr_bwd_bf16: ldy = %d (needs >= %d, a multiple of 8)", ldy, Cc);
    VD_REQUIRE((int64_t)B * (C / CC) <= 65535, "vd_corr_bwd_bf16: B * C / 32 = %lld exceeds the grid's z extent",
               (long long)B * (C / CC));
    const int tx = (int)vd_cdiv(W, TS), ty = (int)vd_cdiv(H, TS);
    const dim3 grid(tx * ty, K, B * (C / CC));
    hipStream_t s = (hipStream_t)stream;
    const __bf16 *g = (const __bf16*)dy, *xs = (const __bf16*)x;
    __bf16* o = (__bf16*)dx;
    switch (d) {
        case 0: hipLaunchKernelGGL(k_corr_bwd_bf16<0>, grid, dim3(256), 0, s, g, xs, o, K, H, W, C, ldy, tx); break;
        case 1: hipLaunchKernelGGL(k_corr_bwd_bf16<1>, grid, dim3(256), 0, s, g, xs, o, K, H, W, C, ldy, tx); break;
        case 2: hipLaunchKernelGGL(k_corr_bwd_bf16<2>, grid, dim3(256), 0, s, g, xs, o, K, H, W, C, ldy, tx); break;
        case 3: hipLaunchKernelGGL(k_corr_bwd_bf16<3>, grid, dim3(256), 0, s, g, xs, o, K, H, W, C, ldy, tx); break;
        case 4: hipLaunchKernelGGL(k_corr_bwd_bf16<4>, grid, dim3(256), 0, s, g, xs, o, K, H, W, C, ldy, tx); break;
        default: hipLaunchKernelGGL(k_corr_bwd_bf16<5>, grid, dim3(256), 0, s, g, xs, o, K, H, W, C, ldy, tx); break;
    }
    VD_CHECK_LAUNCH("vd_corr_bwd_bf16");
    return VD_OK;
}

}  // extern "C"
