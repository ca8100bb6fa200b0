// vd_tdw.hip — the temporal half of the backbone's R(2+1)D cell over the K frames of a window: a depthwise (3,1,1)
// convolution with REPEAT padding (Conv3DRepPad, /root/reference models/definitions/darknet/three_darknet.py:19-70;
// DESIGN.md 17).  No BatchNorm and no activation follow it (:36), so it is not a GEMM and not a cell: one streaming pass.
//
//   xp = [x_0, x_0, x_1, ..., x_{K-1}, x_{K-2}]          (:61-68; the tail copy is slice_axis(begin=-2, end=-1) = frame K-2,
//   y_t = w0 * xp_t + w1 * xp_{t+1} + w2 * xp_{t+2}        NOT the last frame - restated as written)
//       = w0 * x_{max(t-1,0)} + w1 * x_t + w2 * x_{t+1 < K ? t+1 : K-2}        [+ res_t: the block's `x + residual`, :120-123]
//
// Tensors are fp32 NHWC rows with the frames folded into the batch (frame n = b*K + t): [B*K][HW][C].  The weight keeps the
// reference's layout (C,1,3,1,1) = [C][3].  A lane owns four channels of one pixel and walks the K frames of its column with
// a three-frame register window: every x (and dy) element is read from memory once, every y / dx element written once, all
// as 16-byte accesses.  Backward is ONE launch for dx and the weight gradient: the lane keeps its 4 x 3 products dy_t * xp_{t+j}
// in registers, a workgroup folds them through LDS in a fixed order into one row of a partial table, and a second launch
// sums the rows in a fixed order in fp64.  No floating-point atomics: two runs give the same bits.
#include "vd_common.h"

namespace {

inline bool fits32(int64_t items) { return items + (int64_t)4096 * 256 < ((int64_t)1 << 31); }

inline int gblocks(int64_t n) {
    int64_t nb = vd_cdiv(n, 256);
    if (nb > 4096) nb = 4096;
    if (nb < 1) nb = 1;
    return (int)nb;
}

constexpr int TDW_MAX_ROWS = 2048;      // rows of the partial table (= workgroups of the backward launch) at the most

__device__ __forceinline__ float amax4(float mx, const f32x4 v) {
    return fmaxf(mx, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
}

// the three taps of four channels: w[c][j] at 12 consecutive floats
struct Taps {
    f32x4 w0, w1, w2;
};
__device__ __forceinline__ Taps load_taps(const float* __restrict__ w, int c4) {
    const f32x4 a = vd_ld4(w, 3 * c4), b = vd_ld4(w, 3 * c4 + 1), c = vd_ld4(w, 3 * c4 + 2);
    return Taps{f32x4{a[0], a[3], b[2], c[1]}, f32x4{a[1], b[0], b[3], c[2]}, f32x4{a[2], b[1], c[0], c[3]}};
}

// The index type IT is int32_t where every element index of the launch fits it (the host checks), else int64_t.
template <typename IT>
__global__ void k_tdw_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ res,
                          float* __restrict__ y, IT M, IT HW, int K, int C4, float* __restrict__ amax) {
    const IT total = M * C4, FS = HW * C4;
    float mx = 0.f;
    for (IT i = (IT)blockIdx.x * (IT)blockDim.x + (IT)threadIdx.x; i < total; i += (IT)gridDim.x * (IT)blockDim.x) {
        const IT m = i / C4;
        const int c = (int)(i - m * C4);
        const IT b = m / HW;
        IT at = (b * K * HW + (m - b * HW)) * C4 + c;          // frame 0 of the column
        const Taps tp = load_taps(w, c);
        f32x4 prev = vd_ld4(x, at), cur = prev;
        for (int t = 0; t < K; ++t, at += FS) {
            const f32x4 next = t + 1 < K ? vd_ld4(x, at + FS) : prev;        // the tail pad is frame K-2 = `prev` at t = K-1
            f32x4 o = tp.w0 * prev + tp.w1 * cur + tp.w2 * next;
            if (res) o += vd_ld4(res, at);
            vd_st4(y, at, o);
            mx = amax4(mx, o);
            prev = cur, cur = next;
        }
    }
    if (amax) vd_amax_publish(amax, mx);
}

// blockDim = (TX channel lanes, TY rows), TX * TY = 256.  dx == NULL: no data gradient; part == NULL: no weight gradient.
// part[blockIdx.x][C][3]: every workgroup writes its whole row (zeros where it had no pixel).
template <typename IT>
__global__ void k_tdw_bwd(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                          float* __restrict__ dx, float* __restrict__ part, IT M, IT HW, int K, int C4) {
    __shared__ float red[256 * 12];
    const IT FS = HW * C4;
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    for (int c0 = 0; c0 < C4; c0 += blockDim.x) {
        const int c = c0 + threadIdx.x;
        f32x4 g0 = f32x4{0.f, 0.f, 0.f, 0.f}, g1 = g0, g2 = g0;
        if (c < C4) {
            const Taps tp = load_taps(w, c);
            for (IT m = (IT)blockIdx.x * (IT)blockDim.y + (IT)threadIdx.y; m < M; m += (IT)gridDim.x * (IT)blockDim.y) {
                const IT b = m / HW;
                IT at = (b * K * HW + (m - b * HW)) * C4 + c;
                f32x4 dprev = f32x4{0.f, 0.f, 0.f, 0.f}, dcur = vd_ld4(dy, at), xprev = dprev, xcur = dprev;
                if (part) xprev = xcur = vd_ld4(x, at);
                for (int t = 0; t < K; ++t, at += FS) {
                    const bool last = t + 1 == K;
                    const f32x4 dnext = last ? f32x4{0.f, 0.f, 0.f, 0.f} : vd_ld4(dy, at + FS);
                    if (dx) {
                        // transposed edge map: frame 0 also feeds y_0 through the front pad, frame K-2 feeds y_{K-1} through the
                        // tail pad (at K = 2 both are frame 0)
                        f32x4 o = tp.w0 * dnext + tp.w1 * dcur + tp.w2 * dprev;
                        if (t == 0) o += tp.w0 * dcur;
                        if (t == K - 2) o += tp.w2 * dnext;
                        vd_st4(dx, at, o);
                    }
                    if (part) {
                        const f32x4 xnext = last ? xprev : vd_ld4(x, at + FS);
                        g0 += dcur * xprev, g1 += dcur * xcur, g2 += dcur * xnext;
                        xprev = xcur, xcur = xnext;
                    }
                    dprev = dcur, dcur = dnext;
                }
            }
        }
        if (!part) continue;                                     // (uniform: no barrier is skipped by part of a workgroup)
        // fold the TY rows of the workgroup in a fixed order: lane (x, y) -> red[y][x][channel e][tap j]
        float* r = red + tid * 12;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[3 * e] = g0[e], r[3 * e + 1] = g1[e], r[3 * e + 2] = g2[e];
        __syncthreads();
        for (int q = tid; q < (int)blockDim.x * 12; q += 256) {
            const int lx = q / 12;
            if (c0 + lx < C4) {
                float s = 0.f;
                for (int yy = 0; yy < (int)blockDim.y; ++yy) s += red[(yy * blockDim.x + lx) * 12 + (q - lx * 12)];
                part[(size_t)blockIdx.x * (size_t)(12 * C4) + (size_t)(c0 + lx) * 12 + (q - lx * 12)] = s;
            }
        }
        __syncthreads();
    }
}

// dw[col] = sum over the rows of part, row 0 first, in fp64
__global__ void k_tdw_fold(const float* __restrict__ part, int rows, int cols, float* __restrict__ dw) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= cols) return;
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += (double)part[(size_t)r * cols + col];
    dw[col] = (float)s;
}

inline int tdw_tx(int C4) {
    int tx = 1;
    while (tx < C4 && tx < 64) tx *= 2;
    return tx;
}

inline int tdw_rows(int64_t M, int C4) {
    const int ty = 256 / tdw_tx(C4);
    int64_t nb = vd_cdiv(M, ty);
    if (nb > TDW_MAX_ROWS) nb = TDW_MAX_ROWS;
    return (int)nb;
}

}  // namespace

extern "C" {

int vd_tdw_fwd(const float* x, const float* w, const float* res, float* y, int B, int K, int64_t HW, int C, float* amax_out,
               void* stream) {
    VD_REQUIRE(x && w && y, "vd_tdw_fwd: x, w and y must not be NULL");
    VD_REQUIRE(K >= 2, "vd_tdw_fwd: a window of K >= 2 frames is needed (the tail pad is frame K-2), got K=%d", K);
    VD_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 4 == 0, "vd_tdw_fwd: bad sizes (B=%d HW=%lld, C=%d must be a positive multiple of 4)", B,
               (long long)HW, C);
    VD_REQUIRE(((uintptr_t)x | (uintptr_t)w | (uintptr_t)res | (uintptr_t)y) % 16 == 0, "vd_tdw_fwd: pointers must be 16-byte aligned");
    const int64_t M = (int64_t)B * HW;
    const int C4 = C / 4;
    if (fits32(M * K * C4))
        hipLaunchKernelGGL(k_tdw_fwd<int32_t>, dim3(gblocks(M * C4)), dim3(256), 0, (hipStream_t)stream, x, w, res, y, (int32_t)M,
                           (int32_t)HW, K, C4, amax_out);
    else
        hipLaunchKernelGGL(k_tdw_fwd<int64_t>, dim3(gblocks(M * C4)), dim3(256), 0, (hipStream_t)stream, x, w, res, y, M, HW, K, C4,
                           amax_out);
    VD_CHECK_LAUNCH("vd_tdw_fwd");
    return VD_OK;
}

int64_t vd_tdw_bwd_ws_bytes(int B, int K, int64_t HW, int C) {
    if (B <= 0 || K < 2 || HW <= 0 || C <= 0 || C % 4) return 0;
    return (int64_t)tdw_rows((int64_t)B * HW, C / 4) * 3 * C * (int64_t)sizeof(float);
}

int vd_tdw_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, int B, int K, int64_t HW, int C, void* ws,
               int64_t ws_bytes, void* stream) {
    VD_REQUIRE(dy && w && (dx || dw), "vd_tdw_bwd: dy, w and at least one of dx, dw must not be NULL");
    VD_REQUIRE(!dw || x, "vd_tdw_bwd: dw needs x");
    VD_REQUIRE(K >= 2, "vd_tdw_bwd: a window of K >= 2 frames is needed (the tail pad is frame K-2), got K=%d", K);
    VD_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 4 == 0, "vd_tdw_bwd: bad sizes (B=%d HW=%lld, C=%d must be a positive multiple of 4)", B,
               (long long)HW, C);
    VD_REQUIRE(((uintptr_t)dy | (uintptr_t)x | (uintptr_t)w | (uintptr_t)dx | (uintptr_t)dw | (uintptr_t)ws) % 16 == 0,
               "vd_tdw_bwd: pointers must be 16-byte aligned");
    VD_REQUIRE(!dw || (ws && ws_bytes >= vd_tdw_bwd_ws_bytes(B, K, HW, C)), "vd_tdw_bwd: workspace too small (%lld < %lld bytes)",
               (long long)ws_bytes, (long long)vd_tdw_bwd_ws_bytes(B, K, HW, C));
    const int64_t M = (int64_t)B * HW;
    const int C4 = C / 4, tx = tdw_tx(C4), rows = tdw_rows(M, C4);
    float* part = dw ? (float*)ws : nullptr;
    if (fits32(M * K * C4))
        hipLaunchKernelGGL(k_tdw_bwd<int32_t>, dim3(rows), dim3(tx, 256 / tx), 0, (hipStream_t)stream, dy, x, w, dx, part, (int32_t)M,
                           (int32_t)HW, K, C4);
    else
        hipLaunchKernelGGL(k_tdw_bwd<int64_t>, dim3(rows), dim3(tx, 256 / tx), 0, (hipStream_t)stream, dy, x, w, dx, part, M, HW, K, C4);
    VD_CHECK_LAUNCH("vd_tdw_bwd");
    if (dw) {
        hipLaunchKernelGGL(k_tdw_fold, dim3((int)vd_cdiv(3 * C, 256)), dim3(256), 0, (hipStream_t)stream, part, rows, 3 * C, dw);
        VD_CHECK_LAUNCH("vd_tdw_bwd/fold");
    }
    return VD_OK;
}

}  // extern "C"
