// vd_stream.hip — the temporal joins of streaming video detection (YOLOV3.detect_video): max / mean pooling
// and channel stacking over the K frames of a window, read IN PLACE from a ring of cached per-frame features.
//
// On a clip, frame t sits in up to K windows (the window rule of /root/reference datasets/imgnetvid.py:486-506), and
// everything upstream of a pooled / stacked join is per-frame arithmetic.  So the per-frame part of the network runs once
// per frame into a ring of S slots, and a window is a row of K slot numbers:
//
//   ring  [S][inner]            (= [S][hw][C], NHWC rows of one frame per slot)
//   slots [B][K]  int32         (device memory; values in [0, S), any order, repeats allowed: the clip's ends are padded
//                                by repeating the first / last frame)
//   pool: y [B][inner]          type 0 max, 1 mean - the arithmetic and the summation order of vd_temporal_pool /
//                               vd_temporal_pool_bf16 (vd_pointwise.hip k_tpool, k_tpool_bf16): start from frame 0 of the
//                               window, then frames 1 .. K-1 in order (`t > v` for the fp32 max, fmaxf for the bf16 one, a
//                               running sum and ONE division by K for the mean) -> the same bits as those kernels on the
//                               gathered copy [B][K][inner]
//   cat:  y [B][hw][K*C]        channel index k*C + c: vd_temporal_cat (forward) on the gathered copy; a copy of 16-byte
//                               units, so bf16 tensors go through it with C halved
//
// A lane owns one 16-byte unit of `inner` and walks the K slots of its window: every ring element a window needs is read
// once, every y element written once, no window is materialised.  The kernels do not trust the table: a slot outside
// [0, S) is clamped into range, so a bad table reads a wrong frame, never memory outside the ring (the host validates the
// table before it uploads it).  Plain loads and stores, no atomics: two runs give the same bits.
#include "vd_common.h"

namespace {

inline bool fits32(int64_t items) { return items + (int64_t)4096 * 256 < ((int64_t)1 << 31); }

inline int gblocks(int64_t n) {
    int64_t nb = vd_cdiv(n, 256);
    if (nb > 4096) nb = 4096;
    if (nb < 1) nb = 1;
    return (int)nb;
}

__device__ __forceinline__ int clamp_slot(int s, int S) { return s < 0 ? 0 : (s >= S ? S - 1 : s); }

// The index type IT is int32_t where every element index of the launch fits it (the host checks), else int64_t.
// inner4: 16-byte units (four floats) of one frame; total = B * inner4.
template <typename IT>
__global__ void k_tpool_idx(const float* __restrict__ ring, const int32_t* __restrict__ slots, float* __restrict__ y, int S, int K,
                            IT inner4, IT total, int type) {
    for (IT i = (IT)blockIdx.x * (IT)blockDim.x + (IT)threadIdx.x; i < total; i += (IT)gridDim.x * (IT)blockDim.x) {
        const IT b = i / inner4, r = i - b * inner4;
        const int32_t* sl = slots + (int64_t)b * K;
        f32x4 v = vd_ld4(ring, (IT)clamp_slot(sl[0], S) * inner4 + r);
        if (type == 0) {
            for (int k = 1; k < K; ++k) {
                const f32x4 t = vd_ld4(ring, (IT)clamp_slot(sl[k], S) * inner4 + r);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (t[e] > v[e]) v[e] = t[e];
            }
        } else {
            for (int k = 1; k < K; ++k) {
                const f32x4 t = vd_ld4(ring, (IT)clamp_slot(sl[k], S) * inner4 + r);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += t[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] /= (float)K;
        }
        vd_st4(y, i, v);
    }
}

// bf16 tensors: inner8 = 16-byte units (eight bf16) of one frame, the max / mean in fp32 as k_tpool_bf16 forms them
template <typename IT>
__global__ void k_tpool_idx_bf16(const __bf16* __restrict__ ring, const int32_t* __restrict__ slots, __bf16* __restrict__ y, int S,
                                 int K, IT inner8, IT total, int type) {
    for (IT i = (IT)blockIdx.x * (IT)blockDim.x + (IT)threadIdx.x; i < total; i += (IT)gridDim.x * (IT)blockDim.x) {
        const IT b = i / inner8, r = i - b * inner8;
        const int32_t* sl = slots + (int64_t)b * K;
        f32x8 v = vd_ld8(ring, (IT)clamp_slot(sl[0], S) * inner8 + r);
        for (int k = 1; k < K; ++k) {
            const f32x8 t = vd_ld8(ring, (IT)clamp_slot(sl[k], S) * inner8 + r);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = type == 0 ? fmaxf(v[e], t[e]) : v[e] + t[e];
        }
        if (type != 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] /= (float)K;
        }
        vd_st8(y, i, v);
    }
}

// y[b][px][k][c] = ring[slots[b][k]][px][c] in 16-byte units; total = B * hw * C4 (one lane per unit of a frame)
template <typename IT>
__global__ void k_tcat_idx(const float* __restrict__ ring, const int32_t* __restrict__ slots, float* __restrict__ y, int S, int K,
                           IT frame4, int C4, IT total) {
    for (IT i = (IT)blockIdx.x * (IT)blockDim.x + (IT)threadIdx.x; i < total; i += (IT)gridDim.x * (IT)blockDim.x) {
        const IT b = i / frame4, r = i - b * frame4;           // r = px * C4 + c
        const IT px = r / C4;
        const int32_t* sl = slots + (int64_t)b * K;
        IT o = (b * frame4 + px * C4) * K + (r - px * C4);     // ((b * hw + px) * K + 0) * C4 + c
        for (int k = 0; k < K; ++k, o += C4) vd_st4(y, o, vd_ld4(ring, (IT)clamp_slot(sl[k], S) * frame4 + r));
    }
}

inline bool aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) % 16) == 0; }

}  // namespace

extern "C" {

int vd_temporal_pool_idx(const float* ring, const int32_t* slots, float* y, int S, int B, int K, int64_t inner, int type,
                         void* stream) {
    VD_REQUIRE(ring && slots && y, "vd_temporal_pool_idx: ring, slots and y must not be NULL");
    VD_REQUIRE(K >= 1 && K < 128, "vd_temporal_pool_idx: 1 <= K < 128 needed, got K=%d", K);
    VD_REQUIRE(S >= 1 && B >= 1, "vd_temporal_pool_idx: S >= 1 and B >= 1 needed, got S=%d B=%d", S, B);
    VD_REQUIRE(inner > 0 && inner % 4 == 0 && (type == 0 || type == 1),
               "vd_temporal_pool_idx: bad sizes (inner=%lld must be a positive multiple of 4, type=%d must be 0 or 1)", (long long)inner,
               type);
    VD_REQUIRE(aligned16(ring, y) && (uintptr_t)slots % 4 == 0,
               "vd_temporal_pool_idx: ring and y must be 16-byte aligned, slots 4-byte aligned");
    const int64_t n4 = inner / 4, total = (int64_t)B * n4;
    if (fits32((int64_t)(S > B ? S : B) * n4))
        hipLaunchKernelGGL(k_tpool_idx<int32_t>, dim3(gblocks(total)), dim3(256), 0, (hipStream_t)stream, ring, slots, y, S, K,
                           (int32_t)n4, (int32_t)total, type);
    else
        hipLaunchKernelGGL(k_tpool_idx<int64_t>, dim3(gblocks(total)), dim3(256), 0, (hipStream_t)stream, ring, slots, y, S, K, n4,
                           total, type);
    VD_CHECK_LAUNCH("vd_temporal_pool_idx");
    return VD_OK;
}

int vd_temporal_pool_idx_bf16(const void* ring, const int32_t* slots, void* y, int S, int B, int K, int64_t inner, int type,
                              void* stream) {
    VD_REQUIRE(ring && slots && y, "vd_temporal_pool_idx_bf16: ring, slots and y must not be NULL");
    VD_REQUIRE(K >= 1 && K < 128, "vd_temporal_pool_idx_bf16: 1 <= K < 128 needed, got K=%d", K);
    VD_REQUIRE(S >= 1 && B >= 1, "vd_temporal_pool_idx_bf16: S >= 1 and B >= 1 needed, got S=%d B=%d", S, B);
    VD_REQUIRE(inner > 0 && inner % 8 == 0 && (type == 0 || type == 1),
               "vd_temporal_pool_idx_bf16: bad sizes (inner=%lld must be a positive multiple of 8, type=%d must be 0 or 1)",
               (long long)inner, type);
    VD_REQUIRE(aligned16(ring, y) && (uintptr_t)slots % 4 == 0,
               "vd_temporal_pool_idx_bf16: ring and y must be 16-byte aligned, slots 4-byte aligned");
    const int64_t n8 = inner / 8, total = (int64_t)B * n8;
    if (fits32((int64_t)(S > B ? S : B) * n8))
        hipLaunchKernelGGL(k_tpool_idx_bf16<int32_t>, dim3(gblocks(total)), dim3(256), 0, (hipStream_t)stream, (const __bf16*)ring,
                           slots, (__bf16*)y, S, K, (int32_t)n8, (int32_t)total, type);
    else
        hipLaunchKernelGGL(k_tpool_idx_bf16<int64_t>, dim3(gblocks(total)), dim3(256), 0, (hipStream_t)stream, (const __bf16*)ring,
                           slots, (__bf16*)y, S, K, n8, total, type);
    VD_CHECK_LAUNCH("vd_temporal_pool_idx_bf16");
    return VD_OK;
}

int vd_temporal_cat_idx(const float* ring, const int32_t* slots, float* y, int S, int B, int K, int64_t hw, int C, void* stream) {
    VD_REQUIRE(ring && slots && y, "vd_temporal_cat_idx: ring, slots and y must not be NULL");
    VD_REQUIRE(K >= 1 && K < 128, "vd_temporal_cat_idx: 1 <= K < 128 needed, got K=%d", K);
    VD_REQUIRE(S >= 1 && B >= 1, "vd_temporal_cat_idx: S >= 1 and B >= 1 needed, got S=%d B=%d", S, B);
    VD_REQUIRE(hw > 0 && C > 0 && C % 4 == 0, "vd_temporal_cat_idx: bad sizes (hw=%lld, C=%d must be a positive multiple of 4)",
               (long long)hw, C);
    VD_REQUIRE(aligned16(ring, y) && (uintptr_t)slots % 4 == 0,
               "vd_temporal_cat_idx: ring and y must be 16-byte aligned, slots 4-byte aligned");
    const int C4 = C / 4;
    const int64_t f4 = hw * C4, total = (int64_t)B * f4;
    if (fits32((int64_t)(S > (int64_t)B * K ? S : (int64_t)B * K) * f4))
        hipLaunchKernelGGL(k_tcat_idx<int32_t>, dim3(gblocks(total)), dim3(256), 0, (hipStream_t)stream, ring, slots, y, S, K,
                           (int32_t)f4, C4, (int32_t)total);
    else
        hipLaunchKernelGGL(k_tcat_idx<int64_t>, dim3(gblocks(total)), dim3(256), 0, (hipStream_t)stream, ring, slots, y, S, K, f4, C4,
                           total);
    VD_CHECK_LAUNCH("vd_temporal_cat_idx");
    return VD_OK;
}

}  // extern "C"
