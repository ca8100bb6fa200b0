// vd_appearance.hip — the appearance descriptor of every detected row, pooled from a route tensor of the backbone under the
// row's box (viddet_amd/appearance.py::embed_host is the definition): a fixed 4 x 4 grid of bilinear samples,
// their mean, centred over the channels, scaled by the row's max-abs and rounded to int8.  What embed_host computes, bit for bit.
//
// Arithmetic: fp32, operation for operation what embed_host does: no product and sum is contracted into an FMA, `/` is the
// correctly rounded one (hipcc's default; the Makefile sets no fast-math flag), rintf rounds ties to even.  The sum over the
// channels is embed_host's halving sum - p[:n/2] + p[n/2:n] until one element is left - made in LDS in exactly that
// association; the max-abs is np.maximum's, through which a NaN travels.
//
// One workgroup per (image, row); its threads run along the channels, four a thread, so every tap of a sample is a contiguous
// 16-byte load of the NHWC map (8 bytes of a bf16 map) and the row's C int8 leave as 4-byte stores.  C / 4 threads work, at
// least one wavefront is launched.  The sample positions are the same in every thread and formed by each.
// Every index is formed from clamped values: the map from map_index cut to [0, S), the cells from positions cut to the map.  No
// atomics; plain vector loads and stores; the inputs are never written; every output element is written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_clip_rows.h"

namespace {

constexpr int kEmbMinC = 8, kEmbMaxC = 1024, kEmbMaxN = 128;

// np.maximum of a pair: a NaN on either side gives NaN
__device__ inline float emb_max(float a, float b) { return (a >= b || a != a) ? a : b; }

// the position of sample i along an axis of n cells: the two cells and the weight of the second
__device__ inline void emb_axis(float lo, float side, float k, float inv, int n, int& i0, int& i1, float& a) {
    float c = (lo + side * k) * inv - 0.5f;
    const float hi = (float)(n - 1);
    c = c >= 0.f ? c : 0.f;                           // a NaN becomes 0
    c = c <= hi ? c : hi;
    const int top = n - 2 > 0 ? n - 2 : 0;
    i0 = (int)floorf(c);
    if (i0 > top) i0 = top;
    i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
    a = c - (float)i0;
}

__device__ inline f32x4 emb_ld4(const float* p, int64_t i) { return *reinterpret_cast<const f32x4*>(p + i); }
__device__ inline f32x4 emb_ld4(const __bf16* p, int64_t i) { return vd_ld4(p + i, 0); }

template <typename T>
__global__ __launch_bounds__(256) void k_roi_embed(const T* __restrict__ fmap, int S, int Hf, int Wf, int C, int ld,
                                                   const float* __restrict__ ids, const float4* __restrict__ bboxes,
                                                   const int32_t* __restrict__ map_index, int N, float inv, int8_t* __restrict__ emb) {
    __shared__ float s_sum[kEmbMaxC];
    __shared__ float s_abs[kEmbMaxC];
    const int tid = threadIdx.x, c0 = tid * 4;
    const int b = blockIdx.x / N;
    const int64_t row = blockIdx.x;
    const bool mine = c0 < C;
    const float id = ids[row];
    const float4 box = bboxes[row];
    uint32_t* out = reinterpret_cast<uint32_t*>(emb + row * C);
    if (!(id >= 0.f) || not_finite(box.x) || not_finite(box.y) || not_finite(box.z) || not_finite(box.w)) {
        if (mine) out[tid] = 0u;                      // the whole workgroup alike
        return;
    }
    int m = map_index ? map_index[b] : b;
    m = m < 0 ? 0 : (m >= S ? S - 1 : m);
    const T* f = fmap + (int64_t)m * Hf * Wf * ld;
    const float bw = box.z - box.x, bh = box.w - box.y;
    const float grid[4] = {0.125f, 0.375f, 0.625f, 0.875f};
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (mine) {
        int x0[4], x1[4];
        float ax[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) emb_axis(box.x, bw, grid[i], inv, Wf, x0[i], x1[i], ax[i]);
#pragma unroll
        for (int iy = 0; iy < 4; ++iy) {
            int y0, y1;
            float ay;
            emb_axis(box.y, bh, grid[iy], inv, Hf, y0, y1, ay);
            const int64_t r0 = (int64_t)y0 * Wf, r1 = (int64_t)y1 * Wf;
#pragma unroll
            for (int ix = 0; ix < 4; ++ix) {
                const f32x4 f00 = emb_ld4(f, (r0 + x0[ix]) * ld + c0), f01 = emb_ld4(f, (r0 + x1[ix]) * ld + c0);
                const f32x4 f10 = emb_ld4(f, (r1 + x0[ix]) * ld + c0), f11 = emb_ld4(f, (r1 + x1[ix]) * ld + c0);
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = f00[e] + ax[ix] * (f01[e] - f00[e]);
                    const float u = f10[e] + ax[ix] * (f11[e] - f10[e]);
                    v[e] = t + ay * (u - t);
                }
                if (iy == 0 && ix == 0) {
                    acc = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = acc[e] + v[e];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[e] = acc[e] * 0.0625f;
            s_sum[c0 + e] = acc[e];
        }
    }
    __syncthreads();
    // the halving sum: s[i] = s[i] + s[i + n] for i < n, n = C / 2 ... 1; the writes [0, n) and the reads [n, 2n) are apart
    for (int n = C >> 1; n >= 1; n >>= 1) {
        for (int i = tid; i < n; i += blockDim.x) s_sum[i] = s_sum[i] + s_sum[i + n];
        __syncthreads();
    }
    const float mean = s_sum[0] / (float)C;
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    if (mine) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            d[e] = acc[e] - mean;
            s_abs[c0 + e] = fabsf(d[e]);
        }
    }
    __syncthreads();
    for (int n = C >> 1; n >= 1; n >>= 1) {
        for (int i = tid; i < n; i += blockDim.x) s_abs[i] = emb_max(s_abs[i], s_abs[i + n]);
        __syncthreads();
    }
    const float a = s_abs[0];
    if (!mine) return;
    uint32_t word = 0u;
    if (a != 0.f && !not_finite(a)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int q = (int)rintf((d[e] / a) * 127.f);
            word |= ((uint32_t)q & 0xffu) << (8 * e);
        }
    }
    out[tid] = word;
}

}  // namespace

extern "C" {

int vd_roi_embed(const void* fmap, int is_bf16, int S, int Hf, int Wf, int C, int ld, const float* ids, const float* bboxes,
                 const int32_t* map_index, int B, int N, int stride, int8_t* emb, void* stream) {
    VD_REQUIRE(fmap && ids && bboxes && emb, "vd_roi_embed: fmap, ids, bboxes and emb must not be NULL");
    VD_REQUIRE(C >= kEmbMinC && C <= kEmbMaxC && (C & (C - 1)) == 0, "vd_roi_embed: C=%d, a power of two in [%d, %d] is taken", C,
               kEmbMinC, kEmbMaxC);
    VD_REQUIRE(ld >= C && ld % 4 == 0, "vd_roi_embed: ld=%d, the pitch of a pixel must be >= C=%d and a multiple of 4", ld, C);
    VD_REQUIRE(S >= 1 && Hf >= 1 && Wf >= 1 && (int64_t)S * Hf * Wf * ld <= 0x7fffffffll * 16,
               "vd_roi_embed: S=%d maps of %d x %d cells: all >= 1 needed, and at most 2^35 elements", S, Hf, Wf);
    VD_REQUIRE(B >= 1 && N >= 1 && N <= kEmbMaxN, "vd_roi_embed: B=%d images of N=%d rows, B >= 1 and 1 <= N <= %d are taken", B, N,
               kEmbMaxN);
    VD_REQUIRE((int64_t)B * N <= 0x7fffffff, "vd_roi_embed: B * N = %lld rows, at most 2^31 - 1 are taken", (long long)B * N);
    VD_REQUIRE(stride == 8 || stride == 16 || stride == 32, "vd_roi_embed: stride=%d, 8, 16 or 32 are taken", stride);
    VD_REQUIRE(is_bf16 == 0 || is_bf16 == 1, "vd_roi_embed: is_bf16 must be 0 or 1, got %d", is_bf16);
    VD_REQUIRE(((uintptr_t)fmap % (is_bf16 ? 8 : 16)) == 0 && ((uintptr_t)bboxes % 16) == 0,
               "vd_roi_embed: fmap must be aligned to four of its elements and bboxes to 16 bytes");
    VD_REQUIRE((((uintptr_t)ids | (uintptr_t)map_index | (uintptr_t)emb) % 4) == 0,
               "vd_roi_embed: ids, map_index and emb must be 4-byte aligned");
    const int threads = C / 4 < 64 ? 64 : C / 4;
    const float inv = 1.f / (float)stride;
    hipStream_t s = (hipStream_t)stream;
    if (is_bf16)
        hipLaunchKernelGGL(k_roi_embed<__bf16>, dim3((unsigned)(B * N)), dim3(threads), 0, s, (const __bf16*)fmap, S, Hf, Wf, C, ld, ids,
                           (const float4*)bboxes, map_index, N, inv, emb);
    else
        hipLaunchKernelGGL(k_roi_embed<float>, dim3((unsigned)(B * N)), dim3(threads), 0, s, (const float*)fmap, S, Hf, Wf, C, ld, ids,
                           (const float4*)bboxes, map_index, N, inv, emb);
    VD_CHECK_LAUNCH("vd_roi_embed");
    return VD_OK;
}

}  // extern "C"
