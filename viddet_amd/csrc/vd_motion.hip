// vd_motion.hip — camera-motion compensation of the clip trackers (viddet_amd/motion.py is the definition): the
// luma signature of every frame (vd_motion_sig), the translation between consecutive frames by block matching on the
// signatures (vd_motion_match), and the shift of the boxes into the stabilised coordinate frame and back (vd_motion_shift).
// What signature_host, match_host and stabilise_host / restore_host compute, bit for bit.
//
// Arithmetic: integers everywhere below the box shift, so the order of a sum is free; the shift is one fp32 multiply and one
// fp32 add or subtract per corner, never contracted into an FMA.
//
// vd_motion_sig is a bandwidth pass: a thread owns 16 pixels of one row of cells and walks the `cell` pixel rows under them.
// Where the frames' base, pitch and frame stride are multiples of 16 a pixel row of a thread is one 16-byte load (NV12) or
// three (RGB) and consecutive lanes read consecutive bytes; any other surface, and the last columns of a row where fewer than
// 16 covered pixels are left, are read byte by byte.  Both paths form the same integers.  RGB luma is one v_dot4_u32_u8 per
// pixel on the three bytes that v_alignbyte_b32 cuts out of the loaded words; NV12 bytes are summed four at a time by
// v_sad_u8 against zero.  A thread's 16 / cell words leave in one store where the output row allows, else one by one.
// vd_motion_match: one launch fills the (F, D, D) int64 SAD table, D = 2 * radius + 1, a workgroup per (frame pair,
// displacement); the signatures of a 720 x 1280 clip do not fit LDS, so the cells are read through L1 / L2.  A second launch, a
// workgroup per clip, picks every frame's winner by the packed key, applies the gate and forms the running sum of the clip.
// No atomics.  Every index is formed from checked arguments: a clip's frames are cut to [0, F) (clip_of), the displaced cell
// gy - dy, gx - dx of an interior cell lies in the grid because |dy|, |dx| <= radius.  The inputs are never written.
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_clip_rows.h"

namespace {

constexpr int kMaxRadius = 16, kMaxGrid = 4096, kMaxSide = 16384;
constexpr uint32_t kLumaCoef = 77u | 150u << 8 | 29u << 16;       // R, G, B as the bytes lie in memory; the fourth byte counts 0

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ inline uint32_t luma_rgb(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// frame f at frames + f * frame_stride, rows `pitch` bytes apart; a thread per (frame, row of cells, chunk of 16 pixels)
template <bool kRgb, int kCell>
__global__ __launch_bounds__(256) void k_motion_sig(const uint8_t* __restrict__ frames, int64_t frame_stride, int64_t pitch,
                                                    uint32_t total, int Gh, int Gw, int chunks, int wide, int ovec,
                                                    uint16_t* __restrict__ sig) {
    constexpr int kN = 16 / kCell;                                // the cells of a chunk
    constexpr int kBpp = kRgb ? 3 : 1;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint32_t r = i / (uint32_t)chunks;
    const int j = (int)(i - r * (uint32_t)chunks);
    const uint32_t f = r / (uint32_t)Gh;
    const int gy = (int)(r - f * (uint32_t)Gh);
    const int x0 = j * 16;
    const int left = Gw * kCell - x0;                             // covered pixels from x0 on: a multiple of kCell, >= kCell
    const int npx = left < 16 ? left : 16;
    const uint8_t* row = frames + (int64_t)f * frame_stride + (int64_t)gy * kCell * pitch + (int64_t)x0 * kBpp;
    uint32_t acc[kN];
#pragma unroll
    for (int c = 0; c < kN; ++c) acc[c] = 0u;
    if (wide && npx == 16) {
#pragma unroll
        for (int ry = 0; ry < kCell; ++ry) {
            const u32x4* p = reinterpret_cast<const u32x4*>(row + (int64_t)ry * pitch);
            if (kRgb) {
                const u32x4 a = p[0], b = p[1], c = p[2];
                const uint32_t w[13] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], c[0], c[1], c[2], c[3], 0u};
#pragma unroll
                for (int px = 0; px < 16; ++px) {
                    const uint32_t rgbx = __builtin_amdgcn_alignbyte(w[(3 * px) / 4 + 1], w[(3 * px) / 4], (3 * px) % 4);
                    acc[px / kCell] += __builtin_amdgcn_udot4(rgbx, kLumaCoef, 128u, false) >> 8;
                }
            } else {
                const u32x4 a = p[0];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (kCell == 2) {
                        acc[2 * k] = __builtin_amdgcn_sad_u8(a[k] & 0xffffu, 0u, acc[2 * k]);
                        acc[2 * k + 1] = __builtin_amdgcn_sad_u8(a[k] >> 16, 0u, acc[2 * k + 1]);
                    } else {
                        acc[(4 * k) / kCell] = __builtin_amdgcn_sad_u8(a[k], 0u, acc[(4 * k) / kCell]);
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int ry = 0; ry < kCell; ++ry) {
            const uint8_t* p = row + (int64_t)ry * pitch;
#pragma unroll
            for (int px = 0; px < 16; ++px) {
                if (px < npx) {
                    if (kRgb)
                        acc[px / kCell] += luma_rgb(p[3 * px], p[3 * px + 1], p[3 * px + 2]);
                    else
                        acc[px / kCell] += p[px];
                }
            }
        }
    }
    uint16_t* o = sig + (int64_t)r * Gw + x0 / kCell;
    if (ovec && npx == 16 && kN > 1) {
        if (kN == 8) {
            const u32x4 v = {acc[0] | acc[1 % kN] << 16, acc[2 % kN] | acc[3 % kN] << 16, acc[4 % kN] | acc[5 % kN] << 16,
                             acc[6 % kN] | acc[7 % kN] << 16};
            *reinterpret_cast<u32x4*>(o) = v;
        } else if (kN == 4) {
            const u32x2 v = {acc[0] | acc[1 % kN] << 16, acc[2 % kN] | acc[3 % kN] << 16};
            *reinterpret_cast<u32x2*>(o) = v;
        } else {
            *reinterpret_cast<uint32_t*>(o) = acc[0] | acc[1 % kN] << 16;
        }
    } else {
        const int nc = npx / kCell;
#pragma unroll
        for (int c = 0; c < kN; ++c)
            if (c < nc) o[c] = (uint16_t)acc[c];
    }
}

__device__ inline unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ inline unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

// table[t][dy + R][dx + R] = SAD(dx, dy) of frames t and t - 1, t in [1, F): a workgroup per entry, a wave per row of interior cells
__global__ __launch_bounds__(256) void k_motion_sad(const uint16_t* __restrict__ sig, int Gh, int Gw, int R, int64_t* __restrict__ table) {
    __shared__ unsigned long long s_part[4];
    const int D = 2 * R + 1;
    const uint32_t e = blockIdx.x;                                // ((t - 1) * D + dyi) * D + dxi
    const uint32_t q = e / (uint32_t)D;
    const int dx = (int)(e - q * (uint32_t)D) - R;
    const uint32_t t1 = q / (uint32_t)D;
    const int dy = (int)(q - t1 * (uint32_t)D) - R;
    const int64_t t = (int64_t)t1 + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Ih = Gh - 2 * R, Iw = Gw - 2 * R;
    const uint16_t* cur = sig + (t * Gh + R) * Gw + R;
    const uint16_t* prev = sig + ((t - 1) * Gh + R - dy) * Gw + R - dx;
    unsigned long long sum = 0ull;
    for (int y = wave; y < Ih; y += 4) {
        const uint16_t* c = cur + (int64_t)y * Gw;
        const uint16_t* p = prev + (int64_t)y * Gw;
        uint32_t s = 0u;                                          // a row: at most 4096 * 65280 < 2^32
        for (int x = lane; x < Iw; x += 64) {
            const int d = (int)c[x] - (int)p[x];
            s += (uint32_t)(d < 0 ? -d : d);
        }
        sum += s;
    }
    sum = wave_sum(sum);
    if (lane == 0) s_part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) table[t * D * D + (int64_t)(dy + R) * D + (dx + R)] = (int64_t)(s_part[0] + s_part[1] + s_part[2] + s_part[3]);
}

// a workgroup per clip: a wave per frame picks the winner by the key (SAD, dx*dx + dy*dy, dy, dx) packed into one word,
// applies the gate and writes motion and sad; then one thread forms the clip's running sum
__global__ __launch_bounds__(256) void k_motion_pick(const int64_t* __restrict__ table, const int32_t* __restrict__ clip_start, int F,
                                                     int R, int cell, int gate_q, int32_t* __restrict__ motion,
                                                     int64_t* __restrict__ sad, int32_t* __restrict__ cum) {
    const int D = 2 * R + 1, DD = D * D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int t0, t1;
    clip_of(clip_start, blockIdx.x, F, t0, t1);
    for (int t = t0 + wave; t < t1; t += 4) {
        int mx = 0, my = 0;
        long long best = 0, zero = 0;
        if (t > t0) {
            const int64_t* tab = table + (int64_t)t * DD;
            unsigned long long key = ~0ull;
            for (int e = lane; e < DD; e += 64) {
                const int dyi = e / D, dxi = e - dyi * D;
                const int dx = dxi - R, dy = dyi - R;
                const unsigned long long k =
                    (((unsigned long long)tab[e] << 10 | (unsigned)(dx * dx + dy * dy)) << 6 | (unsigned)dyi) << 6 | (unsigned)dxi;
                key = k < key ? k : key;
            }
            key = wave_min(key);
            const int dxi = (int)(key & 63u), dyi = (int)(key >> 6 & 63u);
            best = (long long)(key >> 22);
            zero = tab[R * D + R];
            if (best * 256 <= zero * gate_q) mx = (dxi - R) * cell, my = (dyi - R) * cell;
        }
        if (lane == 0) {
            motion[2 * (int64_t)t] = mx, motion[2 * (int64_t)t + 1] = my;
            sad[2 * (int64_t)t] = best, sad[2 * (int64_t)t + 1] = zero;
        }
    }
    __syncthreads();                                              // the waves' motion, written above, is read below
    if (threadIdx.x == 0) {
        uint32_t cx = 0u, cy = 0u;                                // int32 sums that wrap
        for (int t = t0; t < t1; ++t) {
            cx += (uint32_t)motion[2 * (int64_t)t], cy += (uint32_t)motion[2 * (int64_t)t + 1];
            cum[2 * (int64_t)t] = (int32_t)cx, cum[2 * (int64_t)t + 1] = (int32_t)cy;
        }
    }
}

// out = boxes -+ (float(cum[t]) * (sx, sy)) on the rows whose key says so (ids: >= 0, a NaN is not; track: >= 0); the others' bits
template <bool kTrack>
__global__ __launch_bounds__(256) void k_motion_shift(const void* __restrict__ key, const float4* __restrict__ boxes,
                                                      const int32_t* __restrict__ cum, int N, int64_t n, float sx, float sy, int add,
                                                      float4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 b = boxes[i];
    const bool on = kTrack ? static_cast<const int32_t*>(key)[i] >= 0 : static_cast<const float*>(key)[i] >= 0.f;
    if (on) {
        const int64_t t = i / N;
        const float ox = (float)cum[2 * t] * sx, oy = (float)cum[2 * t + 1] * sy;
        if (add)
            b.x = b.x + ox, b.y = b.y + oy, b.z = b.z + ox, b.w = b.w + oy;
        else
            b.x = b.x - ox, b.y = b.y - oy, b.z = b.z - ox, b.w = b.w - oy;
    }
    out[i] = b;
}

template <bool kRgb>
void launch_sig(int cell, dim3 grid, hipStream_t s, const uint8_t* frames, int64_t frame_stride, int64_t pitch, uint32_t total, int Gh,
                int Gw, int chunks, int wide, int ovec, uint16_t* sig) {
    switch (cell) {
    case 2: hipLaunchKernelGGL((k_motion_sig<kRgb, 2>), grid, dim3(256), 0, s, frames, frame_stride, pitch, total, Gh, Gw, chunks, wide, ovec, sig); break;
    case 4: hipLaunchKernelGGL((k_motion_sig<kRgb, 4>), grid, dim3(256), 0, s, frames, frame_stride, pitch, total, Gh, Gw, chunks, wide, ovec, sig); break;
    case 8: hipLaunchKernelGGL((k_motion_sig<kRgb, 8>), grid, dim3(256), 0, s, frames, frame_stride, pitch, total, Gh, Gw, chunks, wide, ovec, sig); break;
    default: hipLaunchKernelGGL((k_motion_sig<kRgb, 16>), grid, dim3(256), 0, s, frames, frame_stride, pitch, total, Gh, Gw, chunks, wide, ovec, sig); break;
    }
}

}  // namespace

extern "C" {

int vd_motion_sig(const uint8_t* frames, int64_t frame_stride, int64_t pitch, int fmt, int F, int H0, int W0, int cell, uint16_t* sig,
                  void* stream) {
    VD_REQUIRE(frames && sig, "vd_motion_sig: frames and sig must not be NULL");
    VD_REQUIRE(fmt == 0 || fmt == 1, "vd_motion_sig: fmt must be 0 (RGB) or 1 (NV12), got %d", fmt);
    VD_REQUIRE(cell == 2 || cell == 4 || cell == 8 || cell == 16, "vd_motion_sig: cell=%d, 2, 4, 8 or 16 are taken", cell);
    VD_REQUIRE(F >= 1 && H0 >= cell && W0 >= cell && H0 <= kMaxSide && W0 <= kMaxSide,
               "vd_motion_sig: F=%d frames of %d x %d pixels: F >= 1 and sides in [cell=%d, %d] are taken", F, H0, W0, cell, kMaxSide);
    const int64_t row_bytes = (int64_t)W0 * (fmt == 0 ? 3 : 1);
    VD_REQUIRE(pitch >= row_bytes && pitch <= (int64_t)1 << 20, "vd_motion_sig: pitch=%lld, a row holds %lld bytes (at most 2^20 are taken)",
               (long long)pitch, (long long)row_bytes);
    VD_REQUIRE(frame_stride >= pitch * (H0 - 1) + row_bytes && frame_stride <= (int64_t)1 << 40,
               "vd_motion_sig: frame_stride=%lld does not cover the %d rows of a frame at pitch %lld (at most 2^40 is taken)",
               (long long)frame_stride, H0, (long long)pitch);
    VD_REQUIRE(((uintptr_t)sig % 2) == 0, "vd_motion_sig: sig must be 2-byte aligned");
    const int Gh = H0 / cell, Gw = W0 / cell;
    const int chunks = (int)vd_cdiv((int64_t)Gw * cell, 16);
    const int64_t total = (int64_t)F * Gh * chunks;
    VD_REQUIRE(total <= 0x7fffffffll - 256, "vd_motion_sig: F * Gh * ceil(Gw * cell / 16) = %lld work items, fewer than 2^31 are taken",
               (long long)total);
    const int wide = ((uintptr_t)frames % 16) == 0 && pitch % 16 == 0 && frame_stride % 16 == 0;
    const int ovec = ((uintptr_t)sig % 16) == 0 && Gw % (16 / cell) == 0;
    const dim3 grid((unsigned)vd_cdiv(total, 256));
    hipStream_t s = (hipStream_t)stream;
    if (fmt == 0)
        launch_sig<true>(cell, grid, s, frames, frame_stride, pitch, (uint32_t)total, Gh, Gw, chunks, wide, ovec, sig);
    else
        launch_sig<false>(cell, grid, s, frames, frame_stride, pitch, (uint32_t)total, Gh, Gw, chunks, wide, ovec, sig);
    VD_CHECK_LAUNCH("vd_motion_sig");
    return VD_OK;
}

int64_t vd_motion_match_ws_bytes(int F, int radius) {
    if (F < 1 || radius < 1 || radius > kMaxRadius) return -1;
    const int64_t D = 2 * radius + 1;
    if ((int64_t)F * D * D > 0x7fffffffll) return -1;
    return 8 * (int64_t)F * D * D;
}

int vd_motion_match(const uint16_t* sig, const int32_t* clip_start, int V, int F, int Gh, int Gw, int cell, int radius, float gate,
                    int32_t* motion, int64_t* sad, int32_t* cum, void* ws, int64_t ws_bytes, void* stream) {
    VD_REQUIRE(sig && motion && sad && cum && ws, "vd_motion_match: sig, motion, sad, cum and ws must not be NULL");
    VD_REQUIRE(F >= 1 && V >= 1, "vd_motion_match: F >= 1 and V >= 1 needed, got F=%d V=%d", F, V);
    VD_REQUIRE(clip_start || V == 1, "vd_motion_match: clip_start may be NULL only with V == 1 (one clip [0, F)), got V=%d", V);
    VD_REQUIRE(cell == 2 || cell == 4 || cell == 8 || cell == 16, "vd_motion_match: cell=%d, 2, 4, 8 or 16 are taken", cell);
    VD_REQUIRE(radius >= 1 && radius <= kMaxRadius, "vd_motion_match: radius=%d, 1 <= radius <= %d are taken", radius, kMaxRadius);
    VD_REQUIRE(gate > 0.f && gate <= 1.f, "vd_motion_match: gate=%g, a number in (0, 1] is taken", (double)gate);
    VD_REQUIRE(Gh > 2 * radius && Gw > 2 * radius && Gh <= kMaxGrid && Gw <= kMaxGrid,
               "vd_motion_match: a signature of %d x %d cells: radius=%d needs more than %d a side, at most %d are taken", Gh, Gw, radius,
               2 * radius, kMaxGrid);
    const int64_t need = vd_motion_match_ws_bytes(F, radius);
    VD_REQUIRE(need >= 0, "vd_motion_match: F * (2 * radius + 1)^2 = %lld table entries, at most 2^31 - 1 are taken",
               (long long)F * (2 * radius + 1) * (2 * radius + 1));
    VD_REQUIRE(ws_bytes >= need, "vd_motion_match: ws_bytes=%lld, 8 * F * (2 * radius + 1)^2 = %lld needed", (long long)ws_bytes,
               (long long)need);
    VD_REQUIRE((((uintptr_t)sad | (uintptr_t)ws) % 8) == 0 && (((uintptr_t)motion | (uintptr_t)cum | (uintptr_t)clip_start) % 4) == 0 &&
                   ((uintptr_t)sig % 2) == 0,
               "vd_motion_match: sad and ws must be 8-byte, motion, cum and clip_start 4-byte, sig 2-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int D = 2 * radius + 1;
    if (clip_start) {                                             // a frame that no clip covers comes out as zeros
        (void)hipMemsetAsync(motion, 0, 8 * (size_t)F, s);
        (void)hipMemsetAsync(sad, 0, 16 * (size_t)F, s);
        (void)hipMemsetAsync(cum, 0, 8 * (size_t)F, s);
    }
    if (F > 1)
        hipLaunchKernelGGL(k_motion_sad, dim3((unsigned)((int64_t)(F - 1) * D * D)), dim3(256), 0, s, sig, Gh, Gw, radius, (int64_t*)ws);
    const int gate_q = (int)(gate * 256.f);
    hipLaunchKernelGGL(k_motion_pick, dim3((unsigned)V), dim3(256), 0, s, (const int64_t*)ws, clip_start, F, radius, cell, gate_q, motion,
                       sad, cum);
    VD_CHECK_LAUNCH("vd_motion_match");
    return VD_OK;
}

int vd_motion_shift(const void* key, int key_is_track, const float* boxes, const int32_t* cum, int F, int N, float sx, float sy, int sign,
                    float* out, void* stream) {
    VD_REQUIRE(key && boxes && cum && out, "vd_motion_shift: key, boxes, cum and out must not be NULL");
    VD_REQUIRE(key_is_track == 0 || key_is_track == 1, "vd_motion_shift: key_is_track must be 0 or 1, got %d", key_is_track);
    VD_REQUIRE(sign == 1 || sign == -1, "vd_motion_shift: sign must be +1 (restore) or -1 (stabilise), got %d", sign);
    VD_REQUIRE(F >= 1 && N >= 1 && (int64_t)F * N <= 0x7fffffff, "vd_motion_shift: F=%d frames of N=%d rows: both >= 1, at most 2^31 - 1 rows",
               F, N);
    VD_REQUIRE(boxes != out, "vd_motion_shift: out must not be boxes: the input is never written");
    VD_REQUIRE((((uintptr_t)boxes | (uintptr_t)out) % 16) == 0 && (((uintptr_t)key | (uintptr_t)cum) % 4) == 0,
               "vd_motion_shift: boxes and out must be 16-byte, key and cum 4-byte aligned");
    const int64_t n = (int64_t)F * N;
    hipStream_t s = (hipStream_t)stream;
    if (key_is_track)
        hipLaunchKernelGGL(k_motion_shift<true>, dim3((unsigned)vd_cdiv(n, 256)), dim3(256), 0, s, key, (const float4*)boxes, cum, N, n, sx,
                           sy, sign > 0, (float4*)out);
    else
        hipLaunchKernelGGL(k_motion_shift<false>, dim3((unsigned)vd_cdiv(n, 256)), dim3(256), 0, s, key, (const float4*)boxes, cum, N, n, sx,
                           sy, sign > 0, (float4*)out);
    VD_CHECK_LAUNCH("vd_motion_shift");
    return VD_OK;
}

}  // extern "C"
