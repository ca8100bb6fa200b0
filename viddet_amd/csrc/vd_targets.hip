// vd_targets.hip — the YOLO prefetch targets on the device (viddet_amd/device_targets.py): the (M,5) label rows of
// every image -> the five dense tensors the loss kernel reads, objectness [N][P][1], centre [N][P][2], scale [N][P][2], weight
// [N][P][2] and class [N][P][C].  P = 3 * sum over strides 32, 16, 8 of (H/s)(W/s); row order is the network's training order:
// the stride-32 layer first, (y*w + x)*3 + a inside a layer.
//
// Arithmetic: viddet_amd/targets.py::prefetch_targets restated operation for operation.  Box width, height and the centre
// x0 + w/2 in fp32; everything behind them in fp64: the zero-centred shape IoU against the nine anchors (inter / union, 0 where
// union <= 0, first maximum wins), layer, a = divmod(match, 3), fx = gx / W * gw_layer, lx = (int)fx, centre = fx - lx,
// scale = log(max(gw, 1) / anchor), weight = 2 - gw*gh / W / H, objectness = 1 or the mix ratio.  No product and sum of this
// file is contracted into an FMA (the pragma below): aw*ah + gw*gh - inter must round as NumPy rounds it, or a near-tie of the
// argmax picks another anchor.  With IEEE fp64 division everything except log() is bit-equal to the host.
//
// Work shape: two launches in stream order.
//   1. k_targets_fill: the defaults (0, and -1 for the class tensor) over all five tensors of the whole batch, flat, 16 bytes
//      per lane, with scalar head / tail elements where a tensor's start is not 16-byte aligned or its length no multiple of 4.
//   2. k_targets_rows: one workgroup per image.  Every gt's match and flat row p go to LDS; a reduction finds the valid prefix
//      (the host stops at the first row with a coordinate < 0 or NaN); a gt is LIVE if it lies in the prefix, its p lies in
//      [0, P) and no later gt of the prefix has the same p (the host's later assignment overwrites every column, the whole
//      class row included).  Live gts have distinct rows, so their stores never meet: the owner thread writes the four narrow
//      columns, and the class rows of all live gts are written by the whole workgroup, flat over (live gt, class).
// The fill and the rows never race (stream order), there is no atomic, every element is written on every call, and two calls
// on the same inputs give the same bits.
#include "vd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxM = 512, kPerThread = kMaxM / kThreads, kChunks = kMaxM / 64;
constexpr int kFillBlocks = 2048;             // grid-stride fill: 8 workgroups per CU

// the anchors in output order: stride 32's three first (viddet_amd/targets.py _OUT_ANCHORS)
__device__ const double kAnchorW[9] = {116., 156., 373., 30., 62., 59., 10., 16., 33.};
__device__ const double kAnchorH[9] = {90., 198., 326., 61., 45., 119., 13., 30., 23.};

struct FillSeg {
    float* p;
    int64_t n;
    float v;
};
struct FillArgs {
    FillSeg s[5];
};

__global__ __launch_bounds__(kThreads) void k_targets_fill(FillArgs args) {
    const FillSeg s = args.s[blockIdx.y];
    float* __restrict__ p = s.p;
    const int64_t n = s.n;
    int64_t head = (4 - (int64_t)(((uintptr_t)p >> 2) & 3)) & 3;          // floats up to the next 16-byte boundary
    head = head < n ? head : n;
    const int64_t body = (n - head) >> 2, tail = n - head - 4 * body;
    float4* __restrict__ q = reinterpret_cast<float4*>(p + head);
    const float4 v4 = make_float4(s.v, s.v, s.v, s.v);
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = t; i < body; i += stride) q[i] = v4;
    if (t < head) p[t] = s.v;
    if (t < tail) p[head + 4 * body + t] = s.v;
}

struct Row {
    int p;                                    // flat row of the image, -1: no row (invalid gt, or p outside [0, P))
    float cx, cy, sx, sy, w;
};

// one gt of an image: prefetch_targets' per-gt arithmetic.  valid = all four coordinates >= 0 (NaN fails)
__device__ inline Row target_row(const float* __restrict__ box, int H, int W, int64_t P, bool* valid) {
    const float x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    *valid = x0 >= 0.f && y0 >= 0.f && x1 >= 0.f && y1 >= 0.f;
    const float gwf = x1 - x0, ghf = y1 - y0;
    const float gxf = x0 + gwf / 2.0f, gyf = y0 + ghf / 2.0f;
    const double gw = gwf, gh = ghf, gx = gxf, gy = gyf;
    int match = 0;
    double best = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double aw = kAnchorW[k], ah = kAnchorH[k];
        const double mw = aw < gw ? aw : gw, mh = ah < gh ? ah : gh;
        const double inter = (mw > 0.0 ? mw : 0.0) * (mh > 0.0 ? mh : 0.0);
        const double uni = aw * ah + gw * gh - inter;
        const double iou = uni > 0.0 ? inter / uni : 0.0;
        if (k == 0 || iou > best) best = iou, match = k;
    }
    const int layer = match / 3, a = match - 3 * layer;
    const int s = 32 >> layer, hh = H / s, ww = W / s;
    const int64_t c32 = (int64_t)(H / 32) * (W / 32) * 3;
    const int64_t base = layer == 0 ? 0 : layer == 1 ? c32 : 5 * c32;
    const double fx = gx / (double)W * (double)ww, fy = gy / (double)H * (double)hh;
    // clamped before the cast: whatever the coordinates are, lx and ly are small integers and p is compared with P in 64 bits
    const double kCap = 16777216.0;
    const int lx = (int)fmin(fmax(fx, 0.0), kCap), ly = (int)fmin(fmax(fy, 0.0), kCap);
    const int64_t p = base + ((int64_t)ly * ww + lx) * 3 + a;
    Row r;
    r.p = (*valid && p >= 0 && p < P) ? (int)p : -1;
    r.cx = (float)(fx - (double)lx);
    r.cy = (float)(fy - (double)ly);
    r.sx = (float)log((1.0 > gw ? 1.0 : gw) / kAnchorW[match]);
    r.sy = (float)log((1.0 > gh ? 1.0 : gh) / kAnchorH[match]);
    r.w = (float)(2.0 - gw * gh / (double)W / (double)H);
    return r;
}

__global__ __launch_bounds__(kThreads) void k_targets_rows(const float* __restrict__ gt, const float* __restrict__ ids, int idw,
                                                           const float* __restrict__ mix, int M, int C, int H, int W, int P,
                                                           float* __restrict__ obj, float* __restrict__ ctr,
                                                           float* __restrict__ scl, float* __restrict__ wgt,
                                                           float* __restrict__ cls) {
    __shared__ int s_p[kMaxM];
    __shared__ int s_list[kMaxM];
    __shared__ int s_cnt[kChunks];
    __shared__ int s_red[kWaves];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = blockIdx.x;
    gt += n * M * 4;
    ids += n * M * idw;
    if (mix) mix += n * M;
    obj += n * P;
    ctr += n * P * 2;
    scl += n * P * 2;
    wgt += n * P * 2;
    cls += n * P * C;

    // every gt's row, and the first invalid gt of the image
    Row row[kPerThread];
    int first_bad = M;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int m = tid + k * kThreads;
        row[k].p = -1;
        if (m < M) {
            bool valid;
            row[k] = target_row(gt + 4 * m, H, W, P, &valid);
            if (!valid) first_bad = min(first_bad, m);
        }
        s_p[m] = row[k].p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) first_bad = min(first_bad, __shfl_xor(first_bad, off));
    if (lane == 0) s_red[wave] = first_bad;
    __syncthreads();
    int prefix = s_red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) prefix = min(prefix, s_red[w]);

    // live gts: in the prefix, on a row of the image, and the LAST of the prefix on that row
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int m = tid + k * kThreads, p = row[k].p;
        bool live = m < prefix && p >= 0;
        for (int j = m + 1; live && j < prefix; ++j) live = s_p[j] != p;
        if (live) {
            obj[p] = mix ? mix[m] : 1.0f;
            ctr[2 * p] = row[k].cx, ctr[2 * p + 1] = row[k].cy;
            scl[2 * p] = row[k].sx, scl[2 * p + 1] = row[k].sy;
            wgt[2 * p] = row[k].w, wgt[2 * p + 1] = row[k].w;
        }
        // compaction of the live gts in gt order: chunk = 64 consecutive gts = this wave's ballot
        const unsigned long long mask = __ballot(live);
        const int chunk = wave + k * kWaves;
        if (lane == 0) s_cnt[chunk] = __popcll(mask);
        row[k].p = live ? __popcll(mask & ((1ull << lane) - 1ull)) : -1;      // rank inside the chunk
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) total += s_cnt[c];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int chunk = wave + k * kWaves;
        int off = 0;
#pragma unroll
        for (int c = 0; c < kChunks; ++c)
            if (c < chunk) off += s_cnt[c];
        if (row[k].p >= 0) s_list[off + row[k].p] = tid + k * kThreads;
    }
    __syncthreads();

    // the class rows of the live gts, flat over (live gt, class)
    const int cells = total * C;                                              // <= 512 * C, C checked by the entry point
    for (int e = tid; e < cells; e += kThreads) {
        const int j = e / C, c = e - j * C;
        const int m = s_list[j], p = s_p[m];
        float v;
        if (idw == 1) {
            const float idf = ids[m];
            const int id = (idf >= 0.f && idf < (float)C) ? (int)idf : -1;   // an index outside [0, C) writes no 1
            v = c == id ? 1.0f : 0.0f;
        } else {
            v = ids[(int64_t)m * C + c];
        }
        cls[(int64_t)p * C + c] = v;
    }
}

}  // namespace

extern "C" {

int vd_yolo_targets(const float* gt, const float* ids, int idw, const float* mix, int N, int M, int C, int H, int W, float* obj,
                    float* ctr, float* scl, float* wgt, float* cls, void* stream) {
    VD_REQUIRE(gt && ids && obj && ctr && scl && wgt && cls,
               "vd_yolo_targets: gt, ids and the five outputs (obj, ctr, scl, wgt, cls) must not be NULL (only mix may be)");
    VD_REQUIRE(N >= 1 && M >= 1 && C >= 1, "vd_yolo_targets: N, M and C must be >= 1, got N=%d M=%d C=%d", N, M, C);
    VD_REQUIRE(M <= kMaxM, "vd_yolo_targets: M=%d label rows per image, at most %d are taken", M, kMaxM);
    VD_REQUIRE(H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0,
               "vd_yolo_targets: H and W must be multiples of 32 and >= 32, got H=%d W=%d", H, W);
    VD_REQUIRE(idw == 1 || idw == C, "vd_yolo_targets: idw must be 1 (class index) or C=%d (multi-hot row), got idw=%d", C, idw);
    VD_REQUIRE((((uintptr_t)obj | (uintptr_t)ctr | (uintptr_t)scl | (uintptr_t)wgt | (uintptr_t)cls) % 4) == 0,
               "vd_yolo_targets: the outputs (obj, ctr, scl, wgt, cls) must be 4-byte aligned");
    VD_REQUIRE((((uintptr_t)gt | (uintptr_t)ids | (uintptr_t)mix) % 4) == 0,
               "vd_yolo_targets: gt, ids and mix must be 4-byte aligned");
    const int64_t P = (int64_t)(H / 32) * (W / 32) * 63;                      // 3 * (1 + 4 + 16) rows per stride-32 cell
    VD_REQUIRE(P * C < ((int64_t)1 << 31) && (int64_t)kMaxM * C < ((int64_t)1 << 31),
               "vd_yolo_targets: P*C = %lld elements per image are more than the kernel indexes", (long long)(P * C));
    const int64_t NP = (int64_t)N * P;
    FillArgs fa;
    fa.s[0] = {cls, NP * C, -1.0f};
    fa.s[1] = {obj, NP, 0.0f};
    fa.s[2] = {ctr, NP * 2, 0.0f};
    fa.s[3] = {scl, NP * 2, 0.0f};
    fa.s[4] = {wgt, NP * 2, 0.0f};
    const int64_t most = NP * (C > 2 ? C : 2);
    int64_t blocks = vd_cdiv(vd_cdiv(most, 4), kThreads);
    blocks = blocks < 1 ? 1 : blocks > kFillBlocks ? kFillBlocks : blocks;
    hipLaunchKernelGGL(k_targets_fill, dim3((unsigned)blocks, 5), dim3(kThreads), 0, (hipStream_t)stream, fa);
    VD_CHECK_LAUNCH("vd_yolo_targets (fill)");
    hipLaunchKernelGGL(k_targets_rows, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, gt, ids, idw, mix, M, C, H, W,
                       (int)P, obj, ctr, scl, wgt, cls);
    VD_CHECK_LAUNCH("vd_yolo_targets (rows)");
    return VD_OK;
}

}  // extern "C"
