// vd_coco_eval.hip — the per-image half of the COCO detection metric on the device (viddet_amd/device_coco_metric.py,
// DESIGN.md 26): what viddet_amd.coco_metric.match_image decides for ONE image - COCOeval's computeIoU and evaluateImg for
// every category, the 4 area ranges and the 10 IoU thresholds.  Per detection row it writes its rank in its category's list
// and, per area range, 10 matched bits (`dtm != 0`) and 10 ignore bits; per category and area range it counts the ground
// truths the range does not ignore.  The set-wide sort by score, the cumulative sums, precision and recall stay on the host.
// Every output is an integer.
//
// Arithmetic: float64, operation for operation what the host does (no product and sum is contracted into an FMA, `/` is the
// correctly rounded division):
//   iou   = 0 where w <= 0 or h <= 0, w = min(dx+dw, gx+gw) - max(dx, gx), h likewise; else i / u with i = w*h and
//           u = dw*dh for a crowd ground truth, (dw*dh + gw*gh) - i otherwise
//   a ground truth is ignored by area range r where it is a crowd or area < lo_r or area > hi_r (`area` is the row's own column)
//   per threshold t and detection in rank order: iou = min(t, 1 - 1e-10), m = -1; over the ground truths, not-ignored ones
//           first: skip one matched at t that is no crowd; stop at the first ignored one once m is a not-ignored one; skip where
//           ious[d][g] < iou; else iou = ious[d][g], m = g (on equal IoUs the LATER one wins)
//   a match records `annotation id != 0` as the matched bit and the ground truth's ignore flag as the ignore bit; afterwards
//           ignore |= (not matched bit) & (dw*dh < lo_r or dw*dh > hi_r)
// The reference stable-sorts the ground truths not-ignored first and walks them once.  Here they stay in place and one walk
// keeps two running pairs, (iou_n, m_n) over the not-ignored and (iou_i, m_i) over the ignored ones, each from the threshold
// with the comparison above; m = m_n where there is one, else m_i.  That is the sorted walk: it visits the not-ignored ones in
// row order, breaks before the ignored ones when m_n exists, and otherwise goes on through them with iou still the threshold.
//
// Work shape: one 256-thread workgroup per image.
//   1. label rows -> LDS (box, category, flags), `npig` by integer atomics; detection categories and sort keys -> LDS.
//   2. a thread per detection: its rank among the detections of its category in the stable order of -score.
//   3. wavefront w takes the categories c with (c & 3) == w - categories touch disjoint rows, so there is no barrier between
//      them: it lists the category's first 100 detections by rank and its ground truths in row order, stages the IoU tile in
//      LDS when it fits (else the chains recompute the IoUs - the same operations, the same bits), then lane a*10 + t runs the
//      chain of area range a and threshold t over the tile; its matched flags are a bitmask column in LDS.  Two ballots per
//      detection gather the 40 chains' bits into the four output words.
// The only atomics are integer adds: every output is the same on every run.
#include "vd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxN = 1024, kMaxM = 512;
constexpr int kT = 10, kA = 4, kChains = kT * kA;
constexpr int kTop = 100;                             // maxDets[-1]
constexpr int kTile = 768;                            // IoUs of one category staged per wavefront
constexpr int kWords = kMaxM / 32;

// intra-wave LDS hand-off: LDS ops of one wave execute in order, only the compiler must not reorder the accesses
#define WAVE_SYNC()                                              \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   \
        __builtin_amdgcn_wave_barrier();                         \
    } while (0)

// numpy's sort order of floats: NaN behind everything
__device__ inline bool np_less(double a, double b) { return a < b || (b != b && a == a); }

__device__ inline double box_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh, bool crowd) {
    const double dr = dx + dw, gr = gx + gw, db = dy + dh, gb = gy + gh;
    const double w = (gr < dr ? gr : dr) - (gx > dx ? gx : dx);
    const double h = (gb < db ? gb : db) - (gy > dy ? gy : dy);
    if (w <= 0.0 || h <= 0.0) return 0.0;
    const double i = w * h;
    const double u = crowd ? dw * dh : (dw * dh + gw * gh) - i;
    return i / u;
}

__global__ __launch_bounds__(kThreads) void k_coco_match(const double* __restrict__ det, int N, const double* __restrict__ gt, int M,
                                                         const double* __restrict__ iou_thrs, const double* __restrict__ area_rng,
                                                         int32_t* __restrict__ rec_rank, int32_t* __restrict__ rec_bits,
                                                         int32_t* __restrict__ npig, int K) {
    __shared__ double s_gb[kMaxM * 4];                        // ground-truth boxes x, y, w, h
    __shared__ double s_tile[kWaves * kTile];                 // phase 2: the first N hold the keys -score; phase 3: a tile per wave
    __shared__ short s_dc[kMaxN];                             // category, -1: a row that takes no part
    __shared__ short s_rank[kMaxN];
    __shared__ short s_gc[kMaxM];
    __shared__ unsigned char s_gf[kMaxM];                     // bit r: ignored by area range r; bit 4: crowd; bit 5: annotation id != 0
    __shared__ unsigned short s_dlist[kWaves][kTop];          // rank -> detection row
    __shared__ unsigned short s_glist[kWaves][kMaxM];         // the category's label rows, in row order
    __shared__ unsigned s_gtm[kWaves][kWords][kChains];       // bit g & 31 of word g >> 5: ground truth g is matched in this chain

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    det += b * N * 6;
    gt += b * M * 8;
    rec_rank += b * N;
    rec_bits += b * N * kA;

    double lo[kA], hi[kA];
#pragma unroll
    for (int r = 0; r < kA; ++r) lo[r] = area_rng[2 * r], hi[r] = area_rng[2 * r + 1];

    // 1. the label rows (a padded row may sit anywhere), the detections' categories and keys
    for (int m = tid; m < M; m += kThreads) {
        const double* __restrict__ row = gt + (int64_t)m * 8;
        const double area = row[4], catf = row[5];
        const bool valid = catf >= 0.0 && catf < (double)K;                   // NaN: no row
        const int cls = valid ? (int)catf : -1;
        const bool crowd = row[7] != 0.0;
        unsigned f = (crowd ? 16u : 0u) | (row[6] != 0.0 ? 32u : 0u);
#pragma unroll
        for (int r = 0; r < kA; ++r)
            if (crowd || area < lo[r] || area > hi[r]) f |= 1u << r;
        s_gb[4 * m] = row[0], s_gb[4 * m + 1] = row[1], s_gb[4 * m + 2] = row[2], s_gb[4 * m + 3] = row[3];
        s_gc[m] = (short)cls;
        s_gf[m] = (unsigned char)f;
        if (valid) {
#pragma unroll
            for (int r = 0; r < kA; ++r)
                if (!(f & (1u << r))) atomicAdd(&npig[(int64_t)cls * kA + r], 1);      // 0 <= cls < K
        }
    }
    for (int d = tid; d < N; d += kThreads) {
        const double catf = det[(int64_t)d * 6 + 5];
        s_dc[d] = (catf >= 0.0 && catf < (double)K) ? (short)(int)catf : (short)-1;
        s_tile[d] = -det[(int64_t)d * 6 + 4];
    }
    __syncthreads();

    // 2. the rank inside the category: how many of its detections numpy's stable argsort of -score puts in front
    for (int d = tid; d < N; d += kThreads) {
        const int c = s_dc[d];
        int rank = -1;
        if (c >= 0) {
            const double kd = s_tile[d];
            rank = 0;
            for (int j = 0; j < N; ++j) {
                if (s_dc[j] != c || j == d) continue;
                const double kj = s_tile[j];
                if (np_less(kj, kd) || (!np_less(kd, kj) && j < d)) ++rank;
            }
            if (rank >= kTop) rank = -1;
        }
        s_rank[d] = (short)rank;
        rec_rank[d] = rank;
        if (rank < 0) {                                                       // the others are written by their chains below
#pragma unroll
            for (int r = 0; r < kA; ++r) rec_bits[(int64_t)d * kA + r] = 0;
        }
    }
    __syncthreads();                                                          // the keys are read: the tiles may take their place

    // 3. a wavefront per category group
    const int wave = tid / kWave, lane = tid % kWave;
    const bool chain = lane < kChains;
    const int a = chain ? lane / kT : 0, t = chain ? lane % kT : 0;
    const double t_raw = iou_thrs[t];
    const double thr = t_raw < 1 - 1e-10 ? t_raw : 1 - 1e-10;                 // min([t, 1 - 1e-10])
    const double a_lo = area_rng[2 * a], a_hi = area_rng[2 * a + 1];
    double* __restrict__ tile = s_tile + wave * kTile;
    for (int c = wave; c < K; c += kWaves) {
        int nD = 0, nG = 0;
        for (int base = 0; base < N; base += kWave) {
            const int d = base + lane;
            const bool mine = d < N && s_dc[d] == c && s_rank[d] >= 0;
            if (mine) s_dlist[wave][s_rank[d]] = (unsigned short)d;           // ranks below kTop: a permutation of [0, nD)
            nD += __popcll(__ballot(mine));
        }
        if (nD == 0) continue;                                                // uniform over the wavefront
        for (int base = 0; base < M; base += kWave) {
            const int g = base + lane;
            const bool mine = g < M && s_gc[g] == c;
            const unsigned long long mask = __ballot(mine);
            if (mine) s_glist[wave][nG + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)g;
            nG += __popcll(mask);
        }
        WAVE_SYNC();
        const bool staged = nD * nG <= kTile;
        if (staged) {
            for (int idx = lane; idx < nD * nG; idx += kWave) {
                const int di = idx / nG, gi = idx - di * nG;
                const double* __restrict__ dr = det + (int64_t)s_dlist[wave][di] * 6;
                const int g = s_glist[wave][gi];
                tile[idx] = box_iou(dr[0], dr[1], dr[2], dr[3], s_gb[4 * g], s_gb[4 * g + 1], s_gb[4 * g + 2], s_gb[4 * g + 3],
                                    (s_gf[g] & 16u) != 0);
            }
        }
        if (chain)
            for (int w = 0; w < (nG + 31) / 32; ++w) s_gtm[wave][w][lane] = 0u;
        WAVE_SYNC();
        for (int di = 0; di < nD; ++di) {
            const int d = s_dlist[wave][di];
            const double* __restrict__ dr = det + (int64_t)d * 6;
            const double dx = dr[0], dy = dr[1], dw = dr[2], dh = dr[3];
            bool matched = false, ignore = false;
            if (chain) {
                double iou_n = thr, iou_i = thr;
                int m_n = -1, m_i = -1;
                unsigned word = 0;
                for (int gi = 0; gi < nG; ++gi) {
                    if ((gi & 31) == 0) word = s_gtm[wave][gi >> 5][lane];
                    const int g = s_glist[wave][gi];
                    const unsigned f = s_gf[g];
                    if (((word >> (gi & 31)) & 1u) && !(f & 16u)) continue;   // matched at this threshold, and no crowd
                    const double v = staged ? tile[di * nG + gi]
                                            : box_iou(dx, dy, dw, dh, s_gb[4 * g], s_gb[4 * g + 1], s_gb[4 * g + 2], s_gb[4 * g + 3],
                                                      (f & 16u) != 0);
                    if ((f >> a) & 1u) {
                        if (v < iou_i) continue;
                        iou_i = v, m_i = gi;
                    } else {
                        if (v < iou_n) continue;
                        iou_n = v, m_n = gi;
                    }
                }
                const int m = m_n >= 0 ? m_n : m_i;
                if (m >= 0) {
                    matched = (s_gf[s_glist[wave][m]] & 32u) != 0;            // dtm holds the annotation's id: 0 reads as unmatched
                    ignore = m_n < 0;
                    s_gtm[wave][m >> 5][lane] |= 1u << (m & 31);
                }
                const double darea = dw * dh;
                if (!matched && (darea < a_lo || darea > a_hi)) ignore = true;
            }
            const unsigned long long bm = __ballot(matched), bi = __ballot(ignore);
            if (chain && t == 0)
                rec_bits[(int64_t)d * kA + a] = (int32_t)(((bm >> (a * kT)) & 0x3ffull) | (((bi >> (a * kT)) & 0x3ffull) << kT));
        }
        WAVE_SYNC();                                                          // the lists and the tile are rewritten by the next category
    }
}

}  // namespace

extern "C" {

int vd_coco_match(const double* det, int B, int N, const double* gt, int M, const double* iou_thrs, const double* area_rng,
                  int32_t* rec_rank, int32_t* rec_bits, int32_t* npig, int K, void* stream) {
    VD_REQUIRE(B >= 0 && N >= 0 && M >= 0, "vd_coco_match: B, N, M must be >= 0, got B=%d N=%d M=%d", B, N, M);
    VD_REQUIRE(K >= 1 && K <= 32767, "vd_coco_match: K must be in [1, 32767] (the categories, the rows of npig), got K=%d", K);
    VD_REQUIRE(N <= kMaxN, "vd_coco_match: N=%d detection rows per image (det), at most %d are taken", N, kMaxN);
    VD_REQUIRE(M <= kMaxM, "vd_coco_match: M=%d label rows per image (gt), at most %d are taken", M, kMaxM);
    VD_REQUIRE(iou_thrs && area_rng, "vd_coco_match: iou_thrs and area_rng must not be NULL");
    VD_REQUIRE(npig, "vd_coco_match: npig must not be NULL");
    if (B == 0) return VD_OK;
    VD_REQUIRE(N == 0 || (det && rec_rank && rec_bits), "vd_coco_match: det, rec_rank and rec_bits must not be NULL when N > 0");
    VD_REQUIRE(M == 0 || gt, "vd_coco_match: gt must not be NULL when M > 0");
    VD_REQUIRE((((uintptr_t)det | (uintptr_t)gt | (uintptr_t)iou_thrs | (uintptr_t)area_rng) % 8) == 0,
               "vd_coco_match: det, gt, iou_thrs and area_rng must be 8-byte aligned");
    VD_REQUIRE((((uintptr_t)rec_rank | (uintptr_t)rec_bits | (uintptr_t)npig) % 4) == 0,
               "vd_coco_match: the three output pointers must be 4-byte aligned");
    hipLaunchKernelGGL(k_coco_match, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, det, N, gt, M, iou_thrs, area_rng,
                       rec_rank, rec_bits, npig, K);
    VD_CHECK_LAUNCH("vd_coco_match");
    return VD_OK;
}

}  // extern "C"
