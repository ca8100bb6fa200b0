// vd_vid_eval.hip — the per-image half of the ImageNet VID motion metric on the device (viddet_amd/device_vid_metric.py,
// DESIGN.md 25): what viddet_amd.vid_metric.match_image decides for ONE image - for every detection the ground truth the
// greedy match gives it, and for each of the 16 cells (4 motion ranges x 4 area ranges) whether it is a true positive and
// which of the four false-positive rules applies - and the ground-truth counts per class and cell.  The set-wide sort by
// score, the cumulative sums and AP stay on the host.  Every output is an integer: the float64 false-positive weights
// (`empty_weight`, the image's ignored fraction) are formed on the host from these integers, as the reference writes them.
//
// Arithmetic: float64, operation for operation what metrics/imgnetvid.py does (no product and sum is contracted into an FMA,
// `/` is the correctly rounded division, comparisons are the plain <, >, >= so that a NaN decides as it does in NumPy):
//   thr   = (w*h) / ((w + tol) * (h + tol)), w = x2 - x1 + 1, h = y2 - y1 + 1; thr = iou_thresh where thr > iou_thresh
//   ov    = iw*ih / (((bb.x2-bb.x1+1) * (bb.y2-bb.y1+1) + (gt.x2-gt.x1+1) * (gt.y2-gt.y1+1)) - iw*ih) where iw > 0 and ih > 0,
//           else 0; iw = min(bb.x2, gt.x2) - max(bb.x1, gt.x1) + 1, ih likewise (min / max propagate a NaN)
//   area  = (y2 - y1 + 1) * (x2 - x1 + 1), of a ground truth and of a detection
//   ignored by motion range r: miou < lo_r | miou > hi_r (a NaN is inside every range); by area range r: area < lo_r | area > hi_r
//   match: in score order, the not yet detected ground truth of the detection's class with ov >= thr and the largest ov
//          (from -1, strict >: the lowest row wins a tie; a ground truth with thr = 0 can be matched at ov = 0)
//   unmatched, per cell: 0 where the detection's area is outside the area range; else with ovmax_ig / ovmax_nig = the largest
//          ov (from -1) over ALL ground truths ignored / not ignored by the motion range: 1 where nig > ig, 0 where ig > nig,
//          else `empty_weight` where the image has no ground truth, else the image's ignored fraction
//
// Work shape: one 256-thread workgroup per image.
//   1. the M label rows -> LDS (box, threshold, class or -1 for a padded row, 4 motion-ignore and 4 area-ignore bits);
//      the counts (per image through LDS, per class by integer atomics).
//   2. the scores' keys -> LDS, then a thread per detection: its rank in the stable order of -score (numpy's order: NaN last,
//      ties by row); then, the keys' LDS reused for the boxes, its ovmax_ig / ovmax_nig per motion range and its area gates
//      -> the false-positive code of every cell should it stay unmatched.  None of this depends on the greedy state.
//   3. the greedy.  Matches of different classes touch disjoint ground-truth rows, so wavefront w walks the ranked list and
//      handles the detections with (class & 3) == w, with no barrier between steps: 64 ranks are fetched at once, a ballot picks
//      the wavefront's own, and per detection the lanes stride over the label rows (lane l owns rows l, l + 64, ...: the
//      `detected` flags of its rows are bits of one of its registers, and only the wavefront of that class ever touches them),
//      recompute ov for the rows of the class that are still free and reach thr, and a shuffle reduction takes the largest ov,
//      the lowest row on ties.
//   4. every thread packs its detection's 16 cells.
// The only atomics are integer adds: every output is the same on every run.
#include "vd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMaxN = 1024, kMaxM = 512;

// np.max / np.min of a pair: a NaN on either side gives NaN
__device__ inline double np_max(double a, double b) { return (a >= b || a != a) ? a : b; }
__device__ inline double np_min(double a, double b) { return (a <= b || a != a) ? a : b; }
// ndarray.astype(int) of a non-negative float; values an int cannot hold saturate (they index nothing here)
__device__ inline int to_class(double id) { return id >= 2147483648.0 ? 0x7fffffff : (int)id; }
// numpy's sort order of floats: NaN behind everything
__device__ inline bool np_less(double a, double b) { return a < b || (b != b && a == a); }

// vid_eval_motion :170-179
__device__ inline double overlap(double ax1, double ay1, double ax2, double ay2, double bx1, double by1, double bx2, double by2) {
    const double iw = np_min(ax2, bx2) - np_max(ax1, bx1) + 1.0;
    const double ih = np_min(ay2, by2) - np_max(ay1, by1) + 1.0;
    if (!(iw > 0.0 && ih > 0.0)) return 0.0;
    const double inter = iw * ih;
    const double ua = ((ax2 - ax1 + 1.0) * (ay2 - ay1 + 1.0) + (bx2 - bx1 + 1.0) * (by2 - by1 + 1.0)) - inter;
    return inter / ua;
}

__global__ __launch_bounds__(kThreads) void k_vid_match(const double* __restrict__ det, int N, const double* __restrict__ gt, int M,
                                                        const double* __restrict__ motion_ranges,
                                                        const double* __restrict__ area_ranges, double iou_thresh,
                                                        double pixel_tolerance, int32_t* __restrict__ rec_gt,
                                                        int32_t* __restrict__ rec_tp, int32_t* __restrict__ rec_fp,
                                                        int32_t* __restrict__ img_nig, int32_t* __restrict__ img_ngt,
                                                        int32_t* __restrict__ npos, int32_t* __restrict__ nout, int C) {
    __shared__ double s_gb[kMaxM * 4];                // ground-truth boxes
    __shared__ double s_gthr[kMaxM];
    __shared__ double s_db[kMaxN * 4];                // phase 2a: the first N hold the keys -score; from 2b on: detection boxes
    __shared__ int s_gc[kMaxM];                       // class, -1: a padded row
    __shared__ int s_dc[kMaxN];                       // class, -1: a padded row
    __shared__ unsigned short s_order[kMaxN];         // rank -> detection row
    __shared__ short s_kmax[kMaxN];                   // detection row -> matched label row, -1
    __shared__ unsigned char s_gbits[kMaxM];          // bit r: ignored by motion range r; bit 4 + r: by area range r
    __shared__ int s_cnt[6];                          // ignored by motion range 0..3, valid label rows, valid detections

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    det += b * N * 6;
    gt += b * M * 6;
    rec_gt += b * N;
    rec_tp += b * N;
    rec_fp += b * N;

    double mlo[4], mhi[4], alo[4], ahi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        mlo[r] = motion_ranges[2 * r], mhi[r] = motion_ranges[2 * r + 1];
        alo[r] = area_ranges[2 * r], ahi[r] = area_ranges[2 * r + 1];
    }
    if (tid < 6) s_cnt[tid] = 0;
    __syncthreads();

    // 1. the label rows (a padded row may sit anywhere)
    for (int m = tid; m < M; m += kThreads) {
        const double* __restrict__ row = gt + (int64_t)m * 6;
        const double x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3], idf = row[4], miou = row[5];
        const bool valid = idf >= 0.0;                                        // NaN: no row
        const int cls = valid ? to_class(idf) : -1;
        const double w = x2 - x1 + 1.0, h = y2 - y1 + 1.0;
        double thr = (w * h) / ((w + pixel_tolerance) * (h + pixel_tolerance));
        if (thr > iou_thresh) thr = iou_thresh;
        const double area = (y2 - y1 + 1.0) * (x2 - x1 + 1.0);
        unsigned bits = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if ((miou < mlo[r]) | (miou > mhi[r])) bits |= 1u << r;
            if ((area < alo[r]) | (area > ahi[r])) bits |= 16u << r;
        }
        s_gb[4 * m] = x1, s_gb[4 * m + 1] = y1, s_gb[4 * m + 2] = x2, s_gb[4 * m + 3] = y2;
        s_gthr[m] = thr;
        s_gc[m] = cls;
        s_gbits[m] = (unsigned char)bits;
        if (valid) {
            atomicAdd(&s_cnt[4], 1);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (bits & (1u << r)) atomicAdd(&s_cnt[r], 1);
            if (cls < C) {                                                    // cls >= 0 here: no id writes outside [0, C)
                atomicAdd(&npos[cls], 1);
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if ((bits & (1u << (c >> 2))) | (bits & (16u << (c & 3)))) atomicAdd(&nout[(int64_t)c * C + cls], 1);
            }
        }
    }
    // 2a. the keys of the sort and the classes
    for (int d = tid; d < N; d += kThreads) {
        const double idf = det[(int64_t)d * 6];
        const bool valid = idf >= 0.0;
        s_dc[d] = valid ? to_class(idf) : -1;
        s_db[d] = -det[(int64_t)d * 6 + 1];
        s_kmax[d] = -1;
        if (valid) atomicAdd(&s_cnt[5], 1);
    }
    __syncthreads();
    const int ngt = s_cnt[4], nv = s_cnt[5];
    if (tid < 4) img_nig[b * 4 + tid] = s_cnt[tid];
    if (tid == 4) img_ngt[b] = ngt;

    // the rank among the valid detections: how many of them numpy's stable argsort of -score puts in front
    for (int d = tid; d < N; d += kThreads) {
        if (s_dc[d] < 0) continue;
        const double kd = s_db[d];
        int rank = 0;
        for (int j = 0; j < N; ++j) {
            if (s_dc[j] < 0 || j == d) continue;
            const double kj = s_db[j];
            if (np_less(kj, kd) || (!np_less(kd, kj) && j < d)) ++rank;
        }
        s_order[rank] = (unsigned short)d;                                    // a permutation of [0, nv): rank < nv <= N
    }
    __syncthreads();

    // 2b. the boxes take the keys' place; what an unmatched detection costs in every cell
    for (int d = tid; d < N; d += kThreads) {
        const double* __restrict__ row = det + (int64_t)d * 6;
        const double x1 = row[2], y1 = row[3], x2 = row[4], y2 = row[5];
        s_db[4 * d] = x1, s_db[4 * d + 1] = y1, s_db[4 * d + 2] = x2, s_db[4 * d + 3] = y2;
    }
    __syncthreads();
    for (int d = tid; d < N; d += kThreads) {
        if (s_dc[d] < 0) continue;
        const double x1 = s_db[4 * d], y1 = s_db[4 * d + 1], x2 = s_db[4 * d + 2], y2 = s_db[4 * d + 3];
        double ig[4] = {-1.0, -1.0, -1.0, -1.0}, nig[4] = {-1.0, -1.0, -1.0, -1.0};
        for (int m = 0; m < M; ++m) {
            if (s_gc[m] < 0) continue;
            const double ov = overlap(x1, y1, x2, y2, s_gb[4 * m], s_gb[4 * m + 1], s_gb[4 * m + 2], s_gb[4 * m + 3]);
            const unsigned bits = s_gbits[m];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (bits & (1u << r)) {
                    if (ov > ig[r]) ig[r] = ov;
                } else if (ov > nig[r]) nig[r] = ov;
            }
        }
        const double area = (y2 - y1 + 1.0) * (x2 - x1 + 1.0);
        unsigned code = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int mr = c >> 2, ar = c & 3;
            unsigned v;
            if ((area < alo[ar]) | (area > ahi[ar])) v = 0;
            else if (nig[mr] > ig[mr]) v = 1;
            else if (ig[mr] > nig[mr]) v = 0;
            else v = ngt == 0 ? 2 : 3;
            code |= v << (2 * c);
        }
        rec_fp[d] = (int32_t)code;
    }

    // 3. the greedy, a wavefront per class group (phase 2b wrote nothing this phase reads after the barrier above)
    {
        const int wave = tid / kWave, lane = tid % kWave;
        unsigned detected = 0;                                                // bit i: this lane's row lane + 64 * i
        for (int i0 = 0; i0 < nv; i0 += kWave) {
            const int i = i0 + lane;
            const int d_l = i < nv ? (int)s_order[i] : 0;
            const int c_l = i < nv ? s_dc[d_l] : -1;
            unsigned long long mine = __ballot(c_l >= 0 && (c_l & 3) == wave);
            while (mine) {
                const int src = __ffsll((long long)mine) - 1;
                mine &= mine - 1;
                const int d = __shfl(d_l, src, kWave), cls = __shfl(c_l, src, kWave);
                const double x1 = s_db[4 * d], y1 = s_db[4 * d + 1], x2 = s_db[4 * d + 2], y2 = s_db[4 * d + 3];
                double best = -1.0;
                int bk = 0x7fffffff;
                for (int m = lane, bit = 0; m < M; m += kWave, ++bit) {
                    if (s_gc[m] != cls || (detected >> bit) & 1u) continue;
                    const double ov = overlap(x1, y1, x2, y2, s_gb[4 * m], s_gb[4 * m + 1], s_gb[4 * m + 2], s_gb[4 * m + 3]);
                    if (ov >= s_gthr[m] && ov > best) best = ov, bk = m;
                }
#pragma unroll
                for (int off = kWave / 2; off > 0; off >>= 1) {
                    const double ob = __shfl_xor(best, off, kWave);
                    const int ok = __shfl_xor(bk, off, kWave);
                    if (ob > best || (ob == best && ok < bk)) best = ob, bk = ok;
                }
                if (bk != 0x7fffffff) {                                       // every lane holds the same (best, bk)
                    if ((bk % kWave) == lane) {
                        detected |= 1u << (bk / kWave);
                        s_kmax[d] = (short)bk;
                    }
                }
            }
        }
    }
    __syncthreads();

    // 4. the 16 cells of every detection
    for (int d = tid; d < N; d += kThreads) {
        if (s_dc[d] < 0) {
            rec_gt[d] = -2, rec_tp[d] = 0, rec_fp[d] = 0;
            continue;
        }
        const int k = s_kmax[d];
        rec_gt[d] = k;
        unsigned tp = 0;
        if (k >= 0) {
            const unsigned bits = s_gbits[k];
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (!(bits & (1u << (c >> 2))) && !(bits & (16u << (c & 3)))) tp |= 1u << c;
            rec_fp[d] = 0;
        }
        rec_tp[d] = (int32_t)tp;
    }
}

}  // namespace

extern "C" {

int vd_vid_match(const double* det, int B, int N, const double* gt, int M, const double* motion_ranges, const double* area_ranges,
                 double iou_thresh, double pixel_tolerance, int32_t* rec_gt, int32_t* rec_tp, int32_t* rec_fp, int32_t* img_nig,
                 int32_t* img_ngt, int32_t* npos, int32_t* nout, int C, void* stream) {
    VD_REQUIRE(B >= 0 && N >= 0 && M >= 0, "vd_vid_match: B, N, M must be >= 0, got B=%d N=%d M=%d", B, N, M);
    VD_REQUIRE(C >= 1, "vd_vid_match: C must be >= 1 (the length of npos), got C=%d", C);
    VD_REQUIRE(N <= kMaxN, "vd_vid_match: N=%d detection rows per image (det), at most %d are taken", N, kMaxN);
    VD_REQUIRE(M <= kMaxM, "vd_vid_match: M=%d label rows per image (gt), at most %d are taken", M, kMaxM);
    VD_REQUIRE(motion_ranges && area_ranges, "vd_vid_match: motion_ranges and area_ranges must not be NULL");
    VD_REQUIRE(npos && nout, "vd_vid_match: npos and nout must not be NULL");
    VD_REQUIRE(!(iou_thresh != iou_thresh) && !(pixel_tolerance != pixel_tolerance),
               "vd_vid_match: iou_thresh and pixel_tolerance must not be NaN");
    if (B == 0) return VD_OK;
    VD_REQUIRE(img_nig && img_ngt, "vd_vid_match: img_nig and img_ngt must not be NULL");
    VD_REQUIRE(N == 0 || (det && rec_gt && rec_tp && rec_fp), "vd_vid_match: det, rec_gt, rec_tp and rec_fp must not be NULL when N > 0");
    VD_REQUIRE(M == 0 || gt, "vd_vid_match: gt must not be NULL when M > 0");
    VD_REQUIRE((((uintptr_t)det | (uintptr_t)gt | (uintptr_t)motion_ranges | (uintptr_t)area_ranges) % 8) == 0,
               "vd_vid_match: det, gt, motion_ranges and area_ranges must be 8-byte aligned");
    VD_REQUIRE((((uintptr_t)rec_gt | (uintptr_t)rec_tp | (uintptr_t)rec_fp | (uintptr_t)img_nig | (uintptr_t)img_ngt |
                 (uintptr_t)npos | (uintptr_t)nout) % 4) == 0,
               "vd_vid_match: the seven output pointers must be 4-byte aligned");
    hipLaunchKernelGGL(k_vid_match, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, det, N, gt, M, motion_ranges,
                       area_ranges, iou_thresh, pixel_tolerance, rec_gt, rec_tp, rec_fp, img_nig, img_ngt, npos, nout, C);
    VD_CHECK_LAUNCH("vd_vid_match");
    return VD_OK;
}

}  // extern "C"
