// vd_eval.hip — the per-image half of the VOC mAP metric on the device (viddet_amd/device_metric.py): what
// viddet_amd.metrics.VOCMApMetric.update decides for ONE image - for every detection its class, its score and the code
// 1 (true positive) / 0 (false positive) / -1 (ignored: it lies on a `difficult` ground truth) - and per class the number of
// ground-truth rows that count.  The sort by score over the whole validation set and the cumulative sums stay on the host.
//
// Arithmetic: viddet_amd.bbox.bbox_iou on float32 arrays, operation for operation.  lo = maximum, hi = minimum (a NaN
// propagates as NumPy's do), overlap = lo < hi on both axes, inter = ((hi.x - lo.x + 0) * (hi.y - lo.y + 0)) * overlap,
// area = (x2 - x1 + 0) * (y2 - y1 + 0), iou = inter / ((area_a + area_b) - inter).  Every operation rounds once to fp32: no
// product and sum of this file is contracted into an FMA (the pragma below), and `/` is the correctly rounded division (hipcc's
// default for HIP: the v_div_scale / v_div_fmas / v_div_fixup sequence, not v_rcp).  The outcome is then an integer code, and
// it is the host's bit for bit.
//
// Work shape: one workgroup per image, three phases separated by barriers.
//   1. the M label rows -> LDS (box, class or -1 for a padded row, difficult flag); npos / ndiff gain one per row that counts.
//   2. a thread per detection (N / 256 rounds): the ground truth of its class with the highest IoU in ROW order - numpy.argmax:
//      the first maximum wins, the first NaN beats everything - dropped only where `max < iou_thresh` is true.  best[d] -> LDS.
//   3. the `taken` loop of the host without a loop: the host visits the detections of a class by score descending, ties by row
//      (a stable argsort of -score), and marks a ground truth taken at its first claimant.  So a detection is a true positive
//      iff NO detection with the same best row precedes it in that order - a scan of best[] that every thread does on its own.
// The only atomics are the integer adds into npos / ndiff: every output is the same on every run.
#include "vd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxN = 1024, kMaxM = 512;

// numpy.maximum / numpy.minimum on floats: a NaN on either side gives NaN
__device__ inline float np_max(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ inline float np_min(float a, float b) { return (a <= b || a != a) ? a : b; }
// numpy.clip(x, 0, hi): NaN stays, otherwise min(max(x, 0), hi) by plain comparisons
__device__ inline float np_clip(float x, float hi) {
    if (x != x) return x;
    const float t = x > 0.f ? x : 0.f;
    return t < hi ? t : hi;
}
// ndarray.astype(int) of a non-negative integral float; values an int cannot hold saturate (they index nothing here)
__device__ inline int to_class(float id) { return id >= 2147483648.f ? 0x7fffffff : (int)id; }
// numpy's sort order of floats: NaN behind everything
__device__ inline bool np_less(float a, float b) { return a < b || (b != b && a == a); }

__global__ __launch_bounds__(kThreads) void k_voc_match(const float* __restrict__ det_ids, const float* __restrict__ det_scores,
                                                        const float* __restrict__ det_boxes, int N,
                                                        const float* __restrict__ gt, int M, int gt_w, float clip_hi,
                                                        float iou_thresh, int32_t* __restrict__ rec_cls,
                                                        float* __restrict__ rec_score, int8_t* __restrict__ rec_hit,
                                                        int32_t* __restrict__ npos, int32_t* __restrict__ ndiff, int C) {
    __shared__ float s_gb[kMaxM * 4];
    __shared__ int s_gc[kMaxM];
    __shared__ unsigned char s_gd[kMaxM];
    __shared__ int s_best[kMaxN];
    __shared__ float s_key[kMaxN];                    // -score: the key of the host's stable argsort

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    gt += b * M * gt_w;
    det_ids += b * N;
    det_scores += b * N;
    det_boxes += b * N * 4;
    rec_cls += b * N;
    rec_score += b * N;
    rec_hit += b * N;

    // 1. the label rows (a padded row may sit anywhere: the host strips them with a mask)
    for (int m = tid; m < M; m += kThreads) {
        const float* __restrict__ row = gt + (int64_t)m * gt_w;
        const float idf = row[4];
        const bool valid = idf >= 0.f;                                        // NaN: no row
        const int cls = valid ? to_class(idf) : -1;
        const bool diff = gt_w == 6 && row[5] != 0.f;                         // astype(bool): NaN is true
        s_gb[4 * m] = row[0], s_gb[4 * m + 1] = row[1], s_gb[4 * m + 2] = row[2], s_gb[4 * m + 3] = row[3];
        s_gc[m] = cls;
        s_gd[m] = diff ? 1 : 0;
        if (valid && cls < C) {                                               // cls >= 0 here: no id writes outside [0, C)
            if (!diff) atomicAdd(&npos[cls], 1);
            else if (ndiff) atomicAdd(&ndiff[cls], 1);
        }
    }
    __syncthreads();

    // 2. every detection's best ground truth
    for (int d = tid; d < N; d += kThreads) {
        const float idf = det_ids[d], sc = det_scores[d];
        rec_score[d] = sc;
        s_key[d] = -sc;
        int best = -1;
        if (!(idf >= 0.f)) {                                                  // no detection
            rec_cls[d] = -1;
            rec_hit[d] = -2;
        } else {
            const int cls = to_class(idf);
            float ax1 = det_boxes[4 * d], ay1 = det_boxes[4 * d + 1], ax2 = det_boxes[4 * d + 2], ay2 = det_boxes[4 * d + 3];
            if (clip_hi >= 0.f) ax1 = np_clip(ax1, clip_hi), ay1 = np_clip(ay1, clip_hi), ax2 = np_clip(ax2, clip_hi), ay2 = np_clip(ay2, clip_hi);
            const float area_a = (ax2 - ax1 + 0.f) * (ay2 - ay1 + 0.f);
            float best_iou = 0.f;
            for (int m = 0; m < M; ++m) {
                if (s_gc[m] != cls) continue;
                const float bx1 = s_gb[4 * m], by1 = s_gb[4 * m + 1], bx2 = s_gb[4 * m + 2], by2 = s_gb[4 * m + 3];
                const float lox = np_max(ax1, bx1), loy = np_max(ay1, by1), hix = np_min(ax2, bx2), hiy = np_min(ay2, by2);
                const float overlap = (lox < hix && loy < hiy) ? 1.f : 0.f;
                const float inter = ((hix - lox + 0.f) * (hiy - loy + 0.f)) * overlap;
                const float area_b = (bx2 - bx1 + 0.f) * (by2 - by1 + 0.f);
                const float iou = inter / ((area_a + area_b) - inter);
                // numpy.argmax: the first maximum, and the first NaN ends the search
                if (best < 0 || (best_iou == best_iou && (iou > best_iou || iou != iou))) best = m, best_iou = iou;
            }
            if (best >= 0 && best_iou < iou_thresh) best = -1;               // false for a NaN: it keeps its match
            rec_cls[d] = cls;
            if (best < 0) rec_hit[d] = 0;
        }
        s_best[d] = best;
    }
    __syncthreads();

    // 3. first claimant of a ground truth = true positive, every later one = false positive; a difficult row ignores all
    for (int d = tid; d < N; d += kThreads) {
        const int g = s_best[d];
        if (g < 0) continue;
        int hit = -1;
        if (!s_gd[g]) {
            const float kd = s_key[d];
            bool first = true;
            for (int j = 0; j < N; ++j) {
                if (s_best[j] != g || j == d) continue;
                const float kj = s_key[j];
                if (np_less(kj, kd) || (!np_less(kd, kj) && j < d)) first = false;
            }
            hit = first ? 1 : 0;
        }
        rec_hit[d] = (int8_t)hit;
    }
}

}  // namespace

extern "C" {

int vd_voc_match(const float* det_ids, const float* det_scores, const float* det_boxes, int B, int N, const float* gt, int M,
                 int gt_w, float clip_hi, float iou_thresh, int32_t* rec_cls, float* rec_score, int8_t* rec_hit, int32_t* npos,
                 int32_t* ndiff, int C, void* stream) {
    VD_REQUIRE(B >= 0 && N >= 0 && M >= 0 && C >= 1, "vd_voc_match: B, N, M must be >= 0 and C >= 1, got B=%d N=%d M=%d C=%d", B,
               N, M, C);
    VD_REQUIRE(N <= kMaxN, "vd_voc_match: N=%d detections per image, at most %d are taken", N, kMaxN);
    VD_REQUIRE(M <= kMaxM, "vd_voc_match: M=%d label rows per image, at most %d are taken", M, kMaxM);
    VD_REQUIRE(gt_w == 5 || gt_w == 6, "vd_voc_match: gt_w must be 5 (x1,y1,x2,y2,id) or 6 (+ difficult), got %d", gt_w);
    VD_REQUIRE(npos, "vd_voc_match: npos must not be NULL");
    VD_REQUIRE(!(clip_hi != clip_hi) && !(iou_thresh != iou_thresh), "vd_voc_match: clip_hi and iou_thresh must not be NaN");
    if (B == 0) return VD_OK;
    VD_REQUIRE(N == 0 || (det_ids && det_scores && det_boxes && rec_cls && rec_score && rec_hit),
               "vd_voc_match: det_ids, det_scores, det_boxes and the three record arrays must not be NULL when N > 0");
    VD_REQUIRE(M == 0 || gt, "vd_voc_match: gt must not be NULL when M > 0");
    VD_REQUIRE((((uintptr_t)det_ids | (uintptr_t)det_scores | (uintptr_t)det_boxes | (uintptr_t)gt | (uintptr_t)rec_cls |
                 (uintptr_t)rec_score | (uintptr_t)npos | (uintptr_t)ndiff) % 4) == 0,
               "vd_voc_match: every pointer but rec_hit must be 4-byte aligned");
    hipLaunchKernelGGL(k_voc_match, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, det_ids, det_scores, det_boxes, N,
                       gt, M, gt_w, clip_hi, iou_thresh, rec_cls, rec_score, rec_hit, npos, ndiff, C);
    VD_CHECK_LAUNCH("vd_voc_match");
    return VD_OK;
}

}  // extern "C"
