// vd_track_math.h — the row arithmetic that the tracker kernels share, each rule stated once: vd_track.hip (k_track),
// vd_track_live.hip (k_track_push) and, for the IoU, vd_mot_eval.hip.  The tie rule of choice_before and the rounding order of
// iou are what make the online tracker equal the offline one (viddet_amd/track.py is the definition).
//
// Arithmetic: fp32, no product and sum contracted into an FMA (every includer sets the pragma below ahead of the include; it is
// repeated here so that the header is right on its own), `/` the correctly rounded division.
#pragma once
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_clip_rows.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxN = 128;
constexpr int kMaxAge = 7;
constexpr int kMaxActive = kMaxN * (kMaxAge + 1);
constexpr int kFewHolders = 8;                        // up to this many lanes with a choice are read one by one

// np.minimum / np.maximum of a pair: a NaN on either side gives NaN
__device__ inline float np_max(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ inline float np_min(float a, float b) { return (a <= b || a != a) ? a : b; }

__device__ inline float iou(const float4 a, const float4 b) {
    const float iw = np_min(a.z, b.z) - np_max(a.x, b.x);
    const float ih = np_min(a.w, b.w) - np_max(a.y, b.y);
    const float inter = iw * ih;
    const float aa = (a.z - a.x) * (a.w - a.y), ab = (b.z - b.x) * (b.w - b.y);
    const float q = inter / ((aa + ab) - inter);      // straight-line: the two rows of a lane divide side by side
    return (iw > 0.f && ih > 0.f) ? q : 0.f;
}

// the class of a row for a tracker, -1 where it is no candidate: vd_clip_rows.h's rule, and a score >= sigma_l
__device__ inline int row_class(float id, float score, int num_class, float sigma_l) {
    if (!(id >= 0.f) || not_finite(score) || !(score >= sigma_l)) return -1;
    const int c = class_of(id);
    return c < num_class ? c : -1;
}

// (iou, row) of a choice; row < 0: none.  np.argmax's order: a NaN before every number, the larger value, then the lower row
__device__ inline bool choice_before(float v, int r, float bv, int br) {
    if (r < 0) return false;
    if (br < 0) return true;
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    return v > bv || ((vn || v == bv) && r < br);
}

// The choice of a track (last box tb, class tc) among the rows of the frame that are candidates of its class and whose bit in
// the taken masks is clear: every lane scores its two rows, then the lanes that hold a choice are reduced - a few (a class has
// few rows in a frame) are read in turn, lane by lane, many go through a butterfly; choice_before's order is total, so either
// way every lane of the wavefront ends with the same (bv, br).  br < 0: no such row.
__device__ inline void choose(const float4 tb, int tc, const int (&cls)[2], const float4 (&box)[2], unsigned long long tk_lo,
                              unsigned long long tk_hi, int lane, float& bv, int& br) {
    bv = 0.f, br = -1;
    const bool on[2] = {cls[0] == tc && !((tk_lo >> lane) & 1ull), cls[1] == tc && !((tk_hi >> lane) & 1ull)};
    if (on[0] || on[1]) {
        const float v[2] = {iou(tb, box[0]), iou(tb, box[1])};
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (on[h] && choice_before(v[h], lane + h * kWave, bv, br)) bv = v[h], br = lane + h * kWave;
    }
    unsigned long long holders = __ballot(br >= 0);
    if (__popcll(holders) <= kFewHolders) {
        float cv = 0.f;
        int cr = -1;
        while (holders) {
            const int l = __ffsll((long long)holders) - 1;
            holders &= holders - 1;
            const float ov = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bv), l));
            const int orow = __builtin_amdgcn_readlane(br, l);
            if (choice_before(ov, orow, cv, cr)) cv = ov, cr = orow;
        }
        bv = cv, br = cr;
    } else {
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, kWave);
            const int orow = __shfl_xor(br, off, kWave);
            if (choice_before(ov, orow, bv, br)) bv = ov, br = orow;
        }
    }
}

}  // namespace
