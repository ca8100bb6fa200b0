// vd_track_smooth_math.h — the backward step of the Rauch-Tung-Striebel smoother of vd_track_kf.h's filter and the test of a
// finite box beside it, stated once for the kernels that smooth boxes along tracks: vd_track_smooth.hip (k_smo_seg, a finished
// clip) and vd_track_smooth_live.hip (k_smo_push, a stream in fixed-lag form).  viddet_amd/smooth.py is the definition (rts_step;
// DESIGN.md 37).
//
// Arithmetic: fp32, every operation one operation in smooth.py's order, no product and sum contracted into an FMA (every includer
// sets the pragma below ahead of the include; it is repeated here so that the header is right on its own), `/` the correctly
// rounded one.
#pragma once
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_kf.h"

namespace {

// the smoothed mean: x, xd of the three pairs and the aspect
struct Sm {
    float x[3], xd[3], r;
};

// smooth.py's rts_step: S at the later frame, f the filtered state and p = kf_predict(f) -> S at f's frame
__device__ inline void smo_back(Sm& S, const Kf& f, const Kf& p) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float A = f.p00[i] + f.p01[i], B = f.p01[i], C = f.p01[i] + f.p11[i], D = f.p11[i];
        const float det = p.p00[i] * p.p11[i] - p.p01[i] * p.p01[i];
        const float c00 = (A * p.p11[i] - B * p.p01[i]) / det;
        const float c01 = (B * p.p00[i] - A * p.p01[i]) / det;
        const float c10 = (C * p.p11[i] - D * p.p01[i]) / det;
        const float c11 = (D * p.p00[i] - C * p.p01[i]) / det;
        const float dx = S.x[i] - p.x[i], dxd = S.xd[i] - p.xd[i];
        S.x[i] = f.x[i] + (c00 * dx + c01 * dxd);
        S.xd[i] = f.xd[i] + (c10 * dx + c11 * dxd);
    }
    S.r = f.r + (f.p / p.p) * (S.r - p.r);
}

__device__ inline bool finite4(const float4 b) {
    return !not_finite(b.x) && !not_finite(b.y) && !not_finite(b.z) && !not_finite(b.w);
}

}  // namespace
