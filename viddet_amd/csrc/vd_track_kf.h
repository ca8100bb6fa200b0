// vd_track_kf.h — the Kalman filter of a track, stated once for the kernels that predict tracks: vd_track_sort.hip
// (k_track_sort) and vd_track_byte.hip (k_track_byte).  viddet_amd/sort.py is the definition (measure, kf_start, kf_predict,
// kf_box, kf_update): the decoupled form of Bewley's 7-state filter, (x, xd, p00, p01, p11) for u, v, s and
// (r, p) for the aspect, 17 floats a track, kept field-major in tables of kMaxActive tracks.
//
// Arithmetic: fp32, every operation one operation in sort.py's order, no product and sum contracted into an FMA (every includer
// sets the pragma below ahead of the include; it is repeated here so that the header is right on its own), `/` and sqrtf the
// correctly rounded ones.
#pragma once
#include "vd_common.h"

#pragma clang fp contract(off)

#include "vd_track_math.h"

namespace {

constexpr int kStateFloats = 17;

// the decoupled filter of a track: (x, xd, p00, p01, p11) for u, v, s and (r, p) for the aspect
struct Kf {
    float x[3], xd[3], p00[3], p01[3], p11[3], r, p;
};

__device__ inline void kf_load(const float* st, int k, Kf& s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s.x[i] = st[(0 + i) * kMaxActive + k];
        s.xd[i] = st[(3 + i) * kMaxActive + k];
        s.p00[i] = st[(6 + i) * kMaxActive + k];
        s.p01[i] = st[(9 + i) * kMaxActive + k];
        s.p11[i] = st[(12 + i) * kMaxActive + k];
    }
    s.r = st[15 * kMaxActive + k];
    s.p = st[16 * kMaxActive + k];
}

__device__ inline void kf_store(float* st, int k, const Kf& s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        st[(0 + i) * kMaxActive + k] = s.x[i];
        st[(3 + i) * kMaxActive + k] = s.xd[i];
        st[(6 + i) * kMaxActive + k] = s.p00[i];
        st[(9 + i) * kMaxActive + k] = s.p01[i];
        st[(12 + i) * kMaxActive + k] = s.p11[i];
    }
    st[15 * kMaxActive + k] = s.r;
    st[16 * kMaxActive + k] = s.p;
}

__device__ inline void kf_measure(const float4 b, float (&z)[4]) {
    const float w = b.z - b.x, h = b.w - b.y;
    z[0] = b.x + w / 2.f;
    z[1] = b.y + h / 2.f;
    z[2] = w * h;
    z[3] = w / h;
}

__device__ inline void kf_start(const float (&z)[4], Kf& s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) s.x[i] = z[i], s.xd[i] = 0.f, s.p00[i] = 10.f, s.p01[i] = 0.f, s.p11[i] = 1e4f;
    s.r = z[3];
    s.p = 10.f;
}

__device__ inline void kf_predict(Kf& s) {
    const float q1[3] = {0.01f, 0.01f, 1e-4f};
    if (s.x[2] + s.xd[2] <= 0.f) s.xd[2] = 0.f;       // a NaN compares false
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float p00 = s.p00[i], p01 = s.p01[i], p11 = s.p11[i];
        s.x[i] = s.x[i] + s.xd[i];
        s.p00[i] = ((p00 + p01) + (p01 + p11)) + 1.f;
        s.p01[i] = p01 + p11;
        s.p11[i] = p11 + q1[i];
    }
    s.p = s.p + 1.f;
}

__device__ inline float4 kf_box(const Kf& s) {
    const float w = sqrtf(s.x[2] * s.r);
    const float h = s.x[2] / w;
    return make_float4(s.x[0] - w / 2.f, s.x[1] - h / 2.f, s.x[0] + w / 2.f, s.x[1] + h / 2.f);
}

__device__ inline void kf_update(Kf& s, const float (&z)[4]) {
    const float rn[3] = {1.f, 1.f, 10.f};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float p00 = s.p00[i], p01 = s.p01[i], p11 = s.p11[i];
        const float S = p00 + rn[i];
        const float k0 = p00 / S, k1 = p01 / S;
        const float y = z[i] - s.x[i];
        s.x[i] = s.x[i] + k0 * y;
        s.xd[i] = s.xd[i] + k1 * y;
        s.p11[i] = p11 - k1 * p01;
        s.p01[i] = p01 - k0 * p01;
        s.p00[i] = p00 - k0 * p00;
    }
    const float S = s.p + 10.f;
    const float k = s.p / S;
    s.r = s.r + k * (z[3] - s.r);
    s.p = s.p - k * s.p;
}

}  // namespace
