// vd_gru.hip — gate arithmetic of the bidirectional convolutional GRU over the K frames of a window
// (RNN(k, type='gru', bi=True), /root/reference models/definitions/layers.py:267-306; the cell is restated from MXNet 1.x
// gluon/contrib/rnn/conv_rnn_cell.py Conv2DGRUCell and gluon/rnn/rnn_cell.py BidirectionalCell.unroll — DESIGN.md 16).
//
// The convolutions of the cell (i2h over all B*K frames, h2h per step) are vd_conv_igemm launches with the bias in the
// epilogue; these kernels are the element-wise part between them, forward and backward through time:
//   r = sigmoid(I_r + H_r)   z = sigmoid(I_z + H_z)   n = tanh(I_o + r * H_o)   h = (1 - z) * n + z * h_prev
// with the 3*Ch channels of I and H in three blocks of Ch in the order r, z, o.
//
// Layouts (fp32 NHWC rows): I is the i2h output of the FOLDED frames [B*K, HW, 3*Ch] (frame b*K + t), because one conv
// launch over the folded input writes it; H, h and the carried state gradient are per-step slabs [B*HW, .] (the operand /
// result of a conv on B frames); dy is the folded gradient of the layer's output y = (hl + hr) / 2.
//
// Memory-bound passes: one lane owns four channels of one row, every operand moves as one 16-byte access and is read once.
// Nothing is kept for backward beyond I and H (the conv outputs themselves): the backward kernel recomputes r, z, n from
// them and writes dI over I and dH over H in place.  expf / tanhf are the accurate library functions.
#include "vd_common.h"

namespace {

// largest 16-byte element index of a launch plus one grid stride (the loop variable runs past `total` once) fits int32
inline bool fits32(int64_t items) { return items + (int64_t)4096 * 256 < ((int64_t)1 << 31); }

inline int gblocks(int64_t n) {
    int64_t nb = vd_cdiv(n, 256);
    if (nb > 4096) nb = 4096;
    if (nb < 1) nb = 1;
    return (int)nb;
}

// The index type IT is int32_t where every element index of the launch fits it (the host checks), else int64_t: the row /
// channel / frame split of a lane's item is two integer divisions, and 64-bit ones are long software sequences.
#define GRID_STRIDE(i, n)                                                              \
    for (IT i = (IT)blockIdx.x * (IT)blockDim.x + (IT)threadIdx.x; i < (n);            \
         i += (IT)gridDim.x * (IT)blockDim.x)

__device__ __forceinline__ f32x4 sigmoid4(const f32x4 a) {
    return f32x4{vd_sigmoid(a[0]), vd_sigmoid(a[1]), vd_sigmoid(a[2]), vd_sigmoid(a[3])};
}
__device__ __forceinline__ f32x4 tanh4(const f32x4 a) { return f32x4{tanhf(a[0]), tanhf(a[1]), tanhf(a[2]), tanhf(a[3])}; }

// row (b, p) of frame t in the folded tensor
template <typename IT>
__device__ __forceinline__ IT folded_row(IT m, IT HW, int K, int t) {
    const IT b = m / HW;
    return (b * K + t) * HW + (m - b * HW);
}

// H == NULL: the state is zero, H is the h2h bias alone (no conv was launched); hprev == NULL: zero state
template <typename IT>
__global__ void k_gru_gate_fwd(const float* __restrict__ I, const float* __restrict__ H, const float* __restrict__ hbias,
                               const float* __restrict__ hprev, float* __restrict__ h, IT M, IT HW, int K, int t,
                               int C4) {
    const IT total = M * C4;
    GRID_STRIDE(i, total) {
        const IT m = i / C4;
        const int c = (int)(i - m * C4);
        const IT ri = folded_row<IT>(m, HW, K, t) * 3 * C4 + c;
        const f32x4 ir = vd_ld4(I, ri), iz = vd_ld4(I, ri + C4), io = vd_ld4(I, ri + 2 * C4);
        f32x4 hr, hz, ho;
        if (H) {
            const IT rh = m * 3 * C4 + c;
            hr = vd_ld4(H, rh), hz = vd_ld4(H, rh + C4), ho = vd_ld4(H, rh + 2 * C4);
        } else {
            hr = vd_ld4(hbias, c), hz = vd_ld4(hbias, c + C4), ho = vd_ld4(hbias, c + 2 * C4);
        }
        const f32x4 r = sigmoid4(ir + hr), z = sigmoid4(iz + hz), n = tanh4(io + r * ho);
        f32x4 o = (1.0f - z) * n;
        if (hprev) o += z * vd_ld4(hprev, i);
        vd_st4(h, i, o);
    }
}

// dh = dy_scale * dy[frame t] + (carry ? dh : 0);  dI -> I, dH -> H (in place), dh <- dh * z when the step had a state
template <typename IT>
__global__ void k_gru_gate_bwd(float* __restrict__ I, float* __restrict__ H, int h_valid, const float* __restrict__ hbias,
                               const float* __restrict__ hprev, const float* __restrict__ dy, float dy_scale,
                               float* __restrict__ dh, int carry, IT M, IT HW, int K, int t, int C4) {
    const IT total = M * C4;
    GRID_STRIDE(i, total) {
        const IT m = i / C4;
        const int c = (int)(i - m * C4);
        const IT fr = folded_row<IT>(m, HW, K, t);
        const IT ri = fr * 3 * C4 + c, rh = m * 3 * C4 + c;
        const f32x4 ir = vd_ld4(I, ri), iz = vd_ld4(I, ri + C4), io = vd_ld4(I, ri + 2 * C4);
        f32x4 hr, hz, ho;
        if (h_valid) {
            hr = vd_ld4(H, rh), hz = vd_ld4(H, rh + C4), ho = vd_ld4(H, rh + 2 * C4);
        } else {
            hr = vd_ld4(hbias, c), hz = vd_ld4(hbias, c + C4), ho = vd_ld4(hbias, c + 2 * C4);
        }
        const f32x4 r = sigmoid4(ir + hr), z = sigmoid4(iz + hz), n = tanh4(io + r * ho);
        f32x4 g = dy_scale * vd_ld4(dy, fr * C4 + c);
        if (carry) g += vd_ld4(dh, i);
        f32x4 hp = f32x4{0.f, 0.f, 0.f, 0.f};
        if (hprev) hp = vd_ld4(hprev, i);
        const f32x4 da = g * (1.0f - z) * (1.0f - n * n);
        const f32x4 dr = da * ho * r * (1.0f - r);
        const f32x4 dz = g * (hp - n) * z * (1.0f - z);
        vd_st4(I, ri, dr), vd_st4(I, ri + C4, dz), vd_st4(I, ri + 2 * C4, da);
        vd_st4(H, rh, dr), vd_st4(H, rh + C4, dz), vd_st4(H, rh + 2 * C4, da * r);
        if (hprev) vd_st4(dh, i, g * z);
    }
}

// y[b*K + t] = (hl[step t][b] + hr[step K-1-t][b]) / 2: the two directions' step-major states -> the folded output
template <typename IT>
__global__ void k_gru_avg(const float* __restrict__ hl, const float* __restrict__ hr, float* __restrict__ y, int B, int K,
                          IT inner4, float* __restrict__ amax) {
    const IT total = (IT)B * K * inner4;
    float mx = 0.f;
    GRID_STRIDE(i, total) {
        const IT f = i / inner4, e = i - f * inner4;
        const IT b = f / K;
        const int t = (int)(f - b * K);
        const f32x4 v = 0.5f * (vd_ld4(hl, ((IT)t * B + b) * inner4 + e) + vd_ld4(hr, ((IT)(K - 1 - t) * B + b) * inner4 + e));
        vd_st4(y, i, v);
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
    if (amax) vd_amax_publish(amax, mx);
}

}  // namespace

extern "C" {

int vd_gru_gate_fwd(const float* I, const float* H, const float* hbias, const float* hprev, float* h, int B, int K, int t,
                    int64_t HW, int Ch, void* stream) {
    VD_REQUIRE(I && h && (H || hbias) && B > 0 && K > 0 && t >= 0 && t < K && HW > 0 && Ch > 0 && Ch % 4 == 0,
               "vd_gru_gate_fwd: bad args (Ch=%d must be a positive multiple of 4, 0 <= t=%d < K=%d, H or hbias)", Ch, t, K);
    VD_REQUIRE(((uintptr_t)I | (uintptr_t)H | (uintptr_t)hbias | (uintptr_t)hprev | (uintptr_t)h) % 16 == 0,
               "vd_gru_gate_fwd: pointers must be 16-byte aligned");
    const int64_t M = (int64_t)B * HW;
    if (fits32(M * K * 3 * (Ch / 4)))
        hipLaunchKernelGGL(k_gru_gate_fwd<int32_t>, dim3(gblocks(M * (Ch / 4))), dim3(256), 0, (hipStream_t)stream, I, H, hbias, hprev,
                           h, (int32_t)M, (int32_t)HW, K, t, Ch / 4);
    else
        hipLaunchKernelGGL(k_gru_gate_fwd<int64_t>, dim3(gblocks(M * (Ch / 4))), dim3(256), 0, (hipStream_t)stream, I, H, hbias, hprev,
                           h, M, HW, K, t, Ch / 4);
    VD_CHECK_LAUNCH("vd_gru_gate_fwd");
    return VD_OK;
}

int vd_gru_gate_bwd(float* I, float* H, int h_valid, const float* hbias, const float* hprev, const float* dy, float dy_scale,
                    float* dh, int carry, int B, int K, int t, int64_t HW, int Ch, void* stream) {
    VD_REQUIRE(I && H && dy && (h_valid || hbias) && (dh || (!carry && !hprev)) && B > 0 && K > 0 && t >= 0 && t < K && HW > 0 &&
                   Ch > 0 && Ch % 4 == 0,
               "vd_gru_gate_bwd: bad args (Ch=%d must be a positive multiple of 4, 0 <= t=%d < K=%d, hbias without H values, "
               "dh with carry or hprev)", Ch, t, K);
    VD_REQUIRE(((uintptr_t)I | (uintptr_t)H | (uintptr_t)hbias | (uintptr_t)hprev | (uintptr_t)dy | (uintptr_t)dh) % 16 == 0,
               "vd_gru_gate_bwd: pointers must be 16-byte aligned");
    const int64_t M = (int64_t)B * HW;
    if (fits32(M * K * 3 * (Ch / 4)))
        hipLaunchKernelGGL(k_gru_gate_bwd<int32_t>, dim3(gblocks(M * (Ch / 4))), dim3(256), 0, (hipStream_t)stream, I, H, h_valid,
                           hbias, hprev, dy, dy_scale, dh, carry, (int32_t)M, (int32_t)HW, K, t, Ch / 4);
    else
        hipLaunchKernelGGL(k_gru_gate_bwd<int64_t>, dim3(gblocks(M * (Ch / 4))), dim3(256), 0, (hipStream_t)stream, I, H, h_valid,
                           hbias, hprev, dy, dy_scale, dh, carry, M, HW, K, t, Ch / 4);
    VD_CHECK_LAUNCH("vd_gru_gate_bwd");
    return VD_OK;
}

int vd_gru_avg(const float* hl, const float* hr, float* y, int B, int K, int64_t inner, float* amax_out, void* stream) {
    VD_REQUIRE(hl && hr && y && B > 0 && K > 0 && inner > 0 && inner % 4 == 0, "vd_gru_avg: bad args (inner must be a multiple of 4)");
    VD_REQUIRE(((uintptr_t)hl | (uintptr_t)hr | (uintptr_t)y) % 16 == 0, "vd_gru_avg: pointers must be 16-byte aligned");
    if (fits32((int64_t)B * K * (inner / 4)))
        hipLaunchKernelGGL(k_gru_avg<int32_t>, dim3(gblocks((int64_t)B * K * (inner / 4))), dim3(256), 0, (hipStream_t)stream, hl, hr,
                           y, B, K, (int32_t)(inner / 4), amax_out);
    else
        hipLaunchKernelGGL(k_gru_avg<int64_t>, dim3(gblocks((int64_t)B * K * (inner / 4))), dim3(256), 0, (hipStream_t)stream, hl, hr,
                           y, B, K, inner / 4, amax_out);
    VD_CHECK_LAUNCH("vd_gru_avg");
    return VD_OK;
}

}  // extern "C"
