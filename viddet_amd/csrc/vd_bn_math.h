// vd_bn_math.h - the per-element arithmetic of the BatchNorm (+ LeakyReLU) backward apply pass, shared by the streaming
// kernels that store dz (vd_bn.hip) and by the stem weight gradient that consumes dz without storing it (vd_stem.hip).
// ONE inlined function, so that the compiler contracts every site identically: the fused stem kernels feed the matrix
// pipe the very bits vd_bn_bwd_apply would have stored.
#pragma once
#include <hip/hip_runtime.h>

// z: the conv output (BatchNorm input), dy: the gradient of the cell's output; sc / sh: the folded scale and shift,
// mu / is: the batch mean and 1 / std, mg / mgx: the batch means of g and g * xhat (sums2 / count, rounded to fp32).
__device__ __forceinline__ float vd_bn_bwd_dz(float z, float dy, float sc, float sh, float mu, float is, float mg, float mgx,
                                              float slope) {
    const float u = z * sc + sh;
    const float g = u > 0.f ? dy : dy * slope;
    const float xh = (z - mu) * is;
    return sc * (g - mg - xh * mgx);
}
