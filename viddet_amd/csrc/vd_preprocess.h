// vd_preprocess.h — the normalise arithmetic of the uint8 input path, shared by the kernels that feed the stem
// (vd_pointwise.hip k_preprocess_u8 / k_preprocess_u8_nchw, vd_resize.hip, vd_augment.hip): ONE copy, so that their outputs are
// bit-equal.
#pragma once
#include "vd_common.h"

// mean/std of transforms.py:167-168; x/255 first (to_tensor), then (x-mean)/std (normalize).  v is a grey level held as a
// float, c its channel: (float)uint8 or a rounded and clamped resample in [0, 255] (vd_pointwise.hip, vd_resize.hip), or an
// unrounded level that a colour distortion may have taken outside [0, 255] (vd_augment.hip).
__device__ __forceinline__ float vd_normalize_level(float v, int c) {
    const float mean[3] = {0.485f, 0.456f, 0.406f};
    const float stdv[3] = {0.229f, 0.224f, 0.225f};
    return (v / 255.0f - mean[c]) / stdv[c];
}
