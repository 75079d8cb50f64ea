// The per-element depth target transform, shared by hs_depth_target (csrc/depth_data.hip: an elementwise pass over strided rows)
// and hs_flat_resize (csrc/flat_data.hip: the same chain applied to a resized and padded depth map in the pass that makes it), so
// that both give the same bits for the same value.  Forward: 0 -> inf (HS_DT_ZERO_BKG), 1000 -> inf (HS_DT_1000_BKG), log /
// inverse_mask, (x - shift) / scale (HS_DT_AFFINE); inverse: x * scale + shift, exp / inverse_mask.  Transcendentals are formed in
// float64 and rounded once; the affine steps are float32, unfused.  Include after `#pragma clang fp contract(off)`.
#pragma once

#include "hs_device.h"

namespace hs {

struct TargetOp {
    int flags, transform;
    float shift, scale;
};

// inverse_mask (depth_utils.py:60-72): +inf -> 0; x < 1e-3 (0, negatives, -inf) -> +inf; NaN stays; the rest 1 / x
__device__ __forceinline__ float inverse_mask(float x) {
    if (x == INFINITY) return 0.f;
    if (x < 1e-3f) return INFINITY;
    return (float)(1.0 / (double)x);
}

__device__ __forceinline__ float target_op(float x, const TargetOp& o) {
    if (!(o.flags & HS_DT_INVERSE)) {
        if ((o.flags & HS_DT_ZERO_BKG) && x == 0.f) x = INFINITY;
        if ((o.flags & HS_DT_1000_BKG) && x == 1000.f) x = INFINITY;
        if (o.transform == HS_DT_LOG) x = (float)log((double)x);
        else if (o.transform == HS_DT_INV) x = inverse_mask(x);
        if (o.flags & HS_DT_AFFINE) x = (x - o.shift) / o.scale;
    } else {
        if (o.flags & HS_DT_AFFINE) x = x * o.scale + o.shift;
        if (o.transform == HS_DT_LOG) x = (float)exp((double)x);
        else if (o.transform == HS_DT_INV) x = inverse_mask(x);
    }
    return x;
}

}  // namespace hs
