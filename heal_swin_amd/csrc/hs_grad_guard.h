// What a guarded optimizer step does to a gradient element before it is used (adam.hip: hs_adam_step_guarded; grad_guard.hip:
// hs_grad_scale): clamp to +-clip_value when that is positive, then scale by the clip coefficient of the guard record.
#pragma once
#include "hs_device.h"

namespace hs {

// (a NaN stays a NaN through the clamp, as through torch's clamp_; the product is rounded on its own -- never contracted into the
// weight-decay FMA behind it -- so that it is the value torch's clip_grad_norm_ leaves in .grad, and g * 1 is g bit for bit)
__device__ __forceinline__ float guard_grad(float g, float clip_value, float coef) {
#pragma clang fp contract(off)
    if (clip_value > 0.f) g = g < -clip_value ? -clip_value : (g > clip_value ? clip_value : g);
    return g * coef;
}

}  // namespace hs
