// Per-pixel terms of the depth-regression losses (heal_swin/training/loss_depth_regression.py, restated by
// heal_swin_amd/losses.py), shared by the standalone kernels (csrc/depth_loss.hip) and the decoder tail's loss epilogues
// (csrc/expand_ln_head.hip, csrc/ln_head.hip), so that both compute the same value and gradient from the same fp32 inputs.
//   p0 = predicted mean (channel 0), p1 = log variance (channel 1, HS_DEPTH_LOGVAR only), t = target, d = p0 - t:
//     HS_DEPTH_L1      |d|
//     HS_DEPTH_L2      d^2 / 2
//     HS_DEPTH_HUBER   SmoothL1 with beta = delta: |d| < delta ? 0.5 d^2 / delta : |d| - 0.5 delta
//     HS_DEPTH_LOGVAR  p1 / 2 + d^2 exp(-p1) / 2
// The caller keeps a pixel when its target is not infinite (NaN targets are kept and propagate) and gives every other pixel a
// gradient of exactly 0.  The gradients are those autograd forms for the compositions of losses.py, including torch's
// sgn(NaN) = 0 in the backward of abs (an L1 pixel with a NaN target gets 0, a Huber pixel NaN).
#pragma once

#include "hs_device.h"

namespace hs {

// the decoder tail's fused depth epilogues: a head of one or two channels, Huber on one, the log variance on two
inline bool depth_head_ok(int kind, float delta, int n_out) {
    if (kind == HS_DEPTH_L1 || kind == HS_DEPTH_L2) return n_out == 1 || n_out == 2;
    if (kind == HS_DEPTH_HUBER) return n_out == 1 && delta > 0.f;
    return kind == HS_DEPTH_LOGVAR && n_out == 2;
}
inline int check_depth_head(const char* who, int kind, float delta, int n_out) {
    HS_CHECK_ARG(depth_head_ok(kind, delta, n_out), "%s: kind %d with %d head channels (1 or 2; Huber 1, log variance 2; huber delta > 0)",
                 who, kind, n_out);
    return HS_OK;
}

__device__ __forceinline__ bool depth_keep(float t) { return !__builtin_isinf(t); }

__device__ __forceinline__ float depth_term(int kind, float delta, float p0, float p1, float t) {
    const float d = p0 - t;
    if (kind == HS_DEPTH_L1) return fabsf(d);
    if (kind == HS_DEPTH_L2) return d * d / 2.f;
    if (kind == HS_DEPTH_HUBER) {
        const float a = fabsf(d);
        return a < delta ? 0.5f * a * a / delta : a - 0.5f * delta;
    }
    return 0.5f * p1 + d * d * (0.5f * expf(-p1));
}

// sgn(d) * g with torch's sgn(0) = sgn(NaN) = 0
__device__ __forceinline__ float depth_sgn(float d, float g) { return d > 0.f ? g : (d < 0.f ? -g : 0.f); }

// (d loss / d p0, d loss / d p1) of one kept pixel, g = upstream gradient / count
__device__ __forceinline__ void depth_grad(int kind, float delta, float p0, float p1, float t, float g, float* g0, float* g1) {
    const float d = p0 - t;
    *g1 = 0.f;
    if (kind == HS_DEPTH_L1) {
        *g0 = depth_sgn(d, g);
    } else if (kind == HS_DEPTH_L2) {
        *g0 = g * d;
    } else if (kind == HS_DEPTH_HUBER) {
        // (a NaN d takes the linear branch, whose abs' backward gives 0, while the quadratic branch's product rule gives
        // 0 * NaN: the composition's gradient is NaN there)
        *g0 = fabsf(d) < delta ? g * d / delta : (d != d ? d : depth_sgn(d, g));
    } else {
        const float e = expf(-p1);
        *g0 = g * (d * e);
        *g1 = g * (0.5f - 0.5f * (d * d) * e);
    }
}

}  // namespace hs
