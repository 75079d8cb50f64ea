// hs_adam_step: the optimizer step of the training loop over FLAT parameter / gradient / moment buffers.
//
// The reference's trainer steps torch.optim.Adam / AdamW over the model's ~330 parameter tensors
// (training/optimizer.py:57-66).  Here the gradients already live in a few flat fp32 buckets (parallel.GradBucketAllReduce);
// heal_swin_amd.optim.FlatAdam lays parameters and moments out the same way, so a step is ONE elementwise launch per bucket that
// also writes the bf16 copy of the updated parameters the next forward's GEMMs read (ops.ParamCastCache): 16 B read + 14 B written
// per parameter instead of a multi-tensor Adam (28 B) plus a separate multi-tensor cast (6 B) plus their ~40 launches -- on the
// launch-heavy HEAL-SWIN-T / nside 128 step the two were 0.86 + 0.4 ms of 16.7 ms (profiles/archive_r01_r04/r04_k_T128_summary.txt).
//
// Arithmetic = torch.optim.Adam (amsgrad = False, maximize = False), single-tensor form:
//   g += wd * p (Adam)   |   p *= 1 - lr * wd (AdamW, `decoupled`)
//   m += (g - m) (1 - b1);   v = b2 v + (1 - b2) g^2;   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// with the step count t = *step + 1 read from DEVICE memory (hs_adam_advance increments it after the last bucket), so that a
// captured HIP graph of the whole training step replays with the right bias corrections.
//
// hs_adam_step_guarded is the same step behind the guard record of csrc/grad_guard.hip: the gradient is clamped / scaled by the
// clip coefficient on its way out of the load, and a step whose gradients are not finite writes nothing.
#include "hs_grad_guard.h"

namespace hs {
namespace {

struct AdamArgs {
    float* p;
    const float* g;
    float* m;
    float* v;
    uint16_t* lowp;  // bf16 copy of the updated parameters, or null
    int64_t n;
    float lr;
    const float* lr_dev;  // overrides lr when non-null (a device scalar: learning-rate schedules under graph replay)
    float beta1, beta2, eps, weight_decay;
    int decoupled;
    const int64_t* step;
};

__device__ __forceinline__ float adam_one(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps, float wd,
                                          int decoupled, float inv_bc1, float inv_sqrt_bc2) {
    if (wd != 0.f) {
        if (decoupled) p *= 1.f - lr * wd;
        else g += wd * p;
    }
    m += (g - m) * (1.f - b1);
    v = v * b2 + (1.f - b2) * g * g;
    const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
    // (m == 0 moves nothing; skipping it keeps the zero alignment gaps of the flat buffers -- p = g = m = v = 0 -- from becoming
    // 0 / 0 when eps is 0)
    if (m != 0.f) p -= (lr * inv_bc1) * (m / denom);
    return p;
}

// GUARDED: every gradient element goes through guard_grad(., clip_value, coef) first
template <bool GUARDED>
__device__ __forceinline__ void adam_body(const AdamArgs& a, float clip_value, float coef) {
    __shared__ float corr[2];
    const float lr = a.lr_dev ? *a.lr_dev : a.lr;
    if (threadIdx.x == 0) {  // bias corrections in double, once per workgroup (torch forms them on the host in double)
        const double t = (double)(*a.step + 1);
        corr[0] = (float)(1.0 / (1.0 - pow((double)a.beta1, t)));
        corr[1] = (float)(1.0 / sqrt(1.0 - pow((double)a.beta2, t)));
    }
    __syncthreads();
    const float inv_bc1 = corr[0], inv_sqrt_bc2 = corr[1];
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < a.n) {
        float4 p = *(const float4*)(a.p + i), m = *(const float4*)(a.m + i), v = *(const float4*)(a.v + i);
        float4 g = *(const float4*)(a.g + i);
        if constexpr (GUARDED) {
            g.x = guard_grad(g.x, clip_value, coef), g.y = guard_grad(g.y, clip_value, coef);
            g.z = guard_grad(g.z, clip_value, coef), g.w = guard_grad(g.w, clip_value, coef);
        }
        adam_one(p.x, g.x, m.x, v.x, lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.decoupled, inv_bc1, inv_sqrt_bc2);
        adam_one(p.y, g.y, m.y, v.y, lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.decoupled, inv_bc1, inv_sqrt_bc2);
        adam_one(p.z, g.z, m.z, v.z, lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.decoupled, inv_bc1, inv_sqrt_bc2);
        adam_one(p.w, g.w, m.w, v.w, lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.decoupled, inv_bc1, inv_sqrt_bc2);
        *(float4*)(a.p + i) = p;
        *(float4*)(a.m + i) = m;
        *(float4*)(a.v + i) = v;
        if (a.lowp) *(uint2*)(a.lowp + i) = make_uint2(pack_bf16x2(p.x, p.y), pack_bf16x2(p.z, p.w));
    } else {
        for (int64_t j = i; j < a.n; ++j) {
            float p = a.p[j], m = a.m[j], v = a.v[j];
            float g = a.g[j];
            if constexpr (GUARDED) g = guard_grad(g, clip_value, coef);
            adam_one(p, g, m, v, lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.decoupled, inv_bc1, inv_sqrt_bc2);
            a.p[j] = p;
            a.m[j] = m;
            a.v[j] = v;
            if (a.lowp) a.lowp[j] = float_to_bf16(p);
        }
    }
}

__global__ void __launch_bounds__(256) adam_kernel(const AdamArgs a) { adam_body<false>(a, 0.f, 1.f); }

__global__ void __launch_bounds__(256) adam_guarded_kernel(const AdamArgs a, float clip_value, const hs_grad_guard* guard, int skip_nonfinite) {
    if (skip_nonfinite && !guard->finite) return;  // (the same for every thread of the grid: p, m, v and the bf16 copy stay as they are)
    adam_body<true>(a, clip_value, guard->clip_coef);
}

__global__ void adam_advance_kernel(int64_t* step) { *step += 1; }

__global__ void adam_advance_guarded_kernel(int64_t* step, const hs_grad_guard* guard, int skip_nonfinite, int64_t* skipped) {
    const bool skip = skip_nonfinite && !guard->finite;
    *step += skip ? 0 : 1;
    *skipped += skip ? 1 : 0;
}

}  // namespace
}  // namespace hs

// the argument checks of hs_adam_step and hs_adam_step_guarded
static int adam_check(const char* who, const hs::AdamArgs& a) {
    HS_CHECK_ARG(a.p && a.g && a.m && a.v && a.step, "%s: null pointer", who);
    HS_CHECK_ARG(a.n > 0 && a.n < ((int64_t)1 << 40), "%s: bad length", who);
    HS_CHECK_ALIGNED(who, 16, a.p, a.g, a.m, a.v);
    HS_CHECK_ALIGNED(who, 8, a.lowp);
    HS_CHECK_ARG(a.beta1 >= 0.f && a.beta1 < 1.f && a.beta2 >= 0.f && a.beta2 < 1.f && a.eps >= 0.f, "%s: bad hyper-parameters", who);
    return HS_OK;
}

extern "C" {

int hs_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, const float* lr_dev, float beta1,
                 float beta2, float eps, float weight_decay, int decoupled, const int64_t* step, void* stream) {
    using namespace hs;
    AdamArgs a{p, g, m, v, (uint16_t*)p_bf16, n, lr, lr_dev, beta1, beta2, eps, weight_decay, decoupled, step};
    if (const int st = adam_check("hs_adam_step", a)) return st;
    const int64_t blocks = (n + 1023) / 1024;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    HS_LAUNCH_CHECK("adam_step");
    return HS_OK;
}

int hs_adam_step_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, const float* lr_dev, float beta1,
                         float beta2, float eps, float weight_decay, int decoupled, const int64_t* step, float clip_value,
                         const hs_grad_guard* guard, int skip_nonfinite, void* stream) {
    using namespace hs;
    AdamArgs a{p, g, m, v, (uint16_t*)p_bf16, n, lr, lr_dev, beta1, beta2, eps, weight_decay, decoupled, step};
    if (const int st = adam_check("hs_adam_step_guarded", a)) return st;
    HS_CHECK_ARG(guard, "hs_adam_step_guarded: null pointer");
    HS_CHECK_ALIGNED("hs_adam_step_guarded (guard)", 16, guard);
    HS_CHECK_ARG(!(clip_value != clip_value), "hs_adam_step_guarded: clip_value is NaN");
    const int64_t blocks = (n + 1023) / 1024;
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, clip_value, guard, skip_nonfinite);
    HS_LAUNCH_CHECK("adam_step_guarded");
    return HS_OK;
}

int hs_adam_advance_guarded(int64_t* step, const hs_grad_guard* guard, int skip_nonfinite, int64_t* skipped, void* stream) {
    using namespace hs;
    HS_CHECK_ARG(step && guard && skipped, "hs_adam_advance_guarded: null pointer");
    HS_CHECK_ALIGNED("hs_adam_advance_guarded (guard)", 16, guard);
    hipLaunchKernelGGL(adam_advance_guarded_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, guard, skip_nonfinite, skipped);
    HS_LAUNCH_CHECK("adam_advance_guarded");
    return HS_OK;
}

int hs_adam_advance(int64_t* step, void* stream) {
    using namespace hs;
    HS_CHECK_ARG(step, "hs_adam_advance: null pointer");
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
    HS_LAUNCH_CHECK("adam_advance");
    return HS_OK;
}

}  // extern "C"
