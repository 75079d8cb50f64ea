// hs_grad_stats / hs_grad_guard_finalize / hs_grad_scale: the guard rails of the flat optimizer step.
//
// The reference's trainer clips gradients, logs their norms and stops on a NaN through Lightning (gradient_clip_val,
// gradient_clip_algorithm, track_grad_norm, terminate_on_nan: training/train_config.py:65-66,76,104), which walks the ~630
// parameter tensors of HEAL-SWIN-B with foreach kernels and rewrites every gradient.  Here the gradients already sit in a few
// flat fp32 buckets (parallel.GradBucketAllReduce), so ONE read-only pass gives every norm: a host-built table cuts each
// parameter's slot into items of at most kPiece elements, one wavefront sums the squares and takes the max |g| of one item
// (16-byte loads, every element converted to double first, every sum in double: the pass is HBM-bound and the fp64 adds ride
// along), and two small launches fold items into parameters and parameters into the total.  The result stays on the device in
// an hs_grad_guard record that hs_adam_step_guarded (adam.hip) and hs_grad_scale read: nothing is decided on the host, the
// guarded step remains one HIP graph.
//
// Determinism: no atomics.  Which elements an item covers, which items a parameter has and in which order they are added is
// fixed by the tables; a wavefront adds its 64 lane sums in a butterfly (commutative at every level: all lanes hold the same
// bits), a workgroup its 256 thread sums in a fixed tree.  No grid here is sized from the CU count or hs_set_reserved_cus.
#include "hs_grad_guard.h"

namespace hs {
namespace {

constexpr int kPiece = 4096;          // elements per item: 16 float4 per lane of a wavefront
constexpr int kVecPerLane = kPiece / 256;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// max that keeps a NaN (fmax drops it): a gradient with a NaN has a NaN inf-norm, as in torch
template <typename T>
__device__ __forceinline__ T nan_max(T m, T a) {
    return (a > m || a != a) ? a : m;
}
template <typename T>
__device__ __forceinline__ T wave_nan_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = nan_max(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ void take(float x, double& ss, float& mx) {
    const double d = (double)x;
    ss += d * d;
    mx = nan_max(mx, fabsf(x));
}
__device__ __forceinline__ void take4(const float4& v, double& ss, float& mx) {
    take(v.x, ss, mx), take(v.y, ss, mx), take(v.z, ss, mx), take(v.w, ss, mx);
}

// one wavefront per item; four items per workgroup, so a 3-element logit_scale costs a wavefront, not a workgroup
__global__ void __launch_bounds__(256) grad_stats_kernel(const float* __restrict__ g, int64_t n, const int64_t* __restrict__ items, int n_items,
                                                         double* __restrict__ partials) {
    const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (item >= n_items) return;
    const int lane = threadIdx.x & 63;
    const int64_t start = items[2 * (int64_t)item], len = items[2 * (int64_t)item + 1];
    double ss = 0.0;
    float mx = 0.f;
    if (start < 0 || (start & 3) || len <= 0 || len > kPiece || start > n - len) {  // not a slice of g: read nothing
        ss = __longlong_as_double(0x7ff8000000000000ll);
        mx = __uint_as_float(0x7fc00000u);
    } else if (len == kPiece) {  // the common case: every load issued before the first use
        const float4* src = (const float4*)(g + start) + lane;
        float4 v[kVecPerLane];
#pragma unroll
        for (int k = 0; k < kVecPerLane; ++k) v[k] = src[64 * k];
#pragma unroll
        for (int k = 0; k < kVecPerLane; ++k) take4(v[k], ss, mx);
    } else {
        const float* src = g + start;
        const int m = (int)len;
        for (int e = 4 * lane; e < m; e += 256) {
            if (e + 3 < m) {
                take4(*(const float4*)(src + e), ss, mx);
            } else {
                for (int j = e; j < m; ++j) take(src[j], ss, mx);
            }
        }
    }
    ss = wave_sum_f64(ss);
    mx = wave_nan_max(mx);
    if (lane == 0) {
        partials[2 * (int64_t)item] = ss;
        partials[2 * (int64_t)item + 1] = (double)mx;
    }
}

// one wavefront per parameter: lane l adds items l, l + 64, ... of the parameter in that order, then the butterfly
__global__ void __launch_bounds__(256) grad_fold_params_kernel(const double* __restrict__ partials, int64_t n_items, const int32_t* __restrict__ params,
                                                               int n_params, int norm_inf, float* __restrict__ param_norm,
                                                               double* __restrict__ work) {
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (p >= n_params) return;
    const int lane = threadIdx.x & 63;
    const int64_t first = params[2 * p], count = params[2 * p + 1];
    double ss = 0.0, mx = 0.0;
    if (first < 0 || count < 0 || first > n_items - count) {
        ss = mx = __longlong_as_double(0x7ff8000000000000ll);
    } else {
        for (int64_t i = lane; i < count; i += 64) {
            ss += partials[2 * (first + i)];
            mx = nan_max(mx, partials[2 * (first + i) + 1]);
        }
    }
    ss = wave_sum_f64(ss);
    mx = wave_nan_max(mx);
    if (lane == 0) {
        work[2 * p] = ss;
        work[2 * p + 1] = mx;
        param_norm[p] = norm_inf ? (float)mx : (float)sqrt(ss);
    }
}

// one workgroup: thread t adds parameters t, t + 256, ... in that order, then a fixed tree through LDS
__global__ void __launch_bounds__(256) grad_fold_total_kernel(const double* __restrict__ work, int n_params, int norm_inf, float max_norm,
                                                              hs_grad_guard* __restrict__ guard) {
    __shared__ double s_ss[256], s_mx[256];
    const int t = threadIdx.x;
    double ss = 0.0, mx = 0.0;
    for (int p = t; p < n_params; p += 256) {
        ss += work[2 * p];
        mx = nan_max(mx, work[2 * p + 1]);
    }
    s_ss[t] = ss;
    s_mx[t] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            s_ss[t] += s_ss[t + s];
            s_mx[t] = nan_max(s_mx[t], s_mx[t + s]);
        }
        __syncthreads();
    }
    if (t == 0) {
        const float total = norm_inf ? (float)s_mx[0] : (float)sqrt(s_ss[0]);
        float coef = 1.f;
        if (max_norm >= 0.f) {  // torch.nn.utils.clip_grad_norm_, in fp32 and evaluated as there (scalar / tensor is reciprocal times
                                // scalar); a NaN norm gives a NaN coefficient, as there
            coef = (1.f / (total + 1e-6f)) * max_norm;
            coef = coef > 1.f ? 1.f : coef;
        }
        guard->total_norm = total;
        guard->clip_coef = coef;
        guard->finite = isfinite(s_ss[0]) ? 1 : 0;
        guard->reserved = 0;
    }
}

__global__ void __launch_bounds__(256) grad_scale_kernel(float* __restrict__ g, int64_t n, float clip_value, const hs_grad_guard* __restrict__ guard) {
    const float coef = guard->clip_coef;
    if (!(clip_value > 0.f) && coef == 1.f) return;  // nothing to change (g * 1 is g)
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        float4 v = *(const float4*)(g + i);
        v.x = guard_grad(v.x, clip_value, coef), v.y = guard_grad(v.y, clip_value, coef);
        v.z = guard_grad(v.z, clip_value, coef), v.w = guard_grad(v.w, clip_value, coef);
        *(float4*)(g + i) = v;
    } else {
        for (int64_t j = i; j < n; ++j) g[j] = guard_grad(g[j], clip_value, coef);
    }
}

}  // namespace
}  // namespace hs

extern "C" {

int hs_grad_guard_piece(void) { return hs::kPiece; }

int hs_grad_stats(const float* g, int64_t n, const int64_t* items, int n_items, double* partials, void* stream) {
    using namespace hs;
    HS_CHECK_ARG(g && items && partials, "hs_grad_stats: null pointer");
    HS_CHECK_ARG(n > 0 && n < ((int64_t)1 << 40), "hs_grad_stats: bad length");
    HS_CHECK_ARG(n_items > 0 && n_items <= (1 << 30), "hs_grad_stats: bad item count");
    HS_CHECK_ALIGNED("hs_grad_stats", 16, g, items, partials);
    hipLaunchKernelGGL(grad_stats_kernel, dim3((unsigned)((n_items + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, n, items, n_items, partials);
    HS_LAUNCH_CHECK("grad_stats");
    return HS_OK;
}

int hs_grad_guard_finalize(const double* partials, int64_t n_items, const int32_t* params, int n_params, int norm_inf, float max_norm,
                           float* param_norm, double* work, hs_grad_guard* guard, void* stream) {
    using namespace hs;
    HS_CHECK_ARG(partials && params && param_norm && work && guard, "hs_grad_guard_finalize: null pointer");
    HS_CHECK_ARG(n_items > 0 && n_items < ((int64_t)1 << 31), "hs_grad_guard_finalize: bad item count");
    HS_CHECK_ARG(n_params > 0 && n_params <= (1 << 28), "hs_grad_guard_finalize: bad parameter count");
    HS_CHECK_ARG(!(max_norm != max_norm), "hs_grad_guard_finalize: max_norm is NaN");
    HS_CHECK_ALIGNED("hs_grad_guard_finalize", 16, partials, work, guard);
    HS_CHECK_ALIGNED("hs_grad_guard_finalize (parameter table)", 8, params);
    HS_CHECK_ALIGNED("hs_grad_guard_finalize (norms)", 4, param_norm);
    hipLaunchKernelGGL(grad_fold_params_kernel, dim3((unsigned)((n_params + 3) / 4)), dim3(256), 0, (hipStream_t)stream, partials, n_items, params,
                       n_params, norm_inf, param_norm, work);
    HS_LAUNCH_CHECK("grad_fold_params");
    hipLaunchKernelGGL(grad_fold_total_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)work, n_params, norm_inf, max_norm, guard);
    HS_LAUNCH_CHECK("grad_fold_total");
    return HS_OK;
}

int hs_grad_scale(float* g, int64_t n, float clip_value, const hs_grad_guard* guard, void* stream) {
    using namespace hs;
    HS_CHECK_ARG(g && guard, "hs_grad_scale: null pointer");
    HS_CHECK_ARG(n > 0 && n < ((int64_t)1 << 40), "hs_grad_scale: bad length");
    HS_CHECK_ARG(!(clip_value != clip_value), "hs_grad_scale: clip_value is NaN");
    HS_CHECK_ALIGNED("hs_grad_scale", 16, g, guard);
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, g, n, clip_value, guard);
    HS_LAUNCH_CHECK("grad_scale");
    return HS_OK;
}

}  // extern "C"
