// Per-element rules and the reduction of the depth error metrics (evaluation/custom_metrics.py:62-468), shared by
// hs_depth_metrics (csrc/depth_eval.hip: both operands through strides) and hs_depth_metrics_gather (csrc/flat_eval.hip: the
// prediction through a table), so that both form the same HS_DEPTH_NSUMS sums from the same values in the same order:
// float64 per-lane sums, a tree over the workgroup, one partial record per workgroup, one ordered merge into the state.
// Include after `#pragma clang fp contract(off)`.
#pragma once

#include "hs_device.h"

namespace hs {
namespace depth_metrics {

constexpr int kThreads = 256;
constexpr int kMaxRanges = 8;
constexpr int kNSums = HS_DEPTH_NSUMS;
constexpr int kBlocksMax = 1024;

struct Rule {
    int use_logvar, n_ranges;
    double total_mean;
    float lo[kMaxRanges], hi[kMaxRanges];
};

// workgroups (= partial records) of a pass over `total` elements
inline int64_t blocks_for(int64_t total) {
    const int64_t blocks = (total + kThreads * 8 - 1) / (kThreads * 8);
    return blocks < 1 ? 1 : (blocks > kBlocksMax ? kBlocksMax : blocks);
}

template <typename C>
__device__ __forceinline__ C load_val(const void* p, int kind, int64_t off) {
    if (kind == HS_F64) return (C)((const double*)p)[off];
    if (kind == HS_BF16) return (C)bf16_to_float(((const uint16_t*)p)[off]);
    return (C)((const float*)p)[off];
}

__device__ __forceinline__ float log_c(float x) { return logf(x); }
__device__ __forceinline__ double log_c(double x) { return log(x); }
__device__ __forceinline__ float std_of(float lv) { return sqrtf(expf(lv)); }
__device__ __forceinline__ double std_of(double lv) { return sqrt(exp(lv)); }
template <typename C>
__device__ __forceinline__ C inv_km(C x) {  // DepthiRMSE's 1 / (0.001 x), the scalar in the tensor's own type
    return (C)1 / ((C)0.001 * x);
}

// One (prediction, target) pair added to a lane's sums.  P, T: the types the reference computes in for the prediction and the
// target (float for fp32 / bf16 tensors, double for the float64 back-projected predictions); a per-element value is formed in
// those types, every sum in float64.  log_var() is called only for the pairs MeanSTD keeps.
template <typename P, typename T, typename LogVar>
__device__ __forceinline__ void accumulate(double (&acc)[kNSums], const Rule& a, P p, T t, LogVar log_var) {
    const double tm = (double)a.total_mean;
    if (isfinite(p) && isfinite(t)) {  // get_non_inf_non_nan_idxs
        const double d = (double)p - (double)t;
        const double dm = tm - (double)t;
        acc[HS_DS_N] += 1.0;
        acc[HS_DS_SE] += d * d;
        acc[HS_DS_AE] += fabs(d);
        acc[HS_DS_MEAN_SE] += dm * dm;
        acc[HS_DS_MEAN_AE] += fabs(dm);
        acc[HS_DS_PRED] += (double)p;
        if (p > (P)0 && t > (T)0) {
            const double dl = (double)log_c(t) - (double)log_c(p);
            acc[HS_DS_SIL_N] += 1.0;
            acc[HS_DS_SIL_D] += dl;
            acc[HS_DS_SIL_D2] += dl * dl;
        }
#pragma unroll
        for (int r = 0; r < kMaxRanges; ++r) {
            if (r < a.n_ranges && (T)a.lo[r] <= t && t < (T)a.hi[r]) {
                acc[HS_DS_RANGE + 2 * r] += 1.0;
                acc[HS_DS_RANGE + 2 * r + 1] += d * d;
            }
        }
    }
    // DepthiRMSE: transformed first, then selected: a target of +inf becomes 0 and counts, a prediction of 0 is dropped
    const P ip = inv_km(p);
    const T it = inv_km(t);
    if (isfinite(ip) && isfinite(it)) {
        const double d = (double)ip - (double)it;
        acc[HS_DS_INV_N] += 1.0;
        acc[HS_DS_INV_SE] += d * d;
    }
    // MeanSTD: +inf targets become NaN, NaN targets are dropped, the prediction is not looked at
    if (a.use_logvar && !isnan(t) && t != (T)INFINITY) {
        acc[HS_DS_STD_N] += 1.0;
        acc[HS_DS_STD] += (double)std_of(log_var());
    }
}

__device__ __forceinline__ double block_sum(double v, double* lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) lds[threadIdx.x] += lds[threadIdx.x + h];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

// the workgroup's record: partial[blockIdx.x][k] = sum over its lanes of acc[k]
__device__ __forceinline__ void store_partials(const double (&acc)[kNSums], double* lds, double* __restrict__ partial) {
    for (int k = 0; k < kNSums; ++k) {
        const double v = block_sum(acc[k], lds);
        if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * kNSums + k] = v;
    }
}

// one workgroup: state[k] += sum over blocks of partial[blk][k], in a fixed order
static __global__ void __launch_bounds__(kThreads) reduce_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ state) {
    __shared__ double lds[kThreads];
    for (int k = 0; k < kNSums; ++k) {
        double v = 0.0;
        for (int j = threadIdx.x; j < blocks; j += kThreads) v += partial[(int64_t)j * kNSums + k];
        v = block_sum(v, lds);
        if (threadIdx.x == 0) state[k] += v;
    }
}

inline int fill_rule(Rule& a, int use_logvar, double total_mean, const float* ranges, int n_ranges) {
    HS_CHECK_ARG(n_ranges >= 0 && n_ranges <= kMaxRanges && (n_ranges == 0 || ranges), "at most %d distance ranges", kMaxRanges);
    a.use_logvar = use_logvar;
    a.n_ranges = n_ranges;
    a.total_mean = total_mean;
    for (int r = 0; r < kMaxRanges; ++r) {
        a.lo[r] = r < n_ranges ? ranges[2 * r] : 0.f;
        a.hi[r] = r < n_ranges ? ranges[2 * r + 1] : 0.f;
    }
    return HS_OK;
}

}  // namespace depth_metrics
}  // namespace hs
