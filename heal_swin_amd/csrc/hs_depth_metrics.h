// Per-element rules and the reduction of the depth error metrics (evaluation/custom_metrics.py:62-468), shared by
// hs_depth_metrics (csrc/depth_eval.hip: both operands through strides) and hs_depth_metrics_gather (csrc/flat_eval.hip: the
// prediction through a table), so that both form the same HS_DEPTH_NSUMS sums from the same values in the same order:
// float64 per-lane sums, a tree over the workgroup, one partial record per workgroup, one ordered merge into the state
// (metric_pass and run_pass; the decoder tail, csrc/expand_ln_head.hip, accumulates in its own kernel and shares launch_reduce).
// Include after `#pragma clang fp contract(off)`.
#pragma once

#include <tuple>

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

// A workgroup's share of a metric pass over `batch` samples of `n` elements (grid of blocks_for(n * batch) workgroups of kThreads,
// element e = b n + i on lane e mod the grid's lanes): pair(b, i) returns std::make_tuple(prediction, target, log_var), log_var a
// callable as accumulate() takes it; the sums leave as the workgroup's partial record.
template <typename Pair>
__device__ __forceinline__ void metric_pass(const Rule& rule, int64_t n, int64_t batch, double* __restrict__ partial, Pair&& pair) {
    __shared__ double lds[kThreads];
    double acc[kNSums];
#pragma unroll
    for (int k = 0; k < kNSums; ++k) acc[k] = 0.0;
    const int64_t total = n * batch;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t b = e / n, i = e - b * n;
        const auto [p, t, log_var] = pair(b, i);
        accumulate(acc, rule, p, t, log_var);
    }
    store_partials(acc, lds, partial);
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

// host: the ordered merge of `blocks` partial records into the state
inline int launch_reduce(const double* partial, int blocks, double* state, hipStream_t s) {
    hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(kThreads), 0, s, partial, blocks, state);
    HS_LAUNCH_CHECK("depth_metrics_reduce");
    return HS_OK;
}

// host: a metric pass over `total` elements: launch(grid, block) starts the caller's metric_pass kernel, then the merge
template <typename Launch>
inline int run_pass(int64_t total, const double* partial, double* state, hipStream_t s, Launch&& launch) {
    const int blocks = (int)blocks_for(total);
    launch(dim3(blocks), dim3(kThreads));
    HS_LAUNCH_CHECK("depth_metrics pass");
    return launch_reduce(partial, blocks, state, s);
}

}  // namespace depth_metrics
}  // namespace hs
