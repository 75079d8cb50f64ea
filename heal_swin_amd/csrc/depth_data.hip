// The depth data path (heal_swin_amd/depth_data.py) after the projection: the target transforms of the reference's datasets and
// Lightning module, and the dataset statistics behind their normalization constants.  (The per-frame samplers of the depth
// projection, hs_sample_bilinear_u8_f32 and hs_sample_nearest_f32, are projection.hip's.)
//
//   hs_depth_target            one elementwise pass over [batch, n] rows read and written through their own strides:
//                              the datasets' target preparation (hp_depth_datasets.py:90-107, flat_depth_datasets.py:122-148),
//                              transform_and_normalize and unnormalize_and_retransform (utils/depth_utils.py:60-104, :140-170).
//   hs_depth_stats_update      compute_depth_stats.py's max / min / mean / std (ddof 0) / background count as a streaming
//                              reduction: per-thread shifted sums, Chan merges in a fixed tree per workgroup, then one workgroup
//                              merges the partials, in workgroup order, into the caller's state.  No float atomics: the same
//                              inputs in the same calls give a bit-identical state.
//   hs_histogram_update        the script's np.histogram(all_data, bins): the same per-element value, widened to float64 and counted
//                              against numpy's own edge table; integer counts, integer atomics.
//
// Transcendentals are formed in float64 and rounded once (fp32(log(double x)), fp32(exp(double x)), fp32(1 / double x)): a
// float32 result that does not depend on the math library's float32 accuracy.  The affine steps are float32, unfused, as the
// reference's tensor-with-scalar arithmetic.
#include "hs_histogram.h"

#pragma clang fp contract(off)

#include "hs_depth_target.h"

namespace {

constexpr int kThreads = 256;
constexpr int kStatsBlocksMax = 1024;
constexpr int kHistBlocksMax = 512;  // every workgroup reads the edge table once

// ------------------------------------------------------------------ target transforms
// the per-element rule: hs_depth_target.h (shared with the flat data path's resize kernel)
using hs::target_op;
using hs::TargetOp;

// grid (column blocks, rows): element i of row b at in[b * isb + i * isp]; out may be in itself (same element, same thread)
__global__ void __launch_bounds__(kThreads) depth_target_kernel(const float* in, int64_t isb, int64_t isp, float* out,
                                                                int64_t osb, int64_t osp, int64_t n, TargetOp o) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t b = blockIdx.y;
    out[b * osb + i * osp] = target_op(in[b * isb + i * isp], o);
}

// unit-stride rows whose starts are 16-byte aligned and n % 4 == 0: four elements per lane, one 16-byte load and store
__global__ void __launch_bounds__(kThreads) depth_target_vec4_kernel(const float* in, int64_t isb, float* out, int64_t osb,
                                                                     int64_t n4, TargetOp o) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n4) return;
    const int64_t b = blockIdx.y;
    float4 v = ((const float4*)(in + b * isb))[i];
    v.x = target_op(v.x, o);
    v.y = target_op(v.y, o);
    v.z = target_op(v.z, o);
    v.w = target_op(v.w, o);
    ((float4*)(out + b * osb))[i] = v;
}

// ------------------------------------------------------------------ dataset statistics
// State, HS_DEPTH_STATS_WORDS 8-byte words: int64 counts [0, HS_DSTAT_NCOUNTS), then float64 mean / M2 (sum of squared deviations)
// / min / max of the finite values and the max of the finite foreground values (raw value != 1000).
struct Stats {
    int64_t c[HS_DSTAT_NCOUNTS];
    double mean, m2, mn, mx, fg_mx;
};
static_assert(sizeof(Stats) == HS_DEPTH_STATS_WORDS * 8, "state layout");

__device__ __forceinline__ void stats_zero(Stats& s) {
#pragma unroll
    for (int k = 0; k < HS_DSTAT_NCOUNTS; ++k) s.c[k] = 0;
    s.mean = 0.0;
    s.m2 = 0.0;
    s.mn = INFINITY;
    s.mx = -INFINITY;
    s.fg_mx = -INFINITY;
}

// a <- a (+) b: counts add, extrema combine, (mean, M2) by Chan et al.'s pairwise update
__device__ __forceinline__ void stats_merge(Stats& a, const Stats& b) {
    const int64_t na = a.c[HS_DSTAT_FINITE], nb = b.c[HS_DSTAT_FINITE];
    if (nb > 0) {
        if (na == 0) {
            a.mean = b.mean;
            a.m2 = b.m2;
        } else {
            const double n = (double)(na + nb);
            const double delta = b.mean - a.mean;
            a.mean = a.mean + delta * ((double)nb / n);
            a.m2 = (a.m2 + b.m2) + delta * delta * ((double)na * (double)nb / n);
        }
    }
#pragma unroll
    for (int k = 0; k < HS_DSTAT_NCOUNTS; ++k) a.c[k] += b.c[k];
    a.mn = fmin(a.mn, b.mn);
    a.mx = fmax(a.mx, b.mx);
    a.fg_mx = fmax(a.fg_mx, b.fg_mx);
}

// one raw value into the thread's accumulator: finite values as sums shifted by the thread's first finite value
struct ThreadStats {
    int64_t c[HS_DSTAT_NCOUNTS];
    double shift, s1, s2, mn, mx, fg_mx;
};

// the value the statistics and the histogram take from one raw depth: false if it is dropped (background under masking), else
// x = the fp32 transform
template <int TRANSFORM>
__device__ __forceinline__ bool stats_value(float raw, bool masking, float& x) {
    if (masking && raw == 1000.f) return false;
    x = raw;
    if (TRANSFORM == HS_DT_LOG) x = (float)log((double)raw);
    else if (TRANSFORM == HS_DT_INV) x = (float)(1.0 / (double)raw);  // the script's plain 1 / x
    return true;
}

template <int TRANSFORM>
__device__ __forceinline__ void stats_add(ThreadStats& t, float raw, bool masking) {
    const bool bkg = raw == 1000.f;
    t.c[HS_DSTAT_TOTAL] += 1;
    t.c[HS_DSTAT_BACKGROUND] += bkg;
    float x;
    if (!stats_value<TRANSFORM>(raw, masking, x)) return;
    t.c[HS_DSTAT_VALUES] += 1;
    t.c[HS_DSTAT_FG_VALUES] += !bkg;
    if (isnan(x)) {
        t.c[HS_DSTAT_NAN] += 1;
        t.c[HS_DSTAT_FG_NAN] += !bkg;
    } else if (x == INFINITY) {
        t.c[HS_DSTAT_POSINF] += 1;
        t.c[HS_DSTAT_FG_POSINF] += !bkg;
    } else if (x == -INFINITY) {
        t.c[HS_DSTAT_NEGINF] += 1;
    } else {
        const double d = (double)x;
        if (t.c[HS_DSTAT_FINITE] == 0) t.shift = d;
        t.c[HS_DSTAT_FINITE] += 1;
        const double e = d - t.shift;
        t.s1 += e;
        t.s2 += e * e;
        t.mn = fmin(t.mn, d);
        t.mx = fmax(t.mx, d);
        if (!bkg) t.fg_mx = fmax(t.fg_mx, d);
    }
}

__device__ __forceinline__ void block_merge(Stats& s, Stats* lds) {
    lds[threadIdx.x] = s;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) stats_merge(lds[threadIdx.x], lds[threadIdx.x + h]);
        __syncthreads();
    }
    s = lds[0];
}

template <int TRANSFORM>
__global__ void __launch_bounds__(kThreads) depth_stats_kernel(const float* __restrict__ x, int64_t n, int vec4, int masking,
                                                               Stats* __restrict__ partial) {
    __shared__ Stats lds[kThreads];
    ThreadStats t;
#pragma unroll
    for (int k = 0; k < HS_DSTAT_NCOUNTS; ++k) t.c[k] = 0;
    t.shift = t.s1 = t.s2 = 0.0;
    t.mn = INFINITY;
    t.mx = t.fg_mx = -INFINITY;
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
    int64_t done = 0;
    if (vec4) {
        const int64_t n4 = n / 4;
        for (int64_t i = tid; i < n4; i += stride) {
            const float4 v = ((const float4*)x)[i];
            stats_add<TRANSFORM>(t, v.x, masking);
            stats_add<TRANSFORM>(t, v.y, masking);
            stats_add<TRANSFORM>(t, v.z, masking);
            stats_add<TRANSFORM>(t, v.w, masking);
        }
        done = n4 * 4;
    }
    for (int64_t i = done + tid; i < n; i += stride) stats_add<TRANSFORM>(t, x[i], masking);
    Stats s;
#pragma unroll
    for (int k = 0; k < HS_DSTAT_NCOUNTS; ++k) s.c[k] = t.c[k];
    const int64_t nf = t.c[HS_DSTAT_FINITE];
    s.mean = nf ? t.shift + t.s1 / (double)nf : 0.0;
    s.m2 = nf ? fmax(t.s2 - t.s1 * (t.s1 / (double)nf), 0.0) : 0.0;
    s.mn = t.mn;
    s.mx = t.mx;
    s.fg_mx = t.fg_mx;
    block_merge(s, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one workgroup: thread j merges partials j, j + 256, ... in order, the fixed tree merges the threads, thread 0 adds the result to
// the state.  states == partials of one call, or the gathered states of several ranks (count of them, merged in that order).
__global__ void __launch_bounds__(kThreads) depth_stats_merge_kernel(const Stats* __restrict__ parts, int count, Stats* __restrict__ state) {
    __shared__ Stats lds[kThreads];
    Stats s;
    stats_zero(s);
    for (int j = threadIdx.x; j < count; j += kThreads) stats_merge(s, parts[j]);
    block_merge(s, lds);
    if (threadIdx.x == 0) {
        Stats a = *state;
        stats_merge(a, s);
        *state = a;
    }
}

// ------------------------------------------------------------------ histogram
// np.histogram over given edges: uint32 counters and the float64 edge table in LDS, merged into the int64 state with integer
// atomics.  Every lane runs every iteration (wave_count needs the whole wave); a lane without a value carries live = false.
template <int TRANSFORM>
__global__ void __launch_bounds__(kThreads) depth_histogram_kernel(const float* __restrict__ x, int64_t n, int vec4, int masking,
                                                                   const double* __restrict__ edges, int bins,
                                                                   unsigned long long* __restrict__ counts) {
    __shared__ uint32_t hist[HS_HISTOGRAM_MAX_BINS];
    __shared__ double edge[HS_HISTOGRAM_MAX_BINS + 1];
    for (int j = threadIdx.x; j < bins; j += kThreads) hist[j] = 0;
    for (int j = threadIdx.x; j <= bins; j += kThreads) edge[j] = edges[j];
    __syncthreads();
    const double lo = edge[0], hi = edge[bins], scale = (double)bins / (hi - lo);
    auto add = [&](bool valid, float raw) {
        float xf = 0.f;
        bool live = valid && stats_value<TRANSFORM>(raw, masking, xf);
        const double v = (double)xf;
        live = live && v >= lo && v <= hi;  // NaN, +-inf and values outside the range are dropped
        int i = 0;
        if (live) {
            i = (int)((v - lo) * scale);  // an estimate only: the table decides
            i = i < 0 ? 0 : i > bins - 1 ? bins - 1 : i;
            while (i > 0 && v < edge[i]) --i;
            while (i < bins - 1 && v >= edge[i + 1]) ++i;
        }
        hs::wave_count(hist, live, (uint32_t)i);
    };
    const int64_t first = (int64_t)blockIdx.x * kThreads, stride = (int64_t)gridDim.x * kThreads;
    int64_t done = 0;
    if (vec4) {
        const int64_t n4 = n / 4;
        for (int64_t base = first; base < n4; base += stride) {
            const bool valid = base + threadIdx.x < n4;
            const float4 v = valid ? ((const float4*)x)[base + threadIdx.x] : make_float4(0.f, 0.f, 0.f, 0.f);
            add(valid, v.x);
            add(valid, v.y);
            add(valid, v.z);
            add(valid, v.w);
        }
        done = n4 * 4;
    }
    for (int64_t base = done + first; base < n; base += stride) {
        const bool valid = base + threadIdx.x < n;
        add(valid, valid ? x[base + threadIdx.x] : 0.f);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < bins; j += kThreads)
        if (hist[j] != 0) atomicAdd(&counts[j], (unsigned long long)hist[j]);
}

}  // namespace

extern "C" {

int hs_depth_target(const float* in, int64_t in_stride_b, int64_t in_stride_p, float* out, int64_t out_stride_b, int64_t out_stride_p,
                    int64_t batch, int64_t n, int flags, int transform, float shift, float scale, void* stream) {
    HS_CHECK_ARG(batch >= 0 && batch <= 65535 && n >= 0, "bad shape (batch <= 65535)");
    HS_CHECK_ARG((flags & ~(HS_DT_ZERO_BKG | HS_DT_1000_BKG | HS_DT_AFFINE | HS_DT_INVERSE)) == 0, "unknown flags %d", flags);
    HS_CHECK_ARG(!((flags & HS_DT_INVERSE) && (flags & (HS_DT_ZERO_BKG | HS_DT_1000_BKG))), "background flags are forward only");
    HS_CHECK_ARG(transform == HS_DT_NONE || transform == HS_DT_LOG || transform == HS_DT_INV, "transform %d", transform);
    HS_CHECK_ARG(in_stride_b >= 0 && in_stride_p >= 0 && out_stride_b >= 0 && out_stride_p >= 0, "negative strides");
    if (batch == 0 || n == 0) return HS_OK;
    HS_CHECK_ARG(in && out, "null pointer");
    const TargetOp o{flags, transform, shift, scale};
    hipStream_t s = (hipStream_t)stream;
    const bool vec = in_stride_p == 1 && out_stride_p == 1 && n % 4 == 0 && in_stride_b % 4 == 0 && out_stride_b % 4 == 0 &&
                     (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
    if (vec) {
        const int64_t n4 = n / 4;
        hipLaunchKernelGGL(depth_target_vec4_kernel, dim3((unsigned)((n4 + kThreads - 1) / kThreads), (unsigned)batch), dim3(kThreads), 0,
                           s, in, in_stride_b, out, out_stride_b, n4, o);
    } else {
        hipLaunchKernelGGL(depth_target_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads), (unsigned)batch), dim3(kThreads), 0, s,
                           in, in_stride_b, in_stride_p, out, out_stride_b, out_stride_p, n, o);
    }
    HS_LAUNCH_CHECK("depth_target");
    return HS_OK;
}

int64_t hs_depth_stats_partials(int64_t n) {
    const int64_t blocks = (n + kThreads * 16 - 1) / (kThreads * 16);
    return std::max<int64_t>(1, std::min<int64_t>(blocks, kStatsBlocksMax));
}

int hs_depth_stats_update(const float* depth, int64_t n, int transform, int use_masking, int64_t* partial, int64_t* state, void* stream) {
    HS_CHECK_ARG(n >= 0, "bad size");
    HS_CHECK_ARG(transform == HS_DT_NONE || transform == HS_DT_LOG || transform == HS_DT_INV, "transform %d", transform);
    if (n == 0) return HS_OK;
    HS_CHECK_ARG(depth && partial && state, "null pointer");
    const int blocks = (int)hs_depth_stats_partials(n);
    const int vec4 = (uintptr_t)depth % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks), block(kThreads);
    Stats* parts = (Stats*)partial;
    if (transform == HS_DT_LOG)
        hipLaunchKernelGGL(depth_stats_kernel<HS_DT_LOG>, grid, block, 0, s, depth, n, vec4, use_masking, parts);
    else if (transform == HS_DT_INV)
        hipLaunchKernelGGL(depth_stats_kernel<HS_DT_INV>, grid, block, 0, s, depth, n, vec4, use_masking, parts);
    else
        hipLaunchKernelGGL(depth_stats_kernel<HS_DT_NONE>, grid, block, 0, s, depth, n, vec4, use_masking, parts);
    HS_LAUNCH_CHECK("depth_stats");
    hipLaunchKernelGGL(depth_stats_merge_kernel, dim3(1), block, 0, s, (const Stats*)parts, blocks, (Stats*)state);
    HS_LAUNCH_CHECK("depth_stats_merge");
    return HS_OK;
}

int hs_depth_stats_merge(const int64_t* states, int count, int64_t* state, void* stream) {
    HS_CHECK_ARG(count >= 0, "bad count");
    if (count == 0) return HS_OK;
    HS_CHECK_ARG(states && state, "null pointer");
    hipLaunchKernelGGL(depth_stats_merge_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const Stats*)states, count,
                       (Stats*)state);
    HS_LAUNCH_CHECK("depth_stats_merge");
    return HS_OK;
}

int hs_histogram_update(const float* depth, int64_t n, int transform, int use_masking, const double* edges, int bins, int64_t* counts,
                        void* stream) {
    HS_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 40), "hs_histogram_update: bad size");
    HS_CHECK_ARG(transform == HS_DT_NONE || transform == HS_DT_LOG || transform == HS_DT_INV, "hs_histogram_update: transform %d",
                 transform);
    HS_CHECK_ARG(bins >= 1 && bins <= HS_HISTOGRAM_MAX_BINS, "hs_histogram_update: bins %d outside [1, %d]", bins, HS_HISTOGRAM_MAX_BINS);
    if (n == 0) return HS_OK;
    HS_CHECK_ARG(depth && edges && counts, "hs_histogram_update: null pointer");
    const int64_t want = (n + kThreads * 16 - 1) / (kThreads * 16);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(want, kHistBlocksMax))), block(kThreads);
    const int vec4 = (uintptr_t)depth % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* c = (unsigned long long*)counts;
    if (transform == HS_DT_LOG)
        hipLaunchKernelGGL(depth_histogram_kernel<HS_DT_LOG>, grid, block, 0, s, depth, n, vec4, use_masking, edges, bins, c);
    else if (transform == HS_DT_INV)
        hipLaunchKernelGGL(depth_histogram_kernel<HS_DT_INV>, grid, block, 0, s, depth, n, vec4, use_masking, edges, bins, c);
    else
        hipLaunchKernelGGL(depth_histogram_kernel<HS_DT_NONE>, grid, block, 0, s, depth, n, vec4, use_masking, edges, bins, c);
    HS_LAUNCH_CHECK("depth_histogram");
    return HS_OK;
}

}  // extern "C"
