// Evaluation of depth predictions (heal_swin_amd/depth_evaluation.py): point clouds, exact Chamfer nearest neighbours, the
// depth error metrics.  (The float back-projection onto the image plane, hs_backproject_depth, is csrc/evaluation.hip's: one
// four-tap kernel with hs_backproject_image.)
//
//   hs_depth_points        create_point_cloud_from_depth_mask (heal_swin/utils/depth_utils.py:465-539) with the kept set of
//                          ChamferDistance.update (evaluation/custom_metrics.py:539-561): point = fp32(d * dir), dir the float64
//                          unit direction already rotated by the extrinsic rotation (a host table).  Compaction in pixel order by
//                          per-block counts, one exclusive scan and the writes: no appended output, deterministic.
//   hs_chamfer_nn          the chamfer_distance extension's nearest neighbours (custom_metrics.py:569): squared fp32 distances
//                          from coordinate differences, exact brute force, lowest index on ties, both directions.
//   hs_depth_metrics       one pass over pred[:, 0] (and pred[:, 1]) and the target producing every sum of DepthMSE, RelSE/AE,
//                          iRMSE, SILogE, DepthRangeMSE, MeanSTD and MeanPredDist (custom_metrics.py:62-468) as fp64 per-workgroup
//                          partials, then a fixed-order reduction added into the caller's fp64 state.  No float atomics.
//
// Chamfer design.  One pass per direction: a workgroup holds kQ = 8 query points per lane in registers (2048 per workgroup) and
// streams the target cloud through LDS in tiles of kTile points (structure of arrays, so one 16-byte broadcast read gives four
// targets' x); a pair costs dx*dx + fma(dy, dy) + fma(dz, dz) after three subtractions and half a v_min3_f32.  The column-min of
// the same pass (the other direction) would need a cross-lane reduction per target and tile, as costly as the row work itself,
// so the other direction is a second pass with the roles swapped.  The target range of a sample is split across workgroups (grid.y)
// when the queries alone do not fill the chip; every split merges its per-query result into a packed 64-bit word
// (float bits << 32 | index) with a vector atomicMin.  Distances are >= 0, so the integer order is the float order, equal
// distances keep the lowest index, and the result does not depend on arrival order or on the split count.  Indices: the
// distance-only loop also remembers the first tile where each query's minimum improved; afterwards that one tile is rescanned
// from global memory for the first target at the minimum, so indices cost one extra tile per query, not a compare-select per pair.
#include <algorithm>

#include "hs_sphere_args.h"

#pragma clang fp contract(off)

#include "hs_depth_metrics.h"

namespace hs {
namespace {

using depth_metrics::block_sum;

constexpr int kThreads = 256;
constexpr int kPtsPer = 8;                     // pixels per lane in the compaction kernels
constexpr int kPtsChunk = kThreads * kPtsPer;  // pixels per compaction workgroup
constexpr int kQ = 8;                          // query points per lane in the Chamfer pass
constexpr int kTile = 512;                     // target points per LDS tile
constexpr int kMaxBg = 4;

// ------------------------------------------------------------------ point clouds
struct DepthIn {
    const void* p;
    int kind;  // HS_F32 / HS_BF16
    int64_t sb, sh, sw, width;
};

__device__ __forceinline__ float load_depth(const DepthIn& d, int64_t b, int64_t i) {
    const int64_t h = i / d.width, w = i - h * d.width;
    const int64_t off = b * d.sb + h * d.sh + w * d.sw;
    return load_val<float>(d.p, d.kind, off);
}

struct KeepRule {
    const uint8_t* fg;  // optional foreground [b * fg_sb + i], nonzero = keep
    int64_t fg_sb;
    int n_bg;
    float bg[kMaxBg];  // further background depths (finite; NaN and +-inf are always dropped)
};

__device__ __forceinline__ bool keep_point(const KeepRule& k, float d, int64_t b, int64_t i) {
    if (!isfinite(d)) return false;  // the reference's "sum of x, y, z is not NaN / inf"
    for (int m = 0; m < k.n_bg; ++m)
        if (d == k.bg[m]) return false;
    return !k.fg || k.fg[b * k.fg_sb + i] != 0;
}

// exclusive rank of this lane's flag among the workgroup's lanes (lane order), and the workgroup's total
__device__ __forceinline__ int block_rank(bool flag, int* wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int in_wave = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
        before += w < wave ? wave_tot[w] : 0;
        total += wave_tot[w];
    }
    return before + in_wave;
}

__global__ void __launch_bounds__(kThreads) points_count_kernel(DepthIn d, KeepRule k, int64_t n, int nblk, int32_t* __restrict__ counts) {
    __shared__ int wave_tot[kThreads / 64];
    const int64_t b = blockIdx.y;
    int c = 0;
    for (int r = 0; r < kPtsPer; ++r) {
        const int64_t i = (int64_t)blockIdx.x * kPtsChunk + r * kThreads + threadIdx.x;
        c += i < n && keep_point(k, load_depth(d, b, i), b, i);
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kThreads / 64; ++w) t += wave_tot[w];
        counts[b * nblk + blockIdx.x] = t;
    }
}

// one workgroup: exclusive scan of counts[batch * nblk] (sample-major) into starts; offsets[b] = start of sample b, offsets[batch] = total
__global__ void __launch_bounds__(1024) points_scan_kernel(const int32_t* __restrict__ counts, int64_t total_blocks, int nblk, int64_t batch,
                                                           int64_t* __restrict__ starts, int64_t* __restrict__ offsets) {
    __shared__ int64_t wave_tot[16];
    __shared__ int64_t carry_lds;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < total_blocks; base += 1024) {
        const int64_t j = base + threadIdx.x;
        const int64_t v = j < total_blocks ? counts[j] : 0;
        int64_t incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int64_t before = carry;
        for (int w = 0; w < wave; ++w) before += wave_tot[w];
        const int64_t excl = before + incl - v;
        if (j < total_blocks) {
            starts[j] = excl;
            if (j % nblk == 0) offsets[j / nblk] = excl;
        }
        if (threadIdx.x == 1023) carry_lds = excl + v;
        __syncthreads();
        carry = carry_lds;
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[batch] = carry;
}

__global__ void __launch_bounds__(kThreads) points_write_kernel(DepthIn d, KeepRule k, int64_t n, int nblk, const double* __restrict__ dir,
                                                                const int64_t* __restrict__ starts, float* __restrict__ out) {
    __shared__ int wave_tot[kThreads / 64];
    const int64_t b = blockIdx.y;
    int64_t pos = starts[b * nblk + blockIdx.x];
    for (int r = 0; r < kPtsPer; ++r) {
        const int64_t i = (int64_t)blockIdx.x * kPtsChunk + r * kThreads + threadIdx.x;
        float dv = 0.f;
        bool keep = false;
        if (i < n) {
            dv = load_depth(d, b, i);
            keep = keep_point(k, dv, b, i);
        }
        int total;
        const int rank = block_rank(keep, wave_tot, total);
        if (keep) {
            const double dd = (double)dv;
            float* o = out + (pos + rank) * 3;
            o[0] = (float)(dd * dir[i]);
            o[1] = (float)(dd * dir[n + i]);
            o[2] = (float)(dd * dir[2 * n + i]);
        }
        pos += total;
    }
}

// ------------------------------------------------------------------ Chamfer nearest neighbours
__device__ __forceinline__ float sqdist(float qx, float qy, float qz, float tx, float ty, float tz) {
    const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
    float s = dx * dx;
    s = fmaf(dy, dy, s);
    return fmaf(dz, dz, s);
}

// queries: cloud q (rows q_off[s] .. q_off[s+1]), targets: cloud t.  grid (query blocks, splits, samples).
template <bool Idx>
__global__ void __launch_bounds__(kThreads) chamfer_pass_kernel(const float* __restrict__ q, const int64_t* __restrict__ q_off,
                                                                const float* __restrict__ t, const int64_t* __restrict__ t_off,
                                                                int nsplit, unsigned long long* __restrict__ best) {
    __shared__ float4 lx[kTile / 4], ly[kTile / 4], lz[kTile / 4];
    const int s = blockIdx.z;
    const int64_t q0 = q_off[s], nq = q_off[s + 1] - q0;
    const int64_t t0 = t_off[s], nt = t_off[s + 1] - t0;
    const int64_t first = (int64_t)blockIdx.x * (kThreads * kQ);
    if (first >= nq || nt <= 0) return;  // uniform over the workgroup
    const int64_t ntiles = (nt + kTile - 1) / kTile;
    const int64_t per = (ntiles + nsplit - 1) / nsplit;
    const int64_t tile_lo = (int64_t)blockIdx.y * per, tile_hi = ntiles < tile_lo + per ? ntiles : tile_lo + per;
    if (tile_lo >= tile_hi) return;

    float qx[kQ], qy[kQ], qz[kQ], m[kQ];
    int mt[kQ];
#pragma unroll
    for (int r = 0; r < kQ; ++r) {
        const int64_t i = first + r * kThreads + threadIdx.x;
        const float* p = q + (q0 + (i < nq ? i : 0)) * 3;
        qx[r] = p[0];
        qy[r] = p[1];
        qz[r] = p[2];
        m[r] = INFINITY;
        mt[r] = (int)tile_lo;
    }
    constexpr int kLoads = kTile / kThreads;
    float px[kLoads], py[kLoads], pz[kLoads];
    auto fetch = [&](int64_t tile) {
#pragma unroll
        for (int l = 0; l < kLoads; ++l) {
            const int64_t j = tile * kTile + l * kThreads + threadIdx.x;
            if (j < nt) {
                const float* p = t + (t0 + j) * 3;
                px[l] = p[0];
                py[l] = p[1];
                pz[l] = p[2];
            } else {  // padding: infinitely far, never the minimum of a finite query
                px[l] = py[l] = pz[l] = INFINITY;
            }
        }
    };
    fetch(tile_lo);
    for (int64_t tile = tile_lo; tile < tile_hi; ++tile) {
        __syncthreads();
#pragma unroll
        for (int l = 0; l < kLoads; ++l) {
            ((float*)lx)[l * kThreads + threadIdx.x] = px[l];
            ((float*)ly)[l * kThreads + threadIdx.x] = py[l];
            ((float*)lz)[l * kThreads + threadIdx.x] = pz[l];
        }
        __syncthreads();
        if (tile + 1 < tile_hi) fetch(tile + 1);
        float tm[kQ];
#pragma unroll
        for (int r = 0; r < kQ; ++r) tm[r] = Idx ? INFINITY : m[r];
#pragma unroll 2
        for (int k = 0; k < kTile / 4; ++k) {
            const float4 x = lx[k], y = ly[k], z = lz[k];
#pragma unroll
            for (int r = 0; r < kQ; ++r) {
                const float d0 = sqdist(qx[r], qy[r], qz[r], x.x, y.x, z.x);
                const float d1 = sqdist(qx[r], qy[r], qz[r], x.y, y.y, z.y);
                const float d2 = sqdist(qx[r], qy[r], qz[r], x.z, y.z, z.z);
                const float d3 = sqdist(qx[r], qy[r], qz[r], x.w, y.w, z.w);
                tm[r] = __builtin_fminf(__builtin_fminf(tm[r], d0), d1);
                tm[r] = __builtin_fminf(__builtin_fminf(tm[r], d2), d3);
            }
        }
#pragma unroll
        for (int r = 0; r < kQ; ++r) {
            if (Idx) {
                if (tm[r] < m[r]) {  // strict: the first tile reaching the minimum is kept
                    m[r] = tm[r];
                    mt[r] = (int)tile;
                }
            } else {
                m[r] = tm[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kQ; ++r) {
        const int64_t i = first + r * kThreads + threadIdx.x;
        if (i >= nq) continue;
        uint32_t arg = 0;
        if (Idx) {
            const int64_t j1 = nt < ((int64_t)mt[r] + 1) * kTile ? nt : ((int64_t)mt[r] + 1) * kTile;
            for (int64_t j = (int64_t)mt[r] * kTile; j < j1; ++j) {
                const float* p = t + (t0 + j) * 3;
                if (sqdist(qx[r], qy[r], qz[r], p[0], p[1], p[2]) == m[r]) {
                    arg = (uint32_t)j;
                    break;
                }
            }
        }
        atomicMin(&best[q0 + i], ((unsigned long long)__float_as_uint(m[r]) << 32) | arg);
    }
}

// packed words -> distances / indices; rows whose other cloud is empty (or past the last cloud) were never written: NaN, -1
__global__ void __launch_bounds__(kThreads) chamfer_unpack_kernel(const unsigned long long* __restrict__ best, int64_t n, float* __restrict__ dist,
                                                                  int64_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned long long w = best[i];
    const bool set = w != ~0ull;
    dist[i] = set ? __uint_as_float((uint32_t)(w >> 32)) : NAN;
    if (idx) idx[i] = set ? (int64_t)(uint32_t)w : -1;
}

// one workgroup per sample: term[s] = mean(dist_a) + mean(dist_b) in float64 (NaN when a cloud is empty: 0 / 0)
__global__ void __launch_bounds__(kThreads) chamfer_term_kernel(const float* __restrict__ da, const int64_t* __restrict__ a_off,
                                                                const float* __restrict__ db, const int64_t* __restrict__ b_off,
                                                                double* __restrict__ term) {
    __shared__ double lds[kThreads];
    const int s = blockIdx.x;
    double sa = 0.0, sb = 0.0;
    const int64_t a0 = a_off[s], a1 = a_off[s + 1], b0 = b_off[s], b1 = b_off[s + 1];
    for (int64_t i = a0 + threadIdx.x; i < a1; i += kThreads) sa += (double)da[i];
    for (int64_t i = b0 + threadIdx.x; i < b1; i += kThreads) sb += (double)db[i];
    sa = block_sum(sa, lds);
    sb = block_sum(sb, lds);
    if (threadIdx.x == 0) term[s] = sa / (double)(a1 - a0) + sb / (double)(b1 - b0);
}

// ------------------------------------------------------------------ depth metrics
struct MetricIn {
    const void* pred;
    int kind;  // HS_F32 / HS_BF16 / HS_F64
    int64_t sb, sc, sh, sw;
    const void* target;
    int tkind;
    int64_t tb, th, tw;
    int64_t width, n, batch;
    depth_metrics::Rule rule;
};

// P, T: the types the reference computes in for the prediction and the target (hs_depth_metrics.h holds the per-element rules)
template <typename P, typename T>
__global__ void __launch_bounds__(kThreads) depth_metrics_kernel(MetricIn a, double* __restrict__ partial) {
    depth_metrics::metric_pass(a.rule, a.n, a.batch, partial, [&a](int64_t b, int64_t i) {
        const int64_t h = i / a.width, w = i - h * a.width;
        const int64_t po = b * a.sb + h * a.sh + w * a.sw;
        return std::make_tuple(load_val<P, true>(a.pred, a.kind, po), load_val<T, true>(a.target, a.tkind, b * a.tb + h * a.th + w * a.tw),
                               [&a, po] { return load_val<P, true>(a.pred, a.kind, po + a.sc); });
    });
}

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

int64_t hs_depth_points_workspace(int64_t batch, int64_t n) {
    if (batch <= 0 || n <= 0) return 0;
    const int64_t nblk = (n + kPtsChunk - 1) / kPtsChunk;
    return batch * nblk * (int64_t)(sizeof(int32_t) + sizeof(int64_t));
}

int hs_depth_points(const void* depth, int kind, int64_t batch, int64_t n, int64_t width, int64_t stride_b, int64_t stride_h,
                    int64_t stride_w, const uint8_t* foreground, int64_t fg_stride_b, const float* background, int n_background,
                    const double* dir, void* workspace, float* points, int64_t* offsets, void* stream) {
    if (int st = sphere::check_float_kind("hs_depth_points", "depth", kind)) return st;
    HS_CHECK_ARG(batch > 0 && batch <= 65535 && n > 0 && n < (1ll << 31) && width > 0 && n % width == 0,
                 "bad shape (batch %lld, n %lld, width %lld)", (long long)batch, (long long)n, (long long)width);
    HS_CHECK_ARG(n_background >= 0 && n_background <= kMaxBg && (n_background == 0 || background), "at most %d background values",
                 kMaxBg);
    HS_CHECK_ARG(depth && dir && workspace && points && offsets, "null pointer");
    const int nblk = (int)((n + kPtsChunk - 1) / kPtsChunk);
    const DepthIn d{depth, kind, stride_b, stride_h, stride_w, width};
    KeepRule k{foreground, fg_stride_b, n_background, {0.f, 0.f, 0.f, 0.f}};
    for (int m = 0; m < n_background; ++m) k.bg[m] = background[m];
    auto* starts = (int64_t*)workspace;
    auto* counts = (int32_t*)(starts + batch * nblk);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk, (unsigned)batch);
    hipLaunchKernelGGL(points_count_kernel, grid, dim3(kThreads), 0, s, d, k, n, nblk, counts);
    HS_LAUNCH_CHECK("depth_points_count");
    hipLaunchKernelGGL(points_scan_kernel, dim3(1), dim3(1024), 0, s, counts, batch * nblk, nblk, batch, starts, offsets);
    HS_LAUNCH_CHECK("depth_points_scan");
    hipLaunchKernelGGL(points_write_kernel, grid, dim3(kThreads), 0, s, d, k, n, nblk, dir, starts, points);
    HS_LAUNCH_CHECK("depth_points_write");
    return HS_OK;
}

int hs_chamfer_nn(const float* a, const int64_t* a_off, int64_t a_rows, int64_t a_max, const float* b, const int64_t* b_off,
                  int64_t b_rows, int64_t b_max, int64_t batch, int splits, void* workspace, float* dist_a, float* dist_b,
                  int64_t* idx_a, int64_t* idx_b, double* term, void* stream) {
    HS_CHECK_ARG(batch > 0 && batch <= 65535, "batch %lld out of range", (long long)batch);
    HS_CHECK_ARG(a_rows >= 0 && b_rows >= 0 && a_rows < (1ll << 32) && b_rows < (1ll << 32), "clouds of up to 2^32 points");
    HS_CHECK_ARG(a_max >= 0 && a_max <= a_rows && b_max >= 0 && b_max <= b_rows, "bad per-sample bounds");
    HS_CHECK_ARG(splits >= 0 && splits <= 4096, "splits must be in [0, 4096] (0: automatic)");
    HS_CHECK_ARG((idx_a == nullptr) == (idx_b == nullptr), "indices are returned for both directions or neither");
    HS_CHECK_ARG(a_off && b_off && workspace && dist_a && dist_b && (a_rows == 0 || a) && (b_rows == 0 || b), "null pointer");
    hipStream_t s = (hipStream_t)stream;
    auto* best_a = (unsigned long long*)workspace;
    auto* best_b = best_a + a_rows;
    if (a_rows + b_rows) HS_HIP_CHECK(hipMemsetAsync(best_a, 0xff, (size_t)(a_rows + b_rows) * 8, s));
    const int64_t per_block = (int64_t)kThreads * kQ;
    const bool want_idx = idx_a != nullptr;
    // one direction: queries q (bound q_max per sample) against targets t (bound t_max)
    auto pass = [&](const float* q, const int64_t* q_off, int64_t q_max, const float* t, const int64_t* t_off, int64_t t_max,
                    unsigned long long* best) -> int {
        if (q_max == 0 || t_max == 0) return HS_OK;
        const int64_t qblocks = (q_max + per_block - 1) / per_block;
        int ns = splits;
        if (ns == 0) {  // fill about 2048 workgroups, keeping at least 4 tiles per split
            const int64_t want = (2048 + qblocks * batch - 1) / (qblocks * batch);
            const int64_t cap = std::max<int64_t>(1, (t_max + 4 * kTile - 1) / (4 * kTile));
            ns = (int)std::min<int64_t>(std::min<int64_t>(want, cap), 4096);
        }
        HS_CHECK_ARG(qblocks < (1ll << 31), "too many query blocks");
        const dim3 grid((unsigned)qblocks, (unsigned)ns, (unsigned)batch);
        if (want_idx)
            hipLaunchKernelGGL(chamfer_pass_kernel<true>, grid, dim3(kThreads), 0, s, q, q_off, t, t_off, ns, best);
        else
            hipLaunchKernelGGL(chamfer_pass_kernel<false>, grid, dim3(kThreads), 0, s, q, q_off, t, t_off, ns, best);
        HS_LAUNCH_CHECK("chamfer_pass");
        return HS_OK;
    };
    if (int st = pass(a, a_off, a_max, b, b_off, b_max, best_a)) return st;
    if (int st = pass(b, b_off, b_max, a, a_off, a_max, best_b)) return st;
    if (a_rows) {
        hipLaunchKernelGGL(chamfer_unpack_kernel, dim3((unsigned)((a_rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, best_a, a_rows,
                           dist_a, idx_a);
        HS_LAUNCH_CHECK("chamfer_unpack");
    }
    if (b_rows) {
        hipLaunchKernelGGL(chamfer_unpack_kernel, dim3((unsigned)((b_rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, best_b, b_rows,
                           dist_b, idx_b);
        HS_LAUNCH_CHECK("chamfer_unpack");
    }
    if (term) {
        hipLaunchKernelGGL(chamfer_term_kernel, dim3((unsigned)batch), dim3(kThreads), 0, s, dist_a, a_off, dist_b, b_off, term);
        HS_LAUNCH_CHECK("chamfer_term");
    }
    return HS_OK;
}

int64_t hs_depth_metrics_partials(int64_t total) { return depth_metrics::blocks_for(total); }

int hs_depth_metrics(const void* pred, int pred_kind, int64_t batch, int64_t n, int64_t width, int64_t stride_b, int64_t stride_c,
                     int64_t stride_h, int64_t stride_w, const void* target, int target_kind, int64_t t_stride_b, int64_t t_stride_h,
                     int64_t t_stride_w, int use_logvar, double total_mean, const float* ranges, int n_ranges, double* partial,
                     double* state, void* stream) {
    HS_CHECK_ARG(pred_kind == HS_F32 || pred_kind == HS_BF16 || pred_kind == HS_F64, "prediction kind %d", pred_kind);
    HS_CHECK_ARG(target_kind == HS_F32 || target_kind == HS_BF16 || target_kind == HS_F64, "target kind %d", target_kind);
    HS_CHECK_ARG(batch > 0 && n > 0 && width > 0 && n % width == 0, "bad shape");
    depth_metrics::Rule rule;
    if (int st = depth_metrics::fill_rule(rule, use_logvar, total_mean, ranges, n_ranges)) return st;
    HS_CHECK_ARG(pred && target && partial && state, "null pointer");
    const MetricIn a{pred, pred_kind, stride_b, stride_c, stride_h, stride_w, target, target_kind, t_stride_b, t_stride_h, t_stride_w,
                     width, n, batch, rule};
    hipStream_t s = (hipStream_t)stream;
    return depth_metrics::run_pass(n * batch, partial, state, s, [&](dim3 grid, dim3 block) {
        if (pred_kind == HS_F64 && target_kind == HS_F64)
            hipLaunchKernelGGL((depth_metrics_kernel<double, double>), grid, block, 0, s, a, partial);
        else if (pred_kind == HS_F64)
            hipLaunchKernelGGL((depth_metrics_kernel<double, float>), grid, block, 0, s, a, partial);
        else if (target_kind == HS_F64)
            hipLaunchKernelGGL((depth_metrics_kernel<float, double>), grid, block, 0, s, a, partial);
        else
            hipLaunchKernelGGL((depth_metrics_kernel<float, float>), grid, block, 0, s, a, partial);
    });
}

}  // extern "C"
