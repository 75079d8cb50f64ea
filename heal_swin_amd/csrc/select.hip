// hs_select_rows: the k-th smallest element of every row of an fp32 matrix, exactly, without sorting (heal_swin_amd/order_stats.py;
// MeanSTDMedian's torch.median in depth_evaluation.py).
//
// Radix select on the order-preserving 32-bit key of a float, most significant digit first, four 8-bit digits.  One launch per
// digit, grid (splits, rows), and one that writes the result:
//   pass p   every workgroup finds the prefix (the p digits already fixed) and the rank left inside it from the bins of passes
//            0 .. p - 1 of its row, counts digit p of its share of the row's elements that match the prefix into 256 LDS counters,
//            and adds its non-empty counters into bins[p][row] with integer atomics.
//   write    one workgroup per row finds the fourth digit the same way; the key is complete.
// Integer adds commute: the bins, and so the result, do not depend on `splits` or on the order in which workgroups arrive.
// Workspace: uint32 bins[4][rows][256], then uint32 nans[rows] (the NaN count of a row, for nan_propagates).
#include <algorithm>

#include "hs_histogram.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBins = 256;
constexpr int kPasses = 4;
constexpr int64_t kChunk = 4096;      // elements a workgroup takes at least before a row is split further (auto splits)
constexpr int kAutoWorkgroups = 1024;  // ... and the grid an automatic split aims at: four workgroups per compute unit

// torch.sort's order as an unsigned compare: -inf < finite < +inf < NaN, every NaN (either sign) last
__device__ __forceinline__ uint32_t float_key(float v) {
    const uint32_t b = __float_as_uint(v);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    return b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t key) {
    if (key == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}

struct Scratch {
    uint32_t wave_total[kThreads / 64];
    uint32_t digit, rank;
};

// (prefix, rank) after `passes` digits: thread t holds bin t of each pass, a workgroup scan finds the bin the rank falls into
__device__ __forceinline__ void find_prefix(const uint32_t* __restrict__ bins, int rows, int row, int passes, uint32_t k, Scratch& s,
                                            uint32_t& prefix, uint32_t& rank) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    prefix = 0;
    rank = k;
    for (int p = 0; p < passes; ++p) {
        const uint32_t c = bins[((int64_t)p * rows + row) * kBins + t];
        uint32_t inc = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(inc, off, 64);
            if (lane >= off) inc += up;
        }
        if (lane == 63) s.wave_total[wave] = inc;
        __syncthreads();
        uint32_t before = inc - c;
        for (int w = 0; w < wave; ++w) before += s.wave_total[w];
        if (c != 0 && rank >= before && rank - before < c) {  // exactly one bin: the counts of a pass sum to more than the rank
            s.digit = (uint32_t)t;
            s.rank = rank - before;
        }
        __syncthreads();
        prefix = (prefix << 8) | s.digit;
        rank = s.rank;
        __syncthreads();
    }
}

struct Counter {
    uint32_t* hist;
    uint32_t prefix;
    int pass;
    uint32_t nans;
    __device__ __forceinline__ void add(bool valid, float v) {
        const uint32_t key = float_key(v);
        nans += valid && key == 0xFFFFFFFFu;
        const int shift = 24 - 8 * pass;
        // the digits above this pass's equal the prefix (pass 0: none; a 32-bit shift by 32 is avoided through 64 bits)
        const bool match = (uint32_t)((uint64_t)key >> (shift + 8)) == prefix;
        hs::wave_count(hist, valid && match, (key >> shift) & 0xFFu);
    }
};

__global__ void __launch_bounds__(kThreads) select_pass_kernel(const float* __restrict__ x, int rows, int64_t n, int64_t row_stride,
                                                               uint32_t k, int pass, uint32_t* bins, uint32_t* nans) {
    __shared__ uint32_t hist[kBins];
    __shared__ Scratch scratch;
    const int t = threadIdx.x, row = blockIdx.y;
    const int64_t split = blockIdx.x, splits = gridDim.x;
    hist[t] = 0;
    uint32_t prefix, rank;
    find_prefix(bins, rows, row, pass, k, scratch, prefix, rank);  // (its barriers also publish the zeroed counters)
    if (pass == 0) __syncthreads();

    // the row as a scalar head up to the first 16-byte boundary, a body of float4 split evenly over the workgroups, a scalar tail
    const float* xr = x + (int64_t)row * row_stride;
    const int64_t to_boundary = (int64_t)((4 - (((uintptr_t)xr >> 2) & 3)) & 3);
    const int64_t head = to_boundary < n ? to_boundary : n;
    const int64_t nv = (n - head) / 4, tail0 = head + nv * 4;
    const float4* body = (const float4*)(xr + head);
    Counter c{hist, prefix, pass, 0u};
    const int64_t v0 = nv * split / splits, v1 = nv * (split + 1) / splits;
    for (int64_t base = v0; base < v1; base += kThreads) {  // wave-uniform trip count: wave_count needs the whole wave
        const int64_t v = base + t;
        const bool valid = v < v1;
        const float4 q = valid ? body[v] : make_float4(0.f, 0.f, 0.f, 0.f);
        c.add(valid, q.x);
        c.add(valid, q.y);
        c.add(valid, q.z);
        c.add(valid, q.w);
    }
    if (split == 0 && t < 64) {  // wave 0 of the row's first workgroup: at most 3 + 3 single elements
        const bool h = t < head, e = t >= 8 && tail0 + (t - 8) < n;
        c.add(h || e, h ? xr[t] : e ? xr[tail0 + (t - 8)] : 0.f);
    }
    __syncthreads();
    if (hist[t] != 0) atomicAdd(&bins[((int64_t)pass * rows + row) * kBins + t], hist[t]);
    if (pass == 0) {
        uint32_t m = c.nans;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off, 64);
        if ((t & 63) == 0 && m != 0) atomicAdd(&nans[row], m);
    }
}

__global__ void __launch_bounds__(kThreads) select_write_kernel(int rows, uint32_t k, int nan_propagates,
                                                                const uint32_t* __restrict__ bins, const uint32_t* __restrict__ nans,
                                                                float* __restrict__ out) {
    __shared__ Scratch scratch;
    const int row = blockIdx.x;
    uint32_t key, rank;
    find_prefix(bins, rows, row, kPasses, k, scratch, key, rank);
    if (threadIdx.x == 0) out[row] = (nan_propagates && nans[row] != 0) ? __uint_as_float(0x7FC00000u) : key_float(key);
}

}  // namespace

extern "C" {

int64_t hs_select_rows_workspace(int rows) {
    return rows > 0 ? (int64_t)rows * (kPasses * kBins + 1) * (int64_t)sizeof(uint32_t) : 0;
}

int hs_select_rows(const float* x, int rows, int64_t n, int64_t row_stride, int64_t k, int nan_propagates, int splits, void* workspace,
                   float* out, void* stream) {
    HS_CHECK_ARG(rows >= 1 && rows <= 65535, "hs_select_rows: rows %d outside [1, 65535]", rows);
    HS_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "hs_select_rows: n %lld outside [1, 2^31)", (long long)n);
    HS_CHECK_ARG(k >= 0 && k < n, "hs_select_rows: k %lld outside [0, n = %lld)", (long long)k, (long long)n);
    HS_CHECK_ARG(row_stride >= n, "hs_select_rows: row_stride %lld < n %lld", (long long)row_stride, (long long)n);
    HS_CHECK_ARG(splits >= 0 && splits <= 65535, "hs_select_rows: splits %d outside [0, 65535]", splits);
    HS_CHECK_ARG(x && workspace && out, "hs_select_rows: null pointer");
    HS_CHECK_ARG((uintptr_t)x % 4 == 0 && (uintptr_t)workspace % 4 == 0 && (uintptr_t)out % 4 == 0,
                 "hs_select_rows: pointers must be 4-byte aligned");
    if (splits == 0) {
        const int64_t by_size = (n + kChunk - 1) / kChunk, by_grid = std::max(1, kAutoWorkgroups / rows);
        splits = (int)std::max<int64_t>(1, std::min(by_size, by_grid));
    }
    hipStream_t s = (hipStream_t)stream;
    uint32_t* bins = (uint32_t*)workspace;
    uint32_t* nans = bins + (int64_t)kPasses * rows * kBins;
    HS_HIP_CHECK(hipMemsetAsync(workspace, 0, (size_t)hs_select_rows_workspace(rows), s));
    for (int pass = 0; pass < kPasses; ++pass) {
        hipLaunchKernelGGL(select_pass_kernel, dim3((unsigned)splits, (unsigned)rows), dim3(kThreads), 0, s, x, rows, n, row_stride,
                           (uint32_t)k, pass, bins, nans);
        HS_LAUNCH_CHECK("select_pass");
    }
    hipLaunchKernelGGL(select_write_kernel, dim3((unsigned)rows), dim3(kThreads), 0, s, rows, (uint32_t)k, nan_propagates,
                       (const uint32_t*)bins, (const uint32_t*)nans, out);
    HS_LAUNCH_CHECK("select_write");
    return HS_OK;
}

}  // extern "C"
