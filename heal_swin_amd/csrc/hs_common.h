// Internal helpers shared by the libhealswin translation units (not part of the ABI).
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstdint>

#include "../../include/healswin.h"

namespace hs {

// thread-local last-error text, returned by hs_last_error()
char* error_buffer();
int fail(int status, const char* fmt, ...);

inline int isqrt_pow2_window(int ws) {
    // window_size must be 4^k (a sqrt(Ws) x sqrt(Ws) nested block, hp_windowing.py:16); returns side or -1
    int side = 1;
    while (side * side < ws) side <<= 1;
    return (side * side == ws) ? side : -1;
}

// every pointer (NULL included) is a multiple of `bytes`: the 16-byte vector / buffer-to-LDS accesses of the kernels drop or
// mis-handle the low address bits, so a misaligned operand is refused on the host (include/healswin.h: "Pointer alignment")
template <typename... P>
inline bool aligned_to(uintptr_t bytes, P... p) {
    return ((((uintptr_t)p) | ... | (uintptr_t)0) % bytes) == 0;
}

inline bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// the classes of a segmentation that the loss (seg_loss.hip) and the evaluation kernels (evaluation.hip) take: a workgroup's
// confusion matrix of 64 x 64 32-bit bins is 16 KB of LDS
constexpr int kMaxSegClasses = 64;

// Compute units the persistent / one-resident-round launches may plan for: 256 minus hs_set_reserved_cus(), spread evenly over
// the 8 XCDs.  The kernels whose grids are sized to exactly the resident capacity of the chip (hs_linear_wgrad, hs_gemm_nt,
// the attention kernels, the module kernel) leave the reserved CUs free for kernels of OTHER streams that must make progress
// at the same time -- RCCL's all-reduce kernels during the backward of a data-parallel run: a persistent grid that fills
// every CU either delays them to its end (no overlap) or, if they were resident first, runs its last workgroups as a second
// round (profiles/archive_r01_r04/r03_cu_contention.json).
int reserved_cus();
inline int usable_cus_per_xcd() { return 32 - reserved_cus() / 8; }
inline int usable_cus() { return 8 * usable_cus_per_xcd(); }

// per translation unit with stochastic kernels (HS_DEFINE_SEED_EPOCH_SETTER); hs_set_seed_epoch (hs_core.cpp) calls them all
int set_seed_epoch_gelu(const void* counter);
int set_seed_epoch_layernorm(const void* counter);
int set_seed_epoch_gemm_nt(const void* counter);
int set_seed_epoch_mlp_fused(const void* counter);
int set_seed_epoch_attn_generic(const void* counter);
int set_seed_epoch_attn_mfma(const void* counter);
int set_seed_epoch_attn_mfma_f32(const void* counter);

// The shape halves of the argument checks of hs_gemm_nt, hs_linear_wgrad*, hs_layernorm_* and hs_window_attn_fwd / _bwd: no
// pointer is read and nothing is launched.  Each entry point runs its own; the operators that chain several of them
// (patch_ops.cpp, module_ops.cpp) run those of every link before their first launch, so that a call one link would refuse
// has deposited nothing by then.  `who` prefixes the message.  Defined next to the entry point concerned.
int gemm_nt_check_shape(const char* who, int64_t lda, int64_t ldb, int k, int64_t lda2, int64_t ldb2, int k2, int64_t m, int n);
int linear_wgrad_check_shape(const char* who, int64_t rows, int n_out, int k_in, int dtype);
int layernorm_check_shape(const char* who, int64_t rows, int width, int dtype);
int window_attn_check_shape(const char* who, int batch, int64_t n_tokens, int channels, int num_heads, int window_size, int64_t roll,
                            int dtype);

}  // namespace hs

#define HS_CHECK_ARG(cond, ...)                                        \
    do {                                                               \
        if (!(cond)) return hs::fail(HS_ERR_INVALID_ARG, __VA_ARGS__); \
    } while (0)

#define HS_CHECK_ALIGNED(entry, bytes, ...)                                                                         \
    do {                                                                                                            \
        if (!hs::aligned_to(bytes, __VA_ARGS__))                                                                    \
            return hs::fail(HS_ERR_MISALIGNED, "%s: operand pointers must be %d-byte aligned", entry, (int)(bytes)); \
    } while (0)
