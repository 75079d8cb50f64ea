// Pieces shared by the two decoder-tail translation units (ln_head.hip, expand_ln_head.hip): the constants of the padded head
// row, packing of a lane's 16-byte chunk, the accumulator-register -> class maps, the LayerNorm statistics of a lane pair's row,
// the hi + lo head product and the width dispatch of the host side.  In both units a wavefront owns 32 rows, lane (l31, half)
// holds every second 16-byte chunk of row l31, and a 32x32x16 MFMA leaves the row's 16 padded classes in registers 0..7 of the
// lane pair (l31, l31 + 32).
#pragma once
#include <type_traits>

#include "hs_device.h"

namespace hs {

constexpr float kEps = 1e-5f;  // nn.LayerNorm default, as everywhere in the reference
constexpr int kKP = 16;        // class columns of the padded logits row

// 8 bf16 of a 16-byte chunk <-> 8 floats
__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = bf_lo(w[i]);
        f[2 * i + 1] = bf_hi(w[i]);
    }
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    return make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7]));
}

// Class held by accumulator register r < 8 of lane half `half` after the head product.  Natural: the MFMA's own row order, with
// the folded head weight as it is.  Exchanged: the fused backward takes the folded weight with row blocks 4..7 and 8..11
// swapped (ops._fold_head_ce), which makes the 8 registers of a lane 8 CONTIGUOUS classes -- they are then, packed, directly
// the B operand of the g = dlogits (gamma W) product and the 16 bytes of D'.  (Classes 0..3 sit in registers 0..3 of half 0
// either way: the depth loss, which reads classes 0 and 1, takes the plain weight.)
__device__ __forceinline__ int class_natural(int r, int half) { return 4 * half + (r & 3) + 8 * (r >> 2); }
__device__ __forceinline__ int class_exchanged(int r, int half) { return 8 * half + r; }

// bk[r] = the head bias (sum_c beta_c W[k, c]) of the class in register r, natural order
__device__ __forceinline__ void load_head_bias(const float* __restrict__ bvec, int half, float (&bk)[8]) {
#pragma unroll
    for (int r = 0; r < 8; ++r) bk[r] = bvec[class_natural(r, half)];
}

// LayerNorm statistics of a lane pair's row: each lane holds M x K of the row's 2 M K values, as v[m][k] (float x[NS][8] of the
// row kernels, f32x16 acc[NB] of the expand kernel).  Sums run over m, then k, ascending, then one lane ^ 32 exchange -- the
// order both call sites always had; v leaves centred (v - mean).
template <int K, int M, typename Regs>
__device__ __forceinline__ void row_stats(Regs (&v)[M], float& mean, float& rstd) {
    constexpr float inv_c = 1.f / (float)(2 * M * K);
    float sum = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int k = 0; k < K; ++k) sum += v[m][k];
    sum += __shfl_xor(sum, 32, 64);
    mean = sum * inv_c;
    float sq = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            v[m][k] -= mean;
            sq = fmaf(v[m][k], v[m][k], sq);
        }
    sq += __shfl_xor(sq, 32, 64);
    rstd = rsqrtf(sq * inv_c + kEps);
}

// One 16-channel step of the head product logits^T += (gamma W) xhat^T with the lane's 8 xhat values in fp32:
//   TERMS 1   wa hi                     xhat rounded to bf16 (bf16 logits)
//   TERMS 2   wa hi + wa lo             xhat as hi + lo: its rounding remainder as a second operand (ln_head_fwd, fp32 logits)
//   TERMS 3   wa hi + wa lo + wl hi     ... and the remainder wl of the folded weight (expand forward, fused backward)
// The kernels are HBM-bound; the extra MFMAs are free.
template <int TERMS>
__device__ __forceinline__ f32x16 head_step(f32x16 acc, const float (&xh)[8], bf16x8 wa, bf16x8 wl) {
    const uint4 hb = pack8(xh);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, __builtin_bit_cast(bf16x8, hb), acc, 0, 0, 0);
    if constexpr (TERMS >= 2) {
        float hi[8], lo[8];
        unpack8(hb, hi);
#pragma unroll
        for (int j = 0; j < 8; ++j) lo[j] = xh[j] - hi[j];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, __builtin_bit_cast(bf16x8, pack8(lo)), acc, 0, 0, 0);
    }
    if constexpr (TERMS >= 3) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, __builtin_bit_cast(bf16x8, hb), acc, 0, 0, 0);
    return acc;
}

// Host side: the class count of a fused cross-entropy
inline int check_class_count(const char* who, int n_classes) {
    HS_CHECK_ARG(n_classes >= 1 && n_classes <= kKP, "%s: 1..16 classes", who);
    return HS_OK;
}

// f(std::integral_constant<int, NB>{}) for NB = width / 32 in 2..MAX_NB (hs_*_supported has passed the width)
template <int MAX_NB, class F>
int with_width_blocks(int width, F&& f) {
    switch (width / 32) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
    }
    if constexpr (MAX_NB >= 8) {
        switch (width / 32) {
            case 5: return f(std::integral_constant<int, 5>{});
            case 6: return f(std::integral_constant<int, 6>{});
            case 7: return f(std::integral_constant<int, 7>{});
            case 8: return f(std::integral_constant<int, 8>{});
        }
    }
    return fail(HS_ERR_UNSUPPORTED, "decoder tail: no kernel for %d columns", width);
}

}  // namespace hs
