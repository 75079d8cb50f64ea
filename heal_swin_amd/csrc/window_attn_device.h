// Device-side pieces shared by the attention translation units (window_attn_mfma.hip, window_attn_mfma_f32.hip,
// window_attn_module.hip; window_attn_generic.hip takes kNormEps): constants of the log2-domain softmax, the vector types of the
// MFMA operands, the accumulator layout of a 32x32 tile and the packing of a transposed output tile into token rows.
#pragma once
#include "window_attn.h"

namespace hs {

constexpr float kNormEps = 1e-12f;             // F.normalize eps, swin_hp_transformer.py:143
constexpr float kMaskLog2 = -100.f * kLog2e;  // hp_shifting.py:25, in the log2 domain
// 1 / max(|x|, eps) from the squared norm: v_rsq_f32 (1 ulp) + a clamp instead of the correctly rounded sqrt and division hipcc
// expands to ~20 instructions each -- four of them per row block were half of what cosine attention added to the kernels' VALU
// count (profiles/r05_attn_pmc_T256_vs_D256.txt: 66 vs 37 VALU per MFMA in the forward); results are bf16 rows
// (the fp32 kernels keep the exact 1.f / fmaxf(sqrtf(s), kNormEps))
__device__ __forceinline__ float inv_norm(float sumsq) { return fminf(__builtin_amdgcn_rsqf(sumsq), 1.f / kNormEps); }

// row (key, query or feature) held by accumulator register r of lane half `half` in a 32x32 MFMA tile
__device__ __forceinline__ int kappa(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// 16 accumulator values of a transposed output tile (lane = token, register r = feature kappa(r, half)) -> two 16-byte pieces of
// the token's 64-byte head slice: lanes < 32 hold bytes [0,16) and [32,48), lanes >= 32 bytes [16,32) and [48,64)
// (v_permlane32_swap pairs the 8-byte pieces of the two lane halves)
__device__ __forceinline__ void swap_rows_t(const uint32_t (&packed)[8], u32x4& p0, u32x4& p1) {  // packed[i] = registers 2i, 2i+1
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = packed[i];
    // groups m = 0..3 are dwords (2m, 2m+1); pair (0,1) and pair (2,3): vdst = group m, src = group m+1
#pragma unroll
    for (int m = 0; m < 4; m += 2)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const auto r = __builtin_amdgcn_permlane32_swap(w[2 * m + d], w[2 * m + 2 + d], false, false);
            w[2 * m + d] = r[0];
            w[2 * m + 2 + d] = r[1];
        }
    p0 = u32x4{w[0], w[1], w[2], w[3]};
    p1 = u32x4{w[4], w[5], w[6], w[7]};
}
__device__ __forceinline__ void pack_rows_t(const f32x16& v, u32x4& p0, u32x4& p1) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
    swap_rows_t(w, p0, p1);
}

}  // namespace hs
