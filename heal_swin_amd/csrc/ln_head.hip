// Decoder tail: the LayerNorm of FinalPatchExpand_X4 and the 1x1 class head in ONE pass over the expanded
// rows, forward and backward, so that the normalised tensor [B, 4 N0, C] never exists in HBM.
// Reference: models_torch/swin_hp_transformer.py:448-452 (`self.norm(x)` of FinalPatchExpand_X4) and :785-788
// (`self.output(x)`, Conv1d(C, f_out, 1, bias=False)); both run on every pixel row (6.3 M rows at nside 256, batch 8).
//
//   forward   logits[row, k] = sum_c xhat[row, c] (gamma_c W[k, c]) + sum_c beta_c W[k, c],   xhat = (y - mean) rstd
//   backward  g[row, c] = sum_k dlogits[row, k] gamma_c W[k, c]          (= dL/dLN_out * gamma)
//             dy = rstd (g - mean_c g - xhat mean_c(g xhat))              (LayerNorm input gradient)
//             D'[row, k] = dlogits[row, k] rstd[row]   (bf16, written),   u[k] = sum_rows dlogits,  t[k] = sum_rows D' mean
//   The parameter gradients follow from ONE weight-gradient product over the raw rows, X[k, c] = sum_rows dlogits xhat =
//   hs_linear_wgrad(D', y)[k, c] - t[k]  (the host side, ops.LnHeadFn):  dW = gamma X + beta u,  dgamma_c = sum_k W X,
//   dbeta_c = sum_k W u.
//
// Layout: a wavefront owns 32 rows per step; lane (l31, half) holds row l31's 16-byte chunks 16 s + 8 half of its C-wide
// row -- which IS the B operand of v_mfma_f32_32x32x16_bf16 with the row index on the accumulator's lane axis.  Row
// statistics are therefore lane-local sums plus one exchange with lane ^ 32, the normalised chunks feed the MFMA straight
// from registers (A = the folded head weight, resident in registers), and the accumulator holds the row's classes
// (forward) or the row's g values in the same chunk order as the lane's y registers (backward: the rows of the A operand
// are permuted to make it so).  HBM-bound: forward reads C x 2 B and writes 32 B per row, backward reads C x 2 + 32 + 8 B
// and writes C x 2 + 32 B.
#include "ln_head_device.h"
#include "hs_depth_loss.h"

namespace hs {
namespace {

// wfold [32][C] bf16: row k = gamma * W[k, :] (rows >= f_out zero); bvec [32] f32: sum_c beta_c W[k, c]
// F32OUT: the logits leave as fp32 rows of 16 (64 B) instead of bf16 (32 B).  The decoder tail is where bf16 rounding is NOT
// averaged away by anything downstream: the four roundings norm_up -> expand -> xhat -> logits account for 6.4e-3 of the
// 7.7e-3 logit error of HEAL-SWIN-B (tests/experiments/bf16_error_budget.py), the whole rest of the network for 2.9e-3.  So
// here the logits keep their fp32 accumulator value and xhat enters the head product as hi + lo (head_step<2>).
template <int NB, bool F32OUT>
__global__ void __launch_bounds__(256) ln_head_fwd_kernel(const uint16_t* __restrict__ y, const uint16_t* __restrict__ wfold,
                                                          const float* __restrict__ bvec, void* __restrict__ logits_v,
                                                          float* __restrict__ mean_out, float* __restrict__ rstd_out, int64_t rows) {
    constexpr int C = NB * 32, NS = NB * 2;
    const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    bf16x8 wa[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) wa[s] = *(const bf16x8*)(wfold + l31 * C + 16 * s + 8 * half);
    float bk[8];
    load_head_bias(bvec, half, bk);
    for (int64_t row0 = wave * 32; row0 < rows; row0 += nwaves * 32) {
        const int64_t row = row0 + l31;
        const bool live = row < rows;
        float x[NS][8];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uint4 v = live ? *(const uint4*)(y + row * C + 16 * s + 8 * half) : make_uint4(0, 0, 0, 0);
            unpack8(v, x[s]);
        }
        float mean, rstd;
        row_stats<8>(x, mean, rstd);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) x[s][j] *= rstd;
            acc = head_step<F32OUT ? 2 : 1>(acc, x[s], wa[s], wa[s]);
        }
        if (live) {
            float o[8];  // classes 0..15 of the row are registers 0..7 of the lane pair (class_natural)
#pragma unroll
            for (int r = 0; r < 8; ++r) o[r] = acc[r] + bk[r];
            if constexpr (F32OUT) {
                float* logits = (float*)logits_v;
                *(float4*)(logits + row * kKP + 4 * half) = make_float4(o[0], o[1], o[2], o[3]);
                *(float4*)(logits + row * kKP + 8 + 4 * half) = make_float4(o[4], o[5], o[6], o[7]);
            } else {
                uint16_t* logits = (uint16_t*)logits_v;
                const uint4 ob = pack8(o);
                *(uint2*)(logits + row * kKP + 4 * half) = make_uint2(ob.x, ob.y);
                *(uint2*)(logits + row * kKP + 8 + 4 * half) = make_uint2(ob.z, ob.w);
            }
            if (half == 0) {
                mean_out[row] = mean;
                rstd_out[row] = rstd;
            }
        }
    }
}

// ---- where the backward takes the row's dlogits from.  A source leaves the lane's 8 classes un-rounded in d[] and returns
// them packed: the B operand of the g product.
// (1) a [rows, 16] tensor, fp32 or bf16
template <typename T>
struct BwdRows {
    static constexpr bool kFused = false;
    const T* dlogits;
    __device__ __forceinline__ uint4 load(int64_t row, int half, float (&d)[8]) const {
        if constexpr (std::is_same<T, float>::value) {
            const float4 a = *(const float4*)(dlogits + row * kKP + 8 * half);
            const float4 b = *(const float4*)(dlogits + row * kKP + 8 * half + 4);
            d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
            return pack8(d);
        } else {
            const uint4 dl = *(const uint4*)(dlogits + row * kKP + 8 * half);
            unpack8(dl, d);
            return dl;
        }
    }
};
// (2) the loss, fused in: instead of reading a [rows, 16] dlogits tensor the kernel recomputes the row's logits
// from the saved expanded rows (xhat = (y - mean) rstd as hi + lo through the folded head weight as hi + lo, head_step<3>: 3
// MFMAs per 16 channels in an HBM-bound kernel) and takes the loss gradient in registers.
struct BwdFused {
    static constexpr bool kFused = true;
    const uint16_t* wfold;  // [64][C]: the folded head weight, rows 32..63 its rounding remainder
    const float* bvec;
    const float* scale;     // [1]: dloss / (the forward's denominator)
};
// ... softmax and the weighted cross-entropy:  dlogits[row, k] = scale w[y] (softmax_k - [k == y]).  Takes the folded weight
// with exchanged rows (class_exchanged)
struct BwdCe : BwdFused {
    const uint8_t* labels;
    const float* class_w;
    int n_classes;
    __device__ __forceinline__ int target(int64_t row, bool live, int) const { return live ? (int)labels[row] : 255; }
    __device__ __forceinline__ void grad(const f32x16& lg, const float (&bk)[8], int yl, int half, float s, float (&d)[8]) const {
        float m = -INFINITY;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            d[r] = lg[r] + bk[r];
            if (class_exchanged(r, half) < n_classes) m = fmaxf(m, d[r]);
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float ssum = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            d[r] = class_exchanged(r, half) < n_classes ? __builtin_amdgcn_exp2f((d[r] - m) * kLog2e) : 0.f;
            ssum += d[r];
        }
        ssum += __shfl_xor(ssum, 32, 64);
        const float wy = yl < n_classes ? (class_w ? class_w[yl] : 1.f) : 0.f;
        const float coef = s * wy, pinv = 1.f / ssum;
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = coef * (d[r] * pinv - (class_exchanged(r, half) == yl ? 1.f : 0.f));
    }
};
// ... or the depth caller's regression loss (hs_depth_loss.h): dpred of the row's one or two channels, classes 0 and 1 =
// registers 0 and 1 of lane half 0
struct BwdDepth : BwdFused {
    const float* target_rows;  // [rows] fp32; rows with an infinite target get a zero gradient
    int kind;                  // HS_DEPTH_*
    float delta;
    __device__ __forceinline__ float target(int64_t row, bool live, int half) const {
        return live && half == 0 ? target_rows[row] : INFINITY;
    }
    __device__ __forceinline__ void grad(const f32x16& lg, const float (&bk)[8], float tgt, int, float s, float (&d)[8]) const {
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = 0.f;
        if (depth_keep(tgt)) depth_grad(kind, delta, lg[0] + bk[0], lg[1] + bk[1], tgt, s, &d[0], &d[1]);
    }
};

// afold [C][16] bf16: afold[c][k] = gamma_c W[k, c] (columns >= f_out zero); part [nwaves][32] f32: u[0..15], t[0..15]
template <int NB, typename Src>
__global__ void __launch_bounds__(256) ln_head_bwd_kernel(const uint16_t* __restrict__ y, const float* __restrict__ mean_in,
                                                          const float* __restrict__ rstd_in, const Src src,
                                                          const uint16_t* __restrict__ afold, uint16_t* __restrict__ dy,
                                                          uint16_t* __restrict__ dprime, float* __restrict__ part, int64_t rows) {
    constexpr int C = NB * 32, NS = NB * 2;
    const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    [[maybe_unused]] bf16x8 wa[NS], wl[NS];  // fused sources: the folded head weight, hi and lo
    [[maybe_unused]] float bk[8], scale = 0.f;
    if constexpr (Src::kFused) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            wa[s] = *(const bf16x8*)(src.wfold + l31 * C + 16 * s + 8 * half);
            wl[s] = *(const bf16x8*)(src.wfold + (32 + l31) * C + 16 * s + 8 * half);
        }
        load_head_bias(src.bvec, half, bk);
        scale = src.scale[0];
    }
    // A operand of block i: lane l31 = accumulator row rho; accumulator register r of lane half h is rho = 4 h + (r & 3) +
    // 8 (r >> 2) and has to be element r % 8 of the lane's chunk 2 i + r / 8, i.e. column c = 32 i + 16 (r / 8) + 8 h + r % 8
    bf16x8 aa[NB];
    {
        const int hh = (l31 >> 2) & 1, j4 = l31 & 3, q = l31 >> 3;
        const int c_in = 16 * (q >> 1) + 8 * hh + j4 + 4 * (q & 1);
#pragma unroll
        for (int i = 0; i < NB; ++i) aa[i] = *(const bf16x8*)(afold + (32 * i + c_in) * kKP + 8 * half);
    }
    float uacc[8], tacc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) uacc[j] = tacc[j] = 0.f;
    const float inv_c = 1.f / (float)C;
    for (int64_t row0 = wave * 32; row0 < rows; row0 += nwaves * 32) {
        const int64_t row = row0 + l31;
        const bool live = row < rows;
        const float mean = live ? mean_in[row] : 0.f, rstd = live ? rstd_in[row] : 0.f;
        uint4 dl = make_uint4(0, 0, 0, 0);
        float d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // this lane's 8 classes of the row's dlogits, un-rounded
        float xh[NS][8];
        if constexpr (!Src::kFused) {
            if (live) dl = src.load(row, half, d);
        }
        uint4 v[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) v[s] = live ? *(const uint4*)(y + row * C + 16 * s + 8 * half) : make_uint4(0, 0, 0, 0);
        if constexpr (Src::kFused) {  // the row's logits again, then the loss gradient on this lane's 8 classes
            const auto tgt = src.target(row, live, half);
            f32x16 lg;
#pragma unroll
            for (int r = 0; r < 16; ++r) lg[r] = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                unpack8(v[s], xh[s]);
#pragma unroll
                for (int j = 0; j < 8; ++j) xh[s][j] = (xh[s][j] - mean) * rstd;
                lg = head_step<3>(lg, xh[s], wa[s], wl[s]);
            }
            src.grad(lg, bk, tgt, half, scale, d);
            dl = pack8(d);
        }
        f32x16 g[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) g[i][r] = 0.f;
            g[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aa[i], __builtin_bit_cast(bf16x8, dl), g[i], 0, 0, 0);
        }
        // D' = dlogits * rstd (bf16) and the two class sums, on this lane's 8 classes
        {
            float dp[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) dp[j] = d[j] * rstd;
            const uint4 pk = pack8(dp);
            float dr[8];
            unpack8(pk, dr);  // the rounded values, as the weight-gradient kernel will read them
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uacc[j] += d[j];
                tacc[j] = fmaf(dr[j], mean, tacc[j]);
            }
            if (live) *(uint4*)(dprime + row * kKP + 8 * half) = pk;
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if constexpr (!Src::kFused) unpack8(v[s], xh[s]);  // (formed only now: not live across the g product)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (!Src::kFused) xh[s][j] = (xh[s][j] - mean) * rstd;
                const float gv = g[s >> 1][8 * (s & 1) + j];
                s1 += gv;
                s2 = fmaf(gv, xh[s][j], s2);
            }
        }
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        const float m1 = s1 * inv_c, m2 = s2 * inv_c;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = rstd * (g[s >> 1][8 * (s & 1) + j] - m1 - xh[s][j] * m2);
            if (live) *(uint4*)(dy + row * C + 16 * s + 8 * half) = pack8(o);
        }
    }
    // class sums over the wave's rows (the 32 lanes of a half hold the same 8 classes)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            uacc[j] += __shfl_xor(uacc[j], off, 64);
            tacc[j] += __shfl_xor(tacc[j], off, 64);
        }
    }
    if (l31 == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            part[wave * 32 + 8 * half + j] = uacc[j];
            part[wave * 32 + 16 + 8 * half + j] = tacc[j];
        }
    }
}

int grid_for(int64_t rows) {
    int64_t b = (rows + 127) / 128;  // 4 waves x 32 rows per workgroup and step
    if (b > 256 * 8) b = 256 * 8;
    return (int)(b < 1 ? 1 : b);
}

template <typename... P>
uintptr_t address_bits(P... p) {
    return (((uintptr_t)p) | ... | (uintptr_t)0);
}

// the argument checks the four entry points share, in two steps (what an entry point checks of its own goes between them).
// all: every required pointer is there; vec16: address_bits of the operands read or written in 16-byte pieces
int check_ln_head_args(const char* who, bool all, uintptr_t vec16, int64_t rows) {
    HS_CHECK_ARG(all, "%s: null pointer", who);
    HS_CHECK_ALIGNED(who, 16, vec16);
    HS_CHECK_ARG(rows > 0, "%s: bad shape", who);
    return HS_OK;
}
// max_width: 256, or 128 where the head weight stays in registers as hi + lo
int check_ln_head_width(const char* who, int width, int n_out, int dtype, int max_width) {
    if (!hs_ln_head_supported(width, n_out, dtype) || width > max_width)
        return fail(HS_ERR_UNSUPPORTED, "%s: bf16 rows of 64..%d (multiple of 32) columns only", who, max_width);
    return HS_OK;
}
int check_logits_dtype(const char* who, int logits_dtype) {
    HS_CHECK_ARG(logits_dtype == HS_BF16 || logits_dtype == HS_F32, "%s: logits_dtype must be HS_BF16 or HS_F32", who);
    return HS_OK;
}

template <int MAX_NB, typename Src>
int launch_ln_head_bwd(const char* who, const void* y, const float* mean, const float* rstd, const Src& src, const void* afold,
                       void* dy, void* dprime, float* partials, int64_t rows, int width, void* stream) {
    return with_width_blocks<MAX_NB>(width, [&](auto nb) {
        hipLaunchKernelGGL((ln_head_bwd_kernel<decltype(nb)::value, Src>), dim3(grid_for(rows)), dim3(256), 0, (hipStream_t)stream,
                           (const uint16_t*)y, mean, rstd, src, (const uint16_t*)afold, (uint16_t*)dy, (uint16_t*)dprime, partials,
                           rows);
        HS_LAUNCH_CHECK("ln_head_bwd");
        return (int)HS_OK;
    });
}

}  // namespace
}  // namespace hs

extern "C" {

int hs_ln_head_supported(int width, int n_classes, int dtype) {
    return dtype == HS_BF16 && width % 32 == 0 && width >= 64 && width <= 256 && n_classes >= 1 && n_classes <= 16;
}

int64_t hs_ln_head_partials(int64_t rows) { return rows > 0 ? (int64_t)hs::grid_for(rows) * 4 : 0; }

int hs_ln_head_fwd(const void* y, const void* wfold, const float* bvec, void* logits, float* mean, float* rstd, int64_t rows,
                   int width, int dtype, int logits_dtype, void* stream) {
    using namespace hs;
    const char* who = "hs_ln_head_fwd";
    const bool all = y && wfold && bvec && logits && mean && rstd;
    if (int e = check_ln_head_args(who, all, address_bits(y, wfold, bvec), rows)) return e;
    if (int e = check_logits_dtype(who, logits_dtype)) return e;
    if (int e = check_ln_head_width(who, width, 1, dtype, 256)) return e;
    return with_width_blocks<8>(width, [&](auto nb) {
        auto kern = logits_dtype == HS_F32 ? ln_head_fwd_kernel<decltype(nb)::value, true> : ln_head_fwd_kernel<decltype(nb)::value, false>;
        hipLaunchKernelGGL(kern, dim3(grid_for(rows)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)y, (const uint16_t*)wfold,
                           bvec, logits, mean, rstd, rows);
        HS_LAUNCH_CHECK("ln_head_fwd");
        return (int)HS_OK;
    });
}

int hs_ln_head_bwd(const void* y, const float* mean, const float* rstd, const void* dlogits, const void* afold, void* dy,
                   void* dprime, float* partials, int64_t rows, int width, int dtype, int logits_dtype, void* stream) {
    using namespace hs;
    const char* who = "hs_ln_head_bwd";
    const bool all = y && mean && rstd && dlogits && afold && dy && dprime && partials;
    if (int e = check_ln_head_args(who, all, address_bits(y, afold, dy, dprime), rows)) return e;
    if (int e = check_logits_dtype(who, logits_dtype)) return e;
    if (int e = check_ln_head_width(who, width, 1, dtype, 256)) return e;
    if (logits_dtype == HS_F32)
        return launch_ln_head_bwd<8>(who, y, mean, rstd, BwdRows<float>{(const float*)dlogits}, afold, dy, dprime, partials, rows, width,
                                     stream);
    return launch_ln_head_bwd<8>(who, y, mean, rstd, BwdRows<uint16_t>{(const uint16_t*)dlogits}, afold, dy, dprime, partials, rows,
                                 width, stream);
}

int hs_ln_head_ce_bwd(const void* y, const float* mean, const float* rstd, const uint8_t* labels, const float* class_weights,
                      const float* scale, int n_classes, const void* wfold, const float* bvec, const void* afold, void* dy,
                      void* dprime, float* partials, int64_t rows, int width, int dtype, void* stream) {
    using namespace hs;
    const char* who = "hs_ln_head_ce_bwd";
    const bool all = y && mean && rstd && labels && scale && wfold && bvec && afold && dy && dprime && partials;
    if (int e = check_ln_head_args(who, all, address_bits(y, wfold, bvec, afold, dy, dprime), rows)) return e;
    if (int e = check_class_count(who, n_classes)) return e;
    if (int e = check_ln_head_width(who, width, n_classes, dtype, 128)) return e;
    const BwdCe src{{(const uint16_t*)wfold, bvec, scale}, labels, class_weights, n_classes};
    return launch_ln_head_bwd<4>(who, y, mean, rstd, src, afold, dy, dprime, partials, rows, width, stream);
}

int hs_ln_head_depth_bwd(const void* y, const float* mean, const float* rstd, const float* target, int kind, float huber_delta,
                         const float* scale, int n_out, const void* wfold, const float* bvec, const void* afold, void* dy,
                         void* dprime, float* partials, int64_t rows, int width, int dtype, void* stream) {
    using namespace hs;
    const char* who = "hs_ln_head_depth_bwd";
    const bool all = y && mean && rstd && target && scale && wfold && bvec && afold && dy && dprime && partials;
    if (int e = check_ln_head_args(who, all, address_bits(y, wfold, bvec, afold, dy, dprime), rows)) return e;
    if (int e = check_depth_head(who, kind, huber_delta, n_out)) return e;
    if (int e = check_ln_head_width(who, width, n_out, dtype, 128)) return e;
    const BwdDepth src{{(const uint16_t*)wfold, bvec, scale}, target, kind, huber_delta};
    return launch_ln_head_bwd<4>(who, y, mean, rstd, src, afold, dy, dprime, partials, rows, width, stream);
}

}  // extern "C"
