// Decoder tail in ONE forward kernel: FinalPatchExpand_X4's Linear(C -> 4C), the 'b n (p c) -> b (n p) c' view, its
// LayerNorm(C) over every pixel row and the 1x1 class head:
//
//     logits[(n, p), k] = sum_c LN_c( sum_j xn[n, j] Wexp[p C + c, j] ) (gamma_c Whead[k, c]) + sum_c beta_c Whead[k, c]
//
// Reference: models_torch/swin_hp_transformer.py:442-452 (`self.expand`, rearrange, `self.norm`) and :785-788 (`self.output`).
// Why fused: (1) parity -- the four bf16 roundings of the tail (norm_up output, expand output, xhat, logits) are not averaged by
// anything downstream and make up 6.4e-3 of the 7.7e-3 logit error of HEAL-SWIN-B, the whole rest of the network 2.9e-3
// (tests/experiments/bf16_error_budget.py); here LayerNorm sees the fp32 accumulators of the expand product, xhat enters the
// head as hi + lo and the logits leave in fp32; with xn_lo (the rounding remainder of the norm_up output) not even that of
// the input remains; (2) traffic -- the [B, 4 N0, C] tensor
// (1.6 GB at nside 256, batch 8) is written at most once (training: the backward's LayerNorm input) and never read by the
// forward; without a gradient it does not exist at all.
//
// Workgroup = 4 wavefronts, persistent, one per CU: Wexp (4C x C bf16, 128 KB at C = 128) stays in LDS for the whole launch.
// A wavefront owns 32 tokens per step: lane (l31, half) holds the 16-byte chunks 2 s + half of token l31's row -- the B operand
// of v_mfma_f32_32x32x16_bf16 with the token on the accumulator's lane axis -- so per child p the product D = Wexp_p xn^T
// (A = weight rows from LDS) leaves the child's C channels of a token in ONE lane pair: LayerNorm statistics are in-register
// sums plus one lane^32 exchange, the normalised registers are (after packing) the B operand of the head product, and the
// logits of the row land in registers 0..7 of the same lane pair.  32 C / 16 + 4 C / 16 MFMAs per 32 pixel rows.
#include "ln_head_device.h"
#include "hs_depth_loss.h"
#include "hs_histogram.h"

// the target transform and the metric rules of TailDepthStep form their values unfused (their headers say why); everything else in
// this file keeps the default contraction
#pragma clang fp contract(off)
#include "hs_depth_target.h"
#include "hs_depth_metrics.h"
#pragma clang fp contract(fast)

namespace hs {
namespace {

constexpr int kP = 4;       // children per token (patch_size 4: every BASELINE config)
constexpr int kRowB = 256;  // bytes per weight row in LDS (C <= 128 bf16; rows of C = 96 / 64 are padded)
constexpr int kPatchRow = 128;

constexpr int kHistBins = kKP * kKP;  // per-wave LDS histogram of TailCeStep: 16 x 16 uint32 bins = 1 KB

// ---- The loss epilogues.  The kernel is a template over one of the four structs below and calls its row() once per pixel
// row, with the row's 16 head outputs in registers 0..7 of the lane pair (class_natural) and TailLane for what the lane carries
// from row to row; instantiations that do not touch a field of TailLane do not hold it.
struct TailLane {
    float num = 0.f, den = 0.f;  // the lane's part of the loss: numerator and denominator
    uint32_t pred4 = 0;          // TailCeStep: the class ids of the token's 4 children, child p in byte p
    uint32_t bad_rows = 0;       // TailCeStep: rows whose label is outside the matrix (wave-uniform: counted with ballots)
    uint32_t* hist = nullptr;    // TailCeStep: the wave's LDS histogram
    float4 m4, lv4;              // TailDepthStep: metres and log variance of the token's 4 children
    double dsum[depth_metrics::kNSums];  // TailDepthStep: the lane's metric sums (half 0 lanes add, one row each)
};

// Optional fused loss (the caller's CrossEntropyLoss(weight), models_lightning/segmentation/model_lightning_swin_hp.py:
// 39-45, 104-111): the 16 logits of a pixel row sit in one lane pair, so log-sum-exp, the label's logit and the row's weighted
// term are eight registers + one lane^32 exchange away; with `logits == nullptr` the [rows, 16] fp32 tensor is never written.
struct TailCe {
    const uint8_t* labels;  // [rows] class ids in pixel order (rows = (token, child)); ids >= n_classes are ignored (weight 0);
                            // null: no loss
    const float* class_w;   // [n_classes] or null (all ones)
    float* loss_part;       // [4 * gridDim.x][2]: per-wave sums of w (lse - logit_y) and of w
    int n_classes;
    __device__ __forceinline__ bool has_loss() const { return labels != nullptr; }
    // weighted cross-entropy of the row, from the fp32 logits in registers; leaves the lane's logits in v[], the label in yl
    __device__ __forceinline__ bool ce_row(TailLane& st, const f32x16& lg, const float (&bk)[8], int64_t orow, bool live, int half,
                                           float (&v)[8], int& yl) const {
        if (!labels) return false;
        float m = -INFINITY;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            v[r] = lg[r] + bk[r];
            if (class_natural(r, half) < n_classes) m = fmaxf(m, v[r]);
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        yl = live ? (int)labels[orow] : 255;
        float ssum = 0.f, pick = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int cls = class_natural(r, half);
            if (cls < n_classes) ssum += __builtin_amdgcn_exp2f((v[r] - m) * kLog2e);
            pick = cls == yl ? v[r] : pick;
        }
        ssum += __shfl_xor(ssum, 32, 64);
        pick += __shfl_xor(pick, 32, 64);  // (the other half holds 0)
        const float wy = yl < n_classes ? (class_w ? class_w[yl] : 1.f) : 0.f;
        if (half == 0) {
            st.num = fmaf(wy, m + __builtin_amdgcn_logf(ssum) * kLn2 - pick, st.num);
            st.den += wy;
        }
        return true;
    }
    __device__ __forceinline__ void row(TailLane& st, const f32x16& lg, const float (&bk)[8], int64_t orow, int, bool live,
                                        int lane) const {
        float v[8];
        int yl;
        ce_row(st, lg, bk, orow, live, lane >> 5, v, yl);
    }
};

// ... or the segmentation caller's whole `shared_step` (model_lightning_swin_hp.py:104-111: argmax, weighted cross-entropy, IoU /
// Accuracy on (preds, masks)): TailCe's loss, plus the row's class id (torch.max(logits, 1): the first maximal class, a NaN
// counts as the maximum -- argmax_step and argmax_merge of hs_device.h) and the confusion matrix behind the metrics
// (hs_seg_confusion's counting: labels >= n_classes stay out of the matrix and are counted in bad[0]).  labels is never null here.
struct TailCeStep : TailCe {
    uint8_t* preds;            // [rows] class ids, or null; 4-byte aligned (the 4 children of a token leave as one dword)
    unsigned long long* conf;  // [n_classes][n_classes] (target, prediction) counts, added to; or null
    unsigned long long* bad;   // [2]; [0] += rows whose label is >= n_classes (with conf)
    __device__ __forceinline__ bool has_loss() const { return true; }
    __device__ __forceinline__ void row(TailLane& st, const f32x16& lg, const float (&bk)[8], int64_t orow, int p, bool live,
                                        int lane) const {
        const int half = lane >> 5;
        float v[8];
        int yl;
        if (!ce_row(st, lg, bk, orow, live, half, v, yl)) return;
        float best = -INFINITY;  // (the lowest class wins over -inf by index; a lane without a class loses every tie)
        int arg = 4 * half < n_classes ? 4 * half : 64;
#pragma unroll
        for (int r = 0; r < 8; ++r) {  // r ascending = class id ascending
            const int cls = class_natural(r, half);
            if (cls < n_classes) argmax_step(v[r], cls, best, arg);
        }
        const int pred = argmax_merge(best, arg, __shfl_xor(best, 32, 64), __shfl_xor(arg, 32, 64));
        st.pred4 |= (uint32_t)pred << (8 * p);
        if (conf) {  // (wave-uniform) one row per lane pair: half 0 counts it
            const bool mine = live && half == 0;
            const int bin = mine && yl < n_classes ? yl * n_classes + pred : -1;
            st.bad_rows += (uint32_t)__popcll(__ballot(mine && yl >= n_classes));
            wave_count_lead(st.hist, bin, lane);
        }
    }
};

// ... or the depth caller's regression loss (hs_depth_loss.h; heal_swin/training/loss_depth_regression.py): a head of one or two
// channels, i.e. accumulator registers 0 and 1 of the lane pair's half 0, against the row's fp32 target.
struct TailDepth {
    const float* target;  // [rows] in pixel order; rows whose target is infinite are masked out
    float* loss_part;     // [4 * gridDim.x][2]: per-wave sums of the depth term and of the kept rows
    int kind;             // HS_DEPTH_*
    float delta;          // huber delta
    __device__ __forceinline__ bool has_loss() const { return true; }
    // the depth term of the row; returns its target
    __device__ __forceinline__ float depth_row(TailLane& st, const f32x16& lg, const float (&bk)[8], int64_t orow, bool live,
                                               int half) const {
        const float t = live && half == 0 ? target[orow] : INFINITY;
        if (depth_keep(t)) {
            st.num += depth_term(kind, delta, lg[0] + bk[0], lg[1] + bk[1], t);
            st.den += 1.f;
        }
        return t;
    }
    __device__ __forceinline__ void row(TailLane& st, const f32x16& lg, const float (&bk)[8], int64_t orow, int, bool live,
                                        int lane) const {
        depth_row(st, lg, bk, orow, live, lane >> 5);
    }
};

// ... or the depth caller's whole `shared_step` (models_lightning/depth_estimation/model_lightning_depth_swin_hp.py:132-159: the
// loss in the normalised space, unnormalize_and_retransform of prediction and target, DepthMSE / MeanSTD on them): TailDepth's
// loss, plus the row's prediction in metres (target_op's inverse chain, hs_depth_target.h), the HS_DEPTH_NSUMS float64 sums of
// hs_depth_metrics over (metres, target in metres, log variance) as per-lane sums that leave as one record per workgroup
// (merged in a fixed order by depth_metrics::reduce_kernel: no float atomics), and the prediction itself.
struct TailDepthStep : TailDepth {
    int n_out;            // head channels: 1 or 2 (channel 1 = the log variance)
    TargetOp inv;         // the inverse chain (HS_DT_INVERSE set)
    depth_metrics::Rule rule;
    double* partial;      // [gridDim.x][HS_DEPTH_NSUMS] or null (no metrics)
    float* preds;         // [n_out][rows] fp32: channel 0 in metres, channel 1 the raw log variance; or null; 16-byte aligned
    float* logvar_out;    // [rows]: channel 1 alone (read when preds is null); or null
    int64_t rows;
    __device__ __forceinline__ void row(TailLane& st, const f32x16& lg, const float (&bk)[8], int64_t orow, int p, bool live,
                                        int lane) const {
        const int half = lane >> 5;
        // (p0 and p1 are named before the loss term, as they always were here: with them the compiler contracts the log-variance
        // term of this instantiation, d d (e / 2) + p1 / 2, into one fma, and TailDepth's not -- profiles/tail_refactor.txt)
        const float p0 = lg[0] + bk[0], p1 = lg[1] + bk[1], t = depth_row(st, lg, bk, orow, live, half);
        if (partial || preds) {  // (uniform) back to metres, as unnormalize_and_retransform on prediction and target
#pragma clang fp contract(off)
            const float m = target_op(p0, inv);
            if (partial && live && half == 0)
                depth_metrics::accumulate<float, float>(st.dsum, rule, m, target_op(t, inv), [&] { return p1; });
            st.m4.x = p == 0 ? m : st.m4.x;  // (selects: an index would put the four values into scratch)
            st.m4.y = p == 1 ? m : st.m4.y;
            st.m4.z = p == 2 ? m : st.m4.z;
            st.m4.w = p == 3 ? m : st.m4.w;
        }
        st.lv4.x = p == 0 ? p1 : st.lv4.x;
        st.lv4.y = p == 1 ? p1 : st.lv4.y;
        st.lv4.z = p == 2 ? p1 : st.lv4.z;
        st.lv4.w = p == 3 ? p1 : st.lv4.w;
    }
};

template <int NB, typename Loss>
__global__ void __launch_bounds__(256, 1) expand_ln_head_fwd_kernel(const uint16_t* __restrict__ xn, const uint16_t* __restrict__ xn_lo,
                                                                    const uint16_t* __restrict__ wexp,
                                                                    const uint16_t* __restrict__ wfold, const float* __restrict__ bvec,
                                                                    uint16_t* __restrict__ y, float* __restrict__ logits,
                                                                    float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                                    int64_t tokens, Loss ce) {
    constexpr bool kStep = std::is_same<Loss, TailCeStep>::value, kDStep = std::is_same<Loss, TailDepthStep>::value;
    constexpr int C = 32 * NB, KS = 2 * NB, NCH = C / 8;  // channels (= input width), 16-deep k-steps, 16-byte chunks per row
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* wl = smem;                                  // [kP * C][kRowB], 16-byte chunk ^ (row & 15)
    unsigned char* patch = smem + kP * C * kRowB + (threadIdx.x >> 6) * (32 * kPatchRow);  // per wave: [32 tokens][64 channels] bf16
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;

    // ---------------------------------------------------------------- one-off: Wexp -> LDS
    for (int q = tid; q < kP * C * NCH; q += 256) {
        const int row = q / NCH, ch = q % NCH;
        *(uint4*)(wl + row * kRowB + ((ch ^ (row & 15)) << 4)) = *(const uint4*)(wexp + (int64_t)row * C + ch * 8);
    }
    // folded head weight (gamma * Whead) as A operands: accumulator register 8 j + i of channel tile ct is channel
    // 32 ct + 16 j + 8 (i >> 2) + 4 half + (i & 3): two 8-byte pieces per fragment
    // wfold holds 64 rows: 0..31 the bf16 rounding of gamma * Whead, 32..63 its rounding remainder (hi + lo = the fp32 product
    // to 16 bits: the head weights are the last rounding between norm_up and the logits)
    bf16x8 wfa[NB][2], wfl[NB][2];
#pragma unroll
    for (int ct = 0; ct < NB; ++ct)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint16_t* src = wfold + l31 * C + 32 * ct + 16 * j + 4 * half;
            const uint2 a = *(const uint2*)src, b = *(const uint2*)(src + 8);
            wfa[ct][j] = __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, b.x, b.y));
            const uint2 al = *(const uint2*)(src + 32 * C), bl = *(const uint2*)(src + 32 * C + 8);
            wfl[ct][j] = __builtin_bit_cast(bf16x8, make_uint4(al.x, al.y, bl.x, bl.y));
        }
    float bk[8];
    load_head_bias(bvec, half, bk);
    // TailCeStep: one histogram per wave behind the patches (4 x 1 KB: 148 KB of LDS at C = 128), flushed once after the loop
    uint32_t* hist = (uint32_t*)(smem + kP * C * kRowB + 4 * 32 * kPatchRow);
    TailLane st;
    st.hist = hist + (tid >> 6) * kHistBins;
    if constexpr (kStep) {
        for (int j = tid; j < 4 * kHistBins; j += 256) hist[j] = 0;
    }
    if constexpr (kDStep) {
#pragma unroll
        for (int k = 0; k < depth_metrics::kNSums; ++k) st.dsum[k] = 0.0;
    }
    __syncthreads();

    const int sx = l31 & 15;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (tid >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t tok0 = wave * 32; tok0 < tokens; tok0 += nwaves * 32) {
        const int64_t tok = tok0 + l31;
        const bool live = tok < tokens;
        bf16x8 xb[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint4 v = live ? *(const uint4*)(xn + tok * C + 16 * ks + 8 * half) : make_uint4(0, 0, 0, 0);
            xb[ks] = __builtin_bit_cast(bf16x8, v);
        }
        st.pred4 = 0;
        st.m4 = st.lv4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
        for (int p = 0; p < kP; ++p) {
            // ------------------------------------------------------------ the child's C channels of 32 tokens: D = Wexp_p xn^T
            f32x16 acc[NB];
#pragma unroll
            for (int ct = 0; ct < NB; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
            const unsigned char* wrow = wl + (p * C + l31) * kRowB;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int co = ((2 * ks + half) ^ sx) << 4;
#pragma unroll
                for (int ct = 0; ct < NB; ++ct) {
                    const bf16x8 a = *(const bf16x8*)(wrow + ct * 32 * kRowB + co);
                    acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xb[ks], acc[ct], 0, 0, 0);
                }
            }
            if (xn_lo) {  // the rounding remainder of the norm_up output as a second operand (re-fetched per child: L1 / L2 hits)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const uint4 v = live ? *(const uint4*)(xn_lo + tok * C + 16 * ks + 8 * half) : make_uint4(0, 0, 0, 0);
                    const int co = ((2 * ks + half) ^ sx) << 4;
#pragma unroll
                    for (int ct = 0; ct < NB; ++ct) {
                        const bf16x8 a = *(const bf16x8*)(wrow + ct * 32 * kRowB + co);
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, v), acc[ct], 0, 0, 0);
                    }
                }
            }
            // ------------------------------------------------------------ the expanded rows, once, for the backward (training)
            const int64_t orow = tok * kP + p;
            if (y) {
#pragma unroll
                for (int pr = 0; pr < (NB + 1) / 2; ++pr) {  // 64 channels (one 128-byte line per row) at a time
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int ct = 2 * pr + t;
                        if (ct < NB) {
#pragma unroll
                            for (int g = 0; g < 4; ++g) {  // registers 4 g .. 4 g + 3 = channels 32 ct + 8 g + 4 half + 0..3
                                const int chunk = 4 * t + g;  // 16-byte chunk inside the 128-byte patch row
                                *(uint2*)(patch + l31 * kPatchRow + ((chunk ^ (l31 & 7)) << 4) + 8 * half) =
                                    make_uint2(pack_bf16x2(acc[ct][4 * g], acc[ct][4 * g + 1]), pack_bf16x2(acc[ct][4 * g + 2], acc[ct][4 * g + 3]));
                            }
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    constexpr int kChunksLast = (NB % 2) ? 4 : 8;
                    const int nchunks = (2 * pr + 1 < NB) ? 8 : kChunksLast;  // valid 16-byte chunks of this pass
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int q = lane + 64 * i, row = q >> 3, chunk = q & 7;
                        const uint4 v = *(const uint4*)(patch + row * kPatchRow + ((chunk ^ (row & 7)) << 4));
                        if (chunk < nchunks && tok0 + row < tokens)
                            *(uint4*)(y + ((tok0 + row) * kP + p) * C + 64 * pr + chunk * 8) = v;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            // ------------------------------------------------------------ LayerNorm statistics of each row (lane pair)
            float mean, rstd;
            row_stats<16>(acc, mean, rstd);
            // ------------------------------------------------------------ head: logits^T = (gamma W) xhat^T, xhat = hi + lo
            f32x16 lg;
#pragma unroll
            for (int r = 0; r < 16; ++r) lg[r] = 0.f;
#pragma unroll
            for (int ct = 0; ct < NB; ++ct)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float xh[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) xh[i] = acc[ct][8 * j + i] * rstd;
                    lg = head_step<3>(lg, xh, wfa[ct][j], wfl[ct][j]);
                }
            ce.row(st, lg, bk, orow, p, live, lane);
            if (live) {
                if (logits) {  // classes 0..15 of the row are registers 0..7 of the lane pair (class_natural)
                    *(float4*)(logits + orow * kKP + 4 * half) = make_float4(lg[0] + bk[0], lg[1] + bk[1], lg[2] + bk[2], lg[3] + bk[3]);
                    *(float4*)(logits + orow * kKP + 8 + 4 * half) = make_float4(lg[4] + bk[4], lg[5] + bk[5], lg[6] + bk[6], lg[7] + bk[7]);
                }
                if (half == 0 && mean_out) {
                    mean_out[orow] = mean;
                    rstd_out[orow] = rstd;
                }
            }
        }
        if constexpr (kStep) {
            if (ce.preds && live && half == 0) *(uint32_t*)(ce.preds + tok * kP) = st.pred4;  // one 128-byte line per wave and step
        }
        if constexpr (kDStep) {  // the token's 4 children as one 16-byte store per channel: 512 contiguous bytes per wave and step
            if (live && half == 0) {
                if (ce.preds) *(float4*)(ce.preds + tok * kP) = st.m4;
                float* lv = ce.preds ? (ce.n_out > 1 ? ce.preds + ce.rows : nullptr) : ce.logvar_out;
                if (lv) *(float4*)(lv + tok * kP) = st.lv4;
            }
        }
    }
    if constexpr (kDStep) {
        if (ce.partial) {
            // partial[blockIdx.x][k] = depth_metrics::store_partials' tree over the lanes (h = 128, 64, .., 1), all sums at once: the
            // loop is over, so the weights' LDS holds the [HS_DEPTH_NSUMS][256] lane sums (58 KB of the >= 80 KB)
            constexpr int NS = depth_metrics::kNSums;
            static_assert(NS * 256 * sizeof(double) <= kP * 64 * kRowB + 4 * 32 * kPatchRow, "lane sums must fit the LDS at C = 64");
            double* red = (double*)smem;
            __syncthreads();  // (every wave has left the weights and its patch)
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k * 256 + tid] = st.dsum[k];
            __syncthreads();
            for (int h = 128; h > 0; h >>= 1) {
                for (int q = tid; q < NS * h; q += 256) {
                    const int k = q / h, j = q - k * h;
                    red[k * 256 + j] += red[k * 256 + j + h];
                }
                __syncthreads();
            }
            if (tid < NS) ce.partial[(int64_t)blockIdx.x * NS + tid] = red[tid * 256];
        }
    }
    if constexpr (kStep) {
        if (ce.conf) {  // the workgroup's four histograms as one 64-bit atomic per non-zero bin; integer counts: order-independent
            __syncthreads();
            const int bins = ce.n_classes * ce.n_classes;
            if (tid < bins) {
                const uint32_t n = hist[tid] + hist[kHistBins + tid] + hist[2 * kHistBins + tid] + hist[3 * kHistBins + tid];
                if (n) atomicAdd(&ce.conf[tid], (unsigned long long)n);
            }
            if (lane == 0 && st.bad_rows) atomicAdd(&ce.bad[0], (unsigned long long)st.bad_rows);
        }
    }
    if (ce.has_loss()) {  // every wave writes its pair (zeros if it owned no rows): the host sums the array
        const float n = wave_sum(st.num), d = wave_sum(st.den);
        if (lane == 0) {
            ce.loss_part[2 * wave] = n;
            ce.loss_part[2 * wave + 1] = d;
        }
    }
}

}  // namespace
}  // namespace hs

extern "C" {

int hs_expand_ln_head_supported(int width, int children, int n_classes, int dtype) {
    return dtype == HS_BF16 && children == hs::kP && width % 32 == 0 && width >= 64 && width <= 128 && n_classes >= 1 && n_classes <= 16;
}

extern "C++" {
namespace {
template <typename Loss>
int launch_expand_ln_head(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec, void* y, float* logits,
                          float* mean, float* rstd, int64_t tokens, int width, int children, int dtype, void* stream, Loss ce,
                          const char* who) {
    using namespace hs;
    HS_CHECK_ARG(xn && wexp && wfold && bvec, "%s: null pointer", who);
    HS_CHECK_ARG(tokens > 0, "%s: bad shape", who);
    HS_CHECK_ARG((y == nullptr) == (mean == nullptr) && (mean == nullptr) == (rstd == nullptr),
                 "%s: y, mean and rstd (what the backward needs) go together", who);
    if (!hs_expand_ln_head_supported(width, children, 1, dtype))
        return fail(HS_ERR_UNSUPPORTED, "%s: bf16, 4 children, C in {64, 96, 128} (got C = %d, children %d): the expand "
                    "weight must fit the LDS", who, width, children);
    HS_CHECK_ALIGNED(who, 16, xn, xn_lo, wexp, wfold, bvec, y);  // 16-byte row chunks, weights staged into the LDS in 16-byte units
    constexpr bool kStep = std::is_same<Loss, TailCeStep>::value;
    const size_t smem = (size_t)kP * width * kRowB + 4 * 32 * kPatchRow + (kStep ? 4 * kHistBins * sizeof(uint32_t) : 0);
    HS_CHECK_ARG(smem <= 160 * 1024, "%s: %zu bytes of LDS", who, smem);  // (148 KB with the histograms at C = 128)
    const dim3 grid((unsigned)hs_expand_ln_head_blocks(tokens)), block(256);
    if constexpr (kStep) {  // a wave owns every (4 grid)-th group of 32 tokens = 128 rows: its 32-bit bins must hold them all
        const int64_t groups = (tokens + 31) / 32, waves = (int64_t)grid.x * 4;
        HS_CHECK_ARG((groups + waves - 1) / waves < (1ll << 25), "%s: %lld tokens on %lld waves overflow the 32-bit histogram bins", who,
                     (long long)tokens, (long long)waves);
    }
    return with_width_blocks<4>(width, [&](auto nb) {
        auto kern = expand_ln_head_fwd_kernel<decltype(nb)::value, Loss>;
        static bool configured = false;  // (one per instantiation)
        if (!configured) {
            HS_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
            configured = true;
        }
        hipLaunchKernelGGL(kern, grid, block, smem, (hipStream_t)stream, (const uint16_t*)xn, (const uint16_t*)xn_lo,
                           (const uint16_t*)wexp, (const uint16_t*)wfold, bvec, (uint16_t*)y, logits, mean, rstd, tokens, ce);
        HS_LAUNCH_CHECK("expand_ln_head_fwd");
        return (int)HS_OK;
    });
}
// what the entry points with a loss check before the common part
int check_ce_loss(const char* who, const void* labels, const void* loss_partials, int n_classes) {
    HS_CHECK_ARG(labels && loss_partials, "%s: null pointer", who);
    return hs::check_class_count(who, n_classes);
}
int check_depth_loss(const char* who, const void* target, const void* loss_partials, int kind, float huber_delta, int n_out) {
    HS_CHECK_ARG(target && loss_partials, "%s: null pointer", who);
    return hs::check_depth_head(who, kind, huber_delta, n_out);
}
}  // namespace
}  // extern "C++"

int64_t hs_expand_ln_head_blocks(int64_t tokens) {
    int64_t blocks = (tokens + 127) / 128;  // 4 waves x 32 tokens per workgroup and step
    const int cus = hs::usable_cus();
    if (blocks > cus) blocks = cus;
    return blocks < 1 ? 1 : blocks;
}

int hs_expand_ln_head_fwd(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec, void* y, float* logits,
                          float* mean, float* rstd, int64_t tokens, int width, int children, int dtype, void* stream) {
    HS_CHECK_ARG(logits, "hs_expand_ln_head_fwd: null pointer");
    return launch_expand_ln_head(xn, xn_lo, wexp, wfold, bvec, y, logits, mean, rstd, tokens, width, children, dtype, stream,
                                 hs::TailCe{nullptr, nullptr, nullptr, 0}, "hs_expand_ln_head_fwd");
}

int hs_expand_ln_head_ce_fwd(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec, const uint8_t* labels,
                             const float* class_weights, int n_classes, void* y, float* logits, float* mean, float* rstd,
                             float* loss_partials, int64_t tokens, int width, int children, int dtype, void* stream) {
    if (int e = check_ce_loss("hs_expand_ln_head_ce_fwd", labels, loss_partials, n_classes)) return e;
    return launch_expand_ln_head(xn, xn_lo, wexp, wfold, bvec, y, logits, mean, rstd, tokens, width, children, dtype, stream,
                                 hs::TailCe{labels, class_weights, loss_partials, n_classes}, "hs_expand_ln_head_ce_fwd");
}

int hs_expand_ln_head_ce_step_fwd(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec,
                                  const uint8_t* labels, const float* class_weights, int n_classes, void* y, float* logits, float* mean,
                                  float* rstd, float* loss_partials, uint8_t* preds, int64_t* confmat, int64_t* bad, int64_t tokens,
                                  int width, int children, int dtype, void* stream) {
    const char* who = "hs_expand_ln_head_ce_step_fwd";
    if (int e = check_ce_loss(who, labels, loss_partials, n_classes)) return e;
    HS_CHECK_ARG(!confmat || bad, "%s: confmat needs bad (the counter of labels >= n_classes)", who);
    HS_CHECK_ARG(((uintptr_t)preds & 3) == 0, "%s: preds must be 4-byte aligned", who);
    return launch_expand_ln_head(xn, xn_lo, wexp, wfold, bvec, y, logits, mean, rstd, tokens, width, children, dtype, stream,
                                 hs::TailCeStep{{labels, class_weights, loss_partials, n_classes}, preds, (unsigned long long*)confmat,
                                                (unsigned long long*)bad}, who);
}

int hs_expand_ln_head_depth_step_fwd(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec,
                                     const float* target, int kind, float huber_delta, int n_out, void* y, float* logits, float* mean,
                                     float* rstd, float* loss_partials, int flags, int transform, float shift, float scale, int use_logvar,
                                     double total_mean, const float* ranges, int n_ranges, double* metric_partials, double* metric_state,
                                     float* preds, float* logvar_out, int64_t tokens, int width, int children, int dtype, void* stream) {
    const char* who = "hs_expand_ln_head_depth_step_fwd";
    if (int e = check_depth_loss(who, target, loss_partials, kind, huber_delta, n_out)) return e;
    HS_CHECK_ARG(transform == HS_DT_NONE || transform == HS_DT_LOG || transform == HS_DT_INV, "%s: transform %d", who, transform);
    HS_CHECK_ARG((flags & ~(HS_DT_AFFINE | HS_DT_INVERSE)) == 0, "%s: flags %d (HS_DT_AFFINE or 0: the inverse chain is applied)", who, flags);
    HS_CHECK_ARG((metric_partials == nullptr) == (metric_state == nullptr), "%s: metric_partials and metric_state go together", who);
    HS_CHECK_ARG(n_out == 2 || !(logvar_out || (use_logvar && metric_state)), "%s: the log variance needs a two-channel head", who);
    hs::TailDepthStep st{{target, loss_partials, kind, huber_delta}, n_out, hs::TargetOp{flags | HS_DT_INVERSE, transform, shift, scale},
                         {}, metric_partials, preds, logvar_out, tokens * hs::kP};
    if (int e = hs::depth_metrics::fill_rule(st.rule, use_logvar, total_mean, ranges, n_ranges)) return e;
    HS_CHECK_ALIGNED(who, 16, preds, logvar_out);  // the 4 children of a token leave as one 16-byte store
    HS_CHECK_ALIGNED(who, 8, metric_partials, metric_state);
    HS_CHECK_ALIGNED(who, 4, target, loss_partials);
    if (int e = launch_expand_ln_head(xn, xn_lo, wexp, wfold, bvec, y, logits, mean, rstd, tokens, width, children, dtype, stream, st, who))
        return e;
    if (!metric_state) return HS_OK;
    // the ordered merge of hs_depth_metrics: state[k] += sum over workgroups of partial[blk][k]
    return hs::depth_metrics::launch_reduce(metric_partials, (int)hs_expand_ln_head_blocks(tokens), metric_state, (hipStream_t)stream);
}

int hs_expand_ln_head_depth_fwd(const void* xn, const void* xn_lo, const void* wexp, const void* wfold, const float* bvec, const float* target,
                                int kind, float huber_delta, int n_out, void* y, float* logits, float* mean, float* rstd, float* loss_partials,
                                int64_t tokens, int width, int children, int dtype, void* stream) {
    if (int e = check_depth_loss("hs_expand_ln_head_depth_fwd", target, loss_partials, kind, huber_delta, n_out)) return e;
    return launch_expand_ln_head(xn, xn_lo, wexp, wfold, bvec, y, logits, mean, rstd, tokens, width, children, dtype, stream,
                                 hs::TailDepth{target, loss_partials, kind, huber_delta}, "hs_expand_ln_head_depth_fwd");
}

}  // extern "C"
