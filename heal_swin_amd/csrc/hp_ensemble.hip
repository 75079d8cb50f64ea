// Rotation ensembles at evaluation: the way back of hp_rotate.hip, behind hp_ensemble.HPRotationEnsemble.  A sample is predicted
// under several rotations M_m (its frame rotated by hs_hp_rotate: pixel q of the rotated frame shows the scene at M_m g_q); every
// prediction is resampled onto the UNROTATED grid and the members are averaged there.
//     d = M_m^T g_p   (the caller passes M^T as `rot`, so hs::healpix::rotated_interp runs unchanged; rot == NULL is the
//                      unrotated member: weight 1 on pixel p itself)
//     (pix[4], wgt[4]) = HEALPix get_interpol of d, nested; each weight rounded to fp32 once
//     a neighbour j is TAKEN when it is covered ((uint64) pix_j < npix), valid[b, pix_j] != 0 where a `valid` plane of the rotated
//     frame is given (hp_ensemble.valid_plane: the rotated input showed real scene there), and, for depth, its value is finite
//     seg    value_j = softmax(pred[b, :, pix_j]) in fp32 (HS_ENSEMBLE_PROB: max, exp, sum in class order, w_j / sum times e_c)
//            or the row itself (HS_ENSEMBLE_LOGIT);  acc[b, p, c] (+)= sum_j w_j value_j[c],  wsum[b, p] (+)= sum_j w_j
//     depth  acc[b, p] (+)= sum_j w_j d_j,  wsum[b, p] (+)= sum_j w_j
// Sums run over j = 0 .. 3 in order, fp32, without FMA contraction; `accumulate == 0` stores instead of adding (the first member
// needs no zero fill) and a pixel that took no neighbour leaves its accumulators alone (stores zeros when accumulate == 0).
//
// One thread per (sample, unrotated pixel); no LDS, no atomics: every accumulator has one writer, the result is bit-reproducible.
// acc rows are KP = 4 ceil(K / 4) floats, one contiguous 16-byte-vector read-modify-write per thread; the kernels are templated on
// KP with the class loops unrolled, so the two live rows (running sum, current neighbour) stay in registers.  The float64 geometry
// of hp_rotate_kernel is the larger part of the time; the rest is the accumulator traffic and the softmax.
//
// The per-pixel functions are __host__ __device__: the *_host entry points run the same statements in a plain loop (the
// exponential is the one call that differs: v_exp_f32 on the device, expf on the host).
#include <cfloat>

#include "hs_device.h"
#include "hs_healpix_device.h"
#include "hs_sphere_args.h"

#pragma clang fp contract(off)

namespace {

using hs::argmax_step;
using hs::bf16_t;
using hs::healpix::covered;
using hs::healpix::rotated_interp;
using hs::healpix::RotatedInterp;
using namespace hs::sphere;

constexpr int kMaxClasses = 16;

struct SegArgs {
    int64_t nside, npix;
    const double* rot;  // null: the unrotated member
    const void* pred;
    int64_t sb, sk, sp;
    const uint8_t* valid;  // nullable
    float* acc;
    float* wsum;
    int K, mode, accumulate;
};

struct DepthArgs {
    int64_t nside, npix;
    const double* rot;
    const void* pred;
    int64_t sb, sp;
    const uint8_t* valid;
    float* acc;
    float* wsum;
    int accumulate;
};

HS_HD float bf16_bits_to_float(uint32_t b) {
    const uint32_t w = b << 16;
    return __builtin_bit_cast(float, w);
}

// e^x for x <= 0: v_exp_f32 of x log2(e) on the device (the product's rounding, |x| 2^-24 relative, is what the tolerance of
// the tests is derived from), expf on the host
HS_HD float exp_neg(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __expf(x);
#else
    return expf(x);
#endif
}

template <typename T>
HS_HD float load_elem(const void* p, int64_t i) {
    if constexpr (std::is_same<T, float>::value) {
        return ((const float*)p)[i];
    } else {
        return bf16_bits_to_float(((const uint16_t*)p)[i]);
    }
}

// the four pixels and fp32 weights of direction rot_b g_p; without rot, pixel p itself with weight 1 (the others uncovered)
HS_HD void neighbours(int64_t nside, const double* rot, int64_t b, int64_t p, int32_t (&pix)[4], float (&w)[4]) {
    if (rot) {
        const RotatedInterp r = rotated_interp(nside, rot + 9 * b, p);
#pragma unroll
        for (int j = 0; j < 4; ++j) pix[j] = r.pix[j], w[j] = (float)r.wgt[j];
    } else {
        pix[0] = (int32_t)p, w[0] = 1.f;
#pragma unroll
        for (int j = 1; j < 4; ++j) pix[j] = -1, w[j] = 0.f;
    }
}

// z[0 .. KP): the logits row of a pixel; elements K .. KP - 1 hold whatever the padding holds (Rows16) or 0 and are never used
template <typename T, bool Rows16, int KP>
HS_HD void load_row(const SegArgs& a, int64_t base, float (&z)[KP]) {
    if constexpr (Rows16 && std::is_same<T, float>::value) {
        const float4* row = (const float4*)((const float*)a.pred + base);
#pragma unroll
        for (int q = 0; q < KP / 4; ++q) {
            const float4 v = row[q];
            z[4 * q] = v.x, z[4 * q + 1] = v.y, z[4 * q + 2] = v.z, z[4 * q + 3] = v.w;
        }
    } else if constexpr (Rows16) {  // bf16 rows are readable up to the next multiple of 8 elements
        const uint4* row = (const uint4*)((const uint16_t*)a.pred + base);
#pragma unroll
        for (int q = 0; q < (KP + 7) / 8; ++q) {
            const uint4 v = row[q];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (8 * q + j < KP) z[8 * q + j] = bf16_bits_to_float((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
        }
    } else {
#pragma unroll
        for (int c = 0; c < KP; ++c) z[c] = c < a.K ? load_elem<T>(a.pred, base + c * a.sk) : 0.f;
    }
}

template <typename T, bool Rows16, int KP>
HS_HD void add_seg_pixel(const SegArgs& a, int64_t b, int64_t p) {
    int32_t pix[4];
    float w[4];
    neighbours(a.nside, a.rot, b, p, pix, w);
    float sum[KP], wtot = 0.f;
#pragma unroll
    for (int c = 0; c < KP; ++c) sum[c] = 0.f;
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!covered(pix[j], a.npix)) continue;
        if (a.valid && !a.valid[b * a.npix + pix[j]]) continue;
        float z[KP];
        load_row<T, Rows16, KP>(a, b * a.sb + (int64_t)pix[j] * a.sp, z);
        float scale = w[j];
        if (a.mode == HS_ENSEMBLE_PROB) {
            float m = z[0];
#pragma unroll
            for (int c = 1; c < KP; ++c)
                if (c < a.K) m = fmaxf(m, z[c]);
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < KP; ++c) {
                z[c] = c < a.K ? exp_neg(z[c] - m) : 0.f;
                s += z[c];
            }
            scale = w[j] / s;
        }
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if (c < a.K) sum[c] += scale * z[c];
        wtot += w[j];
        any = true;
    }
    if (a.accumulate && !any) return;
    float4* row = (float4*)(a.acc + (b * a.npix + p) * KP);
    float& ws = a.wsum[b * a.npix + p];
#pragma unroll
    for (int q = 0; q < KP / 4; ++q) {
        float4 v = {sum[4 * q], sum[4 * q + 1], sum[4 * q + 2], sum[4 * q + 3]};
        if (a.accumulate) {
            const float4 o = row[q];
            v.x += o.x, v.y += o.y, v.z += o.z, v.w += o.w;
        }
        row[q] = v;
    }
    ws = a.accumulate ? ws + wtot : wtot;
}

template <typename T>
HS_HD void add_depth_pixel(const DepthArgs& a, int64_t b, int64_t p) {
    int32_t pix[4];
    float w[4];
    neighbours(a.nside, a.rot, b, p, pix, w);
    float sum = 0.f, wtot = 0.f;
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!covered(pix[j], a.npix)) continue;
        if (a.valid && !a.valid[b * a.npix + pix[j]]) continue;
        const float d = load_elem<T>(a.pred, b * a.sb + (int64_t)pix[j] * a.sp);
        if (!(fabsf(d) <= FLT_MAX)) continue;  // inf and NaN: no depth there
        sum += w[j] * d;
        wtot += w[j];
        any = true;
    }
    if (a.accumulate && !any) return;
    float& acc = a.acc[b * a.npix + p];
    float& ws = a.wsum[b * a.npix + p];
    acc = a.accumulate ? acc + sum : sum;
    ws = a.accumulate ? ws + wtot : wtot;
}

// grid (pixel blocks, samples)
template <typename T, bool Rows16, int KP>
__global__ void __launch_bounds__(kThreads) ensemble_add_seg_kernel(SegArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.npix) return;
    add_seg_pixel<T, Rows16, KP>(a, blockIdx.y, i);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) ensemble_add_depth_kernel(DepthArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.npix) return;
    add_depth_pixel<T>(a, blockIdx.y, i);
}

// preds: torch.max(acc, 1)'s index (argmax_step)
template <int KP>
__global__ void __launch_bounds__(kThreads) ensemble_finish_seg_kernel(int64_t npix, int K, const float* __restrict__ acc,
                                                                       const float* __restrict__ wsum, float min_weight, int background,
                                                                       uint8_t* __restrict__ preds, float* __restrict__ probs, int64_t sb,
                                                                       int64_t sk, int64_t sp) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= npix) return;
    const int64_t b = blockIdx.y;
    const float ws = wsum[b * npix + i];
    const bool live = ws > min_weight;
    float v[KP];
    const float4* row = (const float4*)(acc + (b * npix + i) * KP);
#pragma unroll
    for (int q = 0; q < KP / 4; ++q) {
        const float4 t = row[q];
        v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
    }
    float best = -INFINITY;  // class 0 wins over -inf by index
    int arg = 0;
#pragma unroll
    for (int c = 0; c < KP; ++c)
        if (c < K) argmax_step(v[c], c, best, arg);
    preds[b * npix + i] = live ? (uint8_t)arg : (uint8_t)background;
    if (probs) {
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if (c < K) probs[b * sb + c * sk + i * sp] = live ? v[c] / ws : 0.f;
    }
}

__global__ void __launch_bounds__(kThreads) ensemble_finish_depth_kernel(int64_t npix, const float* __restrict__ acc,
                                                                         const float* __restrict__ wsum, float min_weight,
                                                                         float* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= npix) return;
    const int64_t i = blockIdx.y * npix + p;
    const float ws = wsum[i];
    out[i] = ws > min_weight ? acc[i] / ws : __builtin_nanf("");
}

int check_grid(const char* who, int nside, int64_t npix, int batch) {
    if (int st = check_nside(who, nside)) return st;
    if (int st = check_npix(who, nside, npix)) return st;
    return check_batch(who, batch);
}

int elem_size(int kind) { return (kind & ~HS_PRED_ROWS16) == HS_F32 ? 4 : 2; }

int check_seg(const char* who, int nside, int64_t npix, int batch, const void* pred, int kind, int K, int64_t sb, int64_t sk, int64_t sp,
              int mode, const float* acc, const float* wsum) {
    if (int st = check_grid(who, nside, npix, batch)) return st;
    const int base = kind & ~HS_PRED_ROWS16;
    HS_CHECK_ARG((base == HS_F32 || base == HS_BF16) && (kind & ~(HS_PRED_ROWS16 | HS_BF16)) == 0,
                 "%s: prediction kind %d: expected HS_F32 or HS_BF16, HS_PRED_ROWS16 or'ed in or not", who, kind);
    HS_CHECK_ARG(K >= 1 && K <= kMaxClasses, "%s: n_classes must be in [1, %d], got %d", who, kMaxClasses, K);
    HS_CHECK_ARG(sb >= 0 && sk >= 0 && sp >= 0, "%s: negative stride", who);
    HS_CHECK_ARG(mode == HS_ENSEMBLE_PROB || mode == HS_ENSEMBLE_LOGIT, "%s: mode must be HS_ENSEMBLE_PROB or HS_ENSEMBLE_LOGIT, got %d",
                 who, mode);
    HS_CHECK_ARG(pred && acc && wsum, "%s: null pointer", who);
    const int per16 = 16 / elem_size(kind);
    const int64_t width = (K + per16 - 1) / per16 * per16;
    if (kind & HS_PRED_ROWS16)
        HS_CHECK_ARG(sk == 1 && sb % per16 == 0 && sp % per16 == 0 && ((uintptr_t)pred & 15) == 0 && sp >= width,
                     "%s: HS_PRED_ROWS16 needs contiguous, 16-byte aligned logits rows padded to 16 bytes", who);
    HS_CHECK_ALIGNED(who, 16, acc);
    const int64_t KP = (K + 3) / 4 * 4;
    const int64_t last = (kind & HS_PRED_ROWS16) ? width : (K - 1) * sk + 1;
    const int64_t pred_bytes = ((batch - 1) * sb + (npix - 1) * sp + last) * elem_size(kind);
    const int64_t acc_bytes = (int64_t)batch * npix * KP * 4, wsum_bytes = (int64_t)batch * npix * 4;
    HS_CHECK_ARG(!ranges_overlap(acc, acc_bytes, pred, pred_bytes) && !ranges_overlap(wsum, wsum_bytes, pred, pred_bytes) &&
                     !ranges_overlap(acc, acc_bytes, wsum, wsum_bytes),
                 "%s: acc / wsum overlap the predictions or each other (a pixel reads others' rows)", who);
    return HS_OK;
}

int check_depth(const char* who, int nside, int64_t npix, int batch, const void* pred, int kind, int64_t sb, int64_t sp, const float* acc,
                const float* wsum) {
    if (int st = check_grid(who, nside, npix, batch)) return st;
    if (int st = check_float_kind(who, "prediction", kind)) return st;
    HS_CHECK_ARG(sb >= 0 && sp >= 0, "%s: negative stride", who);
    HS_CHECK_ARG(pred && acc && wsum, "%s: null pointer", who);
    const int64_t pred_bytes = ((batch - 1) * sb + (npix - 1) * sp + 1) * elem_size(kind), bytes = (int64_t)batch * npix * 4;
    HS_CHECK_ARG(!ranges_overlap(acc, bytes, pred, pred_bytes) && !ranges_overlap(wsum, bytes, pred, pred_bytes) &&
                     !ranges_overlap(acc, bytes, wsum, bytes),
                 "%s: acc / wsum overlap the predictions or each other (a pixel reads others' values)", who);
    return HS_OK;
}

// f.template operator()<T, Rows16, KP>() of the prediction kind and class count
template <typename F>
void dispatch_seg(int kind, int K, F&& f) {
    const int kp = (K + 3) / 4 * 4;
#define HS_ENS_KP(T, R)                                    \
    switch (kp) {                                          \
        case 4: f.template operator()<T, R, 4>(); break;   \
        case 8: f.template operator()<T, R, 8>(); break;   \
        case 12: f.template operator()<T, R, 12>(); break; \
        default: f.template operator()<T, R, 16>(); break; \
    }
    switch (kind) {
        case HS_F32: HS_ENS_KP(float, false); break;
        case HS_F32 | HS_PRED_ROWS16: HS_ENS_KP(float, true); break;
        case HS_BF16: HS_ENS_KP(bf16_t, false); break;
        default: HS_ENS_KP(bf16_t, true); break;
    }
#undef HS_ENS_KP
}

struct LaunchSeg {
    SegArgs a;
    dim3 grid;
    hipStream_t s;
    template <typename T, bool R, int KP>
    void operator()() const {
        hipLaunchKernelGGL((ensemble_add_seg_kernel<T, R, KP>), grid, dim3(kThreads), 0, s, a);
    }
};

struct LoopSeg {
    SegArgs a;
    int batch;
    template <typename T, bool R, int KP>
    void operator()() const {
        for (int64_t b = 0; b < batch; ++b)
            for (int64_t p = 0; p < a.npix; ++p) add_seg_pixel<T, R, KP>(a, b, p);
    }
};

}  // namespace

extern "C" {

int hs_hp_ensemble_add_seg(int nside, int64_t npix, const double* rot, int batch, const void* pred, int pred_kind, int n_classes,
                           int64_t stride_b, int64_t stride_k, int64_t stride_p, const uint8_t* valid, int mode, int accumulate, float* acc,
                           float* wsum, void* stream) {
    if (int st = check_seg("hs_hp_ensemble_add_seg", nside, npix, batch, pred, pred_kind, n_classes, stride_b, stride_k, stride_p, mode, acc,
                           wsum))
        return st;
    const SegArgs a{nside, npix, rot, pred, stride_b, stride_k, stride_p, valid, acc, wsum, n_classes, mode, accumulate != 0};
    dispatch_seg(pred_kind, n_classes, LaunchSeg{a, pixel_grid(npix, batch), (hipStream_t)stream});
    HS_LAUNCH_CHECK("hp_ensemble_add_seg");
    return HS_OK;
}

int hs_hp_ensemble_add_seg_host(int nside, int64_t npix, const double* rot, int batch, const void* pred, int pred_kind, int n_classes,
                                int64_t stride_b, int64_t stride_k, int64_t stride_p, const uint8_t* valid, int mode, int accumulate,
                                float* acc, float* wsum) {
    if (int st = check_seg("hs_hp_ensemble_add_seg_host", nside, npix, batch, pred, pred_kind, n_classes, stride_b, stride_k, stride_p, mode,
                           acc, wsum))
        return st;
    const SegArgs a{nside, npix, rot, pred, stride_b, stride_k, stride_p, valid, acc, wsum, n_classes, mode, accumulate != 0};
    dispatch_seg(pred_kind, n_classes, LoopSeg{a, batch});
    return HS_OK;
}

int hs_hp_ensemble_add_depth(int nside, int64_t npix, const double* rot, int batch, const void* pred, int pred_kind, int64_t stride_b,
                             int64_t stride_p, const uint8_t* valid, int accumulate, float* acc, float* wsum, void* stream) {
    if (int st = check_depth("hs_hp_ensemble_add_depth", nside, npix, batch, pred, pred_kind, stride_b, stride_p, acc, wsum)) return st;
    const DepthArgs a{nside, npix, rot, pred, stride_b, stride_p, valid, acc, wsum, accumulate != 0};
    if (pred_kind == HS_F32) {
        hipLaunchKernelGGL(ensemble_add_depth_kernel<float>, pixel_grid(npix, batch), dim3(kThreads), 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(ensemble_add_depth_kernel<bf16_t>, pixel_grid(npix, batch), dim3(kThreads), 0, (hipStream_t)stream, a);
    }
    HS_LAUNCH_CHECK("hp_ensemble_add_depth");
    return HS_OK;
}

int hs_hp_ensemble_add_depth_host(int nside, int64_t npix, const double* rot, int batch, const void* pred, int pred_kind, int64_t stride_b,
                                  int64_t stride_p, const uint8_t* valid, int accumulate, float* acc, float* wsum) {
    if (int st = check_depth("hs_hp_ensemble_add_depth_host", nside, npix, batch, pred, pred_kind, stride_b, stride_p, acc, wsum)) return st;
    const DepthArgs a{nside, npix, rot, pred, stride_b, stride_p, valid, acc, wsum, accumulate != 0};
    for (int64_t b = 0; b < batch; ++b)
        for (int64_t p = 0; p < npix; ++p) {
            if (pred_kind == HS_F32) {
                add_depth_pixel<float>(a, b, p);
            } else {
                add_depth_pixel<bf16_t>(a, b, p);
            }
        }
    return HS_OK;
}

int hs_hp_ensemble_finish_seg(int64_t npix, int batch, int n_classes, const float* acc, const float* wsum, float min_weight, int background,
                              uint8_t* preds, float* probs, int64_t stride_b, int64_t stride_k, int64_t stride_p, void* stream) {
    const char* who = "hs_hp_ensemble_finish_seg";
    if (int st = check_pixel_count(who, "npix", npix)) return st;
    if (int st = check_batch(who, batch)) return st;
    HS_CHECK_ARG(n_classes >= 1 && n_classes <= kMaxClasses, "%s: n_classes must be in [1, %d], got %d", who, kMaxClasses, n_classes);
    HS_CHECK_ARG(background >= 0 && background <= 255, "%s: background must be in [0, 255], got %d", who, background);
    HS_CHECK_ARG(min_weight >= 0.f, "%s: min_weight must be >= 0", who);  // a NaN fails
    HS_CHECK_ARG(acc && wsum && preds, "%s: null pointer", who);
    if (probs) HS_CHECK_ARG(stride_b >= 0 && stride_k >= 0 && stride_p >= 0, "%s: negative stride", who);
    HS_CHECK_ALIGNED(who, 16, acc);
    const dim3 grid = pixel_grid(npix, batch);
    hipStream_t s = (hipStream_t)stream;
#define HS_ENS_FINISH(KP)                                                                                                                 \
    hipLaunchKernelGGL(ensemble_finish_seg_kernel<KP>, grid, dim3(kThreads), 0, s, npix, n_classes, acc, wsum, min_weight, background, preds, \
                       probs, stride_b, stride_k, stride_p)
    switch ((n_classes + 3) / 4) {
        case 1: HS_ENS_FINISH(4); break;
        case 2: HS_ENS_FINISH(8); break;
        case 3: HS_ENS_FINISH(12); break;
        default: HS_ENS_FINISH(16); break;
    }
#undef HS_ENS_FINISH
    HS_LAUNCH_CHECK("hp_ensemble_finish_seg");
    return HS_OK;
}

int hs_hp_ensemble_finish_depth(int64_t npix, int batch, const float* acc, const float* wsum, float min_weight, float* out, void* stream) {
    const char* who = "hs_hp_ensemble_finish_depth";
    if (int st = check_pixel_count(who, "npix", npix)) return st;
    if (int st = check_batch(who, batch)) return st;
    HS_CHECK_ARG(min_weight >= 0.f, "%s: min_weight must be >= 0", who);
    HS_CHECK_ARG(acc && wsum && out, "%s: null pointer", who);
    hipLaunchKernelGGL(ensemble_finish_depth_kernel, pixel_grid(npix, batch), dim3(kThreads), 0, (hipStream_t)stream, npix, acc, wsum,
                       min_weight, out);
    HS_LAUNCH_CHECK("hp_ensemble_finish_depth");
    return HS_OK;
}

}  // extern "C"
