// Evaluation of HEALPix segmentation outputs: the pipeline's other end (heal_swin_amd/evaluation.py).
//
//   hs_backproject_labels  project_hp_mask_back (heal_swin/data/segmentation/project_on_s2.py:319-341): the class of every
//                          image-plane pixel is the prediction at its nearest HEALPix pixel (a host table built once per
//                          calibration); with logits the argmax of torch.max(logits, 1) is taken on the fly.
//   hs_backproject_image   project_hp_img_back (:302-316, healpy get_interp_val): four-pixel bilinear interpolation in float64.
//   hs_backproject_depth   project_depth_hp_mask_back(..., s2_bkgd_class=nan) (data/depth_estimation/project_depth_on_s2.py:370-386):
//                          the same interpolation of fp32 / bf16 values, the map completed with NaN (heal_swin_amd/depth_evaluation.py).
//   hs_seg_confusion       the confusion matrix behind torchmetrics 0.3.2's IoU / Accuracy (bincount(target * K + pred)), in the
//                          HEALPix domain (models_lightning/segmentation/model_lightning_swin_hp.py:47-55) or on the image plane
//                          through the nearest table (evaluation/hp_pred_writers.py:110-222, custom_metrics.py:25-59).
//
// Predictions are logits (HS_F32 / HS_BF16, element (b, c, pixel) at b*stride_b + c*stride_k + pixel*stride_p, the
// hs_seg_ce_fwd convention: the model's padded [B, Npix, K] rows viewed as [B, K, Npix] are read in place) or uint8 labels
// (HS_PRED_LABELS, element (b, pixel) at b*stride_b + pixel*stride_p).  One thread per output pixel: the table entries of a
// pixel are read once and applied to every image of the batch.  All four are gathers bound by one read of the predictions.
//
// The confusion matrix is exact and deterministic: each workgroup histograms its pixels in LDS (32-bit counters; the lanes
// of a wave that share the first lane's bin add with one atomic: wave_count_lead), then adds each non-zero bin to the caller's
// int64 matrix with one global integer atomic.
#include "hs_histogram.h"
#include "hs_sphere_args.h"

#pragma clang fp contract(off)

namespace hs {
namespace {

constexpr int kThreads = 256;
constexpr int kConfBlocksMax = 2048;

struct Pred {
    const void* p;
    int64_t sb, sk, sp;
    int K;
};

struct LabelsIn {};

// Rows16: the caller guarantees (HS_PRED_ROWS16) that a pixel's K logits are contiguous, 16-byte aligned and readable up to the
// next multiple of 16 bytes; they are then read with 16-byte loads (3 instead of 10 load instructions for 10 fp32 classes: the
// gathers here are bound by the number of cache lines each load instruction touches, not by bytes).
template <typename T, bool Rows16>
__device__ __forceinline__ int pred_class(const Pred& a, int64_t b, int64_t px) {
    if constexpr (std::is_same<T, LabelsIn>::value) {
        return ((const uint8_t*)a.p)[b * a.sb + px * a.sp];
    } else {
        const int64_t base = b * a.sb + px * a.sp;
        float best = -INFINITY;  // torch.max(logits, 1)'s index (argmax_step); a NaN class 0 stays the maximum
        int arg = 0;
        if constexpr (Rows16) {
            if constexpr (std::is_same<T, float>::value) {
                const float4* row = (const float4*)((const float*)a.p + base);
                for (int c0 = 0; c0 < a.K; c0 += 4) {
                    const float4 v = row[c0 >> 2];
                    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c0 + j < a.K) argmax_step(e[j], c0 + j, best, arg);
                }
            } else {
                const uint4* row = (const uint4*)((const uint16_t*)a.p + base);
                for (int c0 = 0; c0 < a.K; c0 += 8) {
                    const uint4 v = row[c0 >> 3];
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (c0 + j < a.K) argmax_step(bf16_to_float((uint16_t)(w[j >> 1] >> (16 * (j & 1)))), c0 + j, best, arg);
                }
            }
        } else {
            for (int c = 0; c < a.K; ++c) argmax_step(io<T>::load(a.p, base + c * a.sk), c, best, arg);
        }
        return arg;
    }
}

template <typename T, bool Rows16>
__global__ void __launch_bounds__(kThreads) backproject_labels_kernel(Pred a, int64_t batch, int64_t npix,
                                                                      const int32_t* __restrict__ nearest, int64_t n_out,
                                                                      int background, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const int32_t q = nearest[i];
    const bool covered = q >= 0 && q < npix;
    for (int64_t b = 0; b < batch; ++b)
        out[b * n_out + i] = covered ? (uint8_t)pred_class<T, Rows16>(a, b, q) : (uint8_t)background;
}

// What the four-tap interpolation reads: element q of plane (or sample) p, and the value that completes the map outside [0, npix).
struct ImagePlanes {  // hs_backproject_image: contiguous uint8 planes; the reference's fill of the unused base pixels
    const uint8_t* p;
    int64_t npix;
    static __device__ __forceinline__ double fill() { return 255.0; }
    __device__ __forceinline__ double load(int64_t plane, int32_t q) const { return (double)p[plane * npix + q]; }
};
template <typename T>
struct DepthMaps {  // hs_backproject_depth: strided fp32 / bf16; the map completed to 12 base pixels with NaN (0 * NaN stays NaN)
    const void* p;
    int64_t sb, sp;
    static __device__ __forceinline__ double fill() { return (double)NAN; }
    __device__ __forceinline__ double load(int64_t b, int32_t q) const { return (double)io<T>::load(p, b * sb + q * sp); }
};

// healpy's get_interp_val through a host table of four pixels idx[m * n_out + i] and weights wgt[m * n_out + i] per output pixel
template <typename Src>
__global__ void __launch_bounds__(kThreads) backproject_interp_kernel(Src src, int64_t planes, int64_t npix, const int32_t* __restrict__ idx,
                                                                      const double* __restrict__ wgt, int64_t n_out,
                                                                      double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    int32_t q[4];
    double w[4];
    bool in[4];
    for (int m = 0; m < 4; ++m) {
        q[m] = idx[m * n_out + i];
        w[m] = wgt[m * n_out + i];
        in[m] = q[m] >= 0 && q[m] < npix;
    }
    for (int64_t p = 0; p < planes; ++p) {
        double v[4];
        for (int m = 0; m < 4; ++m) v[m] = in[m] ? src.load(p, q[m]) : Src::fill();
        // np.sum(m[p] * w, 0): ((v0 w0 + v1 w1) + v2 w2) + v3 w3, no fused multiply-add
        out[p * n_out + i] = ((v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]) + v[3] * w[3];
    }
}

// nearest == null: HEALPix domain, pixel i of n = npix.  Otherwise image plane, pixel i of n = n_out read through nearest[i];
// an uncovered pixel (nearest >= npix) counts as class `uncovered`, or is skipped when uncovered < 0.
template <typename T, bool Rows16>
__global__ void __launch_bounds__(kThreads) seg_confusion_kernel(Pred a, int64_t batch, int64_t npix, const int32_t* __restrict__ nearest,
                                                                 int64_t n, const uint8_t* __restrict__ target, int uncovered,
                                                                 unsigned long long* __restrict__ conf, unsigned long long* __restrict__ bad) {
    __shared__ uint32_t hist[kMaxSegClasses * kMaxSegClasses];
    __shared__ uint32_t bad_lds[2];
    const int K = a.K, bins = K * K;
    for (int j = threadIdx.x; j < bins; j += kThreads) hist[j] = 0;
    if (threadIdx.x < 2) bad_lds[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    uint32_t bad_target = 0, bad_pred = 0;
    // every lane runs every iteration (wave_count_lead needs the whole wave): out-of-range lanes carry bin -1
    for (int64_t base = (int64_t)blockIdx.x * kThreads; base < n; base += (int64_t)gridDim.x * kThreads) {
        const int64_t i = base + threadIdx.x;
        int64_t px = i;
        bool live = i < n;
        if (live && nearest) {
            px = nearest[i];
            if (px < 0 || px >= npix) {
                if (uncovered < 0) live = false;
                px = -1;
            }
        }
        for (int64_t b = 0; b < batch; ++b) {
            int bin = -1;
            if (live) {
                const int t = target[b * n + i];
                const int p = px >= 0 ? pred_class<T, Rows16>(a, b, px) : uncovered;
                if (t >= K) {
                    ++bad_target;
                } else if (p >= K) {
                    ++bad_pred;
                } else {
                    bin = t * K + p;
                }
            }
            wave_count_lead(hist, bin, lane);
        }
    }
    if (bad_target) atomicAdd(&bad_lds[0], bad_target);
    if (bad_pred) atomicAdd(&bad_lds[1], bad_pred);
    __syncthreads();
    for (int j = threadIdx.x; j < bins; j += kThreads) {
        const uint32_t v = hist[j];
        if (v) atomicAdd(&conf[j], (unsigned long long)v);
    }
    if (threadIdx.x < 2 && bad_lds[threadIdx.x]) atomicAdd(&bad[threadIdx.x], (unsigned long long)bad_lds[threadIdx.x]);
}

int check_pred(const char* who, const void* pred, int kind, int64_t batch, int64_t npix, int n_classes, int64_t sb, int64_t sk, int64_t sp) {
    const int base = kind & ~HS_PRED_ROWS16;
    HS_CHECK_ARG(base == HS_F32 || base == HS_BF16 || base == HS_PRED_LABELS, "%s: prediction kind %d: expected HS_F32, HS_BF16 or "
                 "HS_PRED_LABELS", who, kind);
    if (kind & HS_PRED_ROWS16) {
        const int per16 = base == HS_F32 ? 4 : 8;
        HS_CHECK_ARG(base != HS_PRED_LABELS && sk == 1 && sb % per16 == 0 && sp % per16 == 0 && ((uintptr_t)pred & 15) == 0 &&
                         sp >= (n_classes + per16 - 1) / per16 * per16,
                     "%s: HS_PRED_ROWS16 needs contiguous, 16-byte aligned logits rows padded to 16 bytes", who);
    }
    HS_CHECK_ARG(batch > 0, "%s: batch must be positive, got %lld", who, (long long)batch);
    if (int st = sphere::check_pixel_count(who, "npix", npix)) return st;
    HS_CHECK_ARG(n_classes >= 1 && n_classes <= kMaxSegClasses, "%s: n_classes must be in [1, %d], got %d", who, kMaxSegClasses, n_classes);
    HS_CHECK_ARG(pred, "%s: null prediction pointer", who);
    return HS_OK;
}

// f(T{}, Rows16{}) of a checked prediction kind: T the element type (float, bf16_t, LabelsIn), Rows16 a std::bool_constant
template <typename F>
void with_pred_kind(int kind, F&& f) {
    switch (kind) {
        case HS_F32: return f(float{}, std::false_type{});
        case HS_F32 | HS_PRED_ROWS16: return f(float{}, std::true_type{});
        case HS_BF16: return f(bf16_t{}, std::false_type{});
        case HS_BF16 | HS_PRED_ROWS16: return f(bf16_t{}, std::true_type{});
        default: return f(LabelsIn{}, std::false_type{});
    }
}

// what both interpolating entry points do after the checks of their own source: `planes` maps (or samples) of npix pixels
template <typename Src>
int launch_interp(const char* who, Src src, int64_t planes, int64_t npix, const int32_t* idx, const double* wgt, int64_t n_out, double* out,
                  void* stream) {
    HS_CHECK_ARG(planes > 0 && n_out >= 0, "%s: bad shape", who);
    if (int st = sphere::check_pixel_count(who, "npix", npix)) return st;
    if (n_out == 0) return HS_OK;
    HS_CHECK_ARG(src.p && idx && wgt && out, "%s: null pointer", who);
    hipLaunchKernelGGL(backproject_interp_kernel<Src>, dim3((unsigned)((n_out + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, src, planes, npix, idx, wgt, n_out, out);
    HS_LAUNCH_CHECK("backproject_interp");
    return HS_OK;
}

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

int hs_backproject_labels(const void* pred, int pred_kind, int64_t batch, int64_t npix, int n_classes, int64_t stride_b,
                          int64_t stride_k, int64_t stride_p, const int32_t* nearest, int64_t n_out, int background, uint8_t* out,
                          void* stream) {
    const char* who = "hs_backproject_labels";
    if (int st = check_pred(who, pred, pred_kind, batch, npix, n_classes, stride_b, stride_k, stride_p)) return st;
    HS_CHECK_ARG(n_out >= 0 && background >= 0 && background <= 255, "%s: bad n_out or background class", who);
    if (n_out == 0) return HS_OK;
    HS_CHECK_ARG(nearest && out, "%s: null pointer", who);
    const Pred a{pred, stride_b, stride_k, stride_p, n_classes};
    const dim3 grid((unsigned)((n_out + kThreads - 1) / kThreads));
    with_pred_kind(pred_kind, [&](auto t, auto rows16) {
        hipLaunchKernelGGL((backproject_labels_kernel<decltype(t), decltype(rows16)::value>), grid, dim3(kThreads), 0, (hipStream_t)stream, a,
                           batch, npix, nearest, n_out, background, out);
    });
    HS_LAUNCH_CHECK("backproject_labels");
    return HS_OK;
}

int hs_backproject_image(const uint8_t* hp_img, int64_t planes, int64_t npix, const int32_t* idx, const double* wgt, int64_t n_out,
                         double* out, void* stream) {
    return launch_interp("hs_backproject_image", ImagePlanes{hp_img, npix}, planes, npix, idx, wgt, n_out, out, stream);
}

int hs_backproject_depth(const void* pred, int kind, int64_t batch, int64_t npix, int64_t stride_b, int64_t stride_p, const int32_t* idx,
                         const double* wgt, int64_t n_out, double* out, void* stream) {
    const char* who = "hs_backproject_depth";
    if (int st = sphere::check_float_kind(who, "depth", kind)) return st;
    if (kind == HS_F32) return launch_interp(who, DepthMaps<float>{pred, stride_b, stride_p}, batch, npix, idx, wgt, n_out, out, stream);
    return launch_interp(who, DepthMaps<bf16_t>{pred, stride_b, stride_p}, batch, npix, idx, wgt, n_out, out, stream);
}

int hs_seg_confusion(const void* pred, int pred_kind, int64_t batch, int64_t npix, int n_classes, int64_t stride_b, int64_t stride_k,
                     int64_t stride_p, const int32_t* nearest, int64_t n_out, const uint8_t* target, int uncovered, int64_t* conf,
                     int64_t* bad, void* stream) {
    const char* who = "hs_seg_confusion";
    if (int st = check_pred(who, pred, pred_kind, batch, npix, n_classes, stride_b, stride_k, stride_p)) return st;
    HS_CHECK_ARG(target && conf && bad, "%s: null pointer", who);
    HS_CHECK_ARG(uncovered >= -1 && uncovered <= 255, "%s: uncovered must be a class id or -1 (skip), got %d", who, uncovered);
    const int64_t n = nearest ? n_out : npix;
    HS_CHECK_ARG(n >= 0 && n < (1ll << 31), "%s: bad pixel count %lld", who, (long long)n);
    if (n == 0) return HS_OK;
    const Pred a{pred, stride_b, stride_k, stride_p, n_classes};
    const int64_t blocks = (n + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(blocks < kConfBlocksMax ? blocks : kConfBlocksMax));
    with_pred_kind(pred_kind, [&](auto t, auto rows16) {
        hipLaunchKernelGGL((seg_confusion_kernel<decltype(t), decltype(rows16)::value>), grid, dim3(kThreads), 0, (hipStream_t)stream, a, batch,
                           npix, nearest, n, target, uncovered, (unsigned long long*)conf, (unsigned long long*)bad);
    });
    HS_LAUNCH_CHECK("seg_confusion");
    return HS_OK;
}

}  // extern "C"
