// The flat Swin-UNet baseline scored on the sphere (heal_swin_amd/flat_evaluation.py): depth predictions of the image plane
// sampled at the HEALPix pixels through a host table (un-pad, resize and projection composed once per calibration).
//
//   hs_flat_depth_to_hp       WoodscapeDepthFlatValOnHPProjectedPredictionWriter's projected map (evaluation/
//                             flat_depth_pred_writers.py:216-239): negative Pad, Resize (nearest or bilinear) and
//                             project_depth_on_s2.sample_mask(..., s2_bkgd_class=nan) as one gather per HEALPix pixel.
//   hs_depth_metrics_gather   the same values fed straight into hs_depth_metrics' sums (hs_depth_metrics.h): the projected map is
//                             never written.  Same grid, same element-to-lane map and same merge as hs_depth_metrics, so the
//                             state equals, bit for bit, hs_depth_metrics on hs_flat_depth_to_hp's output.
//
// Both are gather-bound: one table word (nearest) or eight (bilinear) and one to four scattered prediction reads per HEALPix
// pixel and sample; neighbouring HEALPix pixels land on neighbouring image pixels, so the reads of a wave share cache lines.
#include <algorithm>

#include "hs_sphere_args.h"

#pragma clang fp contract(off)

#include "hs_depth_metrics.h"

namespace hs {
namespace {

constexpr int kThreads = depth_metrics::kThreads;

struct FlatPred {
    const void* p;
    int kind;             // HS_F32 / HS_BF16
    int64_t sb, sc, sp;   // element (b, channel c, source pixel q) at b * sb + c * sc + q * sp
    int64_t n_src;        // source pixels (or rows) per sample
    const int32_t* nearest;  // [n]: the source pixel, outside [0, n_src) where uncovered; or null:
    const int32_t* idx;      // [4][n] taps (y0 x0, y0 x1, y1 x0, y1 x1), any outside [0, n_src) where uncovered
    const float* wgt;        // [4][n] weights (h0, h1, w0, w1)
    int64_t n;               // HEALPix pixels
};

// the prediction of HEALPix pixel i of sample b, channel offset `ch` (0 or sc); NaN where uncovered
__device__ __forceinline__ float gather_pred(const FlatPred& a, int64_t b, int64_t i, int64_t ch) {
    const int64_t base = b * a.sb + ch;
    if (a.nearest) {
        const int64_t q = a.nearest[i];
        return q >= 0 && q < a.n_src ? load_val<float>(a.p, a.kind, base + q * a.sp) : NAN;  // copied, not computed: the bits survive
    }
    int64_t q[4];
    bool in = true;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        q[m] = a.idx[m * a.n + i];
        in = in && q[m] >= 0 && q[m] < a.n_src;
    }
    if (!in) return NAN;
    const float h0 = a.wgt[i], h1 = a.wgt[a.n + i], w0 = a.wgt[2 * a.n + i], w1 = a.wgt[3 * a.n + i];
    const float p00 = load_val<float>(a.p, a.kind, base + q[0] * a.sp), p01 = load_val<float>(a.p, a.kind, base + q[1] * a.sp);
    const float p10 = load_val<float>(a.p, a.kind, base + q[2] * a.sp), p11 = load_val<float>(a.p, a.kind, base + q[3] * a.sp);
    // torch's upsample_bilinear2d on the CPU: h0 * (w0 p00 + w1 p01) + h1 * (w0 p10 + w1 p11), fp32, no fused multiply-add
    return h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11);
}

__global__ void __launch_bounds__(kThreads) flat_depth_to_hp_kernel(FlatPred a, int64_t batch, float* __restrict__ out) {
    const int64_t total = a.n * batch;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t b = e / a.n, i = e - b * a.n;
        out[e] = gather_pred(a, b, i, 0);
    }
}

struct GatherTarget {
    const void* p;
    int kind;  // HS_F32 / HS_BF16
    int64_t sb, sp;
};

__global__ void __launch_bounds__(kThreads) depth_metrics_gather_kernel(FlatPred a, GatherTarget t, int64_t batch, depth_metrics::Rule rule,
                                                                        double* __restrict__ partial) {
    depth_metrics::metric_pass(rule, a.n, batch, partial, [&a, &t](int64_t b, int64_t i) {
        return std::make_tuple(gather_pred(a, b, i, 0), load_val<float>(t.p, t.kind, b * t.sb + i * t.sp),
                               [&a, b, i] { return gather_pred(a, b, i, a.sc); });
    });
}

int make_pred(const char* who, FlatPred& a, const void* pred, int kind, int64_t batch, int64_t n_src, int64_t stride_b, int64_t stride_c,
              int64_t stride_p, const int32_t* nearest, const int32_t* idx, const float* wgt, int64_t n) {
    if (int st = sphere::check_float_kind(who, "prediction", kind)) return st;
    HS_CHECK_ARG(batch > 0, "%s: batch must be positive, got %lld", who, (long long)batch);
    if (int st = sphere::check_pixel_count(who, "n_src", n_src)) return st;
    if (int st = sphere::check_pixel_count(who, "n", n)) return st;
    HS_CHECK_ARG(stride_b >= 0 && stride_c >= 0 && stride_p >= 0, "%s: negative strides", who);
    HS_CHECK_ARG((nearest != nullptr) != (idx != nullptr), "%s: give the nearest table or the bilinear taps, not both", who);
    HS_CHECK_ARG(nearest || wgt, "%s: bilinear taps need their weights", who);
    HS_CHECK_ARG(pred, "%s: null pointer", who);
    a = FlatPred{pred, kind, stride_b, stride_c, stride_p, n_src, nearest, idx, wgt, n};
    return HS_OK;
}

}  // namespace
}  // namespace hs

using namespace hs;

extern "C" {

int hs_flat_depth_to_hp(const void* pred, int kind, int64_t batch, int64_t n_src, int64_t stride_b, int64_t stride_p, const int32_t* nearest,
                        const int32_t* idx, const float* wgt, int64_t n, float* out, void* stream) {
    FlatPred a;
    if (int st = make_pred("hs_flat_depth_to_hp", a, pred, kind, batch, n_src, stride_b, 0, stride_p, nearest, idx, wgt, n)) return st;
    HS_CHECK_ARG(out, "null pointer");
    const int64_t blocks = std::min<int64_t>((n * batch + kThreads - 1) / kThreads, 4096);
    hipLaunchKernelGGL(flat_depth_to_hp_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a, batch, out);
    HS_LAUNCH_CHECK("flat_depth_to_hp");
    return HS_OK;
}

int hs_depth_metrics_gather(const void* pred, int pred_kind, int64_t batch, int64_t n_src, int64_t stride_b, int64_t stride_c, int64_t stride_p,
                            const int32_t* nearest, const int32_t* idx, const float* wgt, int64_t n, const void* target, int target_kind,
                            int64_t t_stride_b, int64_t t_stride_p, int use_logvar, double total_mean, const float* ranges, int n_ranges,
                            double* partial, double* state, void* stream) {
    const char* who = "hs_depth_metrics_gather";
    FlatPred a;
    if (int st = make_pred(who, a, pred, pred_kind, batch, n_src, stride_b, stride_c, stride_p, nearest, idx, wgt, n)) return st;
    if (int st = sphere::check_float_kind(who, "target", target_kind)) return st;
    HS_CHECK_ARG(t_stride_b >= 0 && t_stride_p >= 0, "%s: negative strides", who);
    depth_metrics::Rule rule;
    if (int st = depth_metrics::fill_rule(rule, use_logvar, total_mean, ranges, n_ranges)) return st;
    HS_CHECK_ARG(target && partial && state, "%s: null pointer", who);
    const GatherTarget t{target, target_kind, t_stride_b, t_stride_p};
    hipStream_t s = (hipStream_t)stream;
    return depth_metrics::run_pass(n * batch, partial, state, s, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(depth_metrics_gather_kernel, grid, block, 0, s, a, t, batch, rule, partial);
    });
}

}  // extern "C"
