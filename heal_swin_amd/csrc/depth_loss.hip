// Depth-regression losses of the depth caller (reference: heal_swin/training/loss_depth_regression.py, restated by
// heal_swin_amd/losses.py; per-pixel terms in hs_depth_loss.h), the depth counterpart of seg_loss.hip:
//     loss = sum_{i kept} term(pred_i, target_i) / #kept,   kept = target not infinite
//     dpred_i = scale * dterm/dpred_i (kept),  0 (not kept),   scale = upstream gradient / #kept
// One thread per pixel; the one or two channels a kind reads are fetched through explicit element strides, so the model's padded
// [B, Npix, 16] fp32 rows seen as [B, f_out, Npix] are read in place.  Deterministic: per-workgroup (sum, count) partials in a
// fixed grid, summed by the caller in a fixed order.
#include "hs_device.h"
#include "hs_depth_loss.h"

namespace hs {
namespace {

constexpr int kDlBlocks = 2048;
constexpr int kMaxChannels = 16;

struct DlArgs {
    const void* pred;
    const float* target;  // [batch, npix] contiguous
    int64_t batch, npix;
    int channels;          // channels of pred (the gradient of channels a kind does not read is 0)
    int64_t sb, sc, sp;    // element strides of pred over batch, channel, pixel
    int kind;
    float delta;
};

template <typename T>
__global__ void __launch_bounds__(256) depth_loss_fwd_kernel(DlArgs a, float* __restrict__ partials) {
    const int64_t total = a.batch * a.npix;
    float sum = 0.f, cnt = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const float t = a.target[i];
        if (!depth_keep(t)) continue;
        const int64_t b = i / a.npix, px = i - b * a.npix;
        const int64_t base = b * a.sb + px * a.sp;
        const float p0 = io<T>::load(a.pred, base);
        const float p1 = a.kind == HS_DEPTH_LOGVAR ? io<T>::load(a.pred, base + a.sc) : 0.f;
        sum += depth_term(a.kind, a.delta, p0, p1, t);
        cnt += 1.f;
    }
    __shared__ float red[2][4];
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = sum;
        red[1][wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partials[2 * blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) depth_loss_bwd_kernel(DlArgs a, const float* __restrict__ scale_p, void* __restrict__ dpred,
                                                             int64_t db, int64_t dc, int64_t dp) {
    const int64_t total = a.batch * a.npix;
    const float scale = scale_p[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const float t = a.target[i];
        const int64_t b = i / a.npix, px = i - b * a.npix;
        const int64_t base = b * a.sb + px * a.sp, dbase = b * db + px * dp;
        float g0 = 0.f, g1 = 0.f;
        if (depth_keep(t)) {  // (a masked pixel reads nothing: an overflowing exp(-log_var) there never meets its 0)
            const float p0 = io<T>::load(a.pred, base);
            const float p1 = a.kind == HS_DEPTH_LOGVAR ? io<T>::load(a.pred, base + a.sc) : 0.f;
            depth_grad(a.kind, a.delta, p0, p1, t, scale, &g0, &g1);
        }
        io<T>::store(dpred, dbase, g0);
        for (int c = 1; c < a.channels; ++c) io<T>::store(dpred, dbase + c * dc, c == 1 ? g1 : 0.f);
    }
}

int check_args(const DlArgs& a, int dtype) {
    HS_CHECK_ARG(a.pred && a.target, "null pointer");
    HS_CHECK_ARG(a.batch > 0 && a.npix > 0, "bad shape");
    HS_CHECK_ARG(a.channels >= 1 && a.channels <= kMaxChannels, "channels must be in [1, 16]");
    HS_CHECK_ARG(a.kind == HS_DEPTH_L1 || a.kind == HS_DEPTH_L2 || a.kind == HS_DEPTH_HUBER || a.kind == HS_DEPTH_LOGVAR,
                 "unknown depth loss kind %d", a.kind);
    HS_CHECK_ARG(a.kind != HS_DEPTH_HUBER || a.channels == 1, "the Huber loss needs a one-channel prediction");
    HS_CHECK_ARG(a.kind != HS_DEPTH_LOGVAR || a.channels >= 2, "the log-variance loss needs two channels (mean, log variance)");
    HS_CHECK_ARG(a.kind != HS_DEPTH_HUBER || a.delta > 0.f, "huber delta must be positive");
    HS_CHECK_ARG(dtype == HS_F32 || dtype == HS_BF16, "dtype must be HS_F32 or HS_BF16");
    return HS_OK;
}

unsigned dl_grid(int64_t total) {
    int64_t b = (total + 255) / 256;
    if (b > kDlBlocks) b = kDlBlocks;
    return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace
}  // namespace hs

extern "C" {

int64_t hs_depth_loss_partials(int64_t batch, int64_t npix) { return batch > 0 && npix > 0 ? (int64_t)hs::dl_grid(batch * npix) : 0; }

int hs_depth_loss_fwd(const void* pred, const float* target, float* partials, int64_t batch, int64_t npix, int channels,
                      int64_t stride_b, int64_t stride_c, int64_t stride_p, int kind, float huber_delta, int dtype, void* stream) {
    using namespace hs;
    const DlArgs a{pred, target, batch, npix, channels, stride_b, stride_c, stride_p, kind, huber_delta};
    if (int st = check_args(a, dtype)) return st;
    HS_CHECK_ARG(partials, "null pointer");
    const unsigned grid = dl_grid(batch * npix);
    if (dtype == HS_BF16) hipLaunchKernelGGL(depth_loss_fwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, partials);
    else hipLaunchKernelGGL(depth_loss_fwd_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, partials);
    HS_LAUNCH_CHECK("depth_loss_fwd");
    return HS_OK;
}

int hs_depth_loss_bwd(const void* pred, const float* target, const float* scale, void* dpred, int64_t batch, int64_t npix, int channels,
                      int64_t stride_b, int64_t stride_c, int64_t stride_p, int64_t dstride_b, int64_t dstride_c, int64_t dstride_p,
                      int kind, float huber_delta, int dtype, void* stream) {
    using namespace hs;
    const DlArgs a{pred, target, batch, npix, channels, stride_b, stride_c, stride_p, kind, huber_delta};
    if (int st = check_args(a, dtype)) return st;
    HS_CHECK_ARG(scale && dpred, "null pointer");
    const unsigned grid = dl_grid(batch * npix);
    if (dtype == HS_BF16)
        hipLaunchKernelGGL(depth_loss_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, scale, dpred, dstride_b,
                           dstride_c, dstride_p);
    else
        hipLaunchKernelGGL(depth_loss_bwd_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, scale, dpred, dstride_b,
                           dstride_c, dstride_p);
    HS_LAUNCH_CHECK("depth_loss_bwd");
    return HS_OK;
}

}  // extern "C"
