// hs_weight_avg_*: a running average of the parameters -- SWA (the reference trainer's stochastic_weight_avg, training/train_config.py:112:
// torch.optim.swa_utils.AveragedModel with its default equal average) or EMA -- over the FLAT parameter buffers of optim.FlatAdam.
//
// AveragedModel deep-copies the module and updates the copy with a multi-tensor lerp over ~330 tensors; its parameters live outside the
// flat buffers and have no bf16 copies.  Here the average is one more flat fp32 buffer per bucket, laid out like the parameters, and an
// update is ONE elementwise launch per bucket (heal_swin_amd.optim.FlatWeightAverage): 8 B read + 4 B written per element.
//
// Arithmetic = AveragedModel.update_parameters: the first update copies, every later one is ATen's lerp in fp32
//   avg = w < 0.5 ? avg + w (p - avg) : p - (p - avg)(1 - w),   w = 1 / (n_averaged + 1) (SWA)  |  1 - decay (EMA)
// with n_averaged read from DEVICE memory (hs_weight_avg_advance increments it after the last bucket), so that a captured HIP graph of
// the training step replays with the right weight.  Behind the guard record of csrc/grad_guard.hip an update whose step was skipped
// (gradients not finite) writes nothing, as hs_adam_step_guarded does.
//
// hs_weight_avg_swap exchanges parameters and average in place (validation on the averaged weights, and back) and writes the bf16 copy
// of the parameters it leaves behind: the exchange moves bits, so two swaps restore everything.
#include "hs_device.h"

namespace hs {
namespace {

constexpr int kAvgBlock = 1024;  // elements per workgroup: 256 threads x one float4 (the stream shape of adam.hip)

struct WeightAvgArgs {
    float* avg;
    const float* p;
    int64_t n;
    int kind;  // 0: SWA, 1: EMA
    float decay;
    const int64_t* n_averaged;
};

// at::lerp for float: the form with the smaller error on either side of w = 0.5
__device__ __forceinline__ float lerp_one(float a, float b, float w) {
    const float diff = b - a;
    return w < 0.5f ? a + w * diff : b - diff * (1.f - w);
}

// One float4 of p and avg per thread, the tail of the buffer element by element; both loads are issued before the counter decides
// what is done with them.  The guard's flag and *n_averaged are the same for every thread of the grid.
__global__ void __launch_bounds__(256) weight_avg_kernel(const WeightAvgArgs a, const hs_grad_guard* guard, int skip_nonfinite) {
    if (guard && skip_nonfinite && !guard->finite) return;  // the step this update follows was dropped: avg stays as it is
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int64_t count = *a.n_averaged;
    const bool first = count == 0;  // the first update is a copy (the alignment gaps of p are zero, so those of avg stay zero)
    const float w = a.kind == 0 ? 1.f / (float)(count + 1) : 1.f - a.decay;
    if (i + 3 < a.n) {
        const float4 p = *(const float4*)(a.p + i);
        float4 v = *(const float4*)(a.avg + i);
        v.x = first ? p.x : lerp_one(v.x, p.x, w), v.y = first ? p.y : lerp_one(v.y, p.y, w);
        v.z = first ? p.z : lerp_one(v.z, p.z, w), v.w = first ? p.w : lerp_one(v.w, p.w, w);
        *(float4*)(a.avg + i) = v;
    } else {
        for (int64_t j = i; j < a.n; ++j) {
            const float p = a.p[j], v = a.avg[j];
            a.avg[j] = first ? p : lerp_one(v, p, w);
        }
    }
}

__global__ void weight_avg_advance_kernel(int64_t* n_averaged, const hs_grad_guard* guard, int skip_nonfinite) {
    const bool skip = guard && skip_nonfinite && !guard->finite;
    *n_averaged += skip ? 0 : 1;
}

__global__ void __launch_bounds__(256) weight_avg_swap_kernel(float* p, float* avg, uint16_t* lowp, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        const float4 was_p = *(const float4*)(p + i), now_p = *(const float4*)(avg + i);
        *(float4*)(p + i) = now_p;
        *(float4*)(avg + i) = was_p;
        if (lowp) *(uint2*)(lowp + i) = make_uint2(pack_bf16x2(now_p.x, now_p.y), pack_bf16x2(now_p.z, now_p.w));
    } else {
        for (int64_t j = i; j < n; ++j) {
            const float was_p = p[j], now_p = avg[j];
            p[j] = now_p;
            avg[j] = was_p;
            if (lowp) lowp[j] = float_to_bf16(now_p);
        }
    }
}

}  // namespace
}  // namespace hs

// the argument checks the update and the swap share (adam.hip: adam_check_buffers); every failure is HS_ERR_INVALID_ARG
static int weight_avg_check_buffers(const char* who, const float* a, const float* b, const void* lowp, int64_t n) {
    HS_CHECK_ARG(a && b, "%s: null pointer", who);
    HS_CHECK_ARG(n > 0 && n < ((int64_t)1 << 40), "%s: bad length", who);
    HS_CHECK_ARG(hs::aligned_to(16, a, b), "%s: the fp32 buffers must be 16-byte aligned", who);
    HS_CHECK_ARG(hs::aligned_to(8, lowp), "%s: the bf16 copy must be 8-byte aligned", who);
    return HS_OK;
}

extern "C" {

int hs_weight_avg_update(float* avg, const float* p, int64_t n, int kind, float decay, const int64_t* n_averaged, const hs_grad_guard* guard,
                         int skip_nonfinite, void* stream) {
    using namespace hs;
    const char* who = "hs_weight_avg_update";
    if (const int st = weight_avg_check_buffers(who, avg, p, nullptr, n)) return st;
    HS_CHECK_ARG(n_averaged, "%s: null pointer", who);
    HS_CHECK_ARG(kind == 0 || kind == 1, "%s: kind must be 0 (SWA) or 1 (EMA), got %d", who, kind);
    HS_CHECK_ARG(decay >= 0.f && decay <= 1.f, "%s: decay must be in [0, 1]", who);
    HS_CHECK_ARG(aligned_to(8, n_averaged) && aligned_to(4, guard), "%s: n_averaged (int64) or guard off its natural alignment", who);
    const WeightAvgArgs a{avg, p, n, kind, decay, n_averaged};
    const int64_t blocks = (n + kAvgBlock - 1) / kAvgBlock;
    hipLaunchKernelGGL(weight_avg_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, guard, skip_nonfinite);
    HS_LAUNCH_CHECK("weight_avg_update");
    return HS_OK;
}

int hs_weight_avg_advance(int64_t* n_averaged, const hs_grad_guard* guard, int skip_nonfinite, void* stream) {
    using namespace hs;
    HS_CHECK_ARG(n_averaged, "hs_weight_avg_advance: null pointer");
    HS_CHECK_ARG(aligned_to(8, n_averaged) && aligned_to(4, guard), "hs_weight_avg_advance: n_averaged (int64) or guard off its natural alignment");
    hipLaunchKernelGGL(weight_avg_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, n_averaged, guard, skip_nonfinite);
    HS_LAUNCH_CHECK("weight_avg_advance");
    return HS_OK;
}

int hs_weight_avg_swap(float* p, float* avg, void* p_bf16, int64_t n, void* stream) {
    using namespace hs;
    if (const int st = weight_avg_check_buffers("hs_weight_avg_swap", p, avg, p_bf16, n)) return st;
    HS_CHECK_ARG(p != avg, "hs_weight_avg_swap: p and avg are the same buffer");
    const int64_t blocks = (n + kAvgBlock - 1) / kAvgBlock;
    hipLaunchKernelGGL(weight_avg_swap_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, avg, (uint16_t*)p_bf16, n);
    HS_LAUNCH_CHECK("weight_avg_swap");
    return HS_OK;
}

}  // extern "C"
