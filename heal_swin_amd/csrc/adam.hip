// hs_adam_step: the optimizer step of the training loop over FLAT parameter / gradient / moment buffers.
//
// The reference's trainer steps torch.optim.Adam / AdamW over the model's ~330 parameter tensors
// (training/optimizer.py:57-66).  Here the gradients already live in a few flat fp32 buckets (parallel.GradBucketAllReduce);
// heal_swin_amd.optim.FlatAdam lays parameters and moments out the same way, so a step is ONE elementwise launch per bucket that
// also writes the bf16 copy of the updated parameters the next forward's GEMMs read (ops.ParamCastCache): 16 B read + 14 B written
// per parameter instead of a multi-tensor Adam (28 B) plus a separate multi-tensor cast (6 B) plus their ~40 launches -- on the
// launch-heavy HEAL-SWIN-T / nside 128 step the two were 0.86 + 0.4 ms of 16.7 ms (profiles/archive_r01_r04/r04_k_T128_summary.txt).
//
// Arithmetic = torch.optim.Adam (amsgrad = False, maximize = False), single-tensor form:
//   g += wd * p (Adam)   |   p *= 1 - lr * wd (AdamW, `decoupled`)
//   m += (g - m) (1 - b1);   v = b2 v + (1 - b2) g^2;   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// with the step count t = *step + 1 read from DEVICE memory (hs_adam_advance increments it after the last bucket), so that a
// captured HIP graph of the whole training step replays with the right bias corrections.
//
// hs_adam_step_guarded is the same step behind the guard record of csrc/grad_guard.hip: the gradient is clamped / scaled by the
// clip coefficient on its way out of the load, and a step whose gradients are not finite writes nothing.
//
// hs_adam_step_groups / hs_adam_step_groups_guarded are the same two steps with the hyper-parameters of an element taken from the
// parameter group that owns it (torch's param_groups: per-group lr, betas, eps, weight decay), still ONE launch per bucket.  The
// group records travel by value in the kernel arguments (a host-side change of a group's lr needs no copy and the launch stays
// capturable); who owns what comes from a static table in device memory built once per bucket: `runs` = (first element, group)
// of every maximal stretch of slots of one group -- a slot starts on a multiple of 8 elements, so a float4 never straddles two
// runs, and the gap behind a slot belongs to the run in front of it -- and `block_first` = the run that holds the first element
// of every 1024-element block, from where a thread walks forward to its own element: no search.
#include "hs_grad_guard.h"

namespace hs {
namespace {

constexpr int kAdamBlock = 1024;  // elements per workgroup: 256 threads x one float4 (the granularity of `block_first`)

struct AdamBuffers {
    float* p;
    const float* g;
    float* m;
    float* v;
    uint16_t* lowp;  // bf16 copy of the updated parameters, or null
    int64_t n;
};

struct AdamArgs : AdamBuffers {
    float lr;
    const float* lr_dev;  // overrides lr when non-null (a device scalar: learning-rate schedules under graph replay)
    float beta1, beta2, eps, weight_decay;
    int decoupled;
    const int64_t* step;
};

// what adam_one needs of one parameter group at one step
struct AdamHyper {
    float lr, beta1, beta2, eps, weight_decay;
    int decoupled;
    float inv_bc1, inv_sqrt_bc2;  // 1 / (1 - b1^t), 1 / sqrt(1 - b2^t)
};

struct AdamGroupArgs : AdamBuffers {
    const int64_t* step;
    const int2* runs;  // [n_runs] (first element, group), ascending; run r ends where run r + 1 starts, the last one at n
    const int32_t* block_first;  // [ceil(n / 1024)] the run that holds element 1024 b
    int n_runs, n_groups;
    hs_adam_group groups[HS_ADAM_MAX_GROUPS];
};

__device__ __forceinline__ float adam_one(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps, float wd,
                                          int decoupled, float inv_bc1, float inv_sqrt_bc2) {
    if (wd != 0.f) {
        if (decoupled) p *= 1.f - lr * wd;
        else g += wd * p;
    }
    m += (g - m) * (1.f - b1);
    v = v * b2 + (1.f - b2) * g * g;
    const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
    // (m == 0 moves nothing; skipping it keeps the zero alignment gaps of the flat buffers -- p = g = m = v = 0 -- from becoming
    // 0 / 0 when eps is 0)
    if (m != 0.f) p -= (lr * inv_bc1) * (m / denom);
    return p;
}

// bias corrections in double (torch forms them on the host in double)
__device__ __forceinline__ void adam_corrections(float beta1, float beta2, int64_t step, float& inv_bc1, float& inv_sqrt_bc2) {
    const double t = (double)(step + 1);
    inv_bc1 = (float)(1.0 / (1.0 - pow((double)beta1, t)));
    inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, t)));
}

// The stream itself: one float4 of p, g, m, v per thread (the tail of a buffer element by element), shared by every kernel below.
// hyper_of(j) gives the AdamHyper of element j and is asked in ascending j; the loads are issued before it is asked.
// GUARDED: every gradient element goes through guard_grad(., clip_value, coef) first
template <bool GUARDED, class HyperOf>
__device__ __forceinline__ void adam_stream(const AdamBuffers& a, float clip_value, float coef, HyperOf hyper_of) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < a.n) {
        float4 p = *(const float4*)(a.p + i), m = *(const float4*)(a.m + i), v = *(const float4*)(a.v + i);
        float4 g = *(const float4*)(a.g + i);
        if constexpr (GUARDED) {
            g.x = guard_grad(g.x, clip_value, coef), g.y = guard_grad(g.y, clip_value, coef);
            g.z = guard_grad(g.z, clip_value, coef), g.w = guard_grad(g.w, clip_value, coef);
        }
        const AdamHyper h = hyper_of(i);
        adam_one(p.x, g.x, m.x, v.x, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.decoupled, h.inv_bc1, h.inv_sqrt_bc2);
        adam_one(p.y, g.y, m.y, v.y, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.decoupled, h.inv_bc1, h.inv_sqrt_bc2);
        adam_one(p.z, g.z, m.z, v.z, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.decoupled, h.inv_bc1, h.inv_sqrt_bc2);
        adam_one(p.w, g.w, m.w, v.w, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.decoupled, h.inv_bc1, h.inv_sqrt_bc2);
        *(float4*)(a.p + i) = p;
        *(float4*)(a.m + i) = m;
        *(float4*)(a.v + i) = v;
        if (a.lowp) *(uint2*)(a.lowp + i) = make_uint2(pack_bf16x2(p.x, p.y), pack_bf16x2(p.z, p.w));
    } else {
        for (int64_t j = i; j < a.n; ++j) {
            float p = a.p[j], m = a.m[j], v = a.v[j];
            float g = a.g[j];
            if constexpr (GUARDED) g = guard_grad(g, clip_value, coef);
            const AdamHyper h = hyper_of(j);
            adam_one(p, g, m, v, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.decoupled, h.inv_bc1, h.inv_sqrt_bc2);
            a.p[j] = p;
            a.m[j] = m;
            a.v[j] = v;
            if (a.lowp) a.lowp[j] = float_to_bf16(p);
        }
    }
}

// one set of hyper-parameters for the whole buffer
template <bool GUARDED>
__device__ __forceinline__ void adam_body(const AdamArgs& a, float clip_value, float coef) {
    __shared__ float corr[2];
    const float lr = a.lr_dev ? *a.lr_dev : a.lr;
    if (threadIdx.x == 0) adam_corrections(a.beta1, a.beta2, *a.step, corr[0], corr[1]);  // once per workgroup
    __syncthreads();
    const AdamHyper h{lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.decoupled, corr[0], corr[1]};
    adam_stream<GUARDED>(a, clip_value, coef, [&](int64_t) { return h; });
}

// per-group hyper-parameters: thread k of the workgroup resolves group k's record (its lr, its two bias corrections -- groups may
// differ in betas) into LDS; every thread then finds the run of its element and reads that run's group from LDS
template <bool GUARDED>
__device__ __forceinline__ void adam_groups_body(const AdamGroupArgs& a, float clip_value, float coef) {
    __shared__ AdamHyper hyper[HS_ADAM_MAX_GROUPS];
    // the block's first run and the one behind it are asked for first: they arrive while the records are resolved, and a block inside
    // one run (every block of a large weight) then finds its group without a table load behind the stream's own loads
    int r = a.block_first[blockIdx.x];
    r = r < 0 ? 0 : (r < a.n_runs ? r : a.n_runs - 1);  // (a table that lies cannot send the walk outside `runs`)
    int2 cur = a.runs[r], next = a.runs[r + 1 < a.n_runs ? r + 1 : r];
    if ((int)threadIdx.x < a.n_groups) {
        const hs_adam_group& q = a.groups[threadIdx.x];
        AdamHyper h{q.lr_dev ? *q.lr_dev : q.lr, q.beta1, q.beta2, q.eps, q.weight_decay, q.decoupled, 0.f, 0.f};
        adam_corrections(q.beta1, q.beta2, *a.step, h.inv_bc1, h.inv_sqrt_bc2);
        hyper[threadIdx.x] = h;
    }
    __syncthreads();
    adam_stream<GUARDED>(a, clip_value, coef, [&](int64_t j) {
        while (r + 1 < a.n_runs && next.x <= j) {
            ++r;
            cur = next;
            next = a.runs[r + 1 < a.n_runs ? r + 1 : r];
        }
        return hyper[(unsigned)cur.y % (unsigned)a.n_groups];  // (nor the read outside the staged records)
    });
}

__global__ void __launch_bounds__(256) adam_kernel(const AdamArgs a) { adam_body<false>(a, 0.f, 1.f); }

__global__ void __launch_bounds__(256) adam_guarded_kernel(const AdamArgs a, float clip_value, const hs_grad_guard* guard, int skip_nonfinite) {
    if (skip_nonfinite && !guard->finite) return;  // (the same for every thread of the grid: p, m, v and the bf16 copy stay as they are)
    adam_body<true>(a, clip_value, guard->clip_coef);
}

__global__ void __launch_bounds__(256) adam_groups_kernel(const AdamGroupArgs a) { adam_groups_body<false>(a, 0.f, 1.f); }

__global__ void __launch_bounds__(256) adam_groups_guarded_kernel(const AdamGroupArgs a, float clip_value, const hs_grad_guard* guard,
                                                                  int skip_nonfinite) {
    if (skip_nonfinite && !guard->finite) return;  // one record for all groups: a skipped step skips every group
    adam_groups_body<true>(a, clip_value, guard->clip_coef);
}

__global__ void adam_advance_kernel(int64_t* step) { *step += 1; }

__global__ void adam_advance_guarded_kernel(int64_t* step, const hs_grad_guard* guard, int skip_nonfinite, int64_t* skipped) {
    const bool skip = skip_nonfinite && !guard->finite;
    *step += skip ? 0 : 1;
    *skipped += skip ? 1 : 0;
}

}  // namespace
}  // namespace hs

// the argument checks every step shares: buffers and step counter
static int adam_check_buffers(const char* who, const hs::AdamBuffers& a, const int64_t* step) {
    HS_CHECK_ARG(a.p && a.g && a.m && a.v && step, "%s: null pointer", who);
    HS_CHECK_ARG(a.n > 0 && a.n < ((int64_t)1 << 40), "%s: bad length", who);
    HS_CHECK_ALIGNED(who, 16, a.p, a.g, a.m, a.v);
    HS_CHECK_ALIGNED(who, 8, a.lowp);
    return HS_OK;
}

// the argument checks of hs_adam_step and hs_adam_step_guarded
static int adam_check(const char* who, const hs::AdamArgs& a) {
    if (const int st = adam_check_buffers(who, a, a.step)) return st;
    HS_CHECK_ARG(a.beta1 >= 0.f && a.beta1 < 1.f && a.beta2 >= 0.f && a.beta2 < 1.f && a.eps >= 0.f, "%s: bad hyper-parameters", who);
    return HS_OK;
}

// the argument checks of hs_adam_step_groups and hs_adam_step_groups_guarded; fills the kernel's by-value records
static int adam_groups_check(const char* who, hs::AdamGroupArgs& a, const hs_adam_group* groups, int n_blocks, int64_t covered) {
    if (const int st = adam_check_buffers(who, a, a.step)) return st;
    HS_CHECK_ARG(groups && a.runs && a.block_first, "%s: null pointer", who);
    HS_CHECK_ARG(a.n_groups >= 1 && a.n_groups <= HS_ADAM_MAX_GROUPS, "%s: the group count must be 1 ... %d, got %d", who, HS_ADAM_MAX_GROUPS,
                 a.n_groups);
    HS_CHECK_ARG(a.n < ((int64_t)1 << 31), "%s: the run table addresses elements in 32 bits: n must be below 2^31", who);
    HS_CHECK_ARG(a.n_runs >= 1 && a.n_runs <= (a.n + 7) / 8, "%s: bad run count %d (a run is at least one slot of 8 elements)", who, a.n_runs);
    HS_CHECK_ARG(n_blocks == (a.n + hs::kAdamBlock - 1) / hs::kAdamBlock, "%s: the block table must have one entry per %d elements of n", who,
                 hs::kAdamBlock);
    HS_CHECK_ARG(covered == a.n, "%s: the run table covers %lld elements, the buffers hold %lld", who, (long long)covered, (long long)a.n);
    HS_CHECK_ALIGNED(who, 8, a.runs);
    HS_CHECK_ALIGNED(who, 4, a.block_first);
    for (int k = 0; k < a.n_groups; ++k) {
        const hs_adam_group& q = groups[k];
        HS_CHECK_ARG(q.beta1 >= 0.f && q.beta1 < 1.f && q.beta2 >= 0.f && q.beta2 < 1.f && q.eps >= 0.f && q.weight_decay >= 0.f &&
                         (q.lr_dev || q.lr == q.lr),
                     "%s: bad hyper-parameters in group %d", who, k);
        HS_CHECK_ALIGNED(who, 4, q.lr_dev);
        a.groups[k] = q;
    }
    for (int k = a.n_groups; k < HS_ADAM_MAX_GROUPS; ++k) a.groups[k] = hs_adam_group{};
    return HS_OK;
}

extern "C" {

int hs_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, const float* lr_dev, float beta1,
                 float beta2, float eps, float weight_decay, int decoupled, const int64_t* step, void* stream) {
    using namespace hs;
    AdamArgs a{{p, g, m, v, (uint16_t*)p_bf16, n}, lr, lr_dev, beta1, beta2, eps, weight_decay, decoupled, step};
    if (const int st = adam_check("hs_adam_step", a)) return st;
    const int64_t blocks = (n + kAdamBlock - 1) / kAdamBlock;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    HS_LAUNCH_CHECK("adam_step");
    return HS_OK;
}

int hs_adam_step_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, const float* lr_dev, float beta1,
                         float beta2, float eps, float weight_decay, int decoupled, const int64_t* step, float clip_value,
                         const hs_grad_guard* guard, int skip_nonfinite, void* stream) {
    using namespace hs;
    AdamArgs a{{p, g, m, v, (uint16_t*)p_bf16, n}, lr, lr_dev, beta1, beta2, eps, weight_decay, decoupled, step};
    if (const int st = adam_check("hs_adam_step_guarded", a)) return st;
    HS_CHECK_ARG(guard, "hs_adam_step_guarded: null pointer");
    HS_CHECK_ALIGNED("hs_adam_step_guarded (guard)", 16, guard);
    HS_CHECK_ARG(!(clip_value != clip_value), "hs_adam_step_guarded: clip_value is NaN");
    const int64_t blocks = (n + kAdamBlock - 1) / kAdamBlock;
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, clip_value, guard, skip_nonfinite);
    HS_LAUNCH_CHECK("adam_step_guarded");
    return HS_OK;
}

int hs_adam_max_groups(void) { return HS_ADAM_MAX_GROUPS; }

int hs_adam_step_groups(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, const hs_adam_group* groups, int n_groups,
                        const int32_t* runs, int n_runs, const int32_t* block_first, int n_blocks, int64_t covered, const int64_t* step,
                        void* stream) {
    using namespace hs;
    AdamGroupArgs a{{p, g, m, v, (uint16_t*)p_bf16, n}, step, (const int2*)runs, block_first, n_runs, n_groups, {}};
    if (const int st = adam_groups_check("hs_adam_step_groups", a, groups, n_blocks, covered)) return st;
    hipLaunchKernelGGL(adam_groups_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, a);
    HS_LAUNCH_CHECK("adam_step_groups");
    return HS_OK;
}

int hs_adam_step_groups_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, const hs_adam_group* groups,
                                int n_groups, const int32_t* runs, int n_runs, const int32_t* block_first, int n_blocks, int64_t covered,
                                const int64_t* step, float clip_value, const hs_grad_guard* guard, int skip_nonfinite, void* stream) {
    using namespace hs;
    AdamGroupArgs a{{p, g, m, v, (uint16_t*)p_bf16, n}, step, (const int2*)runs, block_first, n_runs, n_groups, {}};
    if (const int st = adam_groups_check("hs_adam_step_groups_guarded", a, groups, n_blocks, covered)) return st;
    HS_CHECK_ARG(guard, "hs_adam_step_groups_guarded: null pointer");
    HS_CHECK_ALIGNED("hs_adam_step_groups_guarded (guard)", 16, guard);
    HS_CHECK_ARG(!(clip_value != clip_value), "hs_adam_step_groups_guarded: clip_value is NaN");
    hipLaunchKernelGGL(adam_groups_guarded_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, a, clip_value, guard,
                       skip_nonfinite);
    HS_LAUNCH_CHECK("adam_step_groups_guarded");
    return HS_OK;
}

int hs_adam_advance_guarded(int64_t* step, const hs_grad_guard* guard, int skip_nonfinite, int64_t* skipped, void* stream) {
    using namespace hs;
    HS_CHECK_ARG(step && guard && skipped, "hs_adam_advance_guarded: null pointer");
    HS_CHECK_ALIGNED("hs_adam_advance_guarded (guard)", 16, guard);
    hipLaunchKernelGGL(adam_advance_guarded_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, guard, skip_nonfinite, skipped);
    HS_LAUNCH_CHECK("adam_advance_guarded");
    return HS_OK;
}

int hs_adam_advance(int64_t* step, void* stream) {
    using namespace hs;
    HS_CHECK_ARG(step, "hs_adam_advance: null pointer");
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
    HS_LAUNCH_CHECK("adam_advance");
    return HS_OK;
}

}  // extern "C"
