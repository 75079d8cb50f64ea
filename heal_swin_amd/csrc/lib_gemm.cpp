// hs_lib_gemm_nt: the library GEMM (hipBLASLt) in its full product form D = A W^T + bias + C with C != D, for the shapes where the
// library beats hs_gemm_nt (long reductions: fc2 at stages 1-3) and the residual add would otherwise cost a pass of its own.
// No kernel lives here: host code that resolves hipBLASLt at run time (no link dependency), keeps one handle per device and one
// workspace per (device, stream), picks an algorithm per shape class by a first-call trial and calls hipblasLtMatmul on the
// caller's stream.  Nothing is allocated, freed or timed while the stream is capturing.
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <hipblaslt/hipblaslt.h>
#include <link.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

#include "hs_common.h"

namespace {

constexpr size_t WORKSPACE_BYTES = size_t(32) << 20;
constexpr int MAX_CANDIDATES = 8;
constexpr int TRIAL_RUNS = 3;

// ---------------------------------------------------------------------------------------------- hipBLASLt, resolved at run time
struct Api {
    decltype(&hipblasLtCreate) Create = nullptr;
    decltype(&hipblasLtMatmulDescCreate) DescCreate = nullptr;
    decltype(&hipblasLtMatmulDescSetAttribute) DescSet = nullptr;
    decltype(&hipblasLtMatrixLayoutCreate) LayoutCreate = nullptr;
    decltype(&hipblasLtMatmulPreferenceCreate) PrefCreate = nullptr;
    decltype(&hipblasLtMatmulPreferenceSetAttribute) PrefSet = nullptr;
    decltype(&hipblasLtMatmulPreferenceDestroy) PrefDestroy = nullptr;
    decltype(&hipblasLtMatmulAlgoGetHeuristic) Heuristic = nullptr;
    decltype(&hipblasLtMatmul) Matmul = nullptr;
    bool ok = false;
};

int find_loaded(struct dl_phdr_info* info, size_t, void* out) {
    if (info->dlpi_name && strstr(info->dlpi_name, "libhipblaslt.so")) {
        snprintf(static_cast<char*>(out), 1024, "%s", info->dlpi_name);
        return 1;
    }
    return 0;
}

Api resolve() {
    Api a;
    // the copy this process already holds (a PyTorch process: torch's own) -- never a second one beside it
    char loaded[1024] = {0};
    void* so = nullptr;
    if (dl_iterate_phdr(find_loaded, loaded))
        so = dlopen(loaded, RTLD_NOLOAD | RTLD_NOW | RTLD_LOCAL);
    else {  // a process without one (a stand-alone program): the ROCm installation's
        const char* root = getenv("ROCM_PATH");
        char path[1024];
        snprintf(path, sizeof(path), "%s/lib/libhipblaslt.so", root ? root : "/opt/rocm");
        const char* names[] = {"libhipblaslt.so.1", "libhipblaslt.so", path};
        for (const char* name : names)
            if ((so = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    }
    if (!so) return a;
    bool all = true;
    auto sym = [&](auto& fn, const char* name) {
        fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(so, name));
        all = all && fn != nullptr;
    };
    sym(a.Create, "hipblasLtCreate");
    sym(a.DescCreate, "hipblasLtMatmulDescCreate");
    sym(a.DescSet, "hipblasLtMatmulDescSetAttribute");
    sym(a.LayoutCreate, "hipblasLtMatrixLayoutCreate");
    sym(a.PrefCreate, "hipblasLtMatmulPreferenceCreate");
    sym(a.PrefSet, "hipblasLtMatmulPreferenceSetAttribute");
    sym(a.PrefDestroy, "hipblasLtMatmulPreferenceDestroy");
    sym(a.Heuristic, "hipblasLtMatmulAlgoGetHeuristic");
    sym(a.Matmul, "hipblasLtMatmul");
    a.ok = all;
    return a;
}

const Api& api() {
    static const Api a = resolve();
    return a;
}

// ---------------------------------------------------------------------------------------------- per-device state
// (descriptors, layouts and handles live as long as the process: a few hundred bytes per distinct shape)
struct Problem {
    hipblasLtMatmulDesc_t desc = nullptr;
    hipblasLtMatrixLayout_t lw = nullptr, la = nullptr, ld = nullptr;
    hipblasLtMatmulHeuristicResult_t cand[MAX_CANDIDATES];
    int count = 0;
};
struct Pick {
    int index = -1;     // position among the candidates of the call that chose
    int solution = -1;  // the library's own solution index of that candidate (-1: pinned, not met yet)
    bool pinned = false;
};
using ExactKey = std::tuple<int64_t, int, int, int, int>;  // m, n, k, has_c, bias kind
using ClassKey = std::tuple<int, int, int, int>;           // rows bucket, n, k, has_c
struct Device {
    hipblasLtHandle_t handle = nullptr;
    std::map<hipStream_t, void*> workspace;
    std::map<ExactKey, Problem> problems;
    std::map<ClassKey, Pick> picks;
};

std::mutex g_mutex;
std::map<int, Device> g_devices;
bool g_enabled = true;

int rows_bucket(int64_t m) {  // bit_length(max(1, m)): the bucket of the own-kernel-or-library tuner
    int b = 0;
    for (uint64_t v = (uint64_t)(m < 1 ? 1 : m); v; v >>= 1) ++b;
    return b;
}

int solution_of(const hipblasLtMatmulAlgo_t& algo) {
    int s;
    memcpy(&s, algo.data, sizeof(s));
    return s;
}

bool capturing(hipStream_t stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) {
        (void)hipGetLastError();
        return true;  // (the legacy stream beside a capture: nothing that a capture forbids is done)
    }
    return st != hipStreamCaptureStatusNone;
}

bool usable() { return g_enabled && hs_device_count() > 0 && api().ok; }

// the descriptors of one exact shape and the library's candidates for it (host work only)
int problem_for(Device& dev, const ExactKey& key, Problem** out) {
    auto it = dev.problems.find(key);
    if (it != dev.problems.end()) {
        *out = &it->second;
        return HS_OK;
    }
    const Api& L = api();
    const auto [m, n, k, has_c, bias_kind] = key;
    Problem p;
    // row-major D [m, n] = A [m, k] W[n, k]^T is column-major D^T [n, m] = W_cm^T A_cm with W_cm [k, n], A_cm [k, m]; the bias runs along
    // the rows of D^T, i.e. along n
    bool ok = L.DescCreate(&p.desc, HIPBLAS_COMPUTE_32F, HIP_R_32F) == HIPBLAS_STATUS_SUCCESS;
    const int32_t op_t = HIPBLAS_OP_T, op_n = HIPBLAS_OP_N;
    ok = ok && L.DescSet(p.desc, HIPBLASLT_MATMUL_DESC_TRANSA, &op_t, sizeof(op_t)) == HIPBLAS_STATUS_SUCCESS;
    ok = ok && L.DescSet(p.desc, HIPBLASLT_MATMUL_DESC_TRANSB, &op_n, sizeof(op_n)) == HIPBLAS_STATUS_SUCCESS;
    if (ok && bias_kind) {
        const uint32_t epi = HIPBLASLT_EPILOGUE_BIAS;
        const int32_t bt = bias_kind == 1 ? HIP_R_16BF : HIP_R_32F;
        ok = L.DescSet(p.desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &epi, sizeof(epi)) == HIPBLAS_STATUS_SUCCESS &&
             L.DescSet(p.desc, HIPBLASLT_MATMUL_DESC_BIAS_DATA_TYPE, &bt, sizeof(bt)) == HIPBLAS_STATUS_SUCCESS;
    }
    ok = ok && L.LayoutCreate(&p.lw, HIP_R_16BF, k, n, k) == HIPBLAS_STATUS_SUCCESS;
    ok = ok && L.LayoutCreate(&p.la, HIP_R_16BF, k, m, k) == HIPBLAS_STATUS_SUCCESS;
    ok = ok && L.LayoutCreate(&p.ld, HIP_R_16BF, n, m, n) == HIPBLAS_STATUS_SUCCESS;
    hipblasLtMatmulPreference_t pref = nullptr;
    ok = ok && L.PrefCreate(&pref) == HIPBLAS_STATUS_SUCCESS;
    const uint64_t max_ws = WORKSPACE_BYTES;
    ok = ok && L.PrefSet(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &max_ws, sizeof(max_ws)) == HIPBLAS_STATUS_SUCCESS;
    int found = 0;
    ok = ok && L.Heuristic(dev.handle, p.desc, p.lw, p.la, p.ld, p.ld, pref, MAX_CANDIDATES, p.cand, &found) == HIPBLAS_STATUS_SUCCESS;
    if (pref) L.PrefDestroy(pref);
    (void)has_c;  // (C shares D's layout; beta tells the library whether it is read)
    if (!ok || found <= 0)
        return hs::fail(HS_ERR_UNSUPPORTED, "hs_lib_gemm_nt: hipBLASLt offers no algorithm for m=%lld n=%d k=%d", (long long)m, n, k);
    p.count = found;
    *out = &dev.problems.emplace(key, p).first->second;
    return HS_OK;
}

struct Operands {
    const void *a, *w, *bias, *c;
    void* d;
};

hipblasStatus_t run(Device& dev, Problem& p, int idx, const Operands& o, void* ws, size_t ws_bytes, hipStream_t stream) {
    const float one = 1.0f, zero = 0.0f;
    return api().Matmul(dev.handle, p.desc, &one, o.w, p.lw, o.a, p.la, o.c ? &one : &zero, o.c ? o.c : o.d, p.ld, o.d, p.ld,
                        &p.cand[idx].algo, ws, ws_bytes, stream);
}

// first call of a shape class: every candidate 1 + TRIAL_RUNS times on the caller's stream and operands (D is rewritten by the call
// that follows); the fastest single run counts.  Returns the candidate's position, 0 where nothing could be timed.
int trial(Device& dev, Problem& p, const Operands& o, void* ws, hipStream_t stream) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        (void)hipGetLastError();
        if (e0) (void)hipEventDestroy(e0);
        return 0;
    }
    int best = 0;
    float best_ms = -1.0f;
    for (int i = 0; i < p.count; ++i) {
        if (p.cand[i].workspaceSize > WORKSPACE_BYTES || run(dev, p, i, o, ws, WORKSPACE_BYTES, stream) != HIPBLAS_STATUS_SUCCESS) continue;
        float mine = -1.0f;
        for (int r = 0; r < TRIAL_RUNS; ++r) {
            float ms = 0.0f;
            if (hipEventRecord(e0, stream) != hipSuccess || run(dev, p, i, o, ws, WORKSPACE_BYTES, stream) != HIPBLAS_STATUS_SUCCESS ||
                hipEventRecord(e1, stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
                (void)hipGetLastError();
                mine = -1.0f;
                break;
            }
            mine = (mine < 0 || ms < mine) ? ms : mine;
        }
        if (mine >= 0 && (best_ms < 0 || mine < best_ms)) best = i, best_ms = mine;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return best;
}

int device_for_call(Device** out) {
    int id = 0;
    if (hipGetDevice(&id) != hipSuccess) {
        (void)hipGetLastError();
        return hs::fail(HS_ERR_HIP, "hs_lib_gemm: hipGetDevice failed");
    }
    Device& dev = g_devices[id];
    if (!dev.handle && api().Create(&dev.handle) != HIPBLAS_STATUS_SUCCESS) {
        dev.handle = nullptr;
        return hs::fail(HS_ERR_HIP, "hs_lib_gemm: hipblasLtCreate failed on device %d", id);
    }
    *out = &dev;
    return HS_OK;
}

int check_shape(const char* entry, int64_t m, int n, int k) {
    HS_CHECK_ARG(m > 0 && n > 0 && k > 0, "%s: m, n, k must be positive", entry);
    HS_CHECK_ARG(n % 8 == 0 && k % 8 == 0, "%s: n and k must be multiples of 8 (16-byte bf16 rows), got n=%d k=%d", entry, n, k);
    return HS_OK;
}

}  // namespace

extern "C" {

int hs_lib_gemm_supported(void) { return usable() ? 1 : 0; }

int hs_lib_gemm_set_supported(int on) {
    std::lock_guard<std::mutex> lock(g_mutex);
    g_enabled = on != 0;
    return HS_OK;
}

int hs_lib_gemm_nt(const void* a, const void* w, const void* bias, int bias_dtype, const void* c, void* d, int64_t m, int n, int k,
                   void* stream) {
    HS_CHECK_ARG(a && w && d, "hs_lib_gemm_nt: a, w and d must not be NULL");
    if (int st = check_shape("hs_lib_gemm_nt", m, n, k)) return st;
    HS_CHECK_ARG(bias == nullptr || bias_dtype == HS_BF16 || bias_dtype == HS_F32, "hs_lib_gemm_nt: bias_dtype must be HS_BF16 or HS_F32");
    const char *d0 = static_cast<const char*>(d), *d1 = d0 + 2 * m * n;
    auto overlaps = [&](const void* p, int64_t elems) {
        const char* q = static_cast<const char*>(p);
        return q && q < d1 && d0 < q + 2 * elems;
    };
    HS_CHECK_ARG(!overlaps(a, m * k) && !overlaps(w, (int64_t)n * k) && !overlaps(c, m * n),
                 "hs_lib_gemm_nt: d must not alias a, w or c (the residual is read while d is written)");
    HS_CHECK_ALIGNED("hs_lib_gemm_nt", 16, a, w, c, d);
    if (!usable()) return hs::fail(HS_ERR_UNSUPPORTED, "hs_lib_gemm_nt: hipBLASLt is not available in this process (hs_lib_gemm_supported() == 0)");

    std::lock_guard<std::mutex> lock(g_mutex);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Device* dev = nullptr;
    if (int st = device_for_call(&dev)) return st;
    Problem* p = nullptr;
    const int has_c = c != nullptr;
    if (int st = problem_for(*dev, ExactKey{m, n, k, has_c, bias ? (bias_dtype == HS_BF16 ? 1 : 2) : 0}, &p)) return st;
    if (bias && api().DescSet(p->desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bias, sizeof(bias)) != HIPBLAS_STATUS_SUCCESS)
        return hs::fail(HS_ERR_HIP, "hs_lib_gemm_nt: setting the bias pointer failed");

    const bool cap = capturing(s);
    void* ws = nullptr;
    auto wit = dev->workspace.find(s);
    if (wit != dev->workspace.end())
        ws = wit->second;
    else if (!cap) {
        if (hipMalloc(&ws, WORKSPACE_BYTES) != hipSuccess) {
            (void)hipGetLastError();
            return hs::fail(HS_ERR_HIP, "hs_lib_gemm_nt: no memory for the %zu-byte workspace", WORKSPACE_BYTES);
        }
        dev->workspace[s] = ws;
    }
    const Operands o{a, w, bias, c, d};
    const ClassKey ck{rows_bucket(m), n, k, has_c};
    int idx = 0;
    auto pit = dev->picks.find(ck);
    if (pit != dev->picks.end()) {
        Pick& pk = pit->second;
        if (pk.solution < 0) {  // pinned by position: remember which solution that is for the other row counts of the class
            idx = pk.index < p->count ? pk.index : 0;
            pk.solution = solution_of(p->cand[idx].algo);
        } else {
            idx = pk.index < p->count && solution_of(p->cand[pk.index].algo) == pk.solution ? pk.index : -1;
            for (int i = 0; idx < 0 && i < p->count; ++i)
                if (solution_of(p->cand[i].algo) == pk.solution) idx = i;
            if (idx < 0) idx = 0;
        }
    } else if (!cap) {
        idx = p->count > 1 ? trial(*dev, *p, o, ws, s) : 0;
        Pick pk;
        pk.index = idx;
        pk.solution = solution_of(p->cand[idx].algo);
        dev->picks[ck] = pk;
    }  // (capturing and never tried: the library's first candidate, and nothing is remembered)
    if (!ws && p->cand[idx].workspaceSize > 0) {  // a stream first met inside a capture has no workspace and gets none now
        idx = -1;
        for (int i = 0; idx < 0 && i < p->count; ++i)
            if (p->cand[i].workspaceSize == 0) idx = i;
        if (idx < 0) return hs::fail(HS_ERR_UNSUPPORTED, "hs_lib_gemm_nt: every candidate needs a workspace and the stream is capturing");
    }
    const hipblasStatus_t st = run(*dev, *p, idx, o, ws, ws ? WORKSPACE_BYTES : 0, s);
    if (st != HIPBLAS_STATUS_SUCCESS) {
        (void)hipGetLastError();
        return hs::fail(HS_ERR_HIP, "hs_lib_gemm_nt: hipblasLtMatmul failed (status %d) for m=%lld n=%d k=%d candidate %d", (int)st, (long long)m, n, k, idx);
    }
    return HS_OK;
}

int hs_lib_gemm_pick(int64_t m, int n, int k, int has_c, int* index, int* solution, char* name, int name_len) {
    if (int st = check_shape("hs_lib_gemm_pick", m, n, k)) return st;
    std::lock_guard<std::mutex> lock(g_mutex);
    int id = 0;
    if (hipGetDevice(&id) != hipSuccess) {
        (void)hipGetLastError();
        id = 0;
    }
    Pick pk;
    auto dit = g_devices.find(id);
    if (dit != g_devices.end()) {
        auto pit = dit->second.picks.find(ClassKey{rows_bucket(m), n, k, has_c != 0});
        if (pit != dit->second.picks.end()) pk = pit->second;
    }
    if (index) *index = pk.index;
    if (solution) *solution = pk.solution;
    if (name && name_len > 0) {
        if (pk.index < 0)
            snprintf(name, name_len, "none");
        else
            snprintf(name, name_len, "hipblaslt candidate %d solution %d%s", pk.index, pk.solution, pk.pinned ? " (pinned)" : "");
    }
    return HS_OK;
}

int hs_lib_gemm_set_pick(int64_t m, int n, int k, int has_c, int index) {
    if (int st = check_shape("hs_lib_gemm_set_pick", m, n, k)) return st;
    HS_CHECK_ARG(index >= -1 && index < MAX_CANDIDATES, "hs_lib_gemm_set_pick: index must be -1 (forget) or in [0, %d)", MAX_CANDIDATES);
    std::lock_guard<std::mutex> lock(g_mutex);
    int id = 0;
    if (hipGetDevice(&id) != hipSuccess) {
        (void)hipGetLastError();
        id = 0;
    }
    auto& picks = g_devices[id].picks;
    const ClassKey ck{rows_bucket(m), n, k, has_c != 0};
    if (index < 0) {
        picks.erase(ck);
        return HS_OK;
    }
    Pick pk;
    pk.index = index;
    pk.pinned = true;
    picks[ck] = pk;
    return HS_OK;
}

}  // extern "C"
