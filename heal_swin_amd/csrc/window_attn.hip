// C-ABI entry points of the fused shift + window attention op: argument validation and dispatch
// between the MFMA paths (Ws = 64, head_dim = 32; bf16 and fp32) and the fp32-VALU path (everything else).
#include "window_attn.h"

int hs::window_attn_check_shape(const char* who, int batch, int64_t n_tokens, int channels, int num_heads, int window_size, int64_t roll,
                                int dtype) {
    HS_CHECK_ARG(dtype == HS_F32 || dtype == HS_BF16, "%s: dtype must be HS_F32 or HS_BF16", who);
    HS_CHECK_ARG(batch > 0 && n_tokens > 0 && channels > 0 && num_heads > 0, "%s: non-positive size", who);
    HS_CHECK_ARG(n_tokens < (1ll << 31), "%s: n_tokens must fit int32 (gather table is int32)", who);
    HS_CHECK_ARG((int64_t)batch * n_tokens < (1ll << 31), "%s: batch * n_tokens must fit int32 (token rows are carried as 32-bit indices)", who);
    HS_CHECK_ARG(channels % num_heads == 0, "%s: channels %d not divisible by num_heads %d", who, channels, num_heads);
    // hp_windowing.py:16 asserts a power of two.  Square nested blocks (4^k) are only needed by the relative-position index
    // and the grid shift, which are validated where those tables are built; the kernels take any power of two
    // (e.g. a last stage clamped to 8 * 4^k tokens with 8 base pixels, swin_hp_transformer.py:243-246)
    HS_CHECK_ARG((window_size & (window_size - 1)) == 0, "%s: window_size must be a power of two, got %d", who, window_size);
    HS_CHECK_ARG(window_size <= 256, "%s: window_size %d > 256 is not supported", who, window_size);
    HS_CHECK_ARG(n_tokens % window_size == 0, "%s: n_tokens %lld not divisible by window_size %d", who, (long long)n_tokens, window_size);
    HS_CHECK_ARG(window_size >= 4, "%s: window_size must be at least 4", who);
    HS_CHECK_ARG(roll >= 0 && roll < n_tokens, "%s: roll must be in [0, n_tokens)", who);
    return HS_OK;
}

namespace {

void fill_shape(hs::AttnParams& p, int batch, int64_t n_tokens, int channels, int num_heads, int window_size) {
    p.B = batch;
    p.N = n_tokens;
    p.C = channels;
    p.nH = num_heads;
    p.Ws = window_size;
    p.hd = channels / num_heads;
}

int fill_params(hs::AttnParams& p, const void* qkv, void* out, float* lse, const float* bias, const float* head_scale,
                const int32_t* idx, int64_t roll, const uint8_t* labels, int batch, int64_t n_tokens, int channels,
                int num_heads, int window_size, unsigned flags, float attn_drop, uint64_t seed, int dtype) {
    HS_CHECK_ARG(qkv && out && head_scale, "qkv, out and head_scale must not be null");
    if (int st = hs::window_attn_check_shape("hs_window_attn", batch, n_tokens, channels, num_heads, window_size, roll, dtype)) return st;
    HS_CHECK_ARG(attn_drop >= 0.f && attn_drop <= 1.f, "attn_drop must be in [0, 1]");
    p = hs::AttnParams{};
    p.drop_p = attn_drop;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);
    p.qkv = qkv;
    p.out = out;
    p.lse = lse;
    p.bias = bias;
    p.head_scale = head_scale;
    p.idx = idx;
    p.roll = idx ? 0 : roll;
    p.labels = labels;
    fill_shape(p, batch, n_tokens, channels, num_heads, window_size);
    p.flags = flags;
    return HS_OK;
}

// Which kernels serve a shape: the MFMA paths (Ws = 64, head_dim = 32; bf16 and fp32 I/O) unless HS_ATTN_FORCE_VALU asks for the
// fp32-VALU path, which also takes everything else
enum class Route { kMfmaBf16, kMfmaF32, kGeneric };
Route route_of(const hs::AttnParams& p, int dtype, unsigned flags) {
    if (flags & HS_ATTN_FORCE_VALU) return Route::kGeneric;
    if (hs::attn_mfma_supported(p, dtype)) return Route::kMfmaBf16;
    return hs::attn_mfma_f32_supported(p, dtype) ? Route::kMfmaF32 : Route::kGeneric;
}

}  // namespace

extern "C" {

int hs_window_attn_fwd(const void* qkv, void* out, float* lse, const float* bias, const float* head_scale,
                       const int32_t* idx, int64_t roll, const uint8_t* labels, int batch, int64_t n_tokens,
                       int channels, int num_heads, int window_size, unsigned flags, float attn_drop, uint64_t seed, int dtype,
                       void* stream) {
    hs::AttnParams p;
    if (int st = fill_params(p, qkv, out, lse, bias, head_scale, idx, roll, labels, batch, n_tokens, channels, num_heads,
                             window_size, flags, attn_drop, seed, dtype))
        return st;
    hipStream_t s = (hipStream_t)stream;
    switch (route_of(p, dtype, flags)) {
        case Route::kMfmaBf16: return hs::launch_attn_fwd_mfma(p, s);
        case Route::kMfmaF32: return hs::launch_attn_fwd_mfma_f32(p, s);
        default: return hs::launch_attn_fwd_generic(p, dtype, s);
    }
}

int64_t hs_window_attn_bwd_workspace(int batch, int64_t n_tokens, int channels, int num_heads, int window_size, int dtype) {
    hs::AttnParams p{};
    if (batch <= 0 || n_tokens <= 0 || channels <= 0 || num_heads <= 0 || window_size <= 0 || channels % num_heads) return 0;
    fill_shape(p, batch, n_tokens, channels, num_heads, window_size);
    switch (route_of(p, dtype, 0u)) {  // (the size an MFMA path would need, whether or not the call then forces the VALU path)
        case Route::kMfmaBf16: return hs::attn_bwd_mfma_workspace_floats(p);
        case Route::kMfmaF32: return hs::attn_bwd_mfma_f32_workspace_floats(p);
        default: return 0;
    }
}

int hs_window_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* dbias,
                       float* dhead_scale, float* workspace, const float* bias, const float* head_scale, const int32_t* idx,
                       int64_t roll, const uint8_t* labels, int batch, int64_t n_tokens, int channels, int num_heads,
                       int window_size, unsigned flags, float attn_drop, uint64_t seed, int dtype, void* stream) {
    hs::AttnParams p;
    if (int st = fill_params(p, qkv, const_cast<void*>(out), const_cast<float*>(lse), bias, head_scale, idx, roll, labels,
                             batch, n_tokens, channels, num_heads, window_size, flags, attn_drop, seed, dtype))
        return st;
    HS_CHECK_ARG(dout && dqkv && lse, "dout, dqkv and lse must not be null");
    HS_CHECK_ARG(!bias || dbias, "dbias must be given when bias is");
    HS_CHECK_ARG(!(flags & HS_ATTN_COSINE) || dhead_scale, "dhead_scale must be given for cosine attention");
    p.dout = dout;
    p.dqkv = dqkv;
    p.dbias = bias ? dbias : nullptr;
    p.dhead_scale = (flags & HS_ATTN_COSINE) ? dhead_scale : nullptr;
    hipStream_t s = (hipStream_t)stream;
    const Route route = route_of(p, dtype, flags);
    if (route == Route::kMfmaBf16) return hs::launch_attn_bwd_mfma(p, workspace, s);
    // (what the VALU backward cannot serve is refused before the zero fill below: a failing call writes nothing)
    if (route == Route::kGeneric)
        if (int st = hs::check_attn_bwd_generic(p)) return st;
    // HS_ATTN_OVERWRITE_GRADS is a contract of the ENTRY POINT: the bf16 MFMA path writes dbias / dhead_scale, every other path
    // accumulates -- so a caller that set the flag (and handed over uninitialised buffers) gets them zeroed here first
    if (flags & HS_ATTN_OVERWRITE_GRADS) {
        if (p.dbias) HS_HIP_CHECK(hipMemsetAsync(p.dbias, 0, sizeof(float) * (size_t)num_heads * window_size * window_size, s));
        if (p.dhead_scale) HS_HIP_CHECK(hipMemsetAsync(p.dhead_scale, 0, sizeof(float) * (size_t)num_heads, s));
    }
    if (route == Route::kMfmaF32) return hs::launch_attn_bwd_mfma_f32(p, workspace, s);
    return hs::launch_attn_bwd_generic(p, dtype, s);
}

}  // extern "C"
