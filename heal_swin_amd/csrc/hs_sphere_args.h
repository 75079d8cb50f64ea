// Host-side argument checks and launch shapes shared by the entry points of the sphere data path (projection_aug.hip,
// hp_rotate.hip, hp_ensemble.hip, erp_project.hip, surround_project.hip) and of the evaluation path (evaluation.hip, depth_eval.hip, flat_eval.hip): the
// HEALPix grid a call names, its batch, pixel counts and element kinds, and the memory ranges it may not mix.  Host only: nothing
// here is called from a kernel.  `who` prefixes the message.
#pragma once
#include "hs_device.h"

namespace hs {
namespace sphere {

constexpr int kThreads = 256;
constexpr int kMaxBatch = 65535;  // the sample is the grid's y index
constexpr int kMaxNside = 8192;   // 12 nside^2 nested indices fit int32

// nside a power of two; int32_indices: the 12 (nside << supersample)^2 nested indices of the grid fit the int32 the kernels hold
// them in (supersample in [0, 2], checked by the caller)
inline int check_nside(const char* who, int nside, int supersample = 0, bool int32_indices = true) {
    HS_CHECK_ARG(nside >= 1 && hs::is_pow2(nside), "%s: nside must be a power of two, got %d", who, nside);
    if (int32_indices && supersample)
        HS_CHECK_ARG(nside <= (kMaxNside >> supersample), "%s: nside %d << supersample %d above %d: the nested indices are int32", who,
                     nside, supersample, kMaxNside);
    else if (int32_indices)
        HS_CHECK_ARG(nside <= kMaxNside, "%s: nside %d above %d: the nested indices are int32", who, nside, kMaxNside);
    return HS_OK;
}

// a count of pixels (`what` names the argument) that the kernels and their tables index with int32
inline int check_pixel_count(const char* who, const char* what, int64_t n) {
    HS_CHECK_ARG(n > 0 && n < (1ll << 31), "%s: %s must be in [1, 2^31), got %lld", who, what, (long long)n);
    return HS_OK;
}

// the element kind of fp32 / bf16 values (`what` names them)
inline int check_float_kind(const char* who, const char* what, int kind) {
    HS_CHECK_ARG(kind == HS_F32 || kind == HS_BF16, "%s: %s kind %d: expected HS_F32 or HS_BF16", who, what, kind);
    return HS_OK;
}

// a map on the first base_pix base pixels
inline int check_npix(const char* who, int nside, int64_t npix) {
    const int64_t npface = (int64_t)nside * nside;
    HS_CHECK_ARG(npix >= npface && npix <= 12 * npface && npix % npface == 0,
                 "%s: npix must be base_pix nside^2 with base_pix in [1, 12], got %lld for nside %d", who, (long long)npix, nside);
    return HS_OK;
}

// pixels first_pix .. first_pix + count - 1 of the full sphere
inline int check_pixel_range(const char* who, int nside, int64_t first_pix, int64_t count) {
    const int64_t npix = 12 * (int64_t)nside * nside;
    HS_CHECK_ARG(first_pix >= 0 && count >= 0 && first_pix <= npix && count <= npix - first_pix, "%s: pixel range outside [0, 12 nside^2)",
                 who);
    return HS_OK;
}

inline int check_batch(const char* who, int batch) {
    HS_CHECK_ARG(batch > 0 && batch <= kMaxBatch, "%s: batch must be in [1, %d], got %d", who, kMaxBatch, batch);
    return HS_OK;
}

// do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  A null pointer names no range.
inline bool ranges_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + (uintptr_t)b_bytes && y < x + (uintptr_t)a_bytes;
}

// grid (pixel blocks of kThreads, samples)
inline dim3 pixel_grid(int64_t n, int batch) { return dim3((unsigned)((n + kThreads - 1) / kThreads), (unsigned)batch); }

// the word of a depth fill value: the kernels copy depth as words, so that NaNs keep their bits
inline uint32_t float_word(float v) {
    uint32_t w;
    __builtin_memcpy(&w, &v, 4);
    return w;
}

}  // namespace sphere
}  // namespace hs
