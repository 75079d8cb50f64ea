// Equirectangular panoramas onto the sphere: the projection behind erp.ERPProjector, the full-sphere counterpart of the
// fisheye projection (projection.hip, projection_aug.hip).  Output pixel p of sample b shows the panorama at direction
// d = M_b g_p (the convention of hs_hp_rotated_coords; M_b row-major, read from device memory: a captured step changes the
// rotations between replays).  The per-pixel statements are hs::erp::project_pixel (hs_erp_device.h):
//     frame   bilinear, columns wrap and rows clamp, float64 without FMA; with supersample = s the mean over the centres of the
//             4^s nested children; u8: rint clamped to [0, 255], f32: the value cast to float
//     labels  the nearest panorama pixel, copied: classes never mix
//     depth   the nearest panorama pixel's word, copied: NaN and inf keep their bits
// A non-finite matrix or direction gives 0 (u8) or NaN (f32), `background`, `depth_fill`, and issues no load.
//
// One thread per (sample, output pixel), the geometry evaluated once and applied to every plane given; no table is written (at
// nside 256 and 12 base pixels a per-sample coordinate table would be 12.6 MB per sample), no LDS, no atomics.  Bound by float64
// transcendental throughput like hp_rotate_kernel (sincos, hypot, two atan2 per pixel centre; 4^s centres with supersampling),
// against 4 scattered loads per channel and centre.
#include "hs_device.h"
#include "hs_erp_device.h"
#include "hs_sphere_args.h"

#pragma clang fp contract(off)

namespace {

using hs::erp::Args;
using hs::erp::project_pixel;
using namespace hs::sphere;

// grid (pixel blocks, samples)
template <typename T, bool Super>
__global__ void __launch_bounds__(kThreads) erp_to_hp_kernel(Args a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.npix) return;
    project_pixel<T, Super>(a, blockIdx.y, i);  // the matrix is uniform over the workgroup
}

// f.template operator()<T, Super>() of the frame type (u8 without a frame) and of supersample > 0
template <typename F>
void dispatch(const Args& a, int frame_kind, F&& f) {
    const bool f32 = a.frame && frame_kind == HS_F32, super = a.supersample > 0;
    if (f32 && super) f.template operator()<float, true>();
    else if (f32) f.template operator()<float, false>();
    else if (super) f.template operator()<uint8_t, true>();
    else f.template operator()<uint8_t, false>();
}

struct Launch {
    Args a;
    dim3 grid;
    hipStream_t s;
    template <typename T, bool Super>
    void operator()() const {
        hipLaunchKernelGGL((erp_to_hp_kernel<T, Super>), grid, dim3(kThreads), 0, s, a);
    }
};

struct Loop {
    Args a;
    int batch;
    template <typename T, bool Super>
    void operator()() const {
        for (int64_t b = 0; b < batch; ++b)
            for (int64_t p = 0; p < a.npix; ++p) project_pixel<T, Super>(a, b, p);
    }
};

// every refusal of both entry points; on HS_OK `a` is filled in
int check(const char* who, int nside, int64_t npix, const double* rot, int batch, int height, int width, int supersample,
          const void* frame, int frame_kind, int channels, void* frame_out, const uint8_t* labels, uint8_t* labels_out, int background,
          const float* depth, float* depth_out, float depth_fill, Args& a) {
    HS_CHECK_ARG(supersample >= 0 && supersample <= 2, "%s: supersample must be 0, 1 or 2, got %d", who, supersample);
    if (int st = check_nside(who, nside, supersample)) return st;
    if (int st = check_npix(who, nside, npix)) return st;
    if (int st = check_batch(who, batch)) return st;
    HS_CHECK_ARG(height >= 1 && width >= 1 && (int64_t)height * width < (1ll << 31),
                 "%s: the panorama must be at least 1 x 1 with height width < 2^31, got %d x %d", who, height, width);
    HS_CHECK_ARG(!frame == !frame_out && !labels == !labels_out && !depth == !depth_out,
                 "%s: each plane needs both its input and its output pointer, or neither", who);
    HS_CHECK_ARG(frame || labels || depth, "%s: no plane given", who);
    if (frame) {
        HS_CHECK_ARG(frame_kind == HS_U8 || frame_kind == HS_F32, "%s: frame_kind must be HS_U8 or HS_F32, got %d", who, frame_kind);
        HS_CHECK_ARG(channels >= 1 && channels <= 16, "%s: channels must be in [1, 16], got %d", who, channels);
    }
    HS_CHECK_ARG(background >= 0 && background <= 255, "%s: background must be in [0, 255], got %d", who, background);
    HS_CHECK_ARG(rot, "%s: null pointer", who);
    const int64_t src = (int64_t)batch * height * width, dst = (int64_t)batch * npix, elem = frame_kind == HS_F32 ? 4 : 1;
    const void* in[4] = {frame, labels, depth, rot};
    const int64_t in_bytes[4] = {src * channels * elem, src, src * 4, (int64_t)batch * 72};
    const void* out[3] = {frame_out, labels_out, depth_out};
    const int64_t out_bytes[3] = {dst * channels * elem, dst, dst * 4};
    for (int o = 0; o < 3; ++o)
        for (int i = 0; i < 4; ++i)
            HS_CHECK_ARG(!ranges_overlap(out[o], out_bytes[o], in[i], in_bytes[i]),
                         "%s: an output overlaps an input (a pixel reads others' source values)", who);
    a = Args{nside,     npix,     rot,    height,     width,      supersample,            frame,
             frame_out, channels, labels, labels_out, background, (const uint32_t*)depth, (uint32_t*)depth_out, float_word(depth_fill)};
    return HS_OK;
}

}  // namespace

extern "C" {

int hs_erp_to_hp(int nside, int64_t npix, const double* rot, int batch, int height, int width, int supersample, const void* frame,
                 int frame_kind, int channels, void* frame_out, const uint8_t* labels, uint8_t* labels_out, int background,
                 const float* depth, float* depth_out, float depth_fill, void* stream) {
    Args a;
    if (int st = check("hs_erp_to_hp", nside, npix, rot, batch, height, width, supersample, frame, frame_kind, channels, frame_out, labels,
                       labels_out, background, depth, depth_out, depth_fill, a))
        return st;
    dispatch(a, frame_kind, Launch{a, pixel_grid(npix, batch), (hipStream_t)stream});
    HS_LAUNCH_CHECK("erp_to_hp");
    return HS_OK;
}

int hs_erp_to_hp_host(int nside, int64_t npix, const double* rot, int batch, int height, int width, int supersample, const void* frame,
                      int frame_kind, int channels, void* frame_out, const uint8_t* labels, uint8_t* labels_out, int background,
                      const float* depth, float* depth_out, float depth_fill) {
    Args a;
    if (int st = check("hs_erp_to_hp_host", nside, npix, rot, batch, height, width, supersample, frame, frame_kind, channels, frame_out,
                       labels, labels_out, background, depth, depth_out, depth_fill, a))
        return st;
    dispatch(a, frame_kind, Loop{a, batch});
    return HS_OK;
}

}  // extern "C"
