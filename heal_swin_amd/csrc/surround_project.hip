// Surround view: the frames of a rig of calibrated fisheye cameras (WoodScape's FV, RV, MVL, MVR) fused onto one HEALPix sphere,
// the projection behind surround.SurroundProjector and the third table-free projector after hp_rotate.hip and erp_project.hip.
// Output pixel p of sample b is seen by camera c along d = M[b, c] g_p (M row-major, read from device memory: a captured step
// changes the rotations and the present bytes between replays).  The per-pixel statements are hs::surround::project_pixel
// (hs_surround_device.h): every present camera's polynomial fisheye model, a weight that falls off with the angle from the
// optical axis and towards the image border, then
//     frame    bilinear with clamped rows and columns, float64 without FMA; the winner's value (blend 0) or the weighted mean of
//              the counting cameras (blend 1); u8: rint clamped to [0, 255], f32: the value cast to float
//     labels, depth, camera   the winner's nearest image pixel, copied (classes never mix, NaN and inf keep their bits), and
//              the winner's index
// A pixel no camera counts for gives 0 (u8) or NaN (f32), `background`, `depth_fill`, 255, and issues no load.
//
// One thread per (sample, output pixel), the geometry of every camera evaluated once and applied to every plane given; no table
// is written (at nside 256, 12 base pixels, batch 8 and four cameras the coordinate tables of the composition would be 400 MB),
// no LDS, no atomics.  The rig travels by value in the kernel's argument segment.  Bound by float64 arithmetic: one atan2 and
// up to three divisions per present camera and pixel.
#include "hs_device.h"
#include "hs_sphere_args.h"
#include "hs_surround_device.h"

#pragma clang fp contract(off)

namespace {

using hs::surround::Args;
using hs::surround::kMaxCameras;
using hs::surround::project_pixel;
using namespace hs::sphere;

// grid (pixel blocks, samples)
template <typename T, bool Feather>
__global__ void __launch_bounds__(kThreads) surround_to_hp_kernel(Args a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.npix) return;
    project_pixel<T, Feather>(a, blockIdx.y, i);  // the matrices and the present bytes are uniform over the workgroup
}

// f.template operator()<T, Feather>() of the frame type (u8 without a frame) and of the blend.  Per frame type the compiler
// reports, for gfx950 with 256 threads and either frame type: winner 68 VGPRs, 7 waves per SIMD; feather 105 VGPRs (the eight
// cameras' weights and coordinates are 48 of them), 4 waves per SIMD; 106 SGPRs, no scratch, no LDS.  One kernel for both blends
// (110 - 112 VGPRs) would hold every winner-rule call at 4 waves.
template <typename F>
void dispatch(const Args& a, int frame_kind, F&& f) {
    const bool f32 = a.frame && frame_kind == HS_F32, feather = a.rig.blend == 1;
    if (f32 && feather) f.template operator()<float, true>();
    else if (f32) f.template operator()<float, false>();
    else if (feather) f.template operator()<uint8_t, true>();
    else f.template operator()<uint8_t, false>();
}

struct Launch {
    Args a;
    dim3 grid;
    hipStream_t s;
    template <typename T, bool Feather>
    void operator()() const {
        hipLaunchKernelGGL((surround_to_hp_kernel<T, Feather>), grid, dim3(kThreads), 0, s, a);
    }
};

struct Loop {
    Args a;
    int batch;
    template <typename T, bool Feather>
    void operator()() const {
        for (int64_t b = 0; b < batch; ++b)
            for (int64_t p = 0; p < a.npix; ++p) project_pixel<T, Feather>(a, b, p);
    }
};

// every refusal of both entry points; on HS_OK `a` is filled in
int check(const char* who, int nside, int64_t npix, const hs_surround_rig* rig, const double* rot, const uint8_t* present, int batch,
          int height, int width, const void* frame, int frame_kind, int channels, void* frame_out, const uint8_t* labels,
          uint8_t* labels_out, int background, const float* depth, float* depth_out, float depth_fill, uint8_t* camera_out, Args& a) {
    if (int st = check_nside(who, nside)) return st;
    if (int st = check_npix(who, nside, npix)) return st;
    if (int st = check_batch(who, batch)) return st;
    HS_CHECK_ARG(rig && rot, "%s: null pointer", who);
    HS_CHECK_ARG(rig->n_cameras >= 1 && rig->n_cameras <= kMaxCameras, "%s: n_cameras must be in [1, %d], got %d", who, kMaxCameras,
                 rig->n_cameras);
    HS_CHECK_ARG(height >= 1 && width >= 1 && (int64_t)height * width < (1ll << 31),
                 "%s: the images must be at least 1 x 1 with height width < 2^31, got %d x %d", who, height, width);
    const int n_cam = rig->n_cameras;
    for (int c = 0; c < n_cam; ++c) {
        const hs_fisheye_camera& cam = rig->cam[c];
        HS_CHECK_ARG(cam.poly_order >= 1 && cam.poly_order <= 8, "%s: camera %d: poly_order must be in [1, 8], got %d", who, c, cam.poly_order);
        HS_CHECK_ARG(cam.height == height && cam.width == width, "%s: camera %d is %d x %d, the images %d x %d (one size for the rig)", who, c,
                     cam.height, cam.width, height, width);
        const double mt = rig->max_theta[c];  // a NaN fails both comparisons
        HS_CHECK_ARG(mt > 0.0 && mt <= M_PI, "%s: camera %d: max_theta must be in (0, pi], got %g", who, c, mt);
    }
    HS_CHECK_ARG(rig->edge_feather >= 0.0 && rig->edge_feather <= 1.7976931348623157e308, "%s: edge_feather must be finite and >= 0, got %g",
                 who, rig->edge_feather);
    HS_CHECK_ARG(rig->blend == 0 || rig->blend == 1, "%s: blend must be 0 (winner) or 1 (feather), got %d", who, rig->blend);
    HS_CHECK_ARG(!frame == !frame_out && !labels == !labels_out && !depth == !depth_out,
                 "%s: each plane needs both its input and its output pointer, or neither", who);
    HS_CHECK_ARG(frame || labels || depth, "%s: no plane given", who);
    if (frame) {
        HS_CHECK_ARG(frame_kind == HS_U8 || frame_kind == HS_F32, "%s: frame_kind must be HS_U8 or HS_F32, got %d", who, frame_kind);
        HS_CHECK_ARG(channels >= 1 && channels <= 16, "%s: channels must be in [1, 16], got %d", who, channels);
    }
    HS_CHECK_ARG(background >= 0 && background <= 255, "%s: background must be in [0, 255], got %d", who, background);
    const int64_t src = (int64_t)batch * n_cam * height * width, dst = (int64_t)batch * npix, elem = frame_kind == HS_F32 ? 4 : 1;
    const void* in[5] = {frame, labels, depth, rot, present};
    const int64_t in_bytes[5] = {src * channels * elem, src, src * 4, (int64_t)batch * n_cam * 72, (int64_t)batch * n_cam};
    const void* out[4] = {frame_out, labels_out, depth_out, camera_out};
    const int64_t out_bytes[4] = {dst * channels * elem, dst, dst * 4, dst};
    for (int o = 0; o < 4; ++o)
        for (int i = 0; i < 5; ++i)
            HS_CHECK_ARG(!ranges_overlap(out[o], out_bytes[o], in[i], in_bytes[i]),
                         "%s: an output overlaps an input, the matrices or the present bytes (a pixel reads what another wrote)", who);
    a = Args{nside,    npix,   rot,        present,    *rig,                   height,               width,
             frame,    frame_out, channels, labels,     labels_out,             background,           (const uint32_t*)depth,
             (uint32_t*)depth_out, float_word(depth_fill), camera_out};
    return HS_OK;
}

}  // namespace

extern "C" {

int hs_surround_to_hp(int nside, int64_t npix, const hs_surround_rig* rig, const double* rot, const uint8_t* present, int batch, int height,
                      int width, const void* frame, int frame_kind, int channels, void* frame_out, const uint8_t* labels, uint8_t* labels_out,
                      int background, const float* depth, float* depth_out, float depth_fill, uint8_t* camera_out, void* stream) {
    Args a;
    if (int st = check("hs_surround_to_hp", nside, npix, rig, rot, present, batch, height, width, frame, frame_kind, channels, frame_out, labels,
                       labels_out, background, depth, depth_out, depth_fill, camera_out, a))
        return st;
    dispatch(a, frame_kind, Launch{a, pixel_grid(npix, batch), (hipStream_t)stream});
    HS_LAUNCH_CHECK("surround_to_hp");
    return HS_OK;
}

int hs_surround_to_hp_host(int nside, int64_t npix, const hs_surround_rig* rig, const double* rot, const uint8_t* present, int batch,
                           int height, int width, const void* frame, int frame_kind, int channels, void* frame_out, const uint8_t* labels,
                           uint8_t* labels_out, int background, const float* depth, float* depth_out, float depth_fill, uint8_t* camera_out) {
    Args a;
    if (int st = check("hs_surround_to_hp_host", nside, npix, rig, rot, present, batch, height, width, frame, frame_kind, channels, frame_out,
                       labels, labels_out, background, depth, depth_out, depth_fill, camera_out, a))
        return st;
    dispatch(a, frame_kind, Loop{a, batch});
    return HS_OK;
}

}  // extern "C"
