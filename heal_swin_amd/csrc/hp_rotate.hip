// Rotation of maps that already live on the sphere: the sphere-to-sphere resampler behind hp_rotate.HPRotator, the augmentation of
// a dataset that was projected once, offline (hp_img / hp_mask / depth read from stored HEALPix maps; no frame is at hand).
//     g = centre of nested output pixel p, d = M_b g                (M_b row-major, read from device memory: a captured step
//                                                                    changes the rotations between replays)
//     (pix[4], wgt[4], nearest) = HEALPix get_interpol of d, nested  (hs::healpix::rotated_interp, hs_healpix_device.h: healpy's
//                                                                    get_interp_weights, per (sample, pixel), on the device)
//     frame   rint(((w0 v0 + w1 v1) + w2 v2) + w3 v3) clamped to [0, 255], float64 without FMA, an uncovered neighbour reads 0.0
//     labels  labels[b, nearest], `background` where uncovered: classes never mix
//     depth   depth[b, nearest] copied bit for bit, `depth_fill` where uncovered
// A source index is covered iff (uint64_t) idx < (uint64_t) npix (hs::healpix::covered), compared before every load: the base
// pixels the map does not hold, and the -1 of a non-finite matrix, are uncovered.  Convention of hs_hp_rotated_coords: output
// pixel p shows the source map at direction M_b g_p.
//
// One thread per (sample, output pixel), the geometry evaluated once and applied to every plane given; no table is written, no
// LDS, no atomics.  Bound by float64 transcendental throughput like hp_rotated_coords_kernel (sincos, hypot, two atan2, cos,
// fmod and, per bracketing ring, acos or atan2), against 4 scattered byte loads per channel.
#include "hs_device.h"
#include "hs_healpix_device.h"
#include "hs_sphere_args.h"

#pragma clang fp contract(off)

namespace {

using hs::healpix::covered;
using hs::healpix::rotated_interp;
using hs::healpix::RotatedInterp;
using hs::healpix::store_interp;
using namespace hs::sphere;

// grid (pixel blocks, samples)
__global__ void __launch_bounds__(kThreads) hp_rotated_interp_kernel(int64_t nside, int64_t first_pix, int64_t count,
                                                                     const double* __restrict__ rot, int32_t* __restrict__ pix,
                                                                     double* __restrict__ wgt, int32_t* __restrict__ nearest) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const int64_t b = blockIdx.y;
    // the matrix is uniform over the workgroup
    store_interp(rotated_interp(nside, rot + 9 * b, first_pix + i), b, i, count, pix, wgt, nearest);
}

__global__ void __launch_bounds__(kThreads) hp_rotate_kernel(int64_t nside, int64_t npix, const double* __restrict__ rot,
                                                             const uint8_t* __restrict__ img, int channels, uint8_t* __restrict__ img_out,
                                                             const uint8_t* __restrict__ labels, uint8_t* __restrict__ labels_out,
                                                             int background, const uint32_t* __restrict__ depth,
                                                             uint32_t* __restrict__ depth_out, uint32_t depth_fill) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= npix) return;
    const int64_t b = blockIdx.y;
    const RotatedInterp r = rotated_interp(nside, rot + 9 * b, i);
    if (img) {
        const bool c0 = covered(r.pix[0], npix), c1 = covered(r.pix[1], npix), c2 = covered(r.pix[2], npix), c3 = covered(r.pix[3], npix);
        for (int c = 0; c < channels; ++c) {
            const uint8_t* src = img + (b * channels + c) * npix;
            const double v0 = c0 ? (double)src[r.pix[0]] : 0.0, v1 = c1 ? (double)src[r.pix[1]] : 0.0;
            const double v2 = c2 ? (double)src[r.pix[2]] : 0.0, v3 = c3 ? (double)src[r.pix[3]] : 0.0;
            double v = rint(((r.wgt[0] * v0 + r.wgt[1] * v1) + r.wgt[2] * v2) + r.wgt[3] * v3);  // half to even
            v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
            img_out[(b * channels + c) * npix + i] = (uint8_t)(int)v;
        }
    }
    const bool cn = covered(r.nearest, npix);
    if (labels) labels_out[b * npix + i] = cn ? labels[b * npix + r.nearest] : (uint8_t)background;
    if (depth) depth_out[b * npix + i] = cn ? depth[b * npix + r.nearest] : depth_fill;  // the word, not the value: NaNs keep their bits
}

// the grid, the pixel sub-range and the batch of the two hs_hp_rotated_interp entry points
int check_range(const char* who, int nside, int64_t first_pix, int64_t count, int batch) {
    if (int st = check_nside(who, nside)) return st;
    if (int st = check_pixel_range(who, nside, first_pix, count)) return st;
    return check_batch(who, batch);
}

}  // namespace

extern "C" {

int hs_hp_rotated_interp(int nside, int64_t first_pix, int64_t count, const double* rot, int batch, int32_t* pix, double* wgt,
                         int32_t* nearest, void* stream) {
    if (int st = check_range("hs_hp_rotated_interp", nside, first_pix, count, batch)) return st;
    if (count == 0) return HS_OK;
    HS_CHECK_ARG(rot && pix && wgt && nearest, "hs_hp_rotated_interp: null pointer");
    hipLaunchKernelGGL(hp_rotated_interp_kernel, pixel_grid(count, batch), dim3(kThreads), 0, (hipStream_t)stream, (int64_t)nside,
                       first_pix, count, rot, pix, wgt, nearest);
    HS_LAUNCH_CHECK("hp_rotated_interp");
    return HS_OK;
}

int hs_hp_rotated_interp_host(int nside, int64_t first_pix, int64_t count, const double* rot, int batch, int32_t* pix, double* wgt,
                              int32_t* nearest) {
    if (int st = check_range("hs_hp_rotated_interp_host", nside, first_pix, count, batch)) return st;
    if (count == 0) return HS_OK;
    HS_CHECK_ARG(rot && pix && wgt && nearest, "hs_hp_rotated_interp_host: null pointer");
    for (int64_t b = 0; b < batch; ++b)
        for (int64_t i = 0; i < count; ++i)
            store_interp(rotated_interp(nside, rot + 9 * b, first_pix + i), b, i, count, pix, wgt, nearest);
    return HS_OK;
}

int hs_hp_rotate(int nside, int64_t npix, const double* rot, int batch, const uint8_t* img, int channels, uint8_t* img_out,
                 const uint8_t* labels, uint8_t* labels_out, int background, const float* depth, float* depth_out, float depth_fill,
                 void* stream) {
    const char* who = "hs_hp_rotate";
    if (int st = check_nside(who, nside)) return st;
    if (int st = check_npix(who, nside, npix)) return st;
    if (int st = check_batch(who, batch)) return st;
    HS_CHECK_ARG(!img == !img_out && !labels == !labels_out && !depth == !depth_out,
                 "%s: each plane needs both its input and its output pointer, or neither", who);
    HS_CHECK_ARG(img || labels || depth, "%s: no plane given", who);
    if (img) HS_CHECK_ARG(channels >= 1 && channels <= 16, "%s: channels must be in [1, 16], got %d", who, channels);
    HS_CHECK_ARG(background >= 0 && background <= 255, "%s: background must be in [0, 255], got %d", who, background);
    const int64_t plane = (int64_t)batch * npix;
    HS_CHECK_ARG(!ranges_overlap(img, plane * channels, img_out, plane * channels) && !ranges_overlap(labels, plane, labels_out, plane) &&
                     !ranges_overlap(depth, plane * 4, depth_out, plane * 4),
                 "%s: an output overlaps its input (a pixel reads others' source values)", who);
    HS_CHECK_ARG(rot, "%s: null pointer", who);
    hipLaunchKernelGGL(hp_rotate_kernel, pixel_grid(npix, batch), dim3(kThreads), 0, (hipStream_t)stream, (int64_t)nside, npix, rot, img,
                       channels, img_out, labels, labels_out, background, (const uint32_t*)depth, (uint32_t*)depth_out,
                       float_word(depth_fill));
    HS_LAUNCH_CHECK("hp_rotate");
    return HS_OK;
}

}  // extern "C"
