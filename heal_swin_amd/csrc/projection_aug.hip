// Per-sample rotation augmentation of the fisheye -> HEALPix projection: the coordinate table of projection.py, recomputed on
// the device for every sample of a batch under its own 3x3 matrix.
//     g   = centre of nested pixel p as a unit vector            (the steps of hs_pix2ang_nest, healpix_tables.cpp)
//     d   = M_b g                                                (M_b row-major, read from device memory: a captured step
//                                                                 changes the rotations between replays)
//     r   = hypot(d.x, d.y), theta = atan2(r, d.z), cos phi = d.x / r, sin phi = d.y / r  (1, 0 where r == 0)
//     rho = sum_i k_i theta^i                                    (project_s2_points_to_img, the WoodScape polynomial model)
//     u   = rho cos phi + cx_offset + width / 2 - 1/2,  v = rho sin phi aspect_ratio + cy_offset + height / 2 - 1/2
// theta and phi do not depend on the length of d, so any real matrix is accepted.  The rotation acts on the sampling
// coordinates: a rotated sample costs one interpolation (hs_sample_*_per_sample against this kernel's output), not two.
//
// float64 throughout, no FMA contraction, the reference's expression order for rho, u and v.  The result agrees with the host
// table (arccos / cos phi / sin phi of the angles) to rounding, not bit for bit: the exact path is the resident table.
// One thread per (sample, pixel): bound by float64 transcendental throughput (sincos, hypot, atan2, two divisions), 16 B out.
#include "hs_device.h"
#include "hs_healpix_device.h"  // pixel_centre, rotated
#include "hs_sphere_args.h"

#pragma clang fp contract(off)

namespace {

using hs::healpix::pixel_centre;
using hs::healpix::rotated;
using hs::healpix::Vec3;
using namespace hs::sphere;

// grid (pixel blocks, samples)
__global__ void __launch_bounds__(kThreads) hp_rotated_coords_kernel(int64_t nside, int log2_npface, int64_t first_pix, int64_t count,
                                                                     hs_fisheye_camera cam, const double* __restrict__ rot,
                                                                     double* __restrict__ u, double* __restrict__ v) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const int64_t b = blockIdx.y;
    const Vec3 d = rotated(rot + 9 * b, pixel_centre(nside, log2_npface, first_pix + i));  // the matrix is uniform over the workgroup
    const double r = hypot(d.x, d.y);
    const double theta = atan2(r, d.z);
    const double cphi = r == 0.0 ? 1.0 : d.x / r, sphi = r == 0.0 ? 0.0 : d.y / r;
    double rho = 0.0, tp = 1.0;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        tp = tp * theta;
        if (o < cam.poly_order) rho = rho + cam.k[o] * tp;
    }
    u[b * count + i] = rho * cphi + cam.cx_offset + (double)cam.width / 2.0 - 0.5;
    v[b * count + i] = rho * sphi * cam.aspect_ratio + cam.cy_offset + (double)cam.height / 2.0 - 0.5;
}

}  // namespace

extern "C" {

int hs_hp_rotated_coords(int nside, int64_t first_pix, int64_t count, const hs_fisheye_camera* cam, const double* rot, int batch,
                         double* u, double* v, void* stream) {
    const char* who = "hs_hp_rotated_coords";
    if (int st = check_nside(who, nside, 0, /*int32_indices=*/false)) return st;  // u, v are tables of doubles
    HS_CHECK_ARG(nside <= (1 << 29), "nside %d above HEALPix's limit 2^29", nside);
    if (int st = check_pixel_range(who, nside, first_pix, count)) return st;
    HS_CHECK_ARG(count <= (int64_t)INT32_MAX * kThreads, "too many pixels for one launch");
    if (int st = check_batch(who, batch)) return st;
    HS_CHECK_ARG(cam, "null pointer");
    HS_CHECK_ARG(cam->poly_order >= 1 && cam->poly_order <= 8, "poly_order must be in [1, 8], got %d", cam->poly_order);
    HS_CHECK_ARG(cam->width > 0 && cam->height > 0, "image size must be positive");
    if (count == 0) return HS_OK;
    HS_CHECK_ARG(rot && u && v, "null pointer");
    int log2_npface = 0;
    while (((int64_t)1 << log2_npface) < (int64_t)nside * nside) ++log2_npface;
    hipLaunchKernelGGL(hp_rotated_coords_kernel, pixel_grid(count, batch), dim3(kThreads), 0, (hipStream_t)stream, (int64_t)nside,
                       log2_npface, first_pix, count, *cam, rot, u, v);
    HS_LAUNCH_CHECK("hp_rotated_coords");
    return HS_OK;
}

}  // extern "C"
