// Surround view: the frames of a rig of up to eight calibrated fisheye cameras fused onto one HEALPix sphere, per (sample, pixel):
// one copy for the kernel of surround_project.hip and the host loop that restates it.  Every function is __host__ __device__,
// float64, without FMA contraction, and calls no math library (hs::erp::SinCos, hs::erp::atan2_finite, sqrt, floor, rint), so
// the host entry point runs the statements of the kernel and returns its bits.
//     g = centre of nested pixel p (hs::healpix::pixel_centre with SinCos); for camera c of sample b, d = M[b, c] g, M nine
//     row-major doubles; a camera whose present byte is 0, or whose d is not finite, is skipped
//     r = sqrt(dx^2 + dy^2), theta = atan2(r, dz), cos phi = dx / r, sin phi = dy / r (1, 0 where r == 0);
//     theta > max_theta[c]: not seen.  (max_theta is what keeps a non-monotonic polynomial from folding far directions back
//     into the image.)
//     rho = sum_i k_i theta^i (the power and sum order of hp_rotated_coords_kernel),
//     u = rho cos phi + cx_offset + W / 2 - 1/2, v = rho sin phi aspect_ratio + cy_offset + H / 2 - 1/2
//     seen iff -1/2 <= u < W - 1/2 and -1/2 <= v < H - 1/2: the nearest image pixel lies inside the image
//     weight w = a e, a = 1 - theta / max_theta[c], e = min(1, m / edge_feather) (1 without a feather),
//     m = min(u + 1/2, W - 1/2 - u, v + 1/2, H - 1/2 - v); the camera COUNTS iff it is seen and w > 0
// The pixel is covered iff some camera counts; the winner is the counting camera of largest w, the lowest index among equals.
//     frame    per camera the bilinear cell of hs::erp::bilinear at (v, u), rows and columns CLAMPED to the image;
//              blend 0: the winner's value; blend 1: (sum_c w_c val_c) / (sum_c w_c) over the counting cameras in ascending c
//     labels, depth, camera   from the winner, at row rint(v) and column rint(u) (half to even), copied
// The parallax between the cameras' centres is ignored: the rig is treated as one viewpoint, and depth is each camera's own range.
#pragma once
#include "../../include/healswin.h"
#include "hs_erp_device.h"

#pragma clang fp contract(off)

namespace hs {
namespace surround {

constexpr int kMaxCameras = 8;

struct Args {
    int64_t nside, npix;
    const double* rot;       // [batch, n_cameras, 9]
    const uint8_t* present;  // [batch, n_cameras], null: every camera is present
    hs_surround_rig rig;     // by value: it travels in the kernel's argument segment
    int height, width;
    const void* frame;  // u8 or f32 [batch, n_cameras, channels, height, width]
    void* frame_out;    // the same type [batch, channels, npix]
    int channels;
    const uint8_t* labels;  // [batch, n_cameras, height, width]
    uint8_t* labels_out;    // [batch, npix]
    int background;
    const uint32_t* depth;  // the words of f32 [batch, n_cameras, height, width]
    uint32_t* depth_out;
    uint32_t depth_fill;
    uint8_t* camera_out;  // [batch, npix], nullable: the winner's index, 255 where uncovered
};

// one camera's view of a direction: counts == false leaves w = 0
struct View {
    bool counts;
    double w, u, v;
};

HS_HD double min2(double a, double b) { return b < a ? b : a; }

HS_HD View view(const hs_fisheye_camera& cam, double max_theta, double feather, const double* m, const healpix::Vec3& g) {
    View s;
    s.counts = false, s.w = 0.0, s.u = 0.0, s.v = 0.0;
    const healpix::Vec3 d = healpix::rotated(m, g);
    if (!healpix::all_finite(d)) return s;
    const double r = sqrt(d.x * d.x + d.y * d.y);
    const double theta = erp::atan2_finite(r, d.z);
    if (theta > max_theta) return s;
    const double cphi = r == 0.0 ? 1.0 : d.x / r, sphi = r == 0.0 ? 0.0 : d.y / r;
    double rho = 0.0, tp = 1.0;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        tp = tp * theta;
        if (o < cam.poly_order) rho = rho + cam.k[o] * tp;
    }
    const double wd = (double)cam.width, ht = (double)cam.height;
    const double u = rho * cphi + cam.cx_offset + wd / 2.0 - 0.5;
    const double v = rho * sphi * cam.aspect_ratio + cam.cy_offset + ht / 2.0 - 0.5;
    if (!(u >= -0.5 && u < wd - 0.5 && v >= -0.5 && v < ht - 0.5)) return s;  // a NaN is not seen
    const double a = 1.0 - theta / max_theta;
    const double edge = min2(min2(u + 0.5, wd - 0.5 - u), min2(v + 0.5, ht - 0.5 - v));
    const double e = feather > 0.0 ? min2(1.0, edge / feather) : 1.0;
    const double w = a * e;
    if (!(w > 0.0)) return s;
    s.counts = true, s.w = w, s.u = u, s.v = v;
    return s;
}

// the bilinear cell at (v, u) of a seen pixel as an hs::erp::Tap: i0 = floor v in [-1, H - 1], j0 = floor u in [-1, W - 1], rows
// and columns clamped; nearest = row rint(v), column rint(u), inside the image because the pixel is seen
HS_HD erp::Tap cell(double u, double v, int height, int width) {
    erp::Tap t;
    t.ok = true;
    const double uf = floor(u), vf = floor(v);
    t.fx = u - uf, t.fy = v - vf;
    const int32_t w = width, h = height, j0 = (int32_t)uf, i0 = (int32_t)vf;
    const int32_t ja = erp::clamp(j0, w), jb = erp::clamp(j0 + 1, w), ia = erp::clamp(i0, h), ib = erp::clamp(i0 + 1, h);
    t.aa = ia * w + ja, t.ab = ia * w + jb, t.ba = ib * w + ja, t.bb = ib * w + jb;
    t.nearest = erp::clamp((int32_t)rint(v), h) * w + erp::clamp((int32_t)rint(u), w);  // the clamps never act on a seen pixel
    return t;
}

// every plane given of output pixel p of sample b.  Feather is rig.blend == 1: a template parameter, so that the winner kernel does not
// hold the per-camera weights and coordinates (surround_project.hip has the register counts)
template <typename T, bool Feather>
HS_HD void project_pixel(const Args& a, int64_t b, int64_t p) {
    const int n_cam = a.rig.n_cameras;
    const int log2_ns = __builtin_ctzll((unsigned long long)a.nside);
    const healpix::Vec3 g = healpix::pixel_centre(a.nside, 2 * log2_ns, p, erp::SinCos{});
    // the counting cameras' weights and coordinates (w == 0: does not count), held under constant indices so that they stay in
    // registers; every matrix and present byte is read in this loop, before the first store: the outputs are not known to be
    // apart from them in here
    double w[kMaxCameras], u[kMaxCameras], v[kMaxCameras];
#pragma unroll
    for (int k = 0; k < kMaxCameras; ++k) w[k] = 0.0, u[k] = 0.0, v[k] = 0.0;
    int best = -1;
    double wbest = 0.0, ubest = 0.0, vbest = 0.0;
#pragma unroll 1
    for (int c = 0; c < n_cam; ++c) {
        if (a.present && a.present[b * n_cam + c] == 0) continue;
        double m[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = a.rot[(b * n_cam + c) * 9 + k];
        const View s = view(a.rig.cam[c], a.rig.max_theta[c], a.rig.edge_feather, m, g);
        if (!s.counts) continue;
        if constexpr (Feather) {
#pragma unroll
            for (int k = 0; k < kMaxCameras; ++k)
                if (k == c) w[k] = s.w, u[k] = s.u, v[k] = s.v;
        }
        if (s.w > wbest) best = c, wbest = s.w, ubest = s.u, vbest = s.v;  // an equal weight leaves the lower index
    }
    const bool covered = best >= 0;
    const int64_t plane = (int64_t)a.height * a.width;
    erp::Tap win;
    win.ok = false;
    if (covered) win = cell(ubest, vbest, a.height, a.width);
    if (a.frame) {
#pragma unroll 1
        for (int c0 = 0; c0 < a.channels; c0 += 4) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            if constexpr (!Feather) {
                if (covered) {  // no load is issued otherwise
                    const T* src = (const T*)a.frame + ((b * n_cam + best) * a.channels + c0) * plane;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c0 + j < a.channels) acc[j] = erp::bilinear(src + j * plane, win);
                }
            } else {
                double sum = 0.0;
#pragma unroll 1
                for (int k = 0; k < n_cam; ++k) {
                    double wk = 0.0, uk = 0.0, vk = 0.0;
#pragma unroll
                    for (int q = 0; q < kMaxCameras; ++q)
                        if (q == k) wk = w[q], uk = u[q], vk = v[q];
                    if (!(wk > 0.0)) continue;  // no load is issued for a camera that does not count
                    const erp::Tap t = cell(uk, vk, a.height, a.width);
                    const T* src = (const T*)a.frame + ((b * n_cam + k) * a.channels + c0) * plane;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c0 + j < a.channels) acc[j] = acc[j] + wk * erp::bilinear(src + j * plane, t);
                    sum = sum + wk;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = covered ? acc[j] / sum : 0.0;
            }
            T* dst = (T*)a.frame_out + (b * a.channels + c0) * a.npix + p;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j < a.channels) erp::store_value(dst + j * a.npix, acc[j], covered);
        }
    }
    const int64_t src = (b * n_cam + (covered ? best : 0)) * plane + (covered ? (int64_t)win.nearest : 0);
    if (a.labels) a.labels_out[b * a.npix + p] = covered ? a.labels[src] : (uint8_t)a.background;
    if (a.depth) a.depth_out[b * a.npix + p] = covered ? a.depth[src] : a.depth_fill;  // the word: NaNs keep their bits
    if (a.camera_out) a.camera_out[b * a.npix + p] = covered ? (uint8_t)best : (uint8_t)255;
}

}  // namespace surround
}  // namespace hs
