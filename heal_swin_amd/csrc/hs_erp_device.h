// Equirectangular panorama (ERP, the lat/long image) sampled at the nested HEALPix pixels, per (sample, pixel): one copy for
// the kernel of erp_project.hip and the host loop that restates it.  Every function is __host__ __device__ (the macros of
// hs_healpix_device.h are empty in a plain C++ translation unit), float64, without FMA contraction, so that the host entry
// point runs the statements of the kernel -- and, because sine, cosine, hypot and atan2 are evaluated here in correctly rounded
// operations alone (below), returns the kernel's bits.
//     g = centre of nested pixel p (hs::healpix::pixel_centre with SinCos), d = M g, M nine row-major doubles
//     theta = atan2(hypot(dx, dy), dz), phi = atan2(dy, dx) reduced to [0, 2 pi) with HEALPix's fmodulo
//     x = phi W / (2 pi) - 0.5 (column), y = theta H / pi - 0.5 (row): column j is centred at longitude 2 pi (j + 0.5) / W,
//     row i at colatitude pi (i + 0.5) / H
//     frame    bilinear between columns j0 = floor x and j0 + 1, which WRAP, and rows i0 = floor y and i0 + 1, which CLAMP
//     labels, depth   the pixel at column floor(x + 0.5) (wrapped) and row floor(y + 0.5) (clamped)
#pragma once
#include "hs_healpix_device.h"

#pragma clang fp contract(off)

namespace hs {
namespace erp {

struct Args {
    int64_t nside, npix;
    const double* rot;  // [batch, 9]
    int height, width, supersample;
    const void* frame;  // u8 or f32 [batch, channels, height, width]
    void* frame_out;    // the same type [batch, channels, npix]
    int channels;
    const uint8_t* labels;  // [batch, height, width]
    uint8_t* labels_out;    // [batch, npix]
    int background;
    const uint32_t* depth;  // the words of f32 [batch, height, width]
    uint32_t* depth_out;
    uint32_t depth_fill;
};

// where direction M g_p meets the panorama: the four bilinear taps as offsets into an H x W plane with the column and row
// fractions, and the offset of the nearest pixel; ok == false for a non-finite component of d (nothing else is set)
struct Tap {
    bool ok;
    uint32_t aa, ab, ba, bb;  // (ia, ja), (ia, jb), (ib, ja), (ib, jb)
    double fx, fy;
    uint32_t nearest;
};

HS_HD int32_t wrap(int32_t j, int32_t w) {  // j mod w in [0, w)
    const int32_t r = j % w;
    return r < 0 ? r + w : r;
}
HS_HD int32_t clamp(int32_t i, int32_t h) { return i < 0 ? 0 : (i > h - 1 ? h - 1 : i); }

// The transcendental functions of the geometry in +, -, *, / and sqrt alone.  The device's and the host's math libraries round
// sincos, hypot and atan2 differently in the last bit (measured on an MI355X against glibc: up to 2 % of the pixel-centre
// components, 11 - 35 % of the hypot and atan2 values), and with HEALPix centres on column boundaries (every symmetric orientation)
// the last bit picks the column.  With correctly rounded operations only, and no FMA contraction, the host entry point and the kernel
// return the same bits.  The reductions and polynomials are fdlibm's (k_sin.c, k_cos.c, e_rem_pio2.c's medium case, s_atan.c,
// e_atan2.c), about 1 ulp.

// sine and cosine of a longitude in [0, 2 pi]: the nearest multiple of pi / 2 taken off in three parts, the kernels on [-pi/4, pi/4]
struct SinCos {
    HS_HD void operator()(double a, double& s, double& c) const {
        const int k = (int)(a * 6.36619772367581382433e-01 + 0.5);  // 2 / pi
        const double fk = (double)k;
        const double r = ((a - fk * 1.57079632673412561417e+00) - fk * 6.07710050630396597660e-11) - fk * 2.02226624879595063154e-21;
        const double z = r * r;
        const double sr = r + (z * r) * (-1.66666666666666324348e-01 +
                                         z * (8.33333333332248946124e-03 +
                                              z * (-1.98412698298579493134e-04 +
                                                   z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
        const double cr = 1.0 - (0.5 * z - z * (z * (4.16666666666666019037e-02 +
                                                      z * (-1.38888888888741095749e-03 +
                                                           z * (2.48015872894767294178e-05 +
                                                                z * (-2.75573143513906633035e-07 +
                                                                     z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))))));
        switch (k & 3) {
            case 0: s = sr, c = cr; break;
            case 1: s = cr, c = -sr; break;
            case 2: s = -sr, c = -cr; break;
            default: s = -cr, c = sr; break;
        }
    }
};

// atan on [0, inf]: reduced about 0.5, 1, 1.5 or inf, then an odd polynomial of degree 11 in two interleaved halves
HS_HD double atan_pos(double x) {
    double hi = 0.0, lo = 0.0;  // atan of the reduction's centre 0.5, 1, 1.5, inf: leading and trailing part
    if (x < 0.4375) {
        // no reduction
    } else if (x < 0.6875) {
        hi = 4.63647609000806093515e-01, lo = 2.26987774529616870924e-17, x = (2.0 * x - 1.0) / (2.0 + x);
    } else if (x < 1.1875) {
        hi = 7.85398163397448278999e-01, lo = 3.06161699786838301793e-17, x = (x - 1.0) / (x + 1.0);
    } else if (x < 2.4375) {
        hi = 9.82793723247329054082e-01, lo = 1.39033110312309984516e-17, x = (x - 1.5) / (1.0 + 1.5 * x);
    } else {
        hi = 1.57079632679489655800e+00, lo = 6.12323399573676603587e-17, x = -1.0 / x;
    }
    const double z = x * x, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 +
                           w * (1.42857142725034663711e-01 +
                                w * (9.09088713343650656196e-02 +
                                     w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 +
                           w * (-1.11111104054623557880e-01 +
                                w * (-7.69187620504482999495e-02 + w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (hi == 0.0) return x - x * (s1 + s2);
    return hi - ((x * (s1 + s2) - lo) - x);
}

HS_HD double atan2_finite(double y, double x) {  // finite arguments; atan2(+-0, x) is 0 or pi, so (0, 0) gives 0
    if (y == 0.0) return x < 0.0 ? M_PI : 0.0;
    const double pi_lo = 1.2246467991473531772e-16;
    const double z = atan_pos(fabs(y / x));  // x == 0: atan(inf) = pi / 2
    const double a = x < 0.0 ? M_PI - (z - pi_lo) : z;
    return y < 0.0 ? -a : a;
}

HS_HD Tap tap(int64_t nside, const double* m, int64_t p, int height, int width) {
    const int log2_ns = __builtin_ctzll((unsigned long long)nside);
    const healpix::Vec3 d = healpix::rotated(m, healpix::pixel_centre(nside, 2 * log2_ns, p, SinCos{}));
    Tap t;
    t.ok = healpix::all_finite(d);
    if (!t.ok) return t;
    const double twopi = 2.0 * M_PI;
    const double th = atan2_finite(sqrt(d.x * d.x + d.y * d.y), d.z);  // hypot, for components far from over- and underflow
    const double ph = healpix::fmodulo_twopi(atan2_finite(d.y, d.x));
    const double x = ph * (double)width / twopi - 0.5, y = th * (double)height / M_PI - 0.5;
    // x in [-0.5, W - 0.5] and y in [-0.5, H - 0.5] (the upper ends by rounding only), so the floors fit int32; every column goes
    // through the non-negative modulo and every row through the clamp, so the offsets lie in [0, H W) whatever the floors are
    const double xf = floor(x), yf = floor(y);
    t.fx = x - xf, t.fy = y - yf;
    const int32_t w = width, h = height, j0 = (int32_t)xf, i0 = (int32_t)yf;
    const int32_t ja = wrap(j0, w), jb = wrap(j0 + 1, w), ia = clamp(i0, h), ib = clamp(i0 + 1, h);
    t.aa = ia * w + ja, t.ab = ia * w + jb, t.ba = ib * w + ja, t.bb = ib * w + jb;
    t.nearest = clamp((int32_t)floor(y + 0.5), h) * w + wrap((int32_t)floor(x + 0.5), w);
    return t;
}

template <typename T>
HS_HD double bilinear(const T* plane, const Tap& t) {
    const double vaa = (double)plane[t.aa], vab = (double)plane[t.ab], vba = (double)plane[t.ba], vbb = (double)plane[t.bb];
    return (1.0 - t.fy) * ((1.0 - t.fx) * vaa + t.fx * vab) + t.fy * ((1.0 - t.fx) * vba + t.fx * vbb);
}

HS_HD void store_value(uint8_t* out, double v, bool ok) {
    v = rint(v);  // half to even
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    *out = ok ? (uint8_t)(int)v : (uint8_t)0;
}
HS_HD void store_value(float* out, double v, bool ok) { *out = ok ? (float)v : __builtin_nanf(""); }

// every plane given of output pixel p of sample b.  Super == false is supersample 0: the pixel's own centre serves every
// plane.  Super == true: the frame value is the mean of the un-rounded bilinear values at the centres of the 4^s nested
// children p 4^s .. p 4^s + 4^s - 1 at nside 2^s, summed in ascending order and scaled by the exact 2^(-2s); channels go four
// at a time, so the accumulators stay in registers (up to four channels the geometry of a child is evaluated once); labels
// and depth still read at the pixel's own centre.  The flag is a template parameter so that the common kernel holds one copy
// of the geometry and keeps its registers (erp_project.hip).
template <typename T, bool Super>
HS_HD void project_pixel(const Args& a, int64_t b, int64_t p) {
    double m[9];  // read once, before any store: the outputs are not known to be apart from the matrices in here
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = a.rot[9 * b + k];
    const int64_t plane = (int64_t)a.height * a.width;
    Tap own;
    own.ok = false;
    if (!Super || a.labels || a.depth) own = tap(a.nside, m, p, a.height, a.width);
    if constexpr (!Super) {
        if (a.frame)
            for (int c = 0; c < a.channels; ++c) {
                const T* src = (const T*)a.frame + (b * a.channels + c) * plane;
                store_value((T*)a.frame_out + (b * a.channels + c) * a.npix + p, own.ok ? bilinear(src, own) : 0.0, own.ok);
            }
    } else if (a.frame) {
        const int s = a.supersample;
        const int64_t children = (int64_t)1 << (2 * s);
        const double scale = 1.0 / (double)children;
#pragma unroll 1
        for (int c0 = 0; c0 < a.channels; c0 += 4) {
            const T* src = (const T*)a.frame + (b * a.channels + c0) * plane;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            bool ok = true;
#pragma unroll 1
            for (int64_t k = 0; k < children; ++k) {
                const Tap t = tap(a.nside << s, m, p * children + k, a.height, a.width);
                ok = t.ok;
                if (!ok) break;  // no load is issued
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < a.channels) acc[j] = acc[j] + bilinear(src + j * plane, t);
            }
            T* dst = (T*)a.frame_out + (b * a.channels + c0) * a.npix + p;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j < a.channels) store_value(dst + j * a.npix, acc[j] * scale, ok);
        }
    }
    if (a.labels) a.labels_out[b * a.npix + p] = own.ok ? a.labels[b * plane + own.nearest] : (uint8_t)a.background;
    if (a.depth) a.depth_out[b * a.npix + p] = own.ok ? a.depth[b * plane + own.nearest] : a.depth_fill;  // the word: NaNs keep their bits
}

}  // namespace erp
}  // namespace hs
