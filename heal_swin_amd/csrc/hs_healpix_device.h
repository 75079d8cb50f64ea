// HEALPix geometry evaluated per pixel, one copy for the device kernels and the host loops that restate them
// (projection_aug.hip, hp_rotate.hip, hp_ensemble.hip, hs_erp_device.h, hs_surround_device.h): the centre of a nested pixel as a unit vector, its
// rotation d = M g with the finiteness test and the longitude reduction every resampler applies to d, HEALPix's get_interpol of
// a rotated pixel centre in nested order, and the coverage test of a source index.  Every function is __host__ __device__ (the
// macros are empty in a plain C++ translation unit), float64, without FMA contraction, so that the host entry point runs the
// statements of the kernel.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HS_HD __host__ __device__ __forceinline__
#else
#define HS_HD inline
#endif

#pragma clang fp contract(off)

namespace hs {
namespace healpix {

HS_HD uint32_t compact_bits(uint64_t v) {  // keeps the even bits
    v &= 0x5555555555555555ull;
    v = (v | (v >> 1)) & 0x3333333333333333ull;
    v = (v | (v >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v >> 4)) & 0x00FF00FF00FF00FFull;
    v = (v | (v >> 8)) & 0x0000FFFF0000FFFFull;
    v = (v | (v >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)v;
}

HS_HD uint64_t spread_bits(uint64_t v) {  // abc -> 0a0b0c
    v &= 0xFFFFFFFFull;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

struct Vec3 {
    double x, y, z;
};

struct LibmSinCos {  // the math library's sincos: the device's on the device, the host's on the host
    HS_HD void operator()(double a, double& s, double& c) const { sincos(a, &s, &c); }
};

// centre of nested pixel p: hs_pix2ang_nest's (face, ix, iy) -> ring jr -> zone, with the vector built from z and sin(theta)
// directly (caps: sqrt(tmp (2 - tmp)), belt: sqrt((1 - z)(1 + z))) instead of through acos.  `sc(phi, s, c)` evaluates the sine and
// cosine of the longitude: LibmSinCos unless the caller needs the same bits on the host and on the device (hs_erp_device.h).
template <typename SinCos>
HS_HD Vec3 pixel_centre(int64_t nside, int log2_npface, int64_t p, SinCos sc) {
    const int face = (int)(p >> log2_npface);
    const uint64_t in_face = (uint64_t)(p & (((int64_t)1 << log2_npface) - 1));
    const int64_t ix = compact_bits(in_face), iy = compact_bits(in_face >> 1);
    // ring index (units of nside) of the base pixel's northern corner, and its longitude offset (kJrll, kJpll of the host tables)
    const int jrll = 2 + (face >> 2), jpll = (face >> 2) == 1 ? 2 * (face & 3) : 2 * (face & 3) + 1;
    const int64_t jr = jrll * nside - ix - iy - 1;
    const double fact2 = 4.0 / (double)(12 * nside * nside), fact1 = (double)(2 * nside) * fact2, halfpi = 0.5 * M_PI;
    int64_t nr;
    double z, sth;
    if (jr < nside) {  // north polar cap
        nr = jr;
        const double tmp = (double)(nr * nr) * fact2;
        z = 1.0 - tmp;
        sth = sqrt(tmp * (2.0 - tmp));
    } else if (jr > 3 * nside) {  // south polar cap
        nr = 4 * nside - jr;
        const double tmp = (double)(nr * nr) * fact2;
        z = tmp - 1.0;
        sth = sqrt(tmp * (2.0 - tmp));
    } else {  // equatorial belt
        nr = nside;
        z = (double)(2 * nside - jr) * fact1;
        sth = sqrt((1.0 - z) * (1.0 + z));
    }
    int64_t t = jpll * nr + ix - iy;
    if (t < 0) t += 8 * nr;
    const double phi = nr == nside ? 0.75 * halfpi * (double)t * fact1 : (0.5 * halfpi * (double)t) / (double)nr;
    double s, c;
    sc(phi, s, c);
    return {sth * c, sth * s, z};
}

HS_HD Vec3 pixel_centre(int64_t nside, int log2_npface, int64_t p) { return pixel_centre(nside, log2_npface, p, LibmSinCos{}); }

// d = M g, M nine row-major doubles
HS_HD Vec3 rotated(const double* m, const Vec3& g) {
    return {m[0] * g.x + m[1] * g.y + m[2] * g.z, m[3] * g.x + m[4] * g.y + m[5] * g.z, m[6] * g.x + m[7] * g.y + m[8] * g.z};
}

HS_HD bool all_finite(const Vec3& d) {
    const double dmax = 1.7976931348623157e308;  // a NaN fails every comparison
    return fabs(d.x) <= dmax && fabs(d.y) <= dmax && fabs(d.z) <= dmax;
}

// HEALPix fmodulo(phi, 2 pi): a longitude in [0, 2 pi)
HS_HD double fmodulo_twopi(double ph) {
    const double twopi = 2.0 * M_PI;
    if (ph >= 0.0) {
        if (ph >= twopi) ph = fmod(ph, twopi);
    } else {
        ph = fmod(ph, twopi) + twopi;
        if (ph == twopi) ph = 0.0;
    }
    return ph;
}

// a source index is covered iff it names one of the npix pixels the map holds: the base pixels it lacks, and the -1 of a
// non-finite matrix, are not
HS_HD bool covered(int32_t idx, int64_t npix) { return (uint64_t)(int64_t)idx < (uint64_t)npix; }

// T_Healpix_Base::get_ring_info2 without the first pixel: pixel count, centre colatitude and phase shift of ring 1 .. 4 nside - 1
HS_HD void ring_info(int64_t ns, int64_t ring, int64_t& nr, double& th, bool& shifted) {
    const double fact2 = 4.0 / (double)(12 * ns * ns), fact1 = (double)(ns << 1) * fact2;
    const int64_t north = ring > 2 * ns ? 4 * ns - ring : ring;
    if (north < ns) {
        const double tmp = (double)(north * north) * fact2;
        th = atan2(sqrt(tmp * (2.0 - tmp)), 1.0 - tmp);
        nr = 4 * north;
        shifted = true;
    } else {
        th = acos((double)(2 * ns - north) * fact1);
        nr = 4 * ns;
        shifted = ((north - ns) & 1) == 0;
    }
    if (north != ring) th = M_PI - th;
}

// the two pixels of a ring around phi in [0, 2 pi) as positions 0 .. nr - 1 along the ring, the weight of the second and the
// ring's colatitude
HS_HD void ring_bracket(int64_t ns, int64_t ring, double ph, int64_t& i1, int64_t& i2, double& w1, double& th) {
    int64_t nr;
    bool shifted;
    ring_info(ns, ring, nr, th, shifted);
    const double dphi = (2.0 * M_PI) / (double)nr, half = shifted ? 0.5 : 0.0;
    const double tmp = ph / dphi - half;
    i1 = tmp < 0 ? (int64_t)tmp - 1 : (int64_t)tmp;
    w1 = (ph - ((double)i1 + half) * dphi) / dphi;
    i2 = i1 + 1;
    if (i1 < 0) i1 += nr;
    if (i1 >= nr) i1 -= nr;  // phi / dphi rounded up to nr: the seam
    if (i2 >= nr) i2 -= nr;
}

// nested index of position pos (0-based, eastwards) of ring `ring`: ring2xyf from (ring, position), then xyf2nest
HS_HD int64_t ring_pos_to_nest(int64_t ns, int log2_ns, int64_t ring, int64_t pos) {
    const int64_t iphi = pos + 1;
    int64_t nr, kshift;
    int face;
    if (ring < ns) {  // north polar cap
        nr = ring;
        kshift = 0;
        face = (int)((uint32_t)pos / (uint32_t)nr);
    } else if (ring <= 3 * ns) {  // equatorial belt
        const int64_t row = ring - ns;
        nr = ns;
        kshift = (ring + ns) & 1;
        const int64_t ire = row + 1, irm = 2 * ns + 1 - row;
        const int64_t ifm = (iphi - ire / 2 + ns - 1) >> log2_ns;  // numerators >= 0
        const int64_t ifp = (iphi - irm / 2 + ns - 1) >> log2_ns;
        face = (int)((ifp == ifm) ? (ifp | 4) : ((ifp < ifm) ? ifp : (ifm + 8)));
    } else {  // south polar cap
        nr = 4 * ns - ring;
        kshift = 0;
        face = 8 + (int)((uint32_t)pos / (uint32_t)nr);
    }
    const int jrll = 2 + (face >> 2), jpll = (face >> 2) == 1 ? 2 * (face & 3) : 2 * (face & 3) + 1;
    const int64_t irt = ring - jrll * ns + 1;
    int64_t ipt = 2 * iphi - jpll * nr - kshift - 1;
    if (ipt >= 2 * ns) ipt -= 8 * ns;
    // arithmetic shifts on possibly negative numerators floor, as in the HEALPix formulas
    const int64_t ix = (ipt - irt) >> 1, iy = (-(ipt + irt)) >> 1;
    return ((int64_t)face << (2 * log2_ns)) + (int64_t)(spread_bits((uint64_t)ix) | (spread_bits((uint64_t)iy) << 1));
}

struct RotatedInterp {
    int32_t pix[4];
    double wgt[4];
    int32_t nearest;
};

// get_interpol (nested) of the direction d = M g_p, g_p the centre of nested pixel p, M nine row-major doubles; nside a power
// of two with 12 nside^2 < 2^31.  The steps, the order of the four pixels and the pole handling are those of
// hs_hp_interp_weights_nest (healpix_tables.cpp): theta = atan2(hypot(dx, dy), dz) (0 for d = 0), phi = atan2(dy, dx) reduced
// with HEALPix's fmodulo, ring_above(cos theta), the two bracketing rings, the four polar pixels with a quarter of the
// missing ring's weight above the first and below the last ring.  nearest = the pixel of largest weight, the first maximum in
// that order (evaluation.hp_nearest_pix_idcs).  A non-finite component of d gives pix -1, wgt 0, nearest -1.
HS_HD RotatedInterp rotated_interp(int64_t nside, const double* m, int64_t p) {
    const int log2_ns = __builtin_ctzll((unsigned long long)nside);
    const int64_t ns = nside, nl4 = 4 * ns;
    const Vec3 d = rotated(m, pixel_centre(ns, 2 * log2_ns, p));
    RotatedInterp out;
    if (!all_finite(d)) {
        for (int k = 0; k < 4; ++k) out.pix[k] = -1, out.wgt[k] = 0.0;
        out.nearest = -1;
        return out;
    }
    const double r = hypot(d.x, d.y);
    const double t = (r == 0.0 && d.z == 0.0) ? 0.0 : atan2(r, d.z);
    const double ph = fmodulo_twopi(atan2(d.y, d.x));
    const double z = cos(t), az = fabs(z);
    int64_t ir1;  // T_Healpix_Base::ring_above
    if (az <= 2.0 / 3.0) {
        ir1 = (int64_t)((double)ns * (2.0 - 1.5 * z));
    } else {
        const int64_t rr = (int64_t)((double)ns * sqrt(3.0 * (1.0 - az)));
        ir1 = z > 0 ? rr : nl4 - rr - 1;
    }
    const int64_t ir2 = ir1 + 1;
    int64_t a1 = 0, a2 = 0, b1 = 0, b2 = 0, ring_a = ir1, ring_b = ir2;  // positions on the upper (a) and lower (b) ring
    double wa = 0.0, wb = 0.0, th1 = 0.0, th2 = 0.0, w0, w1, w2, w3;
    if (ir1 > 0) ring_bracket(ns, ir1, ph, a1, a2, wa, th1);
    if (ir2 < nl4) ring_bracket(ns, ir2, ph, b1, b2, wb, th2);
    w0 = 1.0 - wa, w1 = wa, w2 = 1.0 - wb, w3 = wb;
    if (ir1 == 0) {  // above the first ring: the four polar pixels share the missing ring's weight
        const double wtheta = t / th2, fac = (1.0 - wtheta) * 0.25;
        w2 *= wtheta;
        w3 *= wtheta;
        w0 = fac;
        w1 = fac;
        w2 += fac;
        w3 += fac;
        ring_a = 1;
        a1 = (b1 + 2) & 3;
        a2 = (b2 + 2) & 3;
    } else if (ir2 == nl4) {  // below the last ring
        const double wtheta = (t - th1) / (M_PI - th1), fac = wtheta * 0.25;
        w0 *= 1.0 - wtheta;
        w1 *= 1.0 - wtheta;
        w0 += fac;
        w1 += fac;
        w2 = fac;
        w3 = fac;
        ring_b = nl4 - 1;
        b1 = (a1 + 2) & 3;
        b2 = (a2 + 2) & 3;
    } else {
        const double wtheta = (t - th1) / (th2 - th1);
        w0 *= 1.0 - wtheta;
        w1 *= 1.0 - wtheta;
        w2 *= wtheta;
        w3 *= wtheta;
    }
    out.pix[0] = (int32_t)ring_pos_to_nest(ns, log2_ns, ring_a, a1);
    out.pix[1] = (int32_t)ring_pos_to_nest(ns, log2_ns, ring_a, a2);
    out.pix[2] = (int32_t)ring_pos_to_nest(ns, log2_ns, ring_b, b1);
    out.pix[3] = (int32_t)ring_pos_to_nest(ns, log2_ns, ring_b, b2);
    out.wgt[0] = w0, out.wgt[1] = w1, out.wgt[2] = w2, out.wgt[3] = w3;
    int32_t best = out.pix[0];
    double wbest = w0;
    if (w1 > wbest) best = out.pix[1], wbest = w1;
    if (w2 > wbest) best = out.pix[2], wbest = w2;
    if (w3 > wbest) best = out.pix[3], wbest = w3;
    out.nearest = best;
    return out;
}

// r as entry (b, i) of pix, wgt [batch, 4, count] and nearest [batch, count]
HS_HD void store_interp(const RotatedInterp& r, int64_t b, int64_t i, int64_t count, int32_t* pix, double* wgt, int32_t* nearest) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pix[(b * 4 + k) * count + i] = r.pix[k];
        wgt[(b * 4 + k) * count + i] = r.wgt[k];
    }
    nearest[b * count + i] = r.nearest;
}

}  // namespace healpix
}  // namespace hs
