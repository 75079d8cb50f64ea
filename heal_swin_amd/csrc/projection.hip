// Fisheye image -> HEALPix sampling, the per-image part of the reference's data preparation
// (heal_swin/data/segmentation/project_on_s2.py:344-372, data/depth_estimation/project_depth_on_s2.py:48-84, :411-412):
//     hp_img  = sample_bilinear(img, v, u).astype(np.uint8)      (:38-73)     hs_sample_bilinear_u8
//     hp_mask = sample_mask(mask, v, u, s2_bkgd_class)           (:76-80)     hs_sample_mask_u8
//     hp_img  = sample_bilinear(img, v, u).astype(np.float32)    (depth path) hs_sample_bilinear_u8_f32
//     hp_mask = sample_mask(depth, v, u, s2_bkgd_class)          (depth path) hs_sample_nearest_f32
// for every image of a camera, against ONE coordinate table (u, v) per calibration (the reference caches it, :141-183).
// One thread per HEALPix pixel: the coordinate arithmetic is done once and applied to all batch x channel planes.
// hs_sample_*_per_sample: the same kernels against one coordinate row PER SAMPLE (rx, ry [batch, n], the output of
// hs_hp_rotated_coords, projection_aug.hip): one thread per (sample, pixel), applied to that sample's planes.
// One bilinear kernel and one nearest kernel serve all eight entry points: the bilinear pair differs in the final conversion
// alone (store_sample), the nearest pair in the element type.
//
// Bit-exact by construction: float64 throughout, the reference's operation order
//     fx1 = (i1 - r) s00 + (r - i0) s10;  fx2 = (i1 - r) s01 + (r - i0) s11;  out = (j1 - q) fx1 + (q - j0) fx2
// with i0 / i1 = floor / ceil (so BOTH weights vanish at integer coordinates and the sample is 0, as in the reference),
// out-of-image neighbours contributing 0, truncation to uint8 or one rounding to float32 -- and no FMA contraction (a fused
// multiply-add rounds once where numpy rounds twice; in constant image regions that decides between c and c - 1 after the
// truncation).  The nearest sampler rounds half to even (np.around) and copies the element: classes never mix, a float32
// depth keeps its bits.
// HBM-bound gather: 2 x 8 B of coordinates + batch x channels x (4 neighbour bytes from L2, 1 or 4 bytes out) per pixel.
#include "hs_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

struct Corner {
    bool ok;
    int64_t off;
};
__device__ __forceinline__ Corner corner(double fx, double fy, int h, int w) {
    // numpy's bounds test on the integer casts; doubles compare the same way, NaN and +-inf fail it
    const bool ok = fx >= 0.0 && fx < (double)h && fy >= 0.0 && fy < (double)w;
    return {ok, ok ? (int64_t)fx * w + (int64_t)fy : 0};
}

// .astype(np.uint8): truncation, and NaN / inf coordinates, whose NaN result the reference casts to 0;  .astype(np.float32): one
// rounding, the NaN stays
__device__ __forceinline__ void store_sample(uint8_t* out, double r, bool finite) { *out = finite ? (uint8_t)(int)r : (uint8_t)0; }
__device__ __forceinline__ void store_sample(float* out, double r, bool) { *out = (float)r; }

// PER_SAMPLE (both kernels): the grid's y index is the sample, which reads row y of rx, ry [batch, n] and owns its `planes`
// (= channels, or 1 map) source planes; otherwise one (rx, ry) [n] serves all `planes` (= batch x channels, or batch maps).  The
// arithmetic below is the same code.
template <bool PER_SAMPLE, typename Out>
__global__ void __launch_bounds__(kThreads) sample_bilinear_kernel(const uint8_t* __restrict__ img, int planes, int h, int w,
                                                                   const double* __restrict__ rx, const double* __restrict__ ry,
                                                                   int64_t n, Out* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (PER_SAMPLE) {
        const int64_t b = blockIdx.y;
        rx += b * n, ry += b * n, img += b * planes * ((int64_t)h * w), out += b * planes * n;
    }
    const double x = rx[i], y = ry[i];
    const double x0 = floor(x), x1 = ceil(x), y0 = floor(y), y1 = ceil(y);
    const Corner c00 = corner(x0, y0, h, w), c10 = corner(x1, y0, h, w), c01 = corner(x0, y1, h, w), c11 = corner(x1, y1, h, w);
    const double wx0 = x1 - x, wx1 = x - x0, wy0 = y1 - y, wy1 = y - y0;  // NaN for NaN / +-inf coordinates
    const bool finite = (x - x == 0.0) && (y - y == 0.0);
    const int64_t plane = (int64_t)h * w;
    for (int p = 0; p < planes; ++p) {
        const uint8_t* s = img + p * plane;
        const double s00 = c00.ok ? (double)s[c00.off] : 0.0, s10 = c10.ok ? (double)s[c10.off] : 0.0;
        const double s01 = c01.ok ? (double)s[c01.off] : 0.0, s11 = c11.ok ? (double)s[c11.off] : 0.0;
        const double fx1 = wx0 * s00 + wx1 * s10;
        const double fx2 = wx0 * s01 + wx1 * s11;
        const double r = wy0 * fx1 + wy1 * fx2;
        store_sample(out + p * n + i, r, finite);
    }
}

template <bool PER_SAMPLE, typename T>
__global__ void __launch_bounds__(kThreads) sample_nearest_kernel(const T* __restrict__ src, int planes, int h, int w,
                                                                  const double* __restrict__ rx, const double* __restrict__ ry,
                                                                  int64_t n, T background, T* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (PER_SAMPLE) {
        const int64_t b = blockIdx.y;
        rx += b * n, ry += b * n, src += b * planes * ((int64_t)h * w), out += b * planes * n;
    }
    const Corner c = corner(rint(rx[i]), rint(ry[i]), h, w);  // np.around: round half to even
    const int64_t plane = (int64_t)h * w;
    for (int p = 0; p < planes; ++p) out[p * n + i] = c.ok ? src[p * plane + c.off] : background;
}

dim3 sample_grid(bool per_sample, int64_t n, int batch) {
    return dim3((unsigned)((n + kThreads - 1) / kThreads), per_sample ? (unsigned)batch : 1u);
}

// one argument check and one launch for the four bilinear entry points
template <bool PER_SAMPLE, typename Out>
int sample_bilinear(const void* img, int batch, int channels, int height, int width, const double* rx,
                    const double* ry, int64_t n, Out* out, void* stream) {
    HS_CHECK_ARG(batch > 0 && channels > 0 && height > 0 && width > 0 && n >= 0, "bad shape");
    HS_CHECK_ARG((int64_t)batch * channels < (1 << 20), "too many image planes");
    HS_CHECK_ARG(!PER_SAMPLE || batch <= 65535, "per-sample tables: batch <= 65535");
    if (n == 0) return HS_OK;
    HS_CHECK_ARG(img && rx && ry && out, "null pointer");
    hipLaunchKernelGGL((sample_bilinear_kernel<PER_SAMPLE, Out>), sample_grid(PER_SAMPLE, n, batch), dim3(kThreads), 0,
                       (hipStream_t)stream, (const uint8_t*)img, PER_SAMPLE ? channels : batch * channels, height, width, rx, ry, n, out);
    HS_LAUNCH_CHECK("sample_bilinear");
    return HS_OK;
}

// the same for the four nearest entry points; `own_ok` / `own_refusal`: the one refusal the u8 pair (a background class outside
// uint8) and the f32 pair (2^20 maps or more) do not share
template <bool PER_SAMPLE, typename T>
int sample_nearest(const T* src, int batch, int height, int width, const double* rx, const double* ry, int64_t n,
                   T background, bool own_ok, const char* own_refusal, T* out, void* stream) {
    HS_CHECK_ARG(batch > 0 && height > 0 && width > 0 && n >= 0, "bad shape");
    HS_CHECK_ARG(own_ok, "%s", own_refusal);
    HS_CHECK_ARG(!PER_SAMPLE || batch <= 65535, "per-sample tables: batch <= 65535");
    if (n == 0) return HS_OK;
    HS_CHECK_ARG(src && rx && ry && out, "null pointer");
    hipLaunchKernelGGL((sample_nearest_kernel<PER_SAMPLE, T>), sample_grid(PER_SAMPLE, n, batch), dim3(kThreads), 0, (hipStream_t)stream,
                       src, PER_SAMPLE ? 1 : batch, height, width, rx, ry, n, background, out);
    HS_LAUNCH_CHECK("sample_nearest");
    return HS_OK;
}

template <bool PER_SAMPLE>
int sample_mask_u8(const void* mask, int batch, int height, int width, const double* rx, const double* ry, int64_t n, int background,
                   void* out, void* stream) {
    return sample_nearest<PER_SAMPLE, uint8_t>((const uint8_t*)mask, batch, height, width, rx, ry, n, (uint8_t)background,
                                               background >= 0 && background <= 255, "background class must fit uint8", (uint8_t*)out,
                                               stream);
}

template <bool PER_SAMPLE>
int sample_nearest_f32(const float* src, int batch, int height, int width, const double* rx, const double* ry, int64_t n, float background,
                       float* out, void* stream) {
    return sample_nearest<PER_SAMPLE, float>(src, batch, height, width, rx, ry, n, background, batch < (1 << 20),
                                             "too many maps", out, stream);
}

}  // namespace

extern "C" {

int hs_sample_bilinear_u8(const void* img, int batch, int channels, int height, int width, const double* rx, const double* ry,
                          int64_t n, void* out, void* stream) {
    return sample_bilinear<false>(img, batch, channels, height, width, rx, ry, n, (uint8_t*)out, stream);
}

int hs_sample_bilinear_u8_per_sample(const void* img, int batch, int channels, int height, int width, const double* rx,
                                     const double* ry, int64_t n, void* out, void* stream) {
    return sample_bilinear<true>(img, batch, channels, height, width, rx, ry, n, (uint8_t*)out, stream);
}

int hs_sample_bilinear_u8_f32(const void* img, int batch, int channels, int height, int width, const double* rx, const double* ry,
                              int64_t n, float* out, void* stream) {
    return sample_bilinear<false>(img, batch, channels, height, width, rx, ry, n, out, stream);
}

int hs_sample_bilinear_u8_f32_per_sample(const void* img, int batch, int channels, int height, int width, const double* rx,
                                         const double* ry, int64_t n, float* out, void* stream) {
    return sample_bilinear<true>(img, batch, channels, height, width, rx, ry, n, out, stream);
}

int hs_sample_mask_u8(const void* mask, int batch, int height, int width, const double* rx, const double* ry, int64_t n,
                      int background, void* out, void* stream) {
    return sample_mask_u8<false>(mask, batch, height, width, rx, ry, n, background, out, stream);
}

int hs_sample_mask_u8_per_sample(const void* mask, int batch, int height, int width, const double* rx, const double* ry, int64_t n,
                                 int background, void* out, void* stream) {
    return sample_mask_u8<true>(mask, batch, height, width, rx, ry, n, background, out, stream);
}

int hs_sample_nearest_f32(const float* src, int batch, int height, int width, const double* rx, const double* ry, int64_t n,
                          float background, float* out, void* stream) {
    return sample_nearest_f32<false>(src, batch, height, width, rx, ry, n, background, out, stream);
}

int hs_sample_nearest_f32_per_sample(const float* src, int batch, int height, int width, const double* rx, const double* ry, int64_t n,
                                     float background, float* out, void* stream) {
    return sample_nearest_f32<true>(src, batch, height, width, rx, ry, n, background, out, stream);
}

}  // extern "C"
