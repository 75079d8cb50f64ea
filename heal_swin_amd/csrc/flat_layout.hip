// Image-boundary layout kernels of the flat Swin-UNet (models_torch/swin_transformer.py).
//
// Inside the model the tokens of a flat image live in tiled Z order (flat_tables.cpp): T x T tiles row-major, Morton order with
// the row bit least significant inside a tile.  These kernels move data between that order and the NCHW images the caller holds:
//
//   hs_flat_img_to_rows   [B, nch, H, W] image -> token rows.  mode HS_FLAT_PATCH_ROWS: row = token, column = (c, kh, kw) as in
//                         the Conv2d weight (PatchEmbed as one Linear); mode HS_FLAT_PIXEL_ROWS: row = token * p^2 + kh * p + kw
//                         (the children of FinalPatchExpand_X4, the reference's up_x4 view), column = c.  Columns past the
//                         valid ones are written as zeros.  uint8 rows are labels: ids outside [0, 254] become 255 (ignored).
//   hs_flat_rows_to_img   the inverse map (logits rows -> NCHW logits, patch-row gradient -> image gradient, uint8 class ids of the
//                         pixel rows -> a uint8 label image).
//
// One workgroup owns an S x S square of tokens that is aligned in Morton order, i.e. S^2 consecutive tokens: its rows are ONE
// contiguous run of memory, its pixels an (S p) x (S p) square per channel.  The square is staged through LDS (fp32, exact for
// every input type), so both the image rows and the token rows are read and written in 16-byte accesses where the sizes allow.
// Pure data movement plus a cast: bit-exact, deterministic, no atomics.
#include <type_traits>

#include "hs_device.h"
#include "hs_flat_rows.h"

namespace {

using hs::bf16_to_float;
using hs::float_to_bf16;

struct Geo {
    int nch, H, W, p, T, S, tiles_w, ntiles, nsub, mode;
    int64_t ld, rows_per_img, nrows;  // row pitch (elements), rows of one image, rows of one workgroup's square
};

using hs::flat_rows::compact;

template <typename T, bool LAB>
__device__ __forceinline__ float cvt_in(T v) {
    if constexpr (std::is_same<T, uint16_t>::value) return bf16_to_float(v);
    else if constexpr (LAB && (std::is_same<T, int32_t>::value || std::is_same<T, int64_t>::value))
        return (v < 0 || v > 254) ? 255.f : (float)v;
    else return (float)v;
}
template <typename T>
__device__ __forceinline__ T cvt_out(float v) {
    if constexpr (std::is_same<T, uint16_t>::value) return float_to_bf16(v);
    else return (T)v;
}

template <typename T>
union Pack {
    uint4 u;
    T e[16 / sizeof(T)];
};

// workgroup -> (image, pixel origin, first row of its square)
struct Square {
    int b, y0, x0;
    int64_t row_base;  // element offset of the square's first row
};
__device__ __forceinline__ Square square_of(const Geo& g) {
    const int q = blockIdx.x % g.nsub;
    const int rest = blockIdx.x / g.nsub;
    const int tile = rest % g.ntiles;
    Square s;
    s.b = rest / g.ntiles;
    const int h0 = (tile / g.tiles_w) * g.T + (int)compact((uint32_t)q) * g.S;
    const int w0 = (tile % g.tiles_w) * g.T + (int)compact((uint32_t)q >> 1) * g.S;
    s.y0 = h0 * g.p;
    s.x0 = w0 * g.p;
    const int64_t z0 = (int64_t)tile * g.T * g.T + (int64_t)q * g.S * g.S;
    const int64_t row0 = g.mode == HS_FLAT_PATCH_ROWS ? z0 : z0 * g.p * g.p;
    s.row_base = ((int64_t)s.b * g.rows_per_img + row0) * g.ld;
    return s;
}

// element e of the square's rows -> LDS index of its pixel, or -1 for a padding column
__device__ __forceinline__ int lds_of(const Geo& g, int e) {
    const int Sp = g.S * g.p;
    const hs::flat_rows::Pixel q = hs::flat_rows::pixel_of(g.mode, g.nch, g.p, (int)g.ld, e);
    return q.c < 0 ? -1 : (q.c * Sp + q.y) * Sp + q.x;
}

template <typename Ti, typename To, bool LAB>
__global__ void __launch_bounds__(256) img_to_rows_kernel(const Ti* __restrict__ img, To* __restrict__ rows, Geo g, int vec_img,
                                                          int vec_rows) {
    extern __shared__ float lds[];
    const Square sq = square_of(g);
    const int Sp = g.S * g.p, nseg = g.nch * Sp;
    if (vec_img) {
        constexpr int V = 16 / sizeof(Ti);
        const int vpr = Sp / V;
        for (int i = threadIdx.x; i < nseg * vpr; i += blockDim.x) {
            const int seg = i / vpr, v = i - seg * vpr, c = seg / Sp, y = seg - c * Sp;
            Pack<Ti> pk;
            pk.u = *(const uint4*)(img + (((int64_t)sq.b * g.nch + c) * g.H + sq.y0 + y) * g.W + sq.x0 + v * V);
#pragma unroll
            for (int j = 0; j < V; ++j) lds[seg * Sp + v * V + j] = cvt_in<Ti, LAB>(pk.e[j]);
        }
    } else {
        for (int i = threadIdx.x; i < nseg * Sp; i += blockDim.x) {
            const int seg = i / Sp, x = i - seg * Sp, c = seg / Sp, y = seg - c * Sp;
            lds[i] = cvt_in<Ti, LAB>(img[(((int64_t)sq.b * g.nch + c) * g.H + sq.y0 + y) * g.W + sq.x0 + x]);
        }
    }
    __syncthreads();
    const int n = (int)(g.nrows * g.ld);
    To* out = rows + sq.row_base;
    if (vec_rows) {
        constexpr int V = 16 / sizeof(To);
        for (int i = threadIdx.x; i < n / V; i += blockDim.x) {
            Pack<To> pk;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int l = lds_of(g, i * V + j);
                pk.e[j] = cvt_out<To>(l < 0 ? 0.f : lds[l]);
            }
            *(uint4*)(out + (int64_t)i * V) = pk.u;
        }
    } else {
        for (int e = threadIdx.x; e < n; e += blockDim.x) {
            const int l = lds_of(g, e);
            out[e] = cvt_out<To>(l < 0 ? 0.f : lds[l]);
        }
    }
}

template <typename Ti, typename To>
__global__ void __launch_bounds__(256) rows_to_img_kernel(const Ti* __restrict__ rows, To* __restrict__ img, Geo g, int vec_img,
                                                          int vec_rows) {
    extern __shared__ float lds[];
    const Square sq = square_of(g);
    const int n = (int)(g.nrows * g.ld);
    const Ti* in = rows + sq.row_base;
    if (vec_rows) {
        constexpr int V = 16 / sizeof(Ti);
        for (int i = threadIdx.x; i < n / V; i += blockDim.x) {
            Pack<Ti> pk;
            pk.u = *(const uint4*)(in + (int64_t)i * V);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int l = lds_of(g, i * V + j);
                if (l >= 0) lds[l] = cvt_in<Ti, false>(pk.e[j]);
            }
        }
    } else {
        for (int e = threadIdx.x; e < n; e += blockDim.x) {
            const int l = lds_of(g, e);
            if (l >= 0) lds[l] = cvt_in<Ti, false>(in[e]);
        }
    }
    __syncthreads();
    const int Sp = g.S * g.p, nseg = g.nch * Sp;
    if (vec_img) {
        constexpr int V = 16 / sizeof(To);
        const int vpr = Sp / V;
        for (int i = threadIdx.x; i < nseg * vpr; i += blockDim.x) {
            const int seg = i / vpr, v = i - seg * vpr, c = seg / Sp, y = seg - c * Sp;
            Pack<To> pk;
#pragma unroll
            for (int j = 0; j < V; ++j) pk.e[j] = cvt_out<To>(lds[seg * Sp + v * V + j]);
            *(uint4*)(img + (((int64_t)sq.b * g.nch + c) * g.H + sq.y0 + y) * g.W + sq.x0 + v * V) = pk.u;
        }
    } else {
        for (int i = threadIdx.x; i < nseg * Sp; i += blockDim.x) {
            const int seg = i / Sp, x = i - seg * Sp, c = seg / Sp, y = seg - c * Sp;
            img[(((int64_t)sq.b * g.nch + c) * g.H + sq.y0 + y) * g.W + sq.x0 + x] = cvt_out<To>(lds[i]);
        }
    }
}

constexpr int kLdsBytes = 32768;

int elt_size(int dt) {
    switch (dt) {
        case HS_F32: case HS_I32: return 4;
        case HS_BF16: return 2;
        case HS_U8: return 1;
        case HS_I64: return 8;
        default: return 0;
    }
}

// shape checks shared by both directions; fills g (and the grid size)
int make_geo(int batch, int nch, int H, int W, int p, int T, int mode, int64_t ld, Geo& g, int64_t& blocks) {
    HS_CHECK_ARG(batch > 0 && nch > 0 && p > 0 && hs::is_pow2(T) && T <= 4096, "bad shape (batch %d, channels %d, patch %d, tile %d)",
                 batch, nch, p, T);
    HS_CHECK_ARG(mode == HS_FLAT_PATCH_ROWS || mode == HS_FLAT_PIXEL_ROWS, "unknown row mode %d", mode);
    HS_CHECK_ARG(H > 0 && W > 0 && H % (p * T) == 0 && W % (p * T) == 0, "image %d x %d is not a multiple of patch %d x tile %d", H,
                 W, p, T);
    const int64_t valid = mode == HS_FLAT_PATCH_ROWS ? (int64_t)nch * p * p : nch;
    HS_CHECK_ARG(ld >= valid && ld < (1 << 20), "row pitch %lld is below the %lld valid columns", (long long)ld, (long long)valid);
    HS_CHECK_ARG((int64_t)batch * nch * H * W < (1ll << 40), "image too large");
    int S = T < 16 ? T : 16;
    while (S > 1 && (int64_t)nch * (S * p) * (S * p) * 4 > kLdsBytes) S /= 2;
    if ((int64_t)nch * p * p * 4 > kLdsBytes) return hs::fail(HS_ERR_UNSUPPORTED, "%d channels x patch %d exceed the LDS staging", nch, p);
    const int Ht = H / p, Wt = W / p;
    g.nch = nch, g.H = H, g.W = W, g.p = p, g.T = T, g.S = S, g.mode = mode, g.ld = ld;
    g.tiles_w = Wt / T;
    g.ntiles = (Ht / T) * (Wt / T);
    g.nsub = (T / S) * (T / S);
    const int64_t tokens = (int64_t)Ht * Wt;
    g.rows_per_img = mode == HS_FLAT_PATCH_ROWS ? tokens : tokens * p * p;
    g.nrows = mode == HS_FLAT_PATCH_ROWS ? (int64_t)S * S : (int64_t)S * S * p * p;
    HS_CHECK_ARG(g.nrows * ld < (1ll << 30), "square too large");
    blocks = (int64_t)batch * g.ntiles * g.nsub;
    HS_CHECK_ARG(blocks < (1ll << 31), "grid too large");
    return HS_OK;
}

bool vec_ok(const void* ptr, int elt, int64_t unit_a, int64_t unit_b) {
    const int V = 16 / elt;
    return ((uintptr_t)ptr % 16 == 0) && unit_a % V == 0 && unit_b % V == 0;
}

template <typename Ti, typename To, bool LAB>
int launch_i2r(const void* img, void* rows, const Geo& g, int64_t blocks, int ei, int eo, hipStream_t s) {
    const int Sp = g.S * g.p;
    const int vi = vec_ok(img, ei, g.W, Sp), vr = vec_ok(rows, eo, g.nrows * g.ld, g.rows_per_img * g.ld);
    hipLaunchKernelGGL((img_to_rows_kernel<Ti, To, LAB>), dim3((unsigned)blocks), dim3(256), (size_t)g.nch * Sp * Sp * 4, s,
                       (const Ti*)img, (To*)rows, g, vi, vr);
    HS_LAUNCH_CHECK("flat_img_to_rows");
    return HS_OK;
}

template <typename Ti, typename To>
int launch_r2i(const void* rows, void* img, const Geo& g, int64_t blocks, int ei, int eo, hipStream_t s) {
    const int Sp = g.S * g.p;
    const int vi = vec_ok(img, eo, g.W, Sp), vr = vec_ok(rows, ei, g.nrows * g.ld, g.rows_per_img * g.ld);
    hipLaunchKernelGGL((rows_to_img_kernel<Ti, To>), dim3((unsigned)blocks), dim3(256), (size_t)g.nch * Sp * Sp * 4, s,
                       (const Ti*)rows, (To*)img, g, vi, vr);
    HS_LAUNCH_CHECK("flat_rows_to_img");
    return HS_OK;
}

template <typename Ti>
int dispatch_i2r_out(const void* img, void* rows, int out_dtype, const Geo& g, int64_t blocks, int ei, hipStream_t s) {
    switch (out_dtype) {
        case HS_F32: return launch_i2r<Ti, float, false>(img, rows, g, blocks, ei, 4, s);
        case HS_BF16: return launch_i2r<Ti, uint16_t, false>(img, rows, g, blocks, ei, 2, s);
        default: return hs::fail(HS_ERR_UNSUPPORTED, "output dtype %d", out_dtype);
    }
}

template <typename Ti>
int dispatch_r2i_out(const void* rows, void* img, int out_dtype, const Geo& g, int64_t blocks, int ei, hipStream_t s) {
    switch (out_dtype) {
        case HS_F32: return launch_r2i<Ti, float>(rows, img, g, blocks, ei, 4, s);
        case HS_BF16: return launch_r2i<Ti, uint16_t>(rows, img, g, blocks, ei, 2, s);
        default: return hs::fail(HS_ERR_UNSUPPORTED, "output dtype %d", out_dtype);
    }
}

}  // namespace

extern "C" int hs_flat_img_to_rows(const void* img, int in_dtype, void* rows, int out_dtype, int batch, int nch, int H, int W, int p,
                                   int T, int mode, int64_t ld, void* stream) {
    HS_CHECK_ARG(img && rows && img != rows, "img and rows must be distinct non-null buffers");
    Geo g;
    int64_t blocks;
    if (int st = make_geo(batch, nch, H, W, p, T, mode, ld, g, blocks)) return st;
    const int ei = elt_size(in_dtype);
    HS_CHECK_ARG(ei > 0, "input dtype %d", in_dtype);
    hipStream_t s = (hipStream_t)stream;
    if (out_dtype == HS_U8) {  // labels: integer ids, out-of-range ones mapped to 255
        switch (in_dtype) {
            case HS_U8: return launch_i2r<uint8_t, uint8_t, true>(img, rows, g, blocks, 1, 1, s);
            case HS_I32: return launch_i2r<int32_t, uint8_t, true>(img, rows, g, blocks, 4, 1, s);
            case HS_I64: return launch_i2r<int64_t, uint8_t, true>(img, rows, g, blocks, 8, 1, s);
            default: return hs::fail(HS_ERR_UNSUPPORTED, "uint8 rows take integer labels, got dtype %d", in_dtype);
        }
    }
    switch (in_dtype) {
        case HS_F32: return dispatch_i2r_out<float>(img, rows, out_dtype, g, blocks, 4, s);
        case HS_BF16: return dispatch_i2r_out<uint16_t>(img, rows, out_dtype, g, blocks, 2, s);
        case HS_U8: return dispatch_i2r_out<uint8_t>(img, rows, out_dtype, g, blocks, 1, s);
        default: return hs::fail(HS_ERR_UNSUPPORTED, "input dtype %d", in_dtype);
    }
}

extern "C" int hs_flat_rows_to_img(const void* rows, int in_dtype, void* img, int out_dtype, int batch, int nch, int H, int W, int p,
                                   int T, int mode, int64_t ld, void* stream) {
    HS_CHECK_ARG(img && rows && img != rows, "img and rows must be distinct non-null buffers");
    Geo g;
    int64_t blocks;
    if (int st = make_geo(batch, nch, H, W, p, T, mode, ld, g, blocks)) return st;
    hipStream_t s = (hipStream_t)stream;
    if (in_dtype == HS_U8 || out_dtype == HS_U8) {  // class ids (the predictions of forward_seg_step): bytes to bytes
        if (in_dtype != out_dtype) return hs::fail(HS_ERR_UNSUPPORTED, "uint8 rows go to a uint8 image (got dtypes %d -> %d)", in_dtype, out_dtype);
        return launch_r2i<uint8_t, uint8_t>(rows, img, g, blocks, 1, 1, s);
    }
    switch (in_dtype) {
        case HS_F32: return dispatch_r2i_out<float>(rows, img, out_dtype, g, blocks, 4, s);
        case HS_BF16: return dispatch_r2i_out<uint16_t>(rows, img, out_dtype, g, blocks, 2, s);
        default: return hs::fail(HS_ERR_UNSUPPORTED, "input dtype %d", in_dtype);
    }
}
