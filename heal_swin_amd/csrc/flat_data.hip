// The flat data path (heal_swin_amd/flat_data.py): a raw camera frame, class mask or depth map -> what the flat Swin-UNet reads,
// the reference's CenterCrop -> Resize -> Pad (data/segmentation/flat_datasets.py:84-125, data/depth_estimation/
// flat_depth_datasets.py:69-147) and, for depth, its target chain, as ONE pass per tensor.
//
//   hs_flat_resize   src [B, nch, H0, W0] (uint8 or fp32, any batch stride) -> EITHER the NCHW result [B, nch, H, W] (HS_FLAT_IMAGE)
//                    OR the model's token rows (HS_FLAT_PATCH_ROWS / HS_FLAT_PIXEL_ROWS, what hs_flat_img_to_rows makes of that
//                    image), never writing the image in between.
//
// Crop, resize and pad are separable, so the host composes them into two per-axis tables (O(H + W)): for every output row / column
// the source row / column (nearest: values copied bit for bit), or the two taps and their fp32 weights (bilinear), or -1 for
// padding (value 0).  Bilinear values are h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11) in fp32 without contraction, the
// order hs_flat_depth_to_hp documents; uint8 sources are then rounded half to even and cast (torchvision's tensor path: float(),
// interpolate, round, to(uint8)).  fp32 sources then go through the depth target chain of hs_depth_target.h when one is given.
//
// One workgroup owns a tile of the OUTPUT: a Morton-aligned square of S x S tokens for the row layouts (its rows are one
// contiguous run of memory, as in flat_layout.hip), a tile_h x tile_w rectangle for the image layout.  It reads the tile's slices of
// the two tables into LDS, takes the window of source rows and columns they name, stages that window in LDS with 16-byte loads
// (neighbouring tiles share at most the rim of a window, which the L2 serves), and then produces its output elements in memory order,
// 16 bytes per lane and store.  The caller sizes the tile so that the largest window (span_h x span_w, known on the host from the
// tables) fits the LDS; taps are clamped into the staged window and the source, so a wrong table gives wrong values, never an
// access outside the buffers.
#include <algorithm>
#include <climits>
#include <type_traits>

#include "hs_device.h"

#pragma clang fp contract(off)

#include "hs_depth_target.h"
#include "hs_flat_rows.h"

namespace {

using hs::float_to_bf16;
using hs::flat_rows::compact;

constexpr int kThreads = 256;
constexpr int kLdsMax = 65536;
constexpr int kTileMax = 256;  // pixels along one side of a tile

struct Job {
    int nch, H0, W0, H, W;
    int64_t src_sb;  // batch stride of the source, elements
    int layout, p, T, S, tiles_w, ntiles, nsub, ld;  // row layouts: as flat_layout.hip's Geo
    int64_t rows_per_img, run;                       // rows of one image, elements of one square's run
    int tile_h, tile_w, tiles_x, tiles_y;            // output tile (pixels) and, for the image layout, the tile grid
    int tmax, sh, sw;                                // table slots per axis, staged window rows, window pitch (elements)
    int vec_src, vec_out, has_op;
    hs::TargetOp op;
};

template <typename T>
union Pack {
    uint4 u;
    T e[16 / sizeof(T)];
};

struct Tables {  // the tile's slices, tap indices relative to the staged window; -1: padding
    const int *r0, *r1, *c0, *c1;
    const float *rl0, *rl1, *cl0, *cl1;
};

template <typename Ts, bool BIL>
__device__ __forceinline__ Ts sample(const Ts* __restrict__ win, const Tables& t, int sw, int y, int x) {
    const int r0 = t.r0[y], c0 = t.c0[x];
    if (r0 < 0 || c0 < 0) return (Ts)0;
    if constexpr (!BIL) {
        return win[r0 * sw + c0];
    } else {
        const int r1 = t.r1[y], c1 = t.c1[x];
        const float h0 = t.rl0[y], h1 = t.rl1[y], w0 = t.cl0[x], w1 = t.cl1[x];
        const float p00 = (float)win[r0 * sw + c0], p01 = (float)win[r0 * sw + c1];
        const float p10 = (float)win[r1 * sw + c0], p11 = (float)win[r1 * sw + c1];
        const float v = h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11);
        if constexpr (std::is_same<Ts, uint8_t>::value) return (uint8_t)rintf(v);  // round half to even; v is in [0, 255]
        else return v;
    }
}

template <typename Ts, typename To>
__device__ __forceinline__ To convert(Ts v, const Job& j) {
    if constexpr (std::is_same<Ts, float>::value) return j.has_op ? hs::target_op(v, j.op) : v;
    else if constexpr (std::is_same<To, uint16_t>::value) return float_to_bf16((float)v);
    else return (To)v;
}

template <typename Ts, typename To, bool BIL>
__global__ void __launch_bounds__(kThreads) flat_resize_kernel(const Ts* __restrict__ src, const int32_t* __restrict__ ridx,
                                                              const float* __restrict__ rwgt, const int32_t* __restrict__ cidx,
                                                              const float* __restrict__ cwgt, To* __restrict__ out, Job j) {
    extern __shared__ uint4 lds_raw[];
    int* ti = (int*)lds_raw;              // [4][tmax]: row tap 0, row tap 1, column tap 0, column tap 1
    float* tf = (float*)(ti + 4 * j.tmax);  // [4][tmax]: their weights
    int* win = (int*)(tf + 4 * j.tmax);   // first / last source row, first / last source column of the tile
    Ts* sbuf = (Ts*)(win + 4);
    const int tid = threadIdx.x;

    // the tile
    int b, y0, x0;
    int64_t out_base;
    if (j.layout == HS_FLAT_IMAGE) {
        const int per = j.tiles_x * j.tiles_y, tile = blockIdx.x % per;
        b = blockIdx.x / per;
        y0 = (tile / j.tiles_x) * j.tile_h;
        x0 = (tile % j.tiles_x) * j.tile_w;
        out_base = (int64_t)b * j.nch * j.H * j.W;
    } else {
        const int q = blockIdx.x % j.nsub, rest = blockIdx.x / j.nsub, tile = rest % j.ntiles;
        b = rest / j.ntiles;
        y0 = ((tile / j.tiles_w) * j.T + (int)compact((uint32_t)q) * j.S) * j.p;
        x0 = ((tile % j.tiles_w) * j.T + (int)compact((uint32_t)q >> 1) * j.S) * j.p;
        const int64_t z0 = (int64_t)tile * j.T * j.T + (int64_t)q * j.S * j.S;
        out_base = ((int64_t)b * j.rows_per_img + (j.layout == HS_FLAT_PATCH_ROWS ? z0 : z0 * j.p * j.p)) * j.ld;
    }
    const int th = min(j.tile_h, j.H - y0), tw = min(j.tile_w, j.W - x0);

    // its table slices and the source window they name
    if (tid == 0) win[0] = INT_MAX, win[1] = -1, win[2] = INT_MAX, win[3] = -1;
    __syncthreads();
    for (int t = tid; t < th + tw; t += kThreads) {
        const bool row = t < th;
        const int k = row ? t : t - th, n = row ? j.H : j.W, at = (row ? y0 : x0) + k, lim = (row ? j.H0 : j.W0) - 1;
        const int32_t* idx = row ? ridx : cidx;
        const float* wgt = row ? rwgt : cwgt;
        int i0 = idx[at], i1 = BIL ? idx[n + at] : i0;
        if (i0 >= 0) {
            i0 = min(i0, lim);
            i1 = min(max(i1, i0), lim);
            atomicMin(&win[row ? 0 : 2], i0);
            atomicMax(&win[row ? 1 : 3], i1);
        }
        const int slot = (row ? 0 : 2) * j.tmax + k;
        ti[slot] = i0;
        ti[slot + j.tmax] = i1;
        if (BIL) {
            tf[slot] = wgt[at];
            tf[slot + j.tmax] = wgt[n + at];
        }
    }
    __syncthreads();
    constexpr int V = 16 / sizeof(Ts);
    const int ylo = win[0], xlo = j.vec_src ? (win[2] / V) * V : win[2];
    const bool any = win[1] >= 0 && win[3] >= 0;
    const int ny = any ? min(win[1] - ylo + 1, j.sh) : 0;
    const int nx = any ? min((j.vec_src ? (win[3] / V + 1) * V : win[3] + 1) - xlo, j.sw) : 0;
    for (int t = tid; t < th + tw; t += kThreads) {  // (each thread rewrites the slots it wrote)
        const bool row = t < th;
        const int slot = (row ? 0 : 2) * j.tmax + (row ? t : t - th), lo = row ? ylo : xlo, last = (row ? ny : nx) - 1;
        if (ti[slot] >= 0) {
            ti[slot] = min(ti[slot] - lo, last);
            ti[slot + j.tmax] = min(ti[slot + j.tmax] - lo, last);
        }
    }

    // stage the window: [nch][ny][nx] at pitch sw
    const Ts* sb = src + (int64_t)b * j.src_sb;
    if (j.vec_src) {
        const int vpr = nx / V;
        for (int i = tid; i < j.nch * ny * vpr; i += kThreads) {
            const int v = i % vpr, r = (i / vpr) % ny, c = i / (vpr * ny);
            *(uint4*)(sbuf + ((int64_t)c * j.sh + r) * j.sw + v * V) =
                *(const uint4*)(sb + ((int64_t)c * j.H0 + ylo + r) * j.W0 + xlo + v * V);
        }
    } else {
        for (int i = tid; i < j.nch * ny * nx; i += kThreads) {
            const int x = i % nx, r = (i / nx) % ny, c = i / (nx * ny);
            sbuf[((int64_t)c * j.sh + r) * j.sw + x] = sb[((int64_t)c * j.H0 + ylo + r) * j.W0 + xlo + x];
        }
    }
    __syncthreads();

    const Tables t{ti, ti + j.tmax, ti + 2 * j.tmax, ti + 3 * j.tmax, tf, tf + j.tmax, tf + 2 * j.tmax, tf + 3 * j.tmax};
    const int plane = j.sh * j.sw;
    constexpr int VO = 16 / sizeof(To);
    To* o = out + out_base;
    if (j.layout == HS_FLAT_IMAGE) {
        if (j.vec_out) {  // W, tile_w and so tw are multiples of VO
            const int vpr = tw / VO;
            for (int i = tid; i < j.nch * th * vpr; i += kThreads) {
                const int v = i % vpr, y = (i / vpr) % th, c = i / (vpr * th);
                Pack<To> pk;
#pragma unroll
                for (int k = 0; k < VO; ++k) pk.e[k] = convert<Ts, To>(sample<Ts, BIL>(sbuf + c * plane, t, j.sw, y, v * VO + k), j);
                *(uint4*)(o + ((int64_t)c * j.H + y0 + y) * j.W + x0 + v * VO) = pk.u;
            }
        } else {
            for (int i = tid; i < j.nch * th * tw; i += kThreads) {
                const int x = i % tw, y = (i / tw) % th, c = i / (tw * th);
                o[((int64_t)c * j.H + y0 + y) * j.W + x0 + x] = convert<Ts, To>(sample<Ts, BIL>(sbuf + c * plane, t, j.sw, y, x), j);
            }
        }
        return;
    }
    const auto element = [&](int e) -> To {  // element e of the square's run
        const hs::flat_rows::Pixel q = hs::flat_rows::pixel_of(j.layout, j.nch, j.p, j.ld, e);
        return q.c < 0 ? (To)0 : convert<Ts, To>(sample<Ts, BIL>(sbuf + q.c * plane, t, j.sw, q.y, q.x), j);
    };
    const int n = (int)j.run;
    if (j.vec_out) {
        for (int i = tid; i < n / VO; i += kThreads) {
            Pack<To> pk;
#pragma unroll
            for (int k = 0; k < VO; ++k) pk.e[k] = element(i * VO + k);
            *(uint4*)(o + (int64_t)i * VO) = pk.u;
        }
    } else {
        for (int e = tid; e < n; e += kThreads) o[e] = element(e);
    }
}

int src_elt(int dt) { return dt == HS_U8 ? 1 : dt == HS_F32 ? 4 : 0; }
int out_elt(int dt) { return dt == HS_U8 ? 1 : dt == HS_BF16 ? 2 : dt == HS_F32 ? 4 : 0; }

// window pitch (elements): the widest 16-byte-aligned cover of span_w consecutive elements
int window_pitch(int span_w, int elt) {
    const int V = 16 / elt;
    return (span_w + 2 * (V - 1)) / V * V;
}

int64_t lds_bytes(int nch, int elt, int tile_h, int tile_w, int span_h, int span_w) {
    const int tmax = (std::max(tile_h, tile_w) + 3) / 4 * 4;
    return (int64_t)8 * tmax * 4 + 16 + (int64_t)nch * span_h * window_pitch(span_w, elt) * elt;
}

template <typename Ts, typename To>
int launch(const void* src, const int32_t* ridx, const float* rwgt, const int32_t* cidx, const float* cwgt, void* out, const Job& j,
           int64_t blocks, size_t lds, hipStream_t s) {
    if (rwgt)
        hipLaunchKernelGGL((flat_resize_kernel<Ts, To, true>), dim3((unsigned)blocks), dim3(kThreads), lds, s, (const Ts*)src, ridx, rwgt,
                           cidx, cwgt, (To*)out, j);
    else
        hipLaunchKernelGGL((flat_resize_kernel<Ts, To, false>), dim3((unsigned)blocks), dim3(kThreads), lds, s, (const Ts*)src, ridx,
                           rwgt, cidx, cwgt, (To*)out, j);
    HS_LAUNCH_CHECK("flat_resize");
    return HS_OK;
}

}  // namespace

extern "C" int64_t hs_flat_resize_lds_bytes(int nch, int src_dtype, int tile_h, int tile_w, int span_h, int span_w) {
    const int elt = src_elt(src_dtype);
    if (!elt || nch < 1 || tile_h < 1 || tile_w < 1 || span_h < 0 || span_w < 0) return -1;
    return lds_bytes(nch, elt, tile_h, tile_w, span_h, span_w);
}

extern "C" int hs_flat_resize(const void* src, int src_dtype, int64_t src_stride_b, int batch, int nch, int H0, int W0,
                              const int32_t* row_idx, const float* row_wgt, const int32_t* col_idx, const float* col_wgt, void* out,
                              int out_dtype, int H, int W, int layout, int p, int T, int64_t ld, int tile_h, int tile_w, int span_h,
                              int span_w, int flags, int transform, float shift, float scale, void* stream) {
    HS_CHECK_ARG(src && out && src != out && row_idx && col_idx, "src, out and the index tables must be distinct non-null buffers");
    HS_CHECK_ARG((row_wgt != nullptr) == (col_wgt != nullptr), "give both weight tables (bilinear) or neither (nearest)");
    HS_CHECK_ARG(batch > 0 && nch > 0 && H0 > 0 && W0 > 0 && H > 0 && W > 0, "bad shape (batch %d, channels %d, %d x %d -> %d x %d)", batch,
                 nch, H0, W0, H, W);
    HS_CHECK_ARG((int64_t)nch * H0 * W0 < (1ll << 31) && (int64_t)nch * H * W < (1ll << 31) && src_stride_b >= (int64_t)nch * H0 * W0,
                 "image too large, or a batch stride below one image");
    const int es = src_elt(src_dtype), eo = out_elt(out_dtype);
    HS_CHECK_ARG(es > 0 && eo > 0, "dtypes: source uint8 / fp32, output uint8 / fp32 / bf16 (got %d -> %d)", src_dtype, out_dtype);
    HS_CHECK_ARG(src_dtype == HS_U8 || out_dtype == HS_F32, "an fp32 source gives an fp32 result");
    HS_CHECK_ARG((flags & ~(HS_DT_1000_BKG | HS_DT_AFFINE)) == 0, "flags: HS_DT_1000_BKG | HS_DT_AFFINE (the flat datasets keep zeros), got %d",
                 flags);
    HS_CHECK_ARG(transform == HS_DT_NONE || transform == HS_DT_LOG || transform == HS_DT_INV, "transform %d", transform);
    HS_CHECK_ARG(src_dtype == HS_F32 || (flags == 0 && transform == HS_DT_NONE), "the depth target chain applies to fp32 sources only");
    HS_CHECK_ARG(tile_h > 0 && tile_w > 0 && tile_h <= kTileMax && tile_w <= kTileMax && span_h >= 0 && span_w >= 0 && span_h <= H0 &&
                     span_w <= W0, "bad tile %d x %d or window %d x %d", tile_h, tile_w, span_h, span_w);
    Job j{};
    j.nch = nch, j.H0 = H0, j.W0 = W0, j.H = H, j.W = W, j.src_sb = src_stride_b, j.layout = layout;
    j.tile_h = tile_h, j.tile_w = tile_w;
    j.tmax = (std::max(tile_h, tile_w) + 3) / 4 * 4;
    j.sh = span_h, j.sw = window_pitch(span_w, es);
    j.has_op = flags != 0 || transform != HS_DT_NONE;
    j.op = hs::TargetOp{flags, transform, shift, scale};
    const int64_t lds = lds_bytes(nch, es, tile_h, tile_w, span_h, span_w);
    if (lds > kLdsMax)
        return hs::fail(HS_ERR_UNSUPPORTED, "a %d x %d tile with a %d x %d window of %d channels needs %lld bytes of LDS (limit %d)", tile_h,
                        tile_w, span_h, span_w, nch, (long long)lds, kLdsMax);
    const int Vs = 16 / es, Vo = 16 / eo;
    j.vec_src = (uintptr_t)src % 16 == 0 && W0 % Vs == 0 && src_stride_b % Vs == 0;
    int64_t blocks;
    if (layout == HS_FLAT_IMAGE) {
        j.tiles_x = (W + tile_w - 1) / tile_w, j.tiles_y = (H + tile_h - 1) / tile_h;
        blocks = (int64_t)batch * j.tiles_x * j.tiles_y;
        j.vec_out = (uintptr_t)out % 16 == 0 && W % Vo == 0 && tile_w % Vo == 0;
    } else {
        HS_CHECK_ARG(layout == HS_FLAT_PATCH_ROWS || layout == HS_FLAT_PIXEL_ROWS, "unknown layout %d", layout);
        HS_CHECK_ARG(p > 0 && hs::is_pow2(T) && T <= 4096 && H % (p * T) == 0 && W % (p * T) == 0,
                     "image %d x %d is not a multiple of patch %d x tile %d (a power of two)", H, W, p, T);
        const int S = tile_h / p;
        HS_CHECK_ARG(tile_h == tile_w && S * p == tile_h && hs::is_pow2(S) && S <= T, "a row-layout tile is S p pixels square, S a power of "
                     "two <= T (got %d x %d, p %d, T %d)", tile_h, tile_w, p, T);
        const int64_t valid = layout == HS_FLAT_PATCH_ROWS ? (int64_t)nch * p * p : nch;
        HS_CHECK_ARG(ld >= valid && ld < (1 << 20), "row pitch %lld is below the %lld valid columns", (long long)ld, (long long)valid);
        const int Ht = H / p, Wt = W / p;
        j.p = p, j.T = T, j.S = S, j.ld = (int)ld;
        j.tiles_w = Wt / T, j.ntiles = (Ht / T) * (Wt / T), j.nsub = (T / S) * (T / S);
        const int64_t per_token = layout == HS_FLAT_PATCH_ROWS ? 1 : (int64_t)p * p;
        j.rows_per_img = (int64_t)Ht * Wt * per_token;
        j.run = (int64_t)S * S * per_token * ld;
        HS_CHECK_ARG(j.run < (1ll << 30), "square too large");
        blocks = (int64_t)batch * j.ntiles * j.nsub;
        j.vec_out = (uintptr_t)out % 16 == 0 && j.run % Vo == 0 && (j.rows_per_img * ld) % Vo == 0;
    }
    HS_CHECK_ARG(blocks < (1ll << 31), "grid too large");
    hipStream_t s = (hipStream_t)stream;
    if (src_dtype == HS_F32) return launch<float, float>(src, row_idx, row_wgt, col_idx, col_wgt, out, j, blocks, (size_t)lds, s);
    switch (out_dtype) {
        case HS_U8: return launch<uint8_t, uint8_t>(src, row_idx, row_wgt, col_idx, col_wgt, out, j, blocks, (size_t)lds, s);
        case HS_F32: return launch<uint8_t, float>(src, row_idx, row_wgt, col_idx, col_wgt, out, j, blocks, (size_t)lds, s);
        default: return launch<uint8_t, uint16_t>(src, row_idx, row_wgt, col_idx, col_wgt, out, j, blocks, (size_t)lds, s);
    }
}
