// The token-row layouts of the flat Swin-UNet inside one Morton-aligned square of S x S tokens (S^2 consecutive tokens in tiled Z
// order, so the square's rows are one contiguous run): which pixel of the square's (S p) x (S p) pixels an element of that run
// holds.  Shared by the layout kernels (csrc/flat_layout.hip) and the resize kernel that writes the same rows (csrc/flat_data.hip).
#pragma once

#include "hs_device.h"

namespace hs {
namespace flat_rows {

// the even bits of v, packed: the column (v) or row (v >> 1 ... see callers) of a Morton index
__host__ __device__ __forceinline__ uint32_t compact(uint32_t v) {
    v &= 0x55555555u;
    v = (v | (v >> 1)) & 0x33333333u;
    v = (v | (v >> 2)) & 0x0F0F0F0Fu;
    v = (v | (v >> 4)) & 0x00FF00FFu;
    v = (v | (v >> 8)) & 0x0000FFFFu;
    return v;
}

struct Pixel {
    int c, y, x;  // channel and pixel inside the square; c < 0: a padding column
};

// element e of the square's run (row pitch ld) -> its pixel.  HS_FLAT_PATCH_ROWS: row = token, column = (c, kh, kw);
// HS_FLAT_PIXEL_ROWS: row = token * p^2 + kh * p + kw, column = c.  The row bit of a token is the least significant one.
__device__ __forceinline__ Pixel pixel_of(int mode, int nch, int p, int ld, int e) {
    const int pp = p * p;
    const int r = e / ld, col = e - r * ld;
    int t, kk, c;
    if (mode == HS_FLAT_PATCH_ROWS) {
        if (col >= nch * pp) return {-1, 0, 0};
        t = r;
        c = col / pp;
        kk = col - c * pp;
    } else {
        if (col >= nch) return {-1, 0, 0};
        t = r / pp;
        kk = r - t * pp;
        c = col;
    }
    const int kh = kk / p, kw = kk - kh * p;
    return {c, (int)compact((uint32_t)t) * p + kh, (int)compact((uint32_t)t >> 1) * p + kw};
}

}  // namespace flat_rows
}  // namespace hs
