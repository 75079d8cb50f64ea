// Host-side tables of the flat Swin-UNet (SwinTransformerSys) in tiled Z order (plain C++).
//
// The token grid Ht x Wt is cut into T x T tiles laid out row-major; inside a tile the tokens follow a Morton order whose
// least-significant bit is the ROW bit.  With T = w * 2^(L-1) every window of every stage is w*w consecutive tokens, the 2 x 2
// children of a PatchMerging token are 4 consecutive tokens in the order (0,0), (1,0), (0,1), (1,1), and the cyclic shift plus
// window partition of a shifted block is a row permutation (idx) with per-position region labels, exactly like the HEALPix
// shifters of healpix_tables.cpp.
#include <vector>

#include "hs_common.h"

namespace {

inline uint32_t spread(uint32_t v) {  // abc -> 0a0b0c
    v &= 0xFFFFu;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}
inline uint32_t compact(uint32_t v) {  // keeps the even bits
    v &= 0x55555555u;
    v = (v | (v >> 1)) & 0x33333333u;
    v = (v | (v >> 2)) & 0x0F0F0F0Fu;
    v = (v | (v >> 4)) & 0x00FF00FFu;
    v = (v | (v >> 8)) & 0x0000FFFFu;
    return v;
}

struct Grid {
    int Ht, Wt, T, tiles_w;
    int64_t z_of(int h, int w) const {
        const int64_t tile = (int64_t)(h / T) * tiles_w + (w / T);
        return tile * T * T + (spread(h % T) | (spread(w % T) << 1));
    }
    void cell_of(int64_t z, int& h, int& w) const {
        const int64_t tile = z / ((int64_t)T * T);
        const uint32_t m = (uint32_t)(z - tile * T * T);
        h = (int)(tile / tiles_w) * T + (int)compact(m);
        w = (int)(tile % tiles_w) * T + (int)compact(m >> 1);
    }
};

int check_grid(int Ht, int Wt, int T) {
    HS_CHECK_ARG(Ht > 0 && Wt > 0 && (int64_t)Ht * Wt < (1ll << 31), "token grid %d x %d out of range", Ht, Wt);
    HS_CHECK_ARG(hs::is_pow2(T) && T <= 32768, "tile side must be a power of two, got %d", T);
    HS_CHECK_ARG(Ht % T == 0 && Wt % T == 0, "token grid %d x %d is not a multiple of the tile side %d", Ht, Wt, T);
    return HS_OK;
}

// region of one coordinate in the reference's img_mask slices (0, -w), (-w, -s), (-s, None)
inline int region(int v, int n, int w, int s) { return v < n - w ? 0 : (v < n - s ? 1 : 2); }

}  // namespace

extern "C" {

int hs_flat_zorder(int Ht, int Wt, int T, int32_t* z_of_rm, int32_t* rm_of_z) {
    if (int st = check_grid(Ht, Wt, T)) return st;
    const Grid g{Ht, Wt, T, Wt / T};
    for (int h = 0; h < Ht; ++h)
        for (int w = 0; w < Wt; ++w) {
            const int64_t z = g.z_of(h, w), rm = (int64_t)h * Wt + w;
            if (z_of_rm) z_of_rm[rm] = (int32_t)z;
            if (rm_of_z) rm_of_z[z] = (int32_t)rm;
        }
    return HS_OK;
}

int hs_build_flat_shift(int Ht, int Wt, int T, int w, int s, int32_t* idx, int32_t* inv, uint8_t* labels) {
    if (int st = check_grid(Ht, Wt, T)) return st;
    HS_CHECK_ARG(hs::is_pow2(w) && w <= T, "window side %d must be a power of two no larger than the tile side %d", w, T);
    HS_CHECK_ARG(s >= 0 && s < w, "shift %d must be in [0, window %d)", s, w);
    const Grid g{Ht, Wt, T, Wt / T};
    const int64_t n = (int64_t)Ht * Wt;
    for (int64_t j = 0; j < n; ++j) {
        int h, x;
        g.cell_of(j, h, x);
        // torch.roll(x, (-s, -s)): shifted cell (h, x) holds the token of (h + s, x + s)
        const int64_t src = g.z_of((h + s) % Ht, (x + s) % Wt);
        if (idx) idx[j] = (int32_t)src;
        if (inv) inv[src] = (int32_t)j;
        if (labels) labels[j] = (uint8_t)(3 * region(h, Ht, w, s) + region(x, Wt, w, s));
    }
    return HS_OK;
}

int hs_flat_rel_pos_index(int w, int64_t* row_major, int64_t* zorder) {
    HS_CHECK_ARG(hs::is_pow2(w) && w <= 256, "window side must be a power of two, got %d", w);
    const int n = w * w, span = 2 * w - 1;
    auto rel = [&](int ra, int ca, int rb, int cb) { return (int64_t)(ra - rb + w - 1) * span + (ca - cb + w - 1); };
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            if (row_major) row_major[(int64_t)a * n + b] = rel(a / w, a % w, b / w, b % w);
            if (zorder)
                zorder[(int64_t)a * n + b] = rel((int)compact(a), (int)compact(a >> 1), (int)compact(b), (int)compact(b >> 1));
        }
    return HS_OK;
}

int hs_flat_attn_mask(int Ht, int Wt, int w, int s, float* out) {
    HS_CHECK_ARG(out && w > 0 && Ht % w == 0 && Wt % w == 0, "grid %d x %d is not a multiple of the window %d", Ht, Wt, w);
    HS_CHECK_ARG(s > 0 && s < w, "shift %d must be in (0, window %d)", s, w);
    const int n = w * w, nwh = Ht / w, nww = Wt / w;
    std::vector<uint8_t> lab(n);
    for (int wy = 0; wy < nwh; ++wy)
        for (int wx = 0; wx < nww; ++wx) {
            for (int a = 0; a < n; ++a) lab[a] = (uint8_t)(3 * region(wy * w + a / w, Ht, w, s) + region(wx * w + a % w, Wt, w, s));
            float* m = out + ((int64_t)wy * nww + wx) * n * n;
            for (int a = 0; a < n; ++a)
                for (int b = 0; b < n; ++b) m[(int64_t)a * n + b] = lab[a] == lab[b] ? 0.f : -100.f;
        }
    return HS_OK;
}

}  // extern "C"
