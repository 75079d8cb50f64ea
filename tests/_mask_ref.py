"""Host reference of the library's dropout mask (csrc/hs_device.h, the comment above `ElemRng`), in numpy on uint64 values
masked to 32 bits.  Independent of every kernel: the GPU tests compare the zero pattern of the kernels' outputs with `keep`.

The keep decision of element i under (p, seed):
  mix32(x)     x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (all mod 2^32)
  key_lo       lo32(seed);   key_hi = mix32(hi32(seed) + 0x85EBCA6B)
  chunk        c = i >> 3;   ck = mix32(mix32(lo32(c) ^ key_hi ^ hi32(c) * 0x9E3779B9) ^ key_lo)
  pair         u = ck * M[(i >> 1) & 3],  h = u ^ (u >> 16);  an even element takes lo16(h), an odd one hi16(h)
  kept         when those 16 bits are >= floor(fp32(p) * 65536); everything is dropped at p >= 1
  epoch        a registered counter e replaces seed by seed + e * 0x9E3779B97F4A7C15 (mod 2^64)
A kept element is multiplied by fp32(1 / (1 - p)).
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PAIR_MULT = np.array([0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F], dtype=np.uint64)
EPOCH_MULT = 0x9E3779B97F4A7C15


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def threshold(p):
    """Drop threshold on the 16 random bits: the drop probability in steps of 2^-16 (fp32 product, truncated)."""
    return 65536 if p >= 1.0 else int(np.float32(p) * np.float32(65536.0))


def keep_scale(p):
    """fp32(1 / (1 - p)) as the kernels compute it (0 at p >= 1)."""
    return 0.0 if p >= 1.0 else float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def bits16(i, seed, epoch=0):
    """The 16 random bits of the elements i (any integer array, values < 2^63)."""
    i = np.asarray(i).astype(np.uint64)
    seed = (int(seed) + int(epoch) * EPOCH_MULT) & 0xFFFFFFFFFFFFFFFF
    key_lo = np.uint64(seed & 0xFFFFFFFF)
    key_hi = mix32(np.uint64(((seed >> 32) + 0x85EBCA6B) & 0xFFFFFFFF))
    c = i >> np.uint64(3)
    c_hi = ((c >> np.uint64(32)) * np.uint64(0x9E3779B9)) & M32
    ck = mix32(mix32((c & M32) ^ key_hi ^ c_hi) ^ key_lo)
    u = (ck * PAIR_MULT[((i >> np.uint64(1)) & np.uint64(3)).astype(np.int64)]) & M32
    h = u ^ (u >> np.uint64(16))
    return np.where((i & np.uint64(1)) == 1, h >> np.uint64(16), h & np.uint64(0xFFFF))


def keep(i, p, seed, epoch=0):
    """Boolean array: element i is kept."""
    return bits16(i, seed, epoch) >= np.uint64(threshold(p))
