"""Host reference of the attention dropout mask (csrc/window_attn.h, `DropRng` and its comment), in numpy on uint64 values masked to
32 bits.  Independent of every kernel: the GPU tests decode the keep decisions from the kernels' outputs and compare them with `keep`.

The keep decision of probability (row, key) under (p, seed), with row = (b * nH + h) * N + shifted query row and key < 256:
  hash32(x)    x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (all mod 2^32)
  base         row * 256 (64 bits)
  row_key      hash32(hash32(lo32(base) ^ hash32(hi32(seed) + hi32(base) * 0x9E3779B9)) ^ lo32(seed))
  row_key2     hash32(row_key ^ 0x5BD1E995): the key of the row for the keys whose bit 2 is set
  pair_mult(q) hash32(q * 0x9E3779B9 + 0x7F4A7C15) | 1, with q the pair index key >> 1 with ITS bit 1 (bit 2 of the key) cleared
  pair         u = (row_key or row_key2) * pair_mult(q),  h = u ^ (u >> 16);  an even key takes lo16(h), an odd one hi16(h)
  kept         when those 16 bits are >= floor(fp32(p) * 65536); everything is dropped at p >= 1
  epoch        a registered counter e replaces seed by seed + e * 0x9E3779B97F4A7C15 (mod 2^64)
A kept probability is multiplied by fp32(1 / (1 - p)).
"""
import numpy as np

from _mask_ref import EPOCH_MULT, keep_scale, threshold  # noqa: F401  (keep_scale: re-exported for the tests)

M32 = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.uint64(x)


def hash32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> _u(16))
    x = (x * _u(0x7FEB352D)) & M32
    x = x ^ (x >> _u(15))
    x = (x * _u(0x846CA68B)) & M32
    return x ^ (x >> _u(16))


def row_keys(row, seed, epoch=0):
    """(row_key, row_key2) of the rows (any integer array, values < 2^55)."""
    row = np.asarray(row).astype(np.uint64)
    seed = (int(seed) + int(epoch) * EPOCH_MULT) & 0xFFFFFFFFFFFFFFFF
    seed_lo, seed_hi = _u(seed & 0xFFFFFFFF), _u(seed >> 32)
    base = row * _u(256)
    hi = hash32((seed_hi + (base >> _u(32)) * _u(0x9E3779B9)) & M32)
    k1 = hash32(hash32((base & M32) ^ hi) ^ seed_lo)
    return k1, hash32(k1 ^ _u(0x5BD1E995))


def pair_mult(q):
    q = np.asarray(q, dtype=np.uint64)
    return hash32((q * _u(0x9E3779B9) + _u(0x7F4A7C15)) & M32) | _u(1)


def bits16(row, key, seed, epoch=0):
    """The 16 random bits of the probabilities (row, key); row and key broadcast against each other."""
    key = np.asarray(key).astype(np.uint64)
    assert int(key.max(initial=0)) < 256
    k1, k2 = row_keys(row, seed, epoch)
    k1, k2, key = np.broadcast_arrays(k1, k2, key)
    rk = np.where((key & _u(4)) != 0, k2, k1)
    u = (rk * pair_mult((key >> _u(1)) & ~_u(2) & M32)) & M32
    h = u ^ (u >> _u(16))
    return np.where((key & _u(1)) == 1, h >> _u(16), h & _u(0xFFFF))


def keep(row, key, p, seed, epoch=0):
    """Boolean array: probability (row, key) is kept."""
    return bits16(row, key, seed, epoch) >= _u(threshold(p))
