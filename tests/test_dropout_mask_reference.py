"""The dropout-mask rule itself (tests/_mask_ref.py, written from the comment in csrc/hs_device.h), on the host: what a keep-rate
check through a kernel cannot see -- rates per position of a chunk, independence inside a chunk, between neighbouring chunks and
between neighbouring seeds -- each within 5 binomial standard deviations of its expectation over 2^20 elements.  Under the null
hypothesis one of the ~50 quantities of a case exceeds 5 sd with probability 3e-5; the rule as written stays below 3.

The GPU tests (test_gpu_stream_kernels.py) pin the kernels to this reference element by element."""
import itertools

import numpy as np
import pytest

from _mask_ref import keep, threshold

N = 1 << 20
SEEDS = [0, 42, 12345, (7 << 32) | 9]
PS = [0.1, 0.3, 0.5]
Z_MAX = 5.0


def _z(count, n, prob):
    return abs(count / n - prob) / np.sqrt(prob * (1.0 - prob) / n)


_KEEP = {}


def _mask(p, seed):
    if (p, seed) not in _KEEP:
        k = keep(np.arange(N, dtype=np.uint64), p, seed)
        k.setflags(write=False)
        _KEEP[(p, seed)] = k
    return _KEEP[(p, seed)]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", PS)
def test_keep_rates_and_independence(p, seed):
    q = 1.0 - threshold(p) / 65536.0
    k = _mask(p, seed).reshape(-1, 8)  # [chunk, position]
    n = k.shape[0]
    worst = 0.0
    for j in range(8):
        z = _z(int(k[:, j].sum()), n, q)
        worst = max(worst, z)
        assert z <= Z_MAX, f"keep rate at position {j}: {z:.2f} sd from {q}"
    for a, b in itertools.combinations(range(8), 2):
        z = _z(int((k[:, a] & k[:, b]).sum()), n, q * q)
        worst = max(worst, z)
        assert z <= Z_MAX, f"joint keep rate of positions {a}, {b}: {z:.2f} sd from {q * q}"
    for j in range(8):
        z = _z(int((k[:-1, j] & k[1:, j]).sum()), n - 1, q * q)
        worst = max(worst, z)
        assert z <= Z_MAX, f"joint keep rate of position {j} in neighbouring chunks: {z:.2f} sd from {q * q}"
    z = _z(int((_mask(p, seed) & keep(np.arange(N, dtype=np.uint64), p, seed + 1)).sum()), N, q * q)
    worst = max(worst, z)
    assert z <= Z_MAX, f"joint keep rate of seeds {seed}, {seed + 1}: {z:.2f} sd from {q * q}"
    print(f"p={p} seed={seed}: worst deviation {worst:.2f} sd")


def test_edges_of_the_threshold():
    i = np.arange(1 << 16, dtype=np.uint64)
    for seed in SEEDS:
        assert not keep(i, 1.0, seed).any(), "p = 1 drops everything"
        assert keep(i, 1e-6, seed).all(), "p = 1e-6 has threshold 0: everything is kept"
    assert threshold(1e-6) == 0 and threshold(1.0) == 65536 and threshold(0.5) == 32768 and threshold(0.25) == 16384
    assert threshold(0.1) == 6553 and threshold(0.3) == 19660  # fp32(p) * 65536, truncated


@pytest.mark.parametrize("seed", SEEDS)
def test_indices_past_32_bits_draw_other_masks(seed):
    """Element 2^32 + j is not element j (the index is not cut to 32 bits before the chunk number is taken), and element
    2^35 + j -- chunk 2^32 + (j >> 3), equal to chunk j >> 3 in its low word -- is not either: the hi32(c) term.  No GPU test
    can hold a tensor of that size."""
    j = np.arange(1 << 16, dtype=np.uint64)
    q, base = 0.5, keep(j, 0.5, seed)
    for shift in (32, 35, 36):
        far = keep(j + (np.uint64(1) << np.uint64(shift)), 0.5, seed)
        assert (far != base).any()
        z = _z(int((far & base).sum()), j.size, q * q)
        assert z <= Z_MAX, f"elements j and 2^{shift} + j: joint keep rate {z:.2f} sd from independent"


def test_epoch_is_a_seed_offset():
    i = np.arange(4096, dtype=np.uint64)
    for seed in SEEDS:
        assert np.array_equal(keep(i, 0.3, seed, epoch=0), keep(i, 0.3, seed))
        assert np.array_equal(keep(i, 0.3, seed, epoch=3), keep(i, 0.3, (seed + 3 * 0x9E3779B97F4A7C15) % (1 << 64)))
        assert (keep(i, 0.3, seed, epoch=3) != keep(i, 0.3, seed)).any()
