"""The attention dropout-mask rule itself (tests/_attn_mask_ref.py, written from `DropRng` in csrc/window_attn.h), on the host:
keep rates overall and per key column within 5 binomial standard deviations over 2^14 rows straddling row 2^24 (where the high
word of row * 256 becomes non-zero), the second row key of the keys whose bit 2 is set, p >= 1, seeds and the epoch rule.  Under the
null hypothesis one of the ~4000 rates checked exceeds 5 sd with probability 2e-3; the rule as written stays below 3.5.

The GPU tests (test_gpu_attn_valu.py) pin all four kernel families to this reference probability by probability."""
import numpy as np
import pytest

import _attn_mask_ref as AR
from _mask_ref import threshold

ROWS = 1 << 14
ROW0 = (1 << 24) - ROWS // 2  # half of the rows below 2^24, half at and above
SEED = (7 << 32) | 9
Z_MAX = 5.0


def _z(count, n, prob):
    return abs(count / n - prob) / np.sqrt(prob * (1.0 - prob) / n)


def _mask(Ws, p, seed=SEED, row0=ROW0):
    rows = np.arange(row0, row0 + ROWS, dtype=np.uint64)[:, None]
    return AR.keep(rows, np.arange(Ws, dtype=np.uint64)[None, :], p, seed)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
@pytest.mark.parametrize("Ws", [4, 8, 64, 256])
def test_keep_rates_overall_and_per_key(Ws, p):
    q = 1.0 - threshold(p) / 65536.0
    k = _mask(Ws, p)
    assert k.shape == (ROWS, Ws)
    z_all = _z(int(k.sum()), k.size, q)
    assert z_all <= Z_MAX, f"keep rate: {z_all:.2f} sd from {q}"
    z_key = [_z(int(k[:, j].sum()), ROWS, q) for j in range(Ws)]
    print(f"Ws={Ws} p={p}: overall {z_all:.2f} sd, worst key column {max(z_key):.2f} sd")
    assert max(z_key) <= Z_MAX, f"keep rate of key {int(np.argmax(z_key))}: {max(z_key):.2f} sd from {q}"
    for half in (k[: ROWS // 2], k[ROWS // 2:]):  # below and from row 2^24 on
        z = _z(int(half.sum()), half.size, q)
        assert z <= Z_MAX, f"keep rate on one side of row 2^24: {z:.2f} sd from {q}"


def test_keys_with_bit_2_use_the_second_row_key():
    """Keys k and k + 4 (bit 2 of k clear) share the pair multiplier and the half of the product; they differ in the row key only."""
    rows = np.arange(ROW0, ROW0 + 4096, dtype=np.uint64)
    k1, k2 = AR.row_keys(rows, SEED)
    assert np.array_equal(k2, AR.hash32(k1 ^ np.uint64(0x5BD1E995))) and (k1 != k2).all()
    for key in range(256):
        m = AR.pair_mult((key >> 1) & ~2)
        assert int(m) & 1 and np.array_equal(m, AR.pair_mult((key | 4) >> 1 & ~2))
        u = ((k2 if key & 4 else k1) * m) & AR.M32
        h = u ^ (u >> np.uint64(16))
        want = (h >> np.uint64(16)) if key & 1 else (h & np.uint64(0xFFFF))
        assert np.array_equal(AR.bits16(rows, key, SEED), want), key
    # the two keys of a row are not the same stream: keys k and k + 4 decide independently
    k = _mask(8, 0.5)
    z = _z(int((k[:, :4] & k[:, 4:]).sum()), k[:, :4].size, 0.25)
    assert z <= Z_MAX, f"joint keep rate of keys k and k + 4: {z:.2f} sd from independent"
    assert (k[:, :4] != k[:, 4:]).any()


def test_pair_multipliers_are_distinct_odd_constants():
    q = np.array(sorted({(key >> 1) & ~2 for key in range(256)}), dtype=np.uint64)
    m = AR.pair_mult(q)
    assert q.size == 64 and np.unique(m).size == 64 and (m & np.uint64(1)).all()
    assert int(AR.hash32(0)) == 0 and int(AR.hash32(1)) != 1  # (the finaliser fixes 0 and nothing nearby)


def test_p_of_one_drops_everything_and_tiny_p_keeps_everything():
    for Ws in (4, 256):
        assert not _mask(Ws, 1.0).any()
        assert not _mask(Ws, 1.5).any()
        assert _mask(Ws, 1e-6).all()  # threshold 0


def test_seeds_and_rows_give_other_masks():
    a = _mask(64, 0.5)
    for other in (SEED + 1, SEED + (1 << 32), 0):
        b = _mask(64, 0.5, seed=other)
        assert (a != b).any()
        z = _z(int((a & b).sum()), a.size, 0.25)
        assert z <= Z_MAX, f"seeds {SEED} and {other}: joint keep rate {z:.2f} sd from independent"
    # row 2^24 + r is not row r (the high word of row * 256 enters the key), and neighbouring rows are unrelated
    lo = _mask(64, 0.5, row0=0)
    hi = _mask(64, 0.5, row0=1 << 24)
    assert (lo != hi).any() and _z(int((lo & hi).sum()), lo.size, 0.25) <= Z_MAX
    assert _z(int((lo[:-1] & lo[1:]).sum()), lo[1:].size, 0.25) <= Z_MAX


def test_epoch_is_a_seed_offset():
    rows, keys = np.arange(ROW0, ROW0 + 512, dtype=np.uint64)[:, None], np.arange(64, dtype=np.uint64)[None, :]
    for seed in (0, 42, SEED):
        assert np.array_equal(AR.keep(rows, keys, 0.3, seed, epoch=0), AR.keep(rows, keys, 0.3, seed))
        assert np.array_equal(AR.keep(rows, keys, 0.3, seed, epoch=3), AR.keep(rows, keys, 0.3, (seed + 3 * 0x9E3779B97F4A7C15) % (1 << 64)))
        assert (AR.keep(rows, keys, 0.3, seed, epoch=3) != AR.keep(rows, keys, 0.3, seed)).any()
