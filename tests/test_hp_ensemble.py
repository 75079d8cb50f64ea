"""Rotation ensembles, the parts that need no GPU: `hs_hp_ensemble_add_seg_host` / `_add_depth_host` (the per-pixel functions the
kernels run, in a host loop) against an oracle written here in numpy, the exact symmetries, the unrotated member, coverage, guards,
the non-finite matrix, and every refusal.  The kernels are checked in test_gpu_hp_ensemble.py, which uses the cases, the oracle and
the comparisons of this file.  Helpers and the exemption cap are those of test_hp_rotate.py.

Oracle.  Host tables `evaluation.hp_nearest_pix_idcs` at the directions M^T g_p formed in numpy (`directions`), float64 softmax,
and the rules of the kernel: a neighbour counts when it is covered, valid and (depth) finite.

Tolerances.
  TOL_P 2e-5 absolute on a mean probability, for |logit| <= 16: the fp32 exp argument carries 16 * 2^-24 ~ 1e-6 relative, about 30
        roundings of 6e-8 follow in softmax, weighting and accumulation, times 4 for margin.  The worst error is printed; the
        float64 weights differ between kernel and oracle by about 1e-12 only (test_hp_rotate.py), and the value is continuous across
        bracket boundaries, so no bracket exemption is needed.
  TOL_L 1.2e-4 absolute on a mean logit (mode "logit"): the same 30 roundings of 6e-8 times 4 on values up to 16, no exp.
  TOL_D 1e-5 relative on a depth mean (positive depths: every term of both sums is positive, the relative error is that of
        about 20 fp32 roundings).
Exemptions, decided from the oracle alone, counted and capped at MAX_EXEMPT (0.1 %) of a case's pixels: the oracle's two largest
mean values differ by no more than GAP (1e-4 on probabilities; 5e-4 on mean logits, 4 TOL_L), or its summed weight lies within
BAND = 1e-6 of min_weight (the pixel may fall on either side).  The logits are drawn N(0, 4^2) clipped to +-16 (with N(0, 2^2) the
oracle alone has about 0.1 % of 1e-4 ties); the cases below keep the oracle under the cap by themselves, which every comparison
asserts, on the CPU first."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_hp_rotate import MAX_EXEMPT, SYMMETRIES, directions, generic_rotations, oracle_table, symmetry_permutation, unstable

TOL_P, TOL_L, TOL_D, BAND, MIN_W = 2e-5, 1.2e-4, 1e-5, 1e-6, 1e-3
GAP = {"prob": 1e-4, "logit": 5e-4}
TOL = {"prob": TOL_P, "logit": TOL_L}
BKGD = 200  # a class id no prediction holds

# nside, base_pix, batch, K, dtype, layout, valid, mode, members (three members: the first one unrotated)
# (4, 12) 192 pixels, under one workgroup; (8, 5) 320, one workgroup and a tail; (16, 8) / (16, 12) with / without uncovered base
# pixels; K over every KP = 4, 8, 12, 16 with ragged last vectors; "rows" = the padded [B, Npix, 16] rows viewed as [B, K, Npix]
SEG_CASES = [
    (4, 12, 2, 1, "f32", "dense", False, "prob", 2),
    (4, 12, 2, 10, "f32", "rows", True, "prob", 3),
    (8, 5, 3, 3, "f32", "rows", True, "prob", 3),
    (8, 5, 2, 16, "f32", "rows", False, "logit", 2),
    (8, 5, 2, 7, "bf16", "rows", True, "prob", 2),
    (16, 8, 2, 4, "bf16", "dense", True, "logit", 2),
    (16, 8, 3, 12, "f32", "dense", True, "prob", 2),
    (16, 12, 2, 10, "bf16", "rows", False, "prob", 3),
    (16, 12, 2, 12, "bf16", "dense", True, "logit", 3),
    (64, 8, 2, 16, "bf16", "rows", True, "prob", 3),
    (64, 8, 2, 10, "f32", "dense", False, "prob", 2),
]
# nside, base_pix, batch, dtype, valid, members
DEPTH_CASES = [(4, 12, 2, "f32", False, 2), (8, 5, 3, "f32", True, 3), (16, 8, 2, "bf16", True, 2), (16, 12, 2, "bf16", False, 3),
               (64, 8, 2, "f32", True, 2)]


@pytest.fixture(scope="module")
def E():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import hp_ensemble
    return hp_ensemble


def case_id(case):
    return "-".join(str(c) for c in case)


def bf16_bits(x):
    """float32 -> bfloat16 bits (uint16), round to nearest even"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def laid_out(values, dtype, layout, seed):
    """values float32 [B, K, n] exactly representable in `dtype` -> the numpy array the host entry reads (float32, or uint16 bits),
    dense or as the padded rows [B, n, 16] viewed as [B, K, n]; the padding holds NaNs and large numbers"""
    arr = values if dtype == "f32" else bf16_bits(values)
    if layout == "dense":
        return np.ascontiguousarray(arr)
    b, k, n = values.shape
    pad = np.random.default_rng(seed).choice(np.array([np.nan, 1e30, -7.0], dtype=np.float32), (b, n, 16))
    rows = pad if dtype == "f32" else bf16_bits(pad)
    rows[:, :, :k] = arr.transpose(0, 2, 1)
    return rows.transpose(0, 2, 1)[:, :k]


def draw_members(seed, nside, base_pix, batch, n_members, with_valid):
    """[(A or None, rot = A^T or None, valid or None)]: A as random_rotations draws it (no pole rotation: M = A)"""
    npix, rng, out = base_pix * nside * nside, np.random.default_rng(seed), []
    for m in range(n_members):
        if m == 0 and n_members == 3:
            a = rot = None
        else:
            a = generic_rotations(seed + 10 * m, batch)
            rot = np.ascontiguousarray(a.transpose(0, 2, 1))
        valid = (rng.random((batch, npix)) < 0.9).astype(np.uint8) if with_valid else None
        out.append((a, rot, valid))
    return out


def member_tables(nside, base_pix, batch, rot):
    """(pix [B, 4, n], wgt [B, 4, n], theta, phi) of the oracle at rot_b g_p; the unrotated member: the pixel itself, weight 1"""
    npix = base_pix * nside * nside
    if rot is None:
        pix = np.full((batch, 4, npix), -1, dtype=np.int64)
        pix[:, 0] = np.arange(npix)
        wgt = np.zeros((batch, 4, npix))
        wgt[:, 0] = 1.0
        return pix, wgt, None, None
    theta, phi = directions(nside, base_pix, rot)
    pix, wgt, _ = oracle_table(nside, theta, phi)
    return pix, wgt, theta, phi


def taken(pix, npix, valid):
    ok = (pix >= 0) & (pix < npix)
    safe = np.where(ok, pix, 0)
    if valid is not None:
        ok &= np.take_along_axis(valid[:, None, :], safe, 2) != 0
    return ok, safe


def softmax64(z, axis):
    e = np.exp(z - z.max(axis, keepdims=True))
    return e / e.sum(axis, keepdims=True)


def oracle_seg(nside, base_pix, values, members, mode):
    """values: per member float32 [B, K, n].  Returns (acc float64 [B, K, n], wsum [B, n], unstable [B, n])"""
    b, k, npix = values[0].shape
    acc, wsum, shaky = np.zeros((b, k, npix)), np.zeros((b, npix)), np.zeros((b, npix), dtype=bool)
    for v, (_, rot, valid) in zip(values, members):
        pix, wgt, theta, phi = member_tables(nside, base_pix, b, rot)
        ok, safe = taken(pix, npix, valid)
        val = v.astype(np.float64)
        val = softmax64(val, 1) if mode == "prob" else val
        w = wgt * ok
        for j in range(4):
            acc += w[:, j, None, :] * np.take_along_axis(val, safe[:, j, None, :], 2)
        wsum += w.sum(1)
        if rot is not None:
            shaky |= unstable(nside, theta, phi, pix)
    return acc, wsum, shaky


def oracle_depth(nside, base_pix, values, members):
    b, npix = values[0].shape
    acc, wsum = np.zeros((b, npix)), np.zeros((b, npix))
    for v, (_, rot, valid) in zip(values, members):
        pix, wgt, _, _ = member_tables(nside, base_pix, b, rot)
        ok, safe = taken(pix, npix, valid)
        d = np.take_along_axis(v.astype(np.float64)[:, None, :], safe, 2)
        ok &= np.isfinite(d)
        w = wgt * ok
        acc += (w * np.where(ok, d, 0.0)).sum(1)
        wsum += w.sum(1)
    return acc, wsum


@functools.lru_cache(maxsize=None)
def seg_case(case):
    """the inputs and the oracle of one case, shared by the CPU and GPU tests and left unchanged"""
    nside, base_pix, batch, k, dtype, layout, with_valid, mode, n_members = case
    seed = 1000 + 7 * nside + 13 * base_pix + 31 * k + n_members
    npix, rng = base_pix * nside * nside, np.random.default_rng(seed)
    members = draw_members(seed, nside, base_pix, batch, n_members, with_valid)
    values = []
    for _ in members:
        v = np.clip(rng.normal(0.0, 4.0, (batch, k, npix)), -16, 16).astype(np.float32)
        values.append(v if dtype == "f32" else bf16_value(bf16_bits(v)))
    acc, wsum, shaky = oracle_seg(nside, base_pix, values, members, mode)
    live = wsum > MIN_W
    mean = np.where(live[:, None], acc / np.where(live, wsum, 1.0)[:, None], 0.0)
    top = np.sort(mean, 1)
    tie = (top[:, -1] - top[:, -2] <= GAP[mode]) if k > 1 else np.zeros_like(live)
    band = np.abs(wsum - MIN_W) <= BAND
    preds = np.where(live, mean.argmax(1), BKGD).astype(np.uint8)
    return dict(members=members, values=values, mean=mean, wsum=wsum, live=live, preds=preds, exempt=(tie & live) | band, band=band,
                shaky=shaky, seed=seed)


@functools.lru_cache(maxsize=None)
def depth_case(case):
    nside, base_pix, batch, dtype, with_valid, n_members = case
    seed = 2000 + 7 * nside + 13 * base_pix + n_members
    npix, rng = base_pix * nside * nside, np.random.default_rng(seed)
    members = draw_members(seed, nside, base_pix, batch, n_members, with_valid)
    values = []
    for _ in members:
        v = rng.uniform(0.2, 400.0, (batch, npix)).astype(np.float32)
        v[rng.random(v.shape) < 0.05] = np.inf
        v[rng.random(v.shape) < 0.03] = -np.inf
        v[rng.random(v.shape) < 0.05] = np.nan
        values.append(v if dtype == "f32" else bf16_value(bf16_bits(v)))
    acc, wsum = oracle_depth(nside, base_pix, values, members)
    live = wsum > MIN_W
    return dict(members=members, values=values, mean=np.where(live, acc / np.where(live, wsum, 1.0), np.nan), wsum=wsum, live=live,
                band=np.abs(wsum - MIN_W) <= BAND, seed=seed)


def compare_seg(case, probs, preds, what):
    """probs [B, K, n] (0 where dead) and preds uint8 [B, n] of the code under test against the oracle of `case`"""
    c, mode = seg_case(case), case[7]
    keep = ~c["band"]
    err = np.abs(probs - c["mean"]).max(1)
    worst = err[keep].max()
    wrong = (preds != c["preds"]) & ~c["exempt"]
    print(f"{what} {case_id(case)}: worst |mean - oracle| {worst:.3e} (tolerance {TOL[mode]:.1e}), {c['exempt'].sum()} of {c['exempt'].size} "
          f"pixels exempt, {wrong.sum()} wrong class ids, {(~c['live']).mean():.3f} without weight")
    assert c["exempt"].mean() <= MAX_EXEMPT
    assert worst <= TOL[mode]
    assert not wrong.any()
    return worst


def compare_depth(case, out, what):
    c = depth_case(case)
    keep = ~c["band"]
    assert np.array_equal(np.isnan(out)[keep], ~c["live"][keep])
    sel = keep & c["live"]
    rel = (np.abs(out[sel] - c["mean"][sel]) / np.abs(c["mean"][sel])).max()
    print(f"{what} {case_id(case)}: worst relative error {rel:.3e}, {c['band'].sum()} pixels exempt, {(~c['live']).mean():.3f} without weight")
    assert c["band"].mean() <= MAX_EXEMPT
    assert rel <= TOL_D
    assert np.isfinite(out[sel]).all()


def finish_seg_numpy(acc, wsum, k, background=BKGD):
    """what hs_hp_ensemble_finish_seg computes, for the host accumulators"""
    live = wsum > np.float32(MIN_W)
    probs = np.where(live[:, None], (acc[:, :, :k] / np.where(live, wsum, 1)[:, :, None]).transpose(0, 2, 1), 0).astype(np.float32)
    return probs, np.where(live, acc[:, :, :k].argmax(2), background).astype(np.uint8)


def run_seg_host(E, case):
    nside, base_pix, _, _, dtype, layout, _, mode, _ = case
    c = seg_case(case)
    acc = wsum = None
    for i, (v, (_, rot, valid)) in enumerate(zip(c["values"], c["members"])):
        acc, wsum = E.add_seg_host(nside, base_pix, laid_out(v, dtype, layout, c["seed"] + i), rot, valid, mode, acc, wsum,
                                   rows16=layout == "rows")
    return acc, wsum


# ------------------------------------------------------------------ 1. the host entries against the oracle
@pytest.mark.parametrize("case", SEG_CASES, ids=case_id)
def test_seg_host_entry_matches_the_oracle(E, case):
    k = case[3]
    acc, wsum = run_seg_host(E, case)
    assert acc.dtype == wsum.dtype == np.float32 and acc.shape == wsum.shape + (-(-k // 4) * 4,)
    assert (acc[:, :, k:] == 0).all()  # the padding classes of a row
    compare_seg(case, *finish_seg_numpy(acc, wsum, k), "host")
    assert np.abs(wsum - seg_case(case)["wsum"]).max() <= 1e-6  # up to three members of weight <= 1 in fp32


def test_both_layouts_give_the_same_bits(E):
    """dense through the strided loads, the padded rows through the 16-byte loads, and those rows through the strided loads"""
    for case in (SEG_CASES[2], SEG_CASES[4], SEG_CASES[9]):
        nside, base_pix, _, _, dtype, _, _, mode, _ = case
        c = seg_case(case)
        v, (_, rot, valid) = c["values"][1], c["members"][1]
        ref = E.add_seg_host(nside, base_pix, laid_out(v, dtype, "dense", 1), rot, valid, mode)
        rows = laid_out(v, dtype, "rows", 1)
        for got in (E.add_seg_host(nside, base_pix, rows, rot, valid, mode, rows16=True), E.add_seg_host(nside, base_pix, rows, rot, valid, mode)):
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.mark.parametrize("case", DEPTH_CASES, ids=case_id)
def test_depth_host_entry_matches_the_oracle(E, case):
    nside, base_pix, _, dtype, _, _ = case
    c = depth_case(case)
    assert all(np.isnan(v).any() and np.isinf(v).any() for v in c["values"])
    acc = wsum = None
    for v, (_, rot, valid) in zip(c["values"], c["members"]):
        acc, wsum = E.add_depth_host(nside, base_pix, v if dtype == "f32" else bf16_bits(v), rot, valid, acc, wsum)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(wsum > np.float32(MIN_W), acc / wsum, np.nan)
    compare_depth(case, out, "host")


# ------------------------------------------------------------------ 2. exact symmetries
def one_hot_logits(labels, k):
    """float32 [B, k, n]: 12 on the pixel's class, 0 elsewhere"""
    return (12.0 * (labels[:, None, :] == np.arange(k)[None, :, None])).astype(np.float32)


@pytest.mark.parametrize("nside", [4, 16])
@pytest.mark.parametrize("mode", ["prob", "logit"])
def test_symmetries_bring_one_hot_predictions_back_exactly(E, nside, mode):
    names, k, npix = list(SYMMETRIES), 10, 12 * nside * nside
    labels = np.random.default_rng(nside).integers(0, k, (len(names), npix))
    mats = np.stack([SYMMETRIES[n] for n in names])
    rotated = np.stack([labels[b][symmetry_permutation(nside, 12, mats[b])] for b in range(len(names))])  # what hs_hp_rotate shows
    assert not np.array_equal(rotated[1:], labels[1:])
    acc, wsum = E.add_seg_host(nside, 12, one_hot_logits(rotated, k), np.ascontiguousarray(mats.transpose(0, 2, 1)), mode=mode)
    assert np.abs(wsum - 1.0).max() <= 1e-6
    assert np.array_equal(acc[:, :, :k].argmax(2), labels)


# ------------------------------------------------------------------ 3. the unrotated member alone
@pytest.mark.parametrize("k", [1, 3, 7, 10, 16])
def test_identity_only_is_the_plain_argmax_and_softmax(E, k):
    nside, base_pix, batch = 8, 5, 2
    v = np.random.default_rng(k).normal(0, 2, (batch, k, base_pix * 64)).astype(np.float32)
    acc, wsum = E.add_seg_host(nside, base_pix, v)
    assert (wsum == 1.0).all()
    probs, preds = finish_seg_numpy(acc, wsum, k)
    want = torch.from_numpy(v)
    assert np.array_equal(preds, torch.max(want, 1)[1].numpy())
    err = np.abs(probs - torch.softmax(want.double(), 1).numpy()).max()
    print(f"K {k}: worst |prob - softmax| {err:.3e}")
    assert err <= TOL_P
    acc_l, _ = E.add_seg_host(nside, base_pix, v, mode="logit")
    assert np.array_equal(acc_l[:, :, :k].transpose(0, 2, 1), v)  # weight 1: the logits themselves


# ------------------------------------------------------------------ 4. coverage, guards, non-finite matrices
def test_untaken_neighbours_carry_no_weight_and_guards_stay(E):
    case = SEG_CASES[6]  # nside 16, 8 base pixels, valid planes, two rotated members
    nside, base_pix, batch, k, _, _, _, mode, _ = case
    c, npix, kp = seg_case(case), 8 * 256, 12
    big_acc, big_wsum = np.full(batch * npix * kp + 8, -7.0, dtype=np.float32), np.full(batch * npix + 8, -7.0, dtype=np.float32)
    acc, wsum = big_acc[:-8].reshape(batch, npix, kp), big_wsum[:-8].reshape(batch, npix)
    for i, (v, (_, rot, valid)) in enumerate(zip(c["values"], c["members"])):
        E.add_seg_host(nside, base_pix, v, rot, valid, mode, acc, wsum, accumulate=i > 0)
    assert (big_acc[-8:] == -7.0).all() and (big_wsum[-8:] == -7.0).all()
    # the weight of a pixel is the oracle's sum over the neighbours it takes; where it takes none (and the brackets are not a
    # rounding matter) the weight is exactly 0 and the finish writes the background class
    assert np.abs(wsum - c["wsum"]).max() <= 1e-6
    none = (c["wsum"] == 0) & ~c["shaky"]
    assert none.any() and (wsum[none] == 0).all() and (acc[none] == 0).all()
    assert (finish_seg_numpy(acc, wsum, k)[1][none] == BKGD).all()
    # without the valid planes more weight arrives, and uncovered base pixels still take theirs away
    acc2 = wsum2 = None
    for v, (_, rot, _) in zip(c["values"], c["members"]):
        acc2, wsum2 = E.add_seg_host(nside, base_pix, v, rot, None, mode, acc2, wsum2)
    assert (wsum2 >= wsum - 1e-6).all() and (wsum2 > wsum + 0.01).any() and (wsum2 < 1.9).any() and wsum2.max() <= 2 + 1e-6


def test_a_non_finite_matrix_leaves_its_sample_alone(E):
    case = SEG_CASES[6]
    nside, base_pix, _, k, _, _, _, mode, _ = case
    c = seg_case(case)
    (v0, v1), ((_, rot0, valid0), (_, rot1, valid1)) = c["values"], c["members"]
    first = E.add_seg_host(nside, base_pix, v0, rot0, valid0, mode)
    bad = rot1.copy()
    bad[1, 0, 2] = np.nan
    acc, wsum = first[0].copy(), first[1].copy()
    E.add_seg_host(nside, base_pix, v1, bad, valid1, mode, acc, wsum)
    good = E.add_seg_host(nside, base_pix, v1, rot1, valid1, mode, first[0].copy(), first[1].copy())
    assert np.array_equal(acc[1], first[0][1]) and np.array_equal(wsum[1], first[1][1])  # unchanged, bit for bit
    for b in (0, 2):
        assert np.array_equal(acc[b], good[0][b]) and np.array_equal(wsum[b], good[1][b])
    bad[1, 0, 2] = np.inf
    acc, wsum = E.add_seg_host(nside, base_pix, v1, bad, valid1, mode)  # as a first member: zeros are stored
    assert (acc[1] == 0).all() and (wsum[1] == 0).all() and (wsum[0] > 0).any()
    d = np.full((3, 8 * 256), 5.0, dtype=np.float32)
    dacc, dwsum = E.add_depth_host(nside, base_pix, d, bad)
    assert (dacc[1] == 0).all() and (dwsum[1] == 0).all() and np.allclose(dacc[0][dwsum[0] > 0.5] / dwsum[0][dwsum[0] > 0.5], 5.0, rtol=1e-6)


# ------------------------------------------------------------------ 5. refusals
def test_the_entry_points_refuse_before_launch(E):
    """Every refusal is decided on the host (status 1 = HS_ERR_INVALID_ARG, 5 = HS_ERR_MISALIGNED): the pointers name host memory
    no kernel could read, so a launch would fault."""
    from heal_swin_amd._lib import lib

    buf = ctypes.create_string_buffer(1 << 20)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    at = lambda off: ctypes.c_void_p(base + off)  # noqa: E731
    # nside 4, 8 base pixels, batch 2, 10 classes: fp32 pred 10240 B, acc (KP 12) 12288 B, wsum 1024 B
    pred, acc, wsum, valid, rot, out = at(0), at(16384), at(32768), at(40960), at(49152), at(65536)

    def seg(fn, nside=4, npix=128, rot=rot, batch=2, pred=pred, kind=0, k=10, sb=1280, sk=128, sp=1, valid=valid, mode=0, accumulate=0, acc=acc,
            wsum=wsum):
        args = (nside, npix, rot, batch, pred, kind, k, sb, sk, sp, valid, mode, accumulate, acc, wsum)
        return fn(*args, None) if fn is lib.hs_hp_ensemble_add_seg else fn(*args)

    def depth(fn, nside=4, npix=128, rot=rot, batch=2, pred=pred, kind=0, sb=128, sp=1, valid=valid, accumulate=0, acc=acc, wsum=wsum):
        args = (nside, npix, rot, batch, pred, kind, sb, sp, valid, accumulate, acc, wsum)
        return fn(*args, None) if fn is lib.hs_hp_ensemble_add_depth else fn(*args)

    shared = [dict(nside=3), dict(nside=0), dict(nside=-4), dict(nside=16384), dict(npix=0), dict(npix=-16), dict(npix=13 * 16), dict(npix=100),
              dict(batch=0), dict(batch=-1), dict(batch=65536), dict(kind=2), dict(kind=3), dict(kind=8), dict(kind=-1), dict(sb=-1), dict(sp=-1),
              dict(pred=None), dict(acc=None), dict(wsum=None), dict(acc=pred), dict(wsum=pred), dict(wsum=acc)]
    # the last 16 bytes / the last byte of the predictions, the last 4 bytes of acc; a strided pred reaching into acc
    seg_only = [dict(acc=at(10240 - 16)), dict(wsum=at(10239)), dict(wsum=at(16384 + 12284)), dict(sp=2, sk=256, sb=8192),
                dict(k=0), dict(k=17), dict(k=-1), dict(sk=-1), dict(mode=2), dict(mode=-1), dict(kind=4, sk=128), dict(kind=4, sk=1, sp=8),
                dict(kind=4, sk=1, sp=10), dict(kind=4, sk=1, sp=12, sb=1538), dict(kind=4, sk=1, sp=12, sb=1536, pred=at(4)),
                dict(kind=5, sk=1, sp=12, sb=1536), dict(kind=5, sk=1, sp=16, sb=2048, pred=at(8))]
    depth_only = [dict(acc=at(1024 - 16)), dict(wsum=at(1023)), dict(wsum=at(16384 + 1020)), dict(sp=64), dict(kind=4), dict(kind=5)]
    for fn in (lib.hs_hp_ensemble_add_seg, lib.hs_hp_ensemble_add_seg_host):
        for kw in shared + seg_only:
            assert seg(fn, **kw) == 1, (fn.__name__, kw)
            assert lib.hs_last_error()
        assert seg(fn, acc=at(16384 + 4)) == 5  # HS_ERR_MISALIGNED: acc rows are read and written as 16-byte vectors
    for fn in (lib.hs_hp_ensemble_add_depth, lib.hs_hp_ensemble_add_depth_host):
        for kw in shared + depth_only:
            assert depth(fn, **kw) == 1, (fn.__name__, kw)
            assert lib.hs_last_error()
    # the host entries accept what the device entries would launch (rows of 12 floats inside sp = 12; 16 bf16 inside sp = 16)
    assert seg(lib.hs_hp_ensemble_add_seg_host, kind=4, sk=1, sp=12, sb=1536) == 0
    assert seg(lib.hs_hp_ensemble_add_seg_host, rot=None, valid=None) == 0 and depth(lib.hs_hp_ensemble_add_depth_host, rot=None, valid=None) == 0

    def fin_seg(npix=128, batch=2, k=10, acc=acc, wsum=wsum, min_weight=1e-3, background=0, preds=out, probs=pred, sb=1280, sk=128, sp=1):
        return lib.hs_hp_ensemble_finish_seg(npix, batch, k, acc, wsum, min_weight, background, preds, probs, sb, sk, sp, None)

    def fin_depth(npix=128, batch=2, acc=acc, wsum=wsum, min_weight=1e-3, out=out):
        return lib.hs_hp_ensemble_finish_depth(npix, batch, acc, wsum, min_weight, out, None)

    for kw in (dict(npix=0), dict(npix=-1), dict(npix=1 << 31), dict(batch=0), dict(batch=65536), dict(k=0), dict(k=17), dict(acc=None),
               dict(wsum=None), dict(preds=None), dict(min_weight=-1.0), dict(min_weight=float("nan")), dict(background=-1),
               dict(background=256), dict(sb=-1), dict(sk=-1), dict(sp=-1)):
        assert fin_seg(**kw) == 1, kw
    assert fin_seg(acc=at(16384 + 8)) == 5
    for kw in (dict(npix=0), dict(npix=1 << 31), dict(batch=0), dict(batch=65536), dict(acc=None), dict(wsum=None), dict(out=None),
               dict(min_weight=-1.0), dict(min_weight=float("nan"))):
        assert fin_depth(**kw) == 1, kw


def test_python_argument_checks(E):
    """Everything is checked before anything touches the device, so the refusals need none."""
    for kw in (dict(nside=3), dict(nside=32768), dict(base_pix=0), dict(base_pix=13), dict(s2_bkgd_class=256), dict(s2_bkgd_class=-1),
               dict(rotate_pole=True), dict(mode="mean"), dict(min_weight=-1.0), dict(min_weight=float("nan")), dict(min_weight=float("inf"))):
        with pytest.raises(ValueError):
            E.HPRotationEnsemble(**dict(dict(nside=4, device="cpu"), **kw))
    ens = E.HPRotationEnsemble(4, 8)  # names the device without touching it
    assert ens.npix == 128 and ens.mode == "prob" and ens.min_weight == 1e-3
    a = generic_rotations(3, 2)
    logits, depth, valid = torch.zeros(2, 10, 128), torch.zeros(2, 128), torch.ones(2, 128, dtype=torch.uint8)
    for bad, err in ((logits.double(), TypeError), (logits.to(torch.uint8), TypeError), (logits.numpy(), TypeError), (logits[:, :, :100], ValueError),
                     (logits[0, 0], ValueError), (logits[None], ValueError), (torch.zeros(2, 17, 128), ValueError), (torch.zeros(2, 0, 128), ValueError),
                     (torch.zeros(0, 10, 128), ValueError)):
        with pytest.raises(err):
            ens.add(bad)
    for kw in (dict(rotations=np.eye(3)), dict(rotations=np.zeros((2, 9))), dict(rotations=generic_rotations(3, 3)), dict(rotations=2.0 * a),
               dict(rotations=a + 1e-6), dict(rotations=np.full((2, 3, 3), np.nan)), dict(rotations=torch.from_numpy(a) * 1.001),
               dict(valid=valid[:1]), dict(valid=valid.float()), dict(valid=valid.numpy()), dict(valid=valid[:, :100]), dict(channel=0)):
        with pytest.raises(ValueError):
            ens.add(depth, **kw)
    for kw in (dict(channel=2), dict(channel=-1)):
        with pytest.raises(ValueError):
            ens.add(torch.zeros(2, 2, 128), **kw)
    with pytest.raises(RuntimeError, match="at least one add"):
        ens.finish()
    for pred, kw in ((logits, {}), (depth, {}), (logits, dict(channel=1)), (logits.bfloat16(), dict(rotations=a, valid=valid))):
        with pytest.raises(RuntimeError, match="GPU tensor"):  # well-formed calls still need the device: there is no CPU path
            ens.add(pred, **kw)
    assert ens._members == 0 and ens._acc is None  # nothing was recorded by a refused call
    # a tilted pole keeps an orthogonal A orthogonal; the refusal looks at M = R^T A R
    from tests.test_projection import calibrations
    pole = E.HPRotationEnsemble(4, 8, cal_info=calibrations()["mvl_96x128"], rotate_pole=True, device="cpu")
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pole.add(depth, rotations=a)
    with pytest.raises(ValueError, match="orthogonal"):
        pole.add(depth, rotations=1.01 * a)
    # the host wrappers
    with pytest.raises(ValueError):
        E.add_seg_host(4, 8, np.zeros((2, 10, 100), dtype=np.float32))
    with pytest.raises(ValueError):
        E.add_seg_host(4, 8, np.zeros((2, 10, 128)))
    with pytest.raises(ValueError):
        E.add_depth_host(4, 8, np.zeros((2, 128), dtype=np.float32), rot=generic_rotations(3, 3))
    with pytest.raises(AssertionError, match="n_classes"):
        E.add_seg_host(4, 8, np.zeros((2, 17, 128), dtype=np.float32))
