"""Rotation of HEALPix-resident maps on the GPU: `hs_hp_rotated_interp` against the host entry point (the same inline function
in a host loop), `hs_hp_rotate` against the host tables (`evaluation.get_interp_weights` at directions formed in numpy, code the
kernel shares nothing with), exact symmetries, the uncovered base pixels, a non-finite matrix, and `HPRotator` under graph
capture.  Helpers, tolerances and the exemption rule are those of test_hp_rotate.py.

Exemptions are decided from the oracle alone and counted against a cap of 0.1 % of the case's pixels:
  tables           the oracle's four pixels change when the direction moves by 1e-9 rad (a bracket boundary within rounding);
  labels, depth    the oracle's two largest weights differ by less than 1e-9 (the nearest pixel is a rounding matter);
  frame            |out - rint(value)| <= 1 everywhere, equal wherever the oracle value is farther than 1e-6 from a half-integer
                   (the values agree to about 1e-11, test_hp_rotate.py)."""
import functools

import numpy as np
import pytest
import torch

from tests.test_hp_rotate import (MAX_EXEMPT, SYMMETRIES, TOL_V, TOL_W, compare_tables, directions, generic_rotations, interp_value,
                                  oracle_table, symmetry_permutation)
from tests.test_projection import calibrations

pytestmark = pytest.mark.gpu
BKGD, FILL = 200, -3.5  # values the random planes do not hold


@pytest.fixture(scope="module")
def R():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import hp_rotate
    return hp_rotate


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def planes(seed, batch, npix, channels=3):
    """random bytes, class ids 0 .. 9, depths with inf, NaN and the 1000 m background among them"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (batch, channels, npix), dtype=np.uint8)
    lab = rng.integers(0, 10, (batch, npix), dtype=np.uint8)
    dep = rng.uniform(0.2, 400, (batch, npix)).astype(np.float32)
    dep[rng.random(dep.shape) < 0.1] = 1000.0
    dep[rng.random(dep.shape) < 0.05] = np.inf
    dep[rng.random(dep.shape) < 0.05] = np.nan
    return img, lab, dep


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_against_oracle(out, src, table, npix, what):
    """out, src: (img [B, C, n], labels [B, n], depth [B, n]) as numpy, the outputs restricted to the n pixels of `table` =
    (pix [B, 4, n], wgt [B, 4, n], nearest [B, n]) of the host tables; the sources whole.  Returns the share of pixels with an
    uncovered neighbour."""
    (o_img, o_lab, o_dep), (img, lab, dep), (pix, wgt, nearest) = out, src, table
    top = np.sort(wgt, 1)
    tie = top[:, 3] - top[:, 2] < 1e-9
    cov = (nearest >= 0) & (nearest < npix)
    safe = np.where(cov, nearest, 0)
    want_lab = np.where(cov, np.take_along_axis(lab, safe, 1), BKGD)
    want_dep = np.where(cov, np.take_along_axis(bits(dep), safe, 1), bits(np.float32(FILL)))
    assert np.array_equal(o_lab[~tie], want_lab[~tie])
    assert np.array_equal(bits(o_dep)[~tie], want_dep[~tie])
    near_half, worst = np.zeros(tie.shape, dtype=bool), 0.0
    for b in range(img.shape[0]):
        for c in range(img.shape[1]):
            val = interp_value(pix[b:b + 1], wgt[b:b + 1], img[b, c], npix)[0]
            half = np.abs(val - np.floor(val) - 0.5) <= TOL_V
            want = np.clip(np.rint(val), 0, 255)
            diff = np.abs(o_img[b, c].astype(np.float64) - want)
            worst = max(worst, diff.max())
            assert (diff[~half] == 0).all(), (b, c)
            near_half[b] |= half
    uncovered = ((pix < 0) | (pix >= npix)).any(1)
    print(f"{what}: {tie.sum()} ties and {near_half.sum()} half-integer values of {tie.size} pixels, max frame difference {worst:.0f}, "
          f"{uncovered.mean():.3f} of the pixels touch an uncovered neighbour, {1 - cov.mean():.3f} are filled")
    assert worst <= 1
    assert tie.mean() <= MAX_EXEMPT and near_half.mean() <= MAX_EXEMPT
    return uncovered.mean()


# ------------------------------------------------------------------ 1. hs_hp_rotated_interp against the host entry point
@pytest.mark.parametrize("nside,base_pix,batch", [(4, 12, 6), (16, 8, 6), (16, 12, 6), (64, 8, 2)])
def test_device_tables_match_the_host_entry(R, nside, base_pix, batch):
    mats = generic_rotations(77 + nside + base_pix, batch)
    count = base_pix * nside * nside
    got = R.rotated_interp(nside, mats, count=count)
    assert [t.dtype for t in got] == [torch.int32, torch.float64, torch.int32] and all(t.is_cuda for t in got)
    assert got[0].shape == got[1].shape == (batch, 4, count) and got[2].shape == (batch, count)
    host = R.rotated_interp_host(nside, mats, count=count)
    theta, phi = directions(nside, base_pix, mats)
    compare_tables(nside, [t.cpu().numpy() for t in got], host, theta, phi, f"nside {nside}, {base_pix} base pixels")
    again = R.rotated_interp(nside, dev(mats), count=count)  # a device tensor
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_sub_range_equals_the_slice_of_the_full_call(R):
    from heal_swin_amd._lib import lib, ptr, stream_ptr

    nside, first, count, batch = 16, 777, 1000, 3
    mats = generic_rotations(9, batch)
    full = [t.cpu().numpy() for t in R.rotated_interp(nside, mats)]
    sub = [t.cpu().numpy() for t in R.rotated_interp(nside, mats, first_pix=first, count=count)]
    for f, s in zip(full, sub):
        assert np.array_equal(f[..., first:first + count], s)
    # nothing is written past [batch, 4, count] / [batch, count]: 8 guard elements at the end of each buffer
    rot = dev(mats)
    pix = torch.full((batch * 4 * count + 8,), -7, dtype=torch.int32, device="cuda")
    wgt = torch.full((batch * 4 * count + 8,), -7.0, dtype=torch.float64, device="cuda")
    near = torch.full((batch * count + 8,), -7, dtype=torch.int32, device="cuda")
    assert lib.hs_hp_rotated_interp(nside, first, count, ptr(rot), batch, ptr(pix), ptr(wgt), ptr(near), stream_ptr(rot.device)) == 0
    for buf, s in zip((pix, wgt, near), sub):
        flat = buf.cpu().numpy()
        assert np.array_equal(flat[:-8].reshape(s.shape), s) and (flat[-8:] == -7).all()


# ------------------------------------------------------------------ 2. exact symmetries
@pytest.mark.parametrize("base_pix", [8, 12])
def test_symmetries_permute_every_plane_exactly(R, base_pix):
    nside = 16
    npix = base_pix * nside * nside
    names = list(SYMMETRIES)
    img, lab, dep = planes(21 + base_pix, len(names), npix)
    assert np.isnan(dep).any() and np.isinf(dep).any()
    rot = R.HPRotator(nside, base_pix, s2_bkgd_class=BKGD, depth_fill=FILL)
    o_img, o_lab, o_dep = (t.cpu().numpy() for t in rot(dev(img), dev(lab), dev(dep), rotations=np.stack([SYMMETRIES[n] for n in names])))
    for b, name in enumerate(names):
        q = symmetry_permutation(nside, base_pix, SYMMETRIES[name])  # derived from the host tables, a bijection of [0, npix)
        assert np.array_equal(o_lab[b], lab[b][q]), name
        assert np.array_equal(bits(o_dep[b]), bits(dep[b])[q]), name
        assert np.array_equal(o_img[b], img[b][:, q]), name
    assert (o_lab != BKGD).all() and (bits(o_dep) != bits(np.float32(FILL))).all()  # nothing is filled


# ------------------------------------------------------------------ 3. generic rotations
@functools.lru_cache(maxsize=None)
def generic_run(base_pix):
    """nside 16, six matrices, three channels: (sources, outputs, oracle table, device tables), shared and left unchanged"""
    from heal_swin_amd import hp_rotate as R

    nside, npix = 16, base_pix * 256
    mats = generic_rotations(40 + base_pix)
    src = planes(50 + base_pix, 6, npix)
    rot = R.HPRotator(nside, base_pix, s2_bkgd_class=BKGD, depth_fill=FILL)
    out = tuple(t.cpu().numpy() for t in rot(*map(dev, src), rotations=mats))
    theta, phi = directions(nside, base_pix, mats)
    own = tuple(t.cpu().numpy() for t in R.rotated_interp(nside, mats, count=npix))
    return src, out, oracle_table(nside, theta, phi), own, mats


@pytest.mark.parametrize("base_pix", [8, 12])
def test_generic_rotations_match_the_host_tables(R, base_pix):
    src, out, table, _, _ = generic_run(base_pix)
    npix = base_pix * 256
    assert [o.dtype for o in out] == [np.uint8, np.uint8, np.float32] and [o.shape for o in out] == [(6, 3, npix), (6, npix), (6, npix)]
    touched = check_against_oracle(out, src, table, npix, f"{base_pix} base pixels")
    o_img, o_lab, o_dep = out
    if base_pix == 8:  # the uncovered base pixels: 0.0 in the sum (checked above), the background class, the depth fill
        assert 0.03 <= touched <= 0.25
        filled = (table[2] >= npix)
        assert filled.any() and (o_lab[filled] == BKGD).all() and (bits(o_dep)[filled] == bits(np.float32(FILL))).all()
        all_out = (table[0] >= npix).all(1)
        assert all_out.any() and (o_img.transpose(0, 2, 1)[all_out] == 0).all()
    else:
        assert touched == 0 and (o_lab != BKGD).all()
    assert len({o_img[b].tobytes() for b in range(6)}) == 6  # every sample under its own matrix


def test_a_constant_frame_stays_constant_where_covered(R):
    _, _, _, (pix, _, _), mats = generic_run(8)
    npix = 8 * 256
    img = np.full((6, 2, npix), 117, dtype=np.uint8)
    out = R.HPRotator(16, 8)(dev(img), rotations=mats).cpu().numpy()
    inside = ((pix >= 0) & (pix < npix)).all(1)  # the kernel's own four pixels
    assert 0.7 < inside.mean() < 1.0
    assert (out.transpose(0, 2, 1)[inside] == 117).all()
    assert (out <= 117).all() and (out.transpose(0, 2, 1)[~inside] < 117).any()  # an uncovered neighbour takes its weight away


def test_single_planes_and_unbatched_calls(R):
    src, out, _, _, mats = generic_run(8)
    d_img, d_lab, d_dep = map(dev, src)
    rot = R.HPRotator(16, 8, s2_bkgd_class=BKGD, depth_fill=FILL)
    one_img, one_lab, one_dep = rot(d_img, rotations=mats), rot(hp_mask=d_lab, rotations=mats), rot(hp_depth=d_dep, rotations=mats)
    assert torch.is_tensor(one_img) and np.array_equal(one_img.cpu().numpy(), out[0])
    assert np.array_equal(one_lab.cpu().numpy(), out[1]) and np.array_equal(bits(one_dep.cpu().numpy()), bits(out[2]))
    pair = rot(d_img, hp_depth=d_dep, rotations=mats)
    assert len(pair) == 2 and np.array_equal(pair[0].cpu().numpy(), out[0]) and np.array_equal(bits(pair[1].cpu().numpy()), bits(out[2]))
    # no batch dimension: a batch of one
    u_img, u_lab, u_dep = rot(d_img[3], d_lab[3], d_dep[3], rotations=mats[3:4])
    assert u_img.shape == (3, 2048) and u_lab.shape == u_dep.shape == (2048,)
    assert np.array_equal(u_img.cpu().numpy(), out[0][3]) and np.array_equal(u_lab.cpu().numpy(), out[1][3])
    assert np.array_equal(bits(u_dep.cpu().numpy()), bits(out[2][3]))
    # a non-contiguous view is taken as it is given
    wide = torch.zeros((6, 3, 2 * 2048), dtype=torch.uint8, device="cuda")
    wide[:, :, ::2] = d_img
    assert np.array_equal(rot(wide[:, :, ::2], rotations=mats).cpu().numpy(), out[0])


def test_a_non_finite_matrix_fills_its_sample_only(R):
    src, out, _, _, mats = generic_run(8)
    bad = mats[:3].copy()
    bad[1, 2, 1] = np.nan
    rot = R.HPRotator(16, 8, s2_bkgd_class=BKGD, depth_fill=FILL)
    o_img, o_lab, o_dep = (t.cpu().numpy() for t in rot(*(dev(s[:3]) for s in src), rotations=bad))
    assert (o_img[1] == 0).all() and (o_lab[1] == BKGD).all() and (bits(o_dep[1]) == bits(np.float32(FILL))).all()
    for b in (0, 2):
        assert np.array_equal(o_img[b], out[0][b]) and np.array_equal(o_lab[b], out[1][b]) and np.array_equal(bits(o_dep[b]), bits(out[2][b]))
    pix, wgt, near = (t.cpu().numpy() for t in R.rotated_interp(16, bad))
    assert (pix[1] == -1).all() and (wgt[1] == 0.0).all() and (near[1] == -1).all() and pix[0].min() >= 0 and pix[2].min() >= 0


# ------------------------------------------------------------------ 4. graph capture
def test_rotations_change_between_graph_replays(R):
    from heal_swin_amd import projection as P

    cal, nside = calibrations()["mvl_96x128"], 16
    img, lab, dep = map(dev, planes(6, 4, 8 * 256))
    first = P.random_rotations(4, 5.0, flip=0.5, generator=torch.Generator().manual_seed(1))
    second = P.random_rotations(4, 5.0, flip=0.5, generator=torch.Generator().manual_seed(2)).cuda()
    a = first.cuda()
    rot = R.HPRotator(nside, 8, cal_info=cal, rotate_pole=True, s2_bkgd_class=BKGD, depth_fill=FILL)

    def step():
        return rot(img, lab, dep, rotations=a)

    def same(x, y):
        return torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2].view(torch.int32), y[2].view(torch.int32))

    eager_first = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    replay_first = [t.clone() for t in out]
    a.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    replay_second = [t.clone() for t in out]
    eager_second = step()
    assert same(replay_first, eager_first)
    assert same(replay_second, eager_second)
    assert not torch.equal(replay_second[0], replay_first[0]) and not torch.equal(replay_second[1], replay_first[1])


# ------------------------------------------------------------------ 5. full size
def test_full_size_on_a_strided_sample(R):
    """nside 256, 8 base pixels, batch 2: 4096 pixels per plane, one every 128, against the host tables"""
    nside, base_pix, batch = 256, 8, 2
    npix = base_pix * nside * nside
    mats = generic_rotations(256, batch)
    src = planes(8, batch, npix)
    rot = R.HPRotator(nside, base_pix, s2_bkgd_class=BKGD, depth_fill=FILL)
    out = [t.cpu().numpy() for t in rot(*map(dev, src), rotations=mats)]
    sel = np.arange(0, npix, npix // 4096)
    assert sel.size == 4096
    theta, phi = directions(nside, base_pix, mats)
    table = oracle_table(nside, theta[:, sel], phi[:, sel])
    touched = check_against_oracle((out[0][:, :, sel], out[1][:, sel], out[2][:, sel]), src, table, npix, "nside 256")
    assert touched > 0.01
    own = [t.cpu().numpy()[..., sel] for t in R.rotated_interp(nside, mats, count=npix)]
    assert (own[0] == table[0]).all(1).mean() >= 1 - MAX_EXEMPT and np.abs(own[1] - table[1]).max(1)[(own[0] == table[0]).all(1)].max() <= TOL_W
