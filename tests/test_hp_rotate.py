"""Rotation of HEALPix-resident maps, the parts that need no GPU: `hs_hp_rotated_interp_host` (the inline function the kernels
run, in a host loop) against the host tables `evaluation.get_interp_weights` / `hp_nearest_pix_idcs` at directions formed here in
numpy, the symmetries and the poles, the non-finite matrix, the frame convention of `HPRotator.matrices`, and every refusal.  The
kernels are checked in test_gpu_hp_rotate.py, which uses the helpers of this file.

Tolerances.  Weights 1e-9: both sides are float64 evaluations of the same formulas at directions that differ by rounding
(the pixel centre through acos / sin / cos here, through sqrt there: about 1e-15 rad); a weight is that difference times the
number of pixels per radian, below 1e-12 up to nside 64.  The four pixels can only differ where the direction lies within that
rounding of a ring or of a pixel boundary along a ring; such pixels are found from the ORACLE alone (its four pixels change when
the direction moves by 1e-9 rad in theta or phi), exempted from the positional comparison, counted, and capped at 0.1 % of the
case's pixels.  The interpolated value is continuous across those boundaries, so it is compared everywhere: 1e-6 of a byte
range of 255 is four orders above 255 * 4 * 1e-12 and four below anything that changes a rounded byte."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_projection import calibrations

TOL_W, TOL_V, EPS_DIR, MAX_EXEMPT = 1e-9, 1e-6, 1e-9, 1e-3
FLIP = np.diag([-1.0, 1.0, 1.0])


def rz(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


# maps pixel centres onto pixel centres: Rz(90 deg) and Rz(180 deg) with exact entries, the mirror of random_rotations
SYMMETRIES = {"identity": np.eye(3), "rz90": np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]),
              "rz180": np.diag([-1.0, -1.0, 1.0]), "mirror": FLIP}


@pytest.fixture(scope="module")
def R():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import hp_rotate
    return hp_rotate


def generic_rotations(seed, n=6):
    """roll, tilt <= 7 degrees, mirror on about half: what a training run draws"""
    from heal_swin_amd import projection as P
    return P.random_rotations(n, 7.0, flip=0.5, generator=torch.Generator().manual_seed(seed)).numpy()


def directions(nside, base_pix, mats):
    """(theta, phi) float64 [B, n] of M_b g_p, the pixel centres from hs_pix2ang_nest"""
    from heal_swin_amd import projection as P
    theta, phi = P.hp_grid(nside, base_pix)
    g = np.stack((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)), -1)
    d = np.stack([g @ np.asarray(m, dtype=np.float64).T for m in mats])
    return np.arctan2(np.hypot(d[..., 0], d[..., 1]), d[..., 2]), np.arctan2(d[..., 1], d[..., 0])


def oracle_table(nside, theta, phi):
    """(pix [B, 4, n], wgt [B, 4, n], nearest [B, n]) of the host tables"""
    from heal_swin_amd import evaluation as E
    nearest, pix, wgt = E.hp_nearest_pix_idcs(nside, theta, phi)
    return np.moveaxis(pix, 0, 1), np.moveaxis(wgt, 0, 1), nearest


def unstable(nside, theta, phi, pix):
    """bool [B, n]: the oracle's four pixels change when the direction moves by EPS_DIR in theta or in phi"""
    out = np.zeros(theta.shape, dtype=bool)
    for dt, dp in ((EPS_DIR, 0.0), (-EPS_DIR, 0.0), (0.0, EPS_DIR), (0.0, -EPS_DIR)):
        moved, _, _ = oracle_table(nside, np.clip(theta + dt, 0.0, np.pi), phi + dp)
        out |= (moved != pix).any(1)
    return out


def byte_map(nside, seed=17):
    return np.random.default_rng(seed).integers(0, 256, 12 * nside * nside, dtype=np.uint8)


def interp_value(pix, wgt, values, npix=None):
    """((w0 v0 + w1 v1) + w2 v2) + w3 v3, an index outside [0, npix) reading 0.0"""
    npix = values.shape[-1] if npix is None else npix
    ok = (pix >= 0) & (pix < npix)
    v = np.where(ok, values[np.where(ok, pix, 0)].astype(np.float64), 0.0)
    return ((wgt[:, 0] * v[:, 0] + wgt[:, 1] * v[:, 1]) + wgt[:, 2] * v[:, 2]) + wgt[:, 3] * v[:, 3]


def compare_tables(nside, got, want, theta, phi, what):
    """pixels equal positionally and weights within TOL_W outside the counted exemptions; returns the exempt mask"""
    (pix, wgt, nearest), (opix, owgt, onear) = got, want
    exempt = unstable(nside, theta, phi, opix)
    keep = ~exempt
    same = (pix == opix).all(1)
    werr = np.abs(wgt - owgt).max(1)
    print(f"{what}: {exempt.sum()} of {exempt.size} pixels exempt, {np.count_nonzero(~same & keep)} differing brackets, max weight error "
          f"{werr[same].max():.3e}")
    assert exempt.mean() <= MAX_EXEMPT
    assert same[keep].all()
    assert werr[keep].max() <= TOL_W
    assert np.array_equal(nearest[keep], onear[keep])
    return exempt


@functools.lru_cache(maxsize=None)
def generic_case(nside):
    """six matrices on all 12 base pixels: (mats, theta, phi, host entry, oracle), shared and left unchanged"""
    from heal_swin_amd import hp_rotate as R
    mats = generic_rotations(1234 + nside)
    theta, phi = directions(nside, 12, mats)
    return mats, theta, phi, R.rotated_interp_host(nside, mats), oracle_table(nside, theta, phi)


# ------------------------------------------------------------------ 1. the host entry point against the host tables
@pytest.mark.parametrize("nside", [1, 2, 4, 16, 64])
def test_host_entry_matches_the_host_tables(R, nside):
    mats, theta, phi, got, want = generic_case(nside)
    pix, wgt, nearest = got
    assert pix.dtype == nearest.dtype == np.int32 and wgt.dtype == np.float64
    assert pix.shape == wgt.shape == (6, 4, 12 * nside * nside) and nearest.shape == (6, 12 * nside * nside)
    compare_tables(nside, got, want, theta, phi, f"nside {nside}")
    assert np.abs(wgt.sum(1) - 1.0).max() <= 1e-12 and pix.min() >= 0 and pix.max() < 12 * nside * nside


@pytest.mark.parametrize("nside", [1, 2, 4, 16, 64])
def test_interpolated_value_matches_everywhere(R, nside):
    _, _, _, (pix, wgt, _), (opix, owgt, _) = generic_case(nside)
    img = byte_map(nside)
    err = np.abs(interp_value(pix, wgt, img) - interp_value(opix, owgt, img)).max()
    print(f"nside {nside}: max |value - oracle| {err:.3e}")
    assert err <= TOL_V


def test_sub_range_and_single_matrix(R):
    mats, _, _, (pix, wgt, nearest), _ = generic_case(16)
    p, w, n = R.rotated_interp_host(16, mats[2:3], first_pix=777, count=1000)
    assert np.array_equal(p[0], pix[2][:, 777:1777]) and np.array_equal(w[0], wgt[2][:, 777:1777]) and np.array_equal(n[0], nearest[2][777:1777])
    p, w, n = R.rotated_interp_host(16, mats, first_pix=100, count=0)
    assert p.shape == (6, 4, 0) and n.shape == (6, 0)


# ------------------------------------------------------------------ 2. symmetries, poles, seam
def symmetry_permutation(nside, base_pix, m):
    """q with output pixel p <- source pixel q[p], derived from the host tables: every rotated centre is a pixel centre (top weight
    >= 1 - 1e-9) and the map is a bijection of the sphere that keeps the first base_pix base pixels closed."""
    theta, phi = directions(nside, 12, [m])
    _, wgt, nearest = oracle_table(nside, theta, phi)
    assert wgt[0].max(0).min() >= 1.0 - 1e-9
    q = nearest[0]
    assert np.array_equal(np.sort(q), np.arange(12 * nside * nside))
    q = q[:base_pix * nside * nside]
    assert np.array_equal(np.sort(q), np.arange(base_pix * nside * nside))
    return q


@pytest.mark.parametrize("nside", [1, 4, 16])
@pytest.mark.parametrize("name", list(SYMMETRIES))
def test_symmetries_send_centres_to_centres(R, name, nside):
    m = SYMMETRIES[name]
    q = symmetry_permutation(nside, 12, m)
    pix, wgt, nearest = R.rotated_interp_host(nside, m[None])
    assert np.array_equal(nearest[0], q)
    assert wgt[0].max(0).min() >= 1.0 - 1e-9
    if name == "identity":
        assert np.array_equal(q, np.arange(q.size))
    else:
        assert (q != np.arange(q.size)).any()
    img = byte_map(nside)
    assert np.array_equal(np.rint(interp_value(pix, wgt, img)[0]), img[q].astype(np.float64))  # the seam and the caps included


@pytest.mark.parametrize("nside", [1, 2, 16])
def test_poles_and_the_zero_vector(R, nside):
    """M with only M[2][2] = 1: every direction is +z, -z or 0 (the equator's centres; theta = 0 by definition).  At a pole the
    four polar pixels share the weight equally; their order follows phi = atan2(+-0, +-0), so sets are compared."""
    m = np.zeros((1, 3, 3))
    m[0, 2, 2] = 1.0
    npf = nside * nside
    pix, wgt, nearest = R.rotated_interp_host(nside, m)
    theta, phi = directions(nside, 12, m)
    assert set(np.unique(theta)) == {0.0, np.pi}
    opix, owgt, _ = oracle_table(nside, theta, phi)
    assert np.array_equal(wgt, np.full(wgt.shape, 0.25)) and np.array_equal(owgt, wgt)
    assert np.array_equal(np.sort(pix, 1), np.sort(opix, 1))
    north = npf * np.arange(4) + npf - 1  # the northernmost pixel of base pixels 0 .. 3
    south = npf * np.arange(8, 12)        # the southernmost pixel of base pixels 8 .. 11
    up = theta[0] == 0.0
    assert (np.sort(pix[0], 0)[:, up] == north[:, None]).all() and (np.sort(pix[0], 0)[:, ~up] == south[:, None]).all()
    assert np.array_equal(nearest[0], pix[0, 0])  # equal weights: the first
    assert up.sum() > (~up).sum() > 0  # the equator went north


def test_a_non_finite_matrix_fills_its_sample_only(R):
    mats = generic_rotations(5, 3)
    bad = mats.copy()
    bad[1, 0, 1] = np.nan
    pix, wgt, nearest = R.rotated_interp_host(8, bad)
    assert (pix[1] == -1).all() and (wgt[1] == 0.0).all() and (nearest[1] == -1).all()
    ref = R.rotated_interp_host(8, mats)
    for got, want in zip((pix, wgt, nearest), ref):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    bad[1] = mats[1]
    bad[1, 2, 0] = np.inf
    pix, wgt, nearest = R.rotated_interp_host(8, bad)
    assert (pix[1] == -1).all() and (wgt[1] == 0.0).all() and (nearest[1] == -1).all()


# ------------------------------------------------------------------ 3. convention
@pytest.mark.parametrize("name", ["fv_966x1280", "mvl_96x128", "rv_60x80"])
def test_matrices_put_the_camera_frame_rotation_into_the_map_frame(R, name):
    """The stored map was projected with rotate_pole: pixel g shows the camera direction R g.  Under M = R^T A R the rotated map
    shows at pixel p what the augmented projection shows there, the image point of the camera direction A R g_p."""
    from heal_swin_amd import projection as P
    from oracle import projection as OP
    from tests.test_gpu_projection_augment import ref_coords

    cal, nside, base_pix = calibrations()[name], 16, 8
    a = generic_rotations(31, 4)
    rot = R.HPRotator(nside, base_pix, cal_info=cal, rotate_pole=True, device="cpu")
    m = rot.matrices(a)
    assert m.dtype == torch.float64 and m.shape == (4, 3, 3)
    pole = OP.grid_rotation(cal, inv=False)
    assert np.abs(m.numpy() - pole.T @ a @ pole).max() <= 1e-14  # nine products of entries <= 1 per element, summed in another order
    theta, phi = directions(nside, base_pix, m.numpy())
    ur, vr = ref_coords(P, nside, base_pix, cal, [x @ pole for x in a])
    err = 0.0
    for b in range(4):
        u, v = P.project_s2_points_to_img(theta[b], phi[b], cal, rotate_pole=True)
        err = max(err, np.abs(u - ur[b]).max(), np.abs(v - vr[b]).max())
    print(f"{name}: max error {err:.3e} px")
    assert err <= 1e-9
    plain = R.HPRotator(nside, base_pix, device="cpu")  # no pole rotation: the matrices themselves
    assert np.array_equal(plain.matrices(a).numpy(), a)
    assert plain.depth_fill == 0.0 and R.HPRotator(4, s2_bkgd_class=7, device="cpu").depth_fill == 7.0
    assert R.HPRotator(4, s2_bkgd_class=7, depth_fill=1000.0, device="cpu").depth_fill == 1000.0


# ------------------------------------------------------------------ 4. refusals
def test_the_interp_entry_points_refuse_before_launch(R):
    """Every refusal is HS_ERR_INVALID_ARG (1), decided on the host: the pointers name host memory no kernel could read."""
    from heal_swin_amd._lib import lib

    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def dev(nside=4, first=0, count=16, rot=p, batch=2, pix=p, wgt=p, nearest=p):
        return lib.hs_hp_rotated_interp(nside, first, count, rot, batch, pix, wgt, nearest, None)

    def host(nside=4, first=0, count=16, rot=p, batch=2, pix=p, wgt=p, nearest=p):
        return lib.hs_hp_rotated_interp_host(nside, first, count, rot, batch, pix, wgt, nearest)

    for call in (dev, host):
        for kw in (dict(nside=3), dict(nside=0), dict(nside=-4), dict(nside=1 << 30), dict(nside=16384), dict(first=12 * 16 - 8), dict(first=-1),
                   dict(count=-1), dict(count=12 * 16 + 1), dict(first=12 * 16 + 1, count=0), dict(batch=0), dict(batch=-3), dict(batch=65536),
                   dict(rot=None), dict(pix=None), dict(wgt=None), dict(nearest=None)):
            assert call(**kw) == 1, (call.__name__, kw)
            assert lib.hs_last_error()
        assert call(count=0) == 0 and call(first=12 * 16, count=0) == 0 and call(count=0, rot=None, pix=None, wgt=None, nearest=None) == 0
    assert host(nside=8192, first=12 * 8192 * 8192 - 4, count=4, batch=1) == 0  # the largest nside: the last index is 2^31 - 2^29 - 1


def test_hs_hp_rotate_refuses_before_launch(R):
    from heal_swin_amd._lib import lib

    buf = ctypes.create_string_buffer(1 << 20)
    base = ctypes.addressof(buf)
    at = lambda off: ctypes.c_void_p(base + off)  # noqa: E731
    # nside 4, 8 base pixels, batch 2, 3 channels: planes of 768 / 256 / 1024 bytes, all apart
    img, img_out, lab, lab_out, dep, dep_out, rot = at(0), at(4096), at(8192), at(12288), at(16384), at(20480), at(32768)

    def call(nside=4, npix=128, rot=rot, batch=2, img=img, channels=3, img_out=img_out, labels=lab, labels_out=lab_out, background=0,
             depth=dep, depth_out=dep_out, fill=0.0):
        return lib.hs_hp_rotate(nside, npix, rot, batch, img, channels, img_out, labels, labels_out, background, depth, depth_out, fill, None)

    none = dict(img=None, img_out=None, labels=None, labels_out=None, depth=None, depth_out=None)
    for kw in (dict(nside=3), dict(nside=0), dict(nside=1 << 30), dict(nside=16384), dict(npix=0), dict(npix=-16), dict(npix=13 * 16),
               dict(npix=100), dict(npix=8), dict(batch=0), dict(batch=65536), dict(channels=0), dict(channels=17), dict(channels=-1),
               dict(img=None), dict(img_out=None), dict(labels=None), dict(labels_out=None), dict(depth=None), dict(depth_out=None), none,
               dict(img_out=img), dict(labels_out=lab), dict(depth_out=dep), dict(img_out=at(700)), dict(img=at(4096 + 100)),
               dict(depth_out=at(16384 + 1020)), dict(labels_out=at(8192 - 255)), dict(background=-1), dict(background=256), dict(rot=None)):
        assert call(**kw) == 1, kw
        assert lib.hs_last_error()
    # channels are not looked at without a frame: the call gets as far as the matrices
    assert call(**dict(none, labels=lab, labels_out=lab_out, channels=0, rot=None)) == 1 and b"null pointer" in lib.hs_last_error()


def test_python_argument_checks(R):
    """Everything is checked before anything touches the device, so the refusals need none."""
    a = generic_rotations(3, 2)
    for bad in (np.eye(3), np.zeros((2, 9)), np.zeros((2, 3, 4)), np.zeros((0, 3, 3)), torch.zeros(2, 4, 3, 3)):
        with pytest.raises(ValueError, match="rotations"):
            R.rotated_interp(4, bad)
        with pytest.raises(ValueError, match="rotations"):
            R.rotated_interp_host(4, bad)
    for fn in (R.rotated_interp, R.rotated_interp_host):
        for kw in (dict(nside=3), dict(nside=0), dict(nside=16384), dict(first_pix=-1), dict(first_pix=190, count=3), dict(count=-1),
                   dict(count=193)):
            with pytest.raises(ValueError):
                fn(**dict(dict(nside=4, rotations=a), **kw))
    with pytest.raises(RuntimeError, match="HIP kernel"):
        R.rotated_interp(4, a, device="cpu")
    for kw in (dict(nside=3), dict(nside=32768), dict(base_pix=0), dict(base_pix=13), dict(s2_bkgd_class=256), dict(s2_bkgd_class=-1),
               dict(rotate_pole=True)):
        with pytest.raises(ValueError):
            R.HPRotator(**dict(dict(nside=4, device="cpu"), **kw))
    rot = R.HPRotator(4, 8)  # names the device without touching it
    assert rot.npix == 128
    img, mask, depth = torch.zeros(2, 3, 128, dtype=torch.uint8), torch.zeros(2, 128, dtype=torch.uint8), torch.zeros(2, 128)
    with pytest.raises(ValueError, match="rotations"):
        rot(img, mask)
    with pytest.raises(ValueError, match="at least one"):
        rot(rotations=a)
    for kw, err in ((dict(hp_img=img.float()), TypeError), (dict(hp_mask=mask.long()), TypeError), (dict(hp_depth=depth.double()), TypeError),
                    (dict(hp_depth=mask), TypeError), (dict(hp_img=img[:, :, :100]), ValueError), (dict(hp_mask=torch.zeros(2, 192, dtype=torch.uint8)), ValueError),
                    (dict(hp_img=img[None]), ValueError), (dict(hp_mask=mask[0, 0]), ValueError), (dict(hp_depth=depth[None]), ValueError),
                    (dict(hp_img=img[:1]), ValueError), (dict(hp_mask=mask[0]), ValueError), (dict(hp_img=img, hp_mask=mask[:1]), ValueError),
                    (dict(hp_img=torch.zeros(2, 17, 128, dtype=torch.uint8)), ValueError), (dict(hp_img=torch.zeros(2, 0, 128, dtype=torch.uint8)), ValueError)):
        with pytest.raises(err):
            rot(rotations=a, **kw)
    with pytest.raises(ValueError, match="batch dimension"):
        rot(img[0], mask[:1], rotations=a[:1])
    for kw in (dict(hp_img=img), dict(hp_mask=mask), dict(hp_depth=depth), dict(hp_img=img, hp_mask=mask, hp_depth=depth)):
        with pytest.raises(RuntimeError, match="GPU tensor"):  # well-formed calls still need the device: there is no CPU path
            rot(rotations=a, **kw)
