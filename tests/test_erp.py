"""Equirectangular panoramas to HEALPix and back, the parts that need no GPU: `hs_erp_to_hp_host` (the inline function the kernel
runs, in a host loop) against a float64 numpy model written here, the seam and the poles, the yaw symmetry, supersampling, the
layout matrices, `ERPBackProjector`'s tables, and every refusal.  The kernel is checked bit for bit against the host entry point
in test_gpu_erp.py, which uses the helpers of this file.

The model shares nothing with the code under test: the pixel centres come from the host tables (`projection.hp_grid`, acos / sin /
cos; the inline function builds the vector from sqrt), the rotation and the angles from numpy's library functions (the inline
function evaluates sine, cosine, hypot and atan2 itself, so this comparison is also their check).  Both sides are float64
evaluations of the same formulas at directions that differ by rounding, about 1e-15 rad, so image coordinates agree to about
1e-13 px at these sizes.

Tolerances.
  frames u8     |out - model| <= 0.5 + 1e-6 everywhere: the bilinear value is continuous across cell boundaries, columns
                through the seam and rows through the clamp included, so a pixel that rounds its cell differently still has the
                model's value to 1e-12, and rint moves it by at most 0.5.
  frames f32    the output is the float64 value cast to float, so it is compared with the model's value cast the same way, to
                1e-9 relative (against the uncast float64 value every float32 is off by up to 2^-24 = 6e-8).
  labels, depth the model's nearest pick, except where the model's own x + 0.5 or y + 0.5 lies within 1e-6 of an integer; such
                pixels are found from the model alone, counted, and capped at 0.1 % of the case.
Rotations are generic (seeded QR factors, and random_rotations composed with them), never the identity: at the identity the
HEALPix centres sit exactly on column-rounding boundaries (92 % of the pixels at nside 4 / 16 x 32), which is what the
bit-for-bit comparison on the GPU covers."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_hp_rotate import directions, rz

TOL_NEAR, TOL_HALF, MAX_EXEMPT, TOL_F32 = 1e-6, 1e-6, 1e-3, 1e-9
SHAPES = [(nside, hw) for nside in (4, 8) for hw in ((5, 7), (12, 25), (16, 32))]
BKGD, FILL = 200, -3.5  # values the random planes do not hold


@pytest.fixture(scope="module")
def E():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import erp
    return erp


def generic_matrices(seed, n=3):
    """n seeded QR factors (orthogonal, either handedness) and n augmentation draws (roll, tilt <= 7 degrees, mirror on about
    half) composed with them: [2 n, 3, 3]"""
    from heal_swin_amd import projection as P
    rng = np.random.default_rng(seed)
    q = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(n)])
    a = P.random_rotations(n, 7.0, flip=0.5, generator=torch.Generator().manual_seed(seed)).numpy()
    return np.concatenate((q, a @ q))


def planes(seed, batch, height, width, channels=3):
    """random bytes, float frames, class ids 0 .. 9, depths with inf, NaN and the 1000 m background among them"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (batch, channels, height, width), dtype=np.uint8)
    fimg = rng.normal(0.0, 3.0, (batch, channels, height, width)).astype(np.float32)
    lab = rng.integers(0, 10, (batch, height, width), dtype=np.uint8)
    dep = rng.uniform(0.2, 400, (batch, height, width)).astype(np.float32)
    dep[rng.random(dep.shape) < 0.1] = 1000.0
    dep[rng.random(dep.shape) < 0.05] = np.inf
    dep[rng.random(dep.shape) < 0.05] = np.nan
    return img, fimg, lab, dep


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------ the numpy model
def model_coords(nside, base_pix, mats, height, width):
    """(x, y) float64 [B, n]: continuous column and row of direction M_b g_p"""
    theta, phi = directions(nside, base_pix, mats)
    phi = np.mod(phi, 2.0 * np.pi)
    return phi * width / (2.0 * np.pi) - 0.5, theta * height / np.pi - 0.5


def model_bilinear(img, x, y):
    """float64 [B, C, n]: columns wrap, rows clamp"""
    b, _, h, w = img.shape
    v = img.astype(np.float64)
    j0, i0 = np.floor(x), np.floor(y)
    fx, fy = (x - j0)[:, None], (y - i0)[:, None]
    ja, jb = np.mod(j0, w).astype(int), np.mod(j0 + 1, w).astype(int)
    ia, ib = np.clip(i0, 0, h - 1).astype(int), np.clip(i0 + 1, 0, h - 1).astype(int)
    s = np.arange(b)[:, None]
    at = lambda i, j: np.moveaxis(v[s, :, i, j], -1, 1)  # noqa: E731
    return (1 - fy) * ((1 - fx) * at(ia, ja) + fx * at(ia, jb)) + fy * ((1 - fx) * at(ib, ja) + fx * at(ib, jb))


def model_frame(img, nside, base_pix, mats, supersample=0):
    """un-rounded frame values float64 [B, C, n]: the mean over the 4^s nested children at nside 2^s"""
    h, w = img.shape[-2:]
    x, y = model_coords(nside << supersample, base_pix, mats, h, w)
    v = model_bilinear(img, x, y)
    return v.reshape(v.shape[0], v.shape[1], -1, 4 ** supersample).mean(-1)


def model_nearest(plane, nside, base_pix, mats):
    """(picked [B, n], unstable bool [B, n]) of a [B, H, W] plane: the nearest panorama pixel, and where that is a rounding matter"""
    b, h, w = plane.shape
    x, y = model_coords(nside, base_pix, mats, h, w)
    xs, ys = x + 0.5, y + 0.5
    jn, i_n = np.mod(np.floor(xs), w).astype(int), np.clip(np.floor(ys), 0, h - 1).astype(int)
    unstable = (np.abs(xs - np.rint(xs)) <= TOL_NEAR) | (np.abs(ys - np.rint(ys)) <= TOL_NEAR)
    return plane[np.arange(b)[:, None], i_n, jn], unstable


def check_nearest(o_lab, o_dep, lab, dep, nside, base_pix, mats, what):
    want_lab, unstable = model_nearest(lab, nside, base_pix, mats)
    want_dep, _ = model_nearest(bits(dep), nside, base_pix, mats)
    print(f"{what}: {unstable.sum()} of {unstable.size} pixels exempt from the nearest comparison")
    assert unstable.mean() <= MAX_EXEMPT
    assert np.array_equal(o_lab[~unstable], want_lab[~unstable])
    assert np.array_equal(bits(o_dep)[~unstable], want_dep[~unstable])


@functools.lru_cache(maxsize=None)
def generic_case(nside, hw):
    """six generic matrices on all 12 base pixels with random planes: (mats, (img, fimg, lab, dep)), shared and left unchanged"""
    return generic_matrices(100 * nside + hw[0]), planes(7 * nside + hw[1], 6, *hw)


# ------------------------------------------------------------------ 1. the host entry point against the model
@pytest.mark.parametrize("nside,hw", SHAPES)
def test_host_entry_matches_the_numpy_model(E, nside, hw):
    mats, (img, fimg, lab, dep) = generic_case(nside, hw)
    npix = 12 * nside * nside
    for s in (0, 1, 2):
        out = E.erp_to_hp_host(nside, mats, img, supersample=s)
        assert out.dtype == np.uint8 and out.shape == (6, 3, npix)
        want = model_frame(img, nside, 12, mats, s)
        err = np.abs(out.astype(np.float64) - want).max()
        print(f"nside {nside}, {hw}, s = {s}: max |byte - model value| {err:.6f}")
        assert err <= 0.5 + 1e-6
        fout = E.erp_to_hp_host(nside, mats, fimg, supersample=s)
        assert fout.dtype == np.float32 and fout.shape == (6, 3, npix)
        fwant = model_frame(fimg, nside, 12, mats, s).astype(np.float32)
        rel = (np.abs(fout.astype(np.float64) - fwant) / np.abs(fwant)).max()
        print(f"nside {nside}, {hw}, s = {s}: max relative f32 error {rel:.3e}")
        assert rel <= TOL_F32
    o_img, o_lab, o_dep = E.erp_to_hp_host(nside, mats, img, lab, dep, s2_bkgd_class=BKGD, depth_fill=FILL)
    assert np.array_equal(o_img, E.erp_to_hp_host(nside, mats, img))  # a plane does not depend on which others are given
    assert o_lab.dtype == np.uint8 and o_dep.dtype == np.float32 and o_lab.shape == o_dep.shape == (6, npix)
    check_nearest(o_lab, o_dep, lab, dep, nside, 12, mats, f"nside {nside}, {hw}")
    assert np.isnan(o_dep).any() and np.isinf(o_dep).any()
    # labels and depth read at the pixel's own centre whatever the supersampling is
    s_lab, s_dep = E.erp_to_hp_host(nside, mats, masks=lab, depth=dep, supersample=2)
    assert np.array_equal(s_lab, o_lab) and np.array_equal(bits(s_dep), bits(o_dep))


def test_fewer_base_pixels_are_the_first_ones(E):
    mats, (img, _, lab, dep) = generic_case(4, (12, 25))
    full = E.erp_to_hp_host(4, mats, img, lab, dep, supersample=1)
    part = E.erp_to_hp_host(4, mats, img, lab, dep, base_pix=8, supersample=1)
    for f, p in zip(full, part):
        assert p.shape[-1] == 128 and np.array_equal(bits(p) if p.dtype == np.float32 else p, (bits(f) if f.dtype == np.float32 else f)[..., :128])


# ------------------------------------------------------------------ 2. seam and poles
@pytest.mark.parametrize("nside,hw", [(8, (5, 7)), (4, (16, 32))])
def test_seam_wraps_and_poles_clamp(E, nside, hw):
    h, w = hw
    mats = generic_matrices(5 + nside)
    x, y = model_coords(nside, 12, mats, h, w)
    tol = 2.0 ** -23 * max(h, w)  # the float32 cast of a value below max(h, w), twice over
    cols = np.broadcast_to(np.arange(w, dtype=np.float32), (6, 1, h, w)).copy()
    out = E.erp_to_hp_host(nside, mats, cols)[:, 0].astype(np.float64)
    right, left = (x >= w - 1 + 1e-9), (x < -1e-9)  # beyond the last, before the first column centre
    inner = (x >= 1e-9) & (x < w - 1 - 1e-9)
    assert right.sum() + left.sum() >= 0.5 * x.size / w and right.any() and left.any()  # about one column's share of the sphere
    # between column W - 1 (weight 1 - fx) and column 0 (weight fx)
    assert np.abs(out[right] - (1 - (x[right] - (w - 1))) * (w - 1)).max() <= tol
    assert np.abs(out[left] - (1 - (x[left] + 1)) * (w - 1)).max() <= tol
    assert np.abs(out[inner] - x[inner]).max() <= tol  # elsewhere the column coordinate itself
    rows = np.broadcast_to(np.arange(h, dtype=np.float32)[:, None], (6, 1, h, w)).copy()
    out = E.erp_to_hp_host(nside, mats, rows)[:, 0].astype(np.float64)
    above, below = y < -1e-9, y > h - 1 + 1e-9
    mid = (y >= 1e-9) & (y <= h - 1 - 1e-9)
    print(f"nside {nside}, {hw}: {right.sum() + left.sum()} pixels across the seam, {above.sum() + below.sum()} beyond the first or last row centre")
    assert above.any() and below.any()
    assert np.abs(out[above]).max() <= tol and np.abs(out[below] - (h - 1)).max() <= tol  # the first / last row's value
    assert np.abs(out[mid] - y[mid]).max() <= tol
    # nearest: columns wrap (floor(x + 0.5) = W is column 0), rows clamp
    lab_c = np.broadcast_to(np.arange(w, dtype=np.uint8), (6, h, w)).copy()
    lab_r = np.broadcast_to(np.arange(h, dtype=np.uint8)[:, None], (6, h, w)).copy()
    safe_x, safe_y = np.abs(x + 0.5 - np.rint(x + 0.5)) > TOL_NEAR, np.abs(y + 0.5 - np.rint(y + 0.5)) > TOL_NEAR
    got_c, got_r = E.erp_to_hp_host(nside, mats, masks=lab_c), E.erp_to_hp_host(nside, mats, masks=lab_r)
    assert np.array_equal(got_c[safe_x], np.mod(np.floor(x + 0.5), w).astype(np.uint8)[safe_x])
    assert np.array_equal(got_r[safe_y], np.clip(np.floor(y + 0.5), 0, h - 1).astype(np.uint8)[safe_y])
    assert (got_c[left & safe_x] == 0).all() and (got_c[right & safe_x] == w - 1).all()  # x >= -0.5: the seam's nearer side
    assert (got_r[above] == 0).all() and (got_r[below] == h - 1).all()


# ------------------------------------------------------------------ 3. yaw symmetry
@pytest.mark.parametrize("nside,hw", SHAPES)
def test_a_yaw_by_whole_columns_rolls_the_panorama(E, nside, hw):
    h, w = hw
    g, (img, _, lab, dep) = generic_case(nside, hw)
    for k, s in ((1, 0), (w // 2, 1), (w - 2, 2)):
        yawed = np.stack([rz(2.0 * np.pi * k / w) @ m for m in g])
        a = E.erp_to_hp_host(nside, yawed, img, lab, dep, supersample=s)
        b = E.erp_to_hp_host(nside, g, *(np.roll(t, -k, axis=-1) for t in (img, lab, dep)), supersample=s)
        value = model_frame(img, nside, 12, yawed, s)
        half = np.abs(value - np.floor(value) - 0.5) <= TOL_HALF
        _, unstable = model_nearest(lab, nside, 12, yawed)
        print(f"nside {nside}, {hw}, k = {k}, s = {s}: {half.sum()} half-integer values, {unstable.sum()} unstable nearest picks")
        assert half.mean() <= MAX_EXEMPT and unstable.mean() <= MAX_EXEMPT
        assert np.array_equal(a[0][~half], b[0][~half])
        assert np.array_equal(a[1][~unstable], b[1][~unstable]) and np.array_equal(bits(a[2])[~unstable], bits(b[2])[~unstable])
        assert not np.array_equal(a[0], E.erp_to_hp_host(nside, g, img, supersample=s))  # the yaw does move the picture


# ------------------------------------------------------------------ 4. supersampling
def test_supersample_is_the_mean_of_the_children(E):
    nside, hw = 4, (12, 25)
    mats, (_, fimg, _, _) = generic_case(nside, hw)
    x, y = model_coords(2 * nside, 12, mats, *hw)
    children = model_bilinear(fimg, x, y).reshape(6, 3, -1, 4)  # pixel p's children are 4 p .. 4 p + 3 at 2 nside
    want = (((children[..., 0] + children[..., 1]) + children[..., 2]) + children[..., 3]) * 0.25
    got = E.erp_to_hp_host(nside, mats, fimg, supersample=1)
    assert (np.abs(got - want.astype(np.float32)) <= TOL_F32 * np.abs(want)).all()
    assert np.abs(got - E.erp_to_hp_host(nside, mats, fimg)).max() > 0.1  # and not the value at the pixel's own centre


@pytest.mark.parametrize("s", [0, 1, 2])
def test_a_constant_panorama_stays_constant(E, s):
    mats = generic_matrices(3)
    for value in (0, 117, 255):
        out = E.erp_to_hp_host(8, mats, np.full((6, 2, 5, 7), value, dtype=np.uint8), supersample=s)
        assert (out == value).all()


# ------------------------------------------------------------------ 5. layouts
@pytest.mark.parametrize("lon_left,right", [(0.0, True), (1.3, True), (-np.pi, True), (0.0, False), (2.1, False), (np.pi, False)])
def test_layout_reads_back_its_longitudes(E, lon_left, right):
    """a panorama painted with its own longitudes (a depth plane: nearest, copied) shows every HEALPix pixel a longitude within
    half a column of its own"""
    from heal_swin_amd import projection as P
    nside, h, w = 8, 12, 25
    layout = E.erp_layout(lon_left, right)
    assert layout.shape == (3, 3) and np.abs(layout @ layout.T - np.eye(3)).max() <= 1e-15
    assert np.linalg.det(layout) * (1 if right else -1) > 0.99
    lon = lon_left + (1 if right else -1) * 2.0 * np.pi * (np.arange(w) + 0.5) / w
    pano = np.broadcast_to(lon.astype(np.float32), (1, h, w)).copy()
    proj = E.ERPProjector(nside, layout=layout, device="cpu")
    m = proj.matrices(None, 1).numpy()
    assert np.abs(m[0] - layout).max() == 0
    out = E.erp_to_hp_host(nside, m, depth=pano)[0].astype(np.float64)
    _, phi = P.hp_grid(nside, 12)
    off = np.abs(np.mod(out - phi + np.pi, 2.0 * np.pi) - np.pi)
    print(f"lon_left {lon_left}, right {right}: max longitude offset {off.max():.4f} of half a column {np.pi / w:.4f}")
    assert off.max() <= np.pi / w + 1e-6
    a = generic_matrices(8)
    assert np.abs(proj.matrices(a).numpy() - layout @ a).max() <= 1e-15  # M_b = L A_b
    assert np.array_equal(E.ERPProjector(nside, device="cpu").matrices(a).numpy(), a)
    assert np.array_equal(E.erp_layout(), np.eye(3))


# ------------------------------------------------------------------ 6. the back projector
@pytest.mark.parametrize("nside,hw", SHAPES)
def test_back_projector_tables(E, nside, hw):
    from heal_swin_amd import evaluation as EV
    theta, phi = E.erp_grid(*hw)
    assert theta.shape == phi.shape == hw and theta.dtype == phi.dtype == np.float64
    assert np.allclose(theta[:, 0], np.pi * (np.arange(hw[0]) + 0.5) / hw[0], rtol=0, atol=1e-15)
    assert np.allclose(phi[0], 2 * np.pi * (np.arange(hw[1]) + 0.5) / hw[1], rtol=0, atol=1e-15)
    nearest, pix, wgt = EV.hp_nearest_pix_idcs(nside, theta, phi)
    back = E.ERPBackProjector(*hw, nside, device="cpu")
    assert isinstance(back, EV.HPBackProjector) and back.shape == hw and back.n_out == hw[0] * hw[1] and back.npix == 12 * nside * nside
    assert back.nearest.dtype == back.idx.dtype == torch.int32 and back.wgt.dtype == torch.float64
    assert np.array_equal(back.nearest.numpy(), nearest) and np.array_equal(back.idx.numpy(), pix) and np.array_equal(back.wgt.numpy(), wgt)
    assert back.valid.all() and back.valid.shape == hw
    part = E.ERPBackProjector(*hw, nside, base_pix=8, s2_bkgd_class=3, device="cpu")
    assert part.npix == 8 * nside * nside and part.s2_bkgd_class == 3
    assert np.array_equal(part.valid.numpy(), nearest < 8 * nside * nside) and not part.valid.all() and part.valid.any()
    same = EV.HPBackProjector.from_angles(theta, phi, nside, 12, device="cpu")
    assert type(same) is EV.HPBackProjector and torch.equal(same.nearest, back.nearest) and torch.equal(same.wgt, back.wgt)


def test_back_projector_layout_undoes_the_projector(E):
    """pixel (i, j) looks along L^T k_ij; at nside 8 a 5 x 7 panorama's pixels are several HEALPix pixels wide, so a label plane
    projected with a layout and read back through the same layout's nearest table is itself"""
    from heal_swin_amd import evaluation as EV
    nside, h, w = 8, 5, 7
    for layout in (E.erp_layout(0.7), E.erp_layout(-2.0, False)):
        theta, phi = E.erp_grid(h, w)
        k = np.stack((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)), -1)
        d = np.einsum("ji,hwj->hwi", layout, k)
        want, _, _ = EV.hp_nearest_pix_idcs(nside, np.arctan2(np.hypot(d[..., 0], d[..., 1]), d[..., 2]), np.arctan2(d[..., 1], d[..., 0]))
        back = E.ERPBackProjector(h, w, nside, layout=layout, device="cpu")
        assert np.array_equal(back.nearest.numpy(), want)
        lab = np.arange(h * w, dtype=np.uint8).reshape(1, h, w)
        hp = E.erp_to_hp_host(nside, E.ERPProjector(nside, layout=layout, device="cpu").matrices(None, 1).numpy(), masks=lab)
        assert np.array_equal(hp[0][back.nearest.numpy()], lab[0])


# ------------------------------------------------------------------ 7. refusals
def test_every_refusal_leaves_the_outputs_untouched(E):
    """Every refusal is HS_ERR_INVALID_ARG (1), decided on the host before anything is launched or written: the pointers name
    host memory no kernel could read, and the guard pattern of the outputs survives."""
    from heal_swin_amd._lib import HS_F32, HS_U8, lib

    buf = (ctypes.c_ubyte * (1 << 16))(*([0xA5] * (1 << 16)))
    base = ctypes.addressof(buf)
    at = lambda off: ctypes.c_void_p(base + off)  # noqa: E731
    # nside 4, 8 base pixels, batch 2, 3 channels, 5 x 7: inputs of 210 / 70 / 280 bytes, outputs of 768 / 256 / 1024, all apart
    img, img_out, lab, lab_out, dep, dep_out, rot = at(0), at(4096), at(8192), at(12288), at(16384), at(20480), at(32768)

    def dev(nside=4, npix=128, rot=rot, batch=2, height=5, width=7, s=0, frame=img, kind=HS_U8, channels=3, frame_out=img_out, labels=lab,
            labels_out=lab_out, background=0, depth=dep, depth_out=dep_out, fill=0.0):
        return lib.hs_erp_to_hp(nside, npix, rot, batch, height, width, s, frame, kind, channels, frame_out, labels, labels_out, background,
                                depth, depth_out, fill, None)

    def host(nside=4, npix=128, rot=rot, batch=2, height=5, width=7, s=0, frame=img, kind=HS_U8, channels=3, frame_out=img_out, labels=lab,
             labels_out=lab_out, background=0, depth=dep, depth_out=dep_out, fill=0.0):
        return lib.hs_erp_to_hp_host(nside, npix, rot, batch, height, width, s, frame, kind, channels, frame_out, labels, labels_out,
                                     background, depth, depth_out, fill)

    none = dict(frame=None, frame_out=None, labels=None, labels_out=None, depth=None, depth_out=None)
    refused = (dict(nside=3), dict(nside=0), dict(nside=-4), dict(nside=16384, npix=12 * 16384 * 16384), dict(nside=8192, npix=8192 * 8192, s=1),
               dict(nside=4096, npix=4096 * 4096, s=2), dict(s=-1), dict(s=3), dict(npix=0), dict(npix=-16), dict(npix=13 * 16), dict(npix=100),
               dict(npix=8), dict(height=0), dict(width=0), dict(height=-5), dict(height=1 << 16, width=1 << 15), dict(height=46341, width=46341),
               dict(batch=0), dict(batch=-3), dict(batch=65536), dict(channels=0), dict(channels=17), dict(kind=HS_F32 + 1), dict(kind=9),
               dict(frame=None), dict(frame_out=None), dict(labels=None), dict(labels_out=None), dict(depth=None), dict(depth_out=None), none,
               dict(frame_out=img), dict(labels_out=lab), dict(depth_out=dep), dict(frame_out=at(200)), dict(frame=at(4096 + 700)),
               dict(labels_out=dep), dict(depth_out=at(8192 + 64)), dict(frame_out=at(8192 - 700)), dict(labels_out=at(32768 + 100)),
               dict(kind=HS_F32, frame_out=at(16384 - 3000)), dict(background=-1), dict(background=256), dict(rot=None))
    for call in (dev, host):
        for kw in refused:
            assert call(**kw) == 1, (call.__name__, kw)
            assert lib.hs_last_error()
    assert bytes(buf) == b"\xa5" * (1 << 16)
    # channels and frame_kind are not looked at without a frame: the call gets as far as the matrices
    assert dev(**dict(none, labels=lab, labels_out=lab_out, channels=0, kind=77, rot=None)) == 1 and b"null pointer" in lib.hs_last_error()
    # the smallest call passes: one pixel of a 1 x 1 panorama
    one = np.zeros((1, 1, 1), dtype=np.uint8)
    eye = np.eye(3)[None]
    assert E.erp_to_hp_host(1, eye, masks=one, base_pix=1).shape == (1, 1)
    lab1, out1 = at(40000), at(40100)
    ident = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    assert host(nside=1, npix=1, rot=ident, batch=1, height=1, width=1, labels=lab1, labels_out=out1, **{k: None for k in ("frame", "frame_out", "depth", "depth_out")}) == 0
    assert buf[40100] == 0xA5 and buf[40101] == 0xA5  # the copied byte is the pattern itself; nothing else moved
    assert bytes(buf) == b"\xa5" * (1 << 16)


def test_a_non_finite_matrix_gives_the_fill_values(E):
    mats, (img, fimg, lab, dep) = generic_case(4, (5, 7))
    ref = E.erp_to_hp_host(4, mats[:3], img[:3], lab[:3], dep[:3], supersample=1, s2_bkgd_class=BKGD, depth_fill=FILL)
    for bad_value in (np.nan, np.inf):
        bad = mats[:3].copy()
        bad[1, 2, 1] = bad_value
        for s in (0, 1):
            o_img, o_lab, o_dep = E.erp_to_hp_host(4, bad, img[:3], lab[:3], dep[:3], supersample=s, s2_bkgd_class=BKGD, depth_fill=FILL)
            assert (o_img[1] == 0).all() and (o_lab[1] == BKGD).all() and (bits(o_dep[1]) == bits(np.float32(FILL))).all()
            assert np.isnan(E.erp_to_hp_host(4, bad, fimg[:3], supersample=s)[1]).all()
            if s == 1:  # its neighbours are projected as ever
                for b in (0, 2):
                    assert np.array_equal(o_img[b], ref[0][b]) and np.array_equal(o_lab[b], ref[1][b]) and np.array_equal(bits(o_dep[b]), bits(ref[2][b]))


def test_python_argument_checks(E):
    """Everything is checked before anything touches the device, so the refusals need none."""
    a = generic_matrices(3, 1)[:1]
    for kw in (dict(nside=3), dict(nside=0), dict(nside=16384), dict(nside=8192, supersample=1), dict(supersample=3), dict(supersample=-1),
               dict(base_pix=0), dict(base_pix=13), dict(s2_bkgd_class=256), dict(s2_bkgd_class=-1), dict(layout=np.eye(4)),
               dict(layout=np.full((3, 3), np.nan))):
        with pytest.raises(ValueError):
            E.ERPProjector(**dict(dict(nside=4, device="cpu"), **kw))
    with pytest.raises(ValueError):
        E.ERPBackProjector(5, 7, 4, layout=np.eye(2), device="cpu")
    with pytest.raises(ValueError):
        E.erp_grid(0, 7)
    proj = E.ERPProjector(4)  # names the device without touching it
    assert proj.npix == 192 and proj.depth_fill == 0.0 and E.ERPProjector(4, s2_bkgd_class=7, device="cpu").depth_fill == 7.0
    img, mask, depth = torch.zeros(2, 3, 5, 7, dtype=torch.uint8), torch.zeros(2, 5, 7, dtype=torch.uint8), torch.zeros(2, 5, 7)
    with pytest.raises(ValueError, match="at least one"):
        proj(rotations=a)
    for kw, err in ((dict(imgs=img.double()), TypeError), (dict(imgs=img.long()), TypeError), (dict(masks=mask.long()), TypeError),
                    (dict(depth=depth.double()), TypeError), (dict(depth=mask), TypeError), (dict(imgs=img, masks=mask[:, :4]), ValueError),
                    (dict(imgs=img, depth=depth[:1]), ValueError), (dict(imgs=img[None]), ValueError), (dict(masks=mask[0, 0]), ValueError),
                    (dict(imgs=torch.zeros(2, 17, 5, 7, dtype=torch.uint8)), ValueError), (dict(imgs=torch.zeros(2, 0, 5, 7, dtype=torch.uint8)), ValueError),
                    (dict(imgs=img[0], masks=mask), ValueError), (dict(imgs=img, rotations=a), ValueError), (dict(imgs=img, rotations=np.eye(3)), ValueError)):
        with pytest.raises(err):
            proj(**kw)
    for kw in (dict(imgs=img), dict(imgs=img.float()), dict(masks=mask), dict(depth=depth), dict(imgs=img, masks=mask, depth=depth)):
        with pytest.raises(RuntimeError, match="GPU tensor"):  # well-formed calls still need the device: there is no CPU path
            proj(**kw)
    with pytest.raises(ValueError):
        E.erp_to_hp_host(4, a, img[:1].numpy()[0])  # the host twin takes batched arrays only
    with pytest.raises(ValueError):
        E.erp_to_hp_host(4, a, img.numpy())  # two samples, one matrix
