"""Per-sample rotation augmentation of the projection on the GPU: `hs_hp_rotated_coords` against a float64 numpy restatement
written here (it does not call the code under test), the four `hs_sample_*_per_sample` entry points against their shared-table
twins and the numpy oracle, both projectors with `rotations=`, and the coordinate launch under graph capture.

Coordinate tolerance 1e-9 px: two independent float64 formulations of these coordinates (the table path's arccos / cos phi /
sin phi and the vector form hypot / atan2 used here) differ by at most 2.9e-12 px over all three calibrations where |u| reaches
1.8e3; 1e-9 leaves a factor of 350 and sits six orders below anything that changes a sample.  Exact comparisons are made at the
device's own coordinates, so they need no rounding-boundary allowance."""
import functools

import numpy as np
import pytest
import torch

from oracle import projection as OP
from tests.test_projection import GOLD, calibrations

pytestmark = pytest.mark.gpu
TOL_PX = 1e-9


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import projection
    return projection


@pytest.fixture(scope="module")
def DD(P):
    from heal_swin_amd import depth_data
    return depth_data


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rodrigues(axis, angle):
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    k = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)


FLIP = np.diag([-1.0, 1.0, 1.0])
# identity; half a turn about the axis; mirror times a tilt; a rotation that sends a large part of the sphere outside the image
ROTATIONS = np.stack([np.eye(3), rodrigues((0, 0, 1), np.pi), FLIP @ rodrigues((1, 1, 0), 0.3), rodrigues((1, 2, 3), 2.0)])


def ref_coords(P, nside, base_pix, cal, mats, used_size=None):
    """(u, v) float64 [B, Npix]: the grid's unit vectors times M_b, r = hypot, theta = atan2(r, z), the calibration's polynomial."""
    theta, phi = P.hp_grid(nside, base_pix)
    g = np.stack((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)), -1)
    it = cal["intrinsic"]
    h, w = (int(it["height"]), int(it["width"])) if used_size is None else used_size
    us, vs = [], []
    for m in mats:
        d = g @ np.asarray(m, dtype=np.float64).T
        r = np.hypot(d[:, 0], d[:, 1])
        th = np.arctan2(r, d[:, 2])
        safe = np.where(r == 0, 1.0, r)
        cphi, sphi = np.where(r == 0, 1.0, d[:, 0] / safe), np.where(r == 0, 0.0, d[:, 1] / safe)
        rho = sum(it[f"k{i}"] * th**i for i in range(1, int(it["poly_order"]) + 1))
        us.append(rho * cphi + it["cx_offset"] + w / 2 - 0.5)
        vs.append(rho * sphi * it["aspect_ratio"] + it["cy_offset"] + h / 2 - 0.5)
    return np.stack(us), np.stack(vs)


@functools.lru_cache(maxsize=None)
def device_coords(name, nside, base_pix, rotate_pole):
    """rotated_coords of ROTATIONS, read back (shared by the tests; not modified)."""
    from heal_swin_amd import projection as P

    u, v = P.rotated_coords(nside, base_pix, calibrations()[name], ROTATIONS, rotate_pole=rotate_pole)
    assert u.dtype == v.dtype == torch.float64 and u.shape == v.shape == (4, base_pix * nside * nside) and u.is_cuda
    u, v = u.cpu().numpy(), v.cpu().numpy()
    u.setflags(write=False), v.setflags(write=False)
    return u, v


# ------------------------------------------------------------------ 1. pixel centres
@pytest.mark.parametrize("nside", [1, 2, 16])
def test_pixel_centres_over_every_face_and_zone(P, nside):
    """k1 = 1 and a 1 x 1 image with the identity: u = theta cos phi, v = theta sin phi of the device's own pixel centres."""
    cal = dict(name="FV", intrinsic=dict(aspect_ratio=1.0, cx_offset=0.0, cy_offset=0.0, width=1, height=1, poly_order=1, k1=1.0))
    u, v = P.rotated_coords(nside, 12, cal, np.eye(3)[None])
    u, v = u[0].cpu().numpy(), v[0].cpu().numpy()
    theta, phi = P.hp_grid(nside, 12)
    err_t = np.abs(np.hypot(u, v) - theta).max()
    err_p = np.abs(np.mod(np.arctan2(v, u), 2 * np.pi) - phi).max()
    print(f"nside {nside}: max |theta| error {err_t:.3e}, max |phi| error {err_p:.3e} rad")
    assert err_t <= 1e-12 and err_p <= 1e-12


# ------------------------------------------------------------------ 2. coordinates
CASES = [(name, 4, 12) for name in ("fv_966x1280", "mvl_96x128", "rv_60x80")] + [(name, 16, 8) for name in ("fv_966x1280", "mvl_96x128", "rv_60x80")]
CASES.append(("fv_966x1280", 256, 8))


@pytest.mark.parametrize("rotate_pole", [False, True])
@pytest.mark.parametrize("name,nside,base_pix", CASES)
def test_coordinates_match_the_numpy_reference(P, name, nside, base_pix, rotate_pole):
    cal = calibrations()[name]
    u, v = device_coords(name, nside, base_pix, rotate_pole)
    pole = OP.grid_rotation(cal, inv=False) if rotate_pole else np.eye(3)
    ur, vr = ref_coords(P, nside, base_pix, cal, [a @ pole for a in ROTATIONS])
    assert np.isfinite(u).all() and np.isfinite(v).all()
    err = max(np.abs(u - ur).max(), np.abs(v - vr).max())
    h, w = int(cal["intrinsic"]["height"]), int(cal["intrinsic"]["width"])
    inside = ((u > 0) & (u < w - 1) & (v > 0) & (v < h - 1)).mean(1)
    print(f"{name} nside {nside} bp {base_pix} pole {rotate_pole}: max error {err:.3e} px, inside the image per rotation {inside}")
    assert err <= TOL_PX
    assert inside[0] > 0.2  # the camera sees a good part of the grid: the case is not vacuous


# ------------------------------------------------------------------ 3. sub-ranges
def test_sub_range_equals_the_slice_of_the_full_call(P):
    from heal_swin_amd._lib import lib, ptr, stream_ptr
    import ctypes

    name, nside = "mvl_96x128", 16
    full_u, full_v = device_coords(name, nside, 12, False)
    cam = P.camera_record(calibrations()[name])
    rot = dev(ROTATIONS)
    first, count = 37, 300
    u = torch.full((4, count + 8), -7.0, dtype=torch.float64, device="cuda")  # 8 guard columns at the end of the buffer
    v = torch.full((4, count + 8), -7.0, dtype=torch.float64, device="cuda")
    st = lib.hs_hp_rotated_coords(nside, first, count, ctypes.byref(cam), ptr(rot), 4, ptr(u), ptr(v), stream_ptr(u.device))
    assert st == 0
    flat_u, flat_v = u.reshape(-1).cpu().numpy(), v.reshape(-1).cpu().numpy()
    assert np.array_equal(flat_u[:4 * count].reshape(4, count), full_u[:, first:first + count])
    assert np.array_equal(flat_v[:4 * count].reshape(4, count), full_v[:, first:first + count])
    assert (flat_u[4 * count:] == -7.0).all() and (flat_v[4 * count:] == -7.0).all()  # nothing written past [batch, count]


# ------------------------------------------------------------------ 4. convention
def test_quarter_turn_moves_centres_by_one_base_pixel(P):
    """d = M g: with M = Rz(pi / 2) pixel p is projected where the identity projects p + nside^2 (the next face of its group of
    four).  A transposed or inverted matrix moves the other way."""
    nside, cal = 8, calibrations()["mvl_96x128"]
    npf = nside * nside
    mats = np.stack([np.eye(3), rodrigues((0, 0, 1), np.pi / 2)])
    u, v = P.rotated_coords(nside, 12, cal, mats)
    u, v = u.cpu().numpy(), v.cpu().numpy()
    p = np.arange(12 * npf)
    nxt = (p // (4 * npf)) * 4 * npf + (p % (4 * npf) + npf) % (4 * npf)
    err = max(np.abs(u[1] - u[0][nxt]).max(), np.abs(v[1] - v[0][nxt]).max())
    print(f"quarter turn: max error {err:.3e} px")
    assert err <= TOL_PX
    prv = (p // (4 * npf)) * 4 * npf + (p % (4 * npf) - npf) % (4 * npf)
    assert np.abs(u[1] - u[0][prv]).max() > 1.0  # the test tells the two directions apart


@pytest.mark.parametrize("rotate_pole", [False, True])
@pytest.mark.parametrize("name", ["fv_966x1280", "mvl_96x128", "rv_60x80"])
def test_identity_agrees_with_the_projector_table(P, name, rotate_pole):
    cal = calibrations()[name]
    proj = P.HPProjector(cal, 16, 8, rotate_pole=rotate_pole)
    u, v = device_coords(name, 16, 8, rotate_pole)
    err = max(np.abs(u[0] - proj.u.cpu().numpy()).max(), np.abs(v[0] - proj.v.cpu().numpy()).max())
    print(f"{name} pole {rotate_pole}: identity against the host table, max error {err:.3e} px")
    assert err <= TOL_PX


# ------------------------------------------------------------------ 5. per-sample sampling
def _nearest_f32(depth, rx, ry, background):
    """oracle.sample_mask without its cast to uint8: the value of the nearest pixel (round half to even), copied."""
    with np.errstate(invalid="ignore"):
        xi, yi = np.around(rx, 0).astype(int), np.around(ry, 0).astype(int)
    return OP._within(np.asarray(depth), xi, yi, np.float32(background)).astype(np.float32)


def _frames(seed, b, h, w):
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (b, 3, h, w), dtype=np.uint8)
    masks = rng.integers(0, 10, (b, h, w), dtype=np.uint8)
    depths = rng.uniform(0.2, 400, (b, h, w)).astype(np.float32)
    depths[rng.random(depths.shape) < 0.1] = 1000.0
    return imgs, masks, depths


def test_per_sample_with_one_repeated_table_equals_the_shared_table(P, DD):
    g = np.load(GOLD)
    proj = P.HPProjector(calibrations()["mvl_96x128"], 16, 8)
    bad = np.array([np.inf, -np.inf, np.nan, 1e300])
    rx = np.concatenate([proj.v.cpu().numpy(), g["edge/rx"], bad, np.ones(4)])
    ry = np.concatenate([proj.u.cpu().numpy(), g["edge/ry"], np.ones(4), bad])
    imgs, masks, depths = _frames(2, 3, 96, 128)
    imgs, masks, depths = dev(imgs), dev(masks), dev(depths)
    rx3, ry3 = dev(np.tile(rx, (3, 1))), dev(np.tile(ry, (3, 1)))
    for fn, src, extra in ((P.sample_bilinear_u8, imgs, ()), (P.sample_mask, masks, (7,)), (DD.sample_bilinear_f32, imgs, ()),
                           (DD.sample_depth, depths, (2.5,))):
        shared = fn(src, rx, ry, *extra).cpu().numpy()
        per = fn(src, rx3, ry3, *extra, per_sample=True).cpu().numpy()
        assert per.shape == shared.shape and per.dtype == shared.dtype
        assert np.array_equal(per, shared, equal_nan=shared.dtype == np.float32), fn.__name__
        one = fn(src[1], rx3[1:2], ry3[1:2], *extra, per_sample=True).cpu().numpy()  # no batch dimension: a batch of one
        assert np.array_equal(one, shared[1], equal_nan=shared.dtype == np.float32), fn.__name__
    assert np.isnan(DD.sample_bilinear_f32(imgs, rx3, ry3, per_sample=True).cpu().numpy()).any()  # the non-finite rows are exercised


@pytest.mark.parametrize("rotate_pole", [False, True])
def test_per_sample_with_distinct_tables_equals_the_oracle(P, DD, rotate_pole):
    u, v = device_coords("mvl_96x128", 16, 8, rotate_pole)
    imgs, masks, depths = _frames(3, 4, 96, 128)
    du, dv = dev(np.array(u)), dev(np.array(v))
    got_u8 = P.sample_bilinear_u8(dev(imgs), dv, du, per_sample=True).cpu().numpy()
    got_f32 = DD.sample_bilinear_f32(dev(imgs), dv, du, per_sample=True).cpu().numpy()
    got_mask = P.sample_mask(dev(masks), dv, du, 7, per_sample=True).cpu().numpy()
    got_depth = DD.sample_depth(dev(depths), dv, du, 2.5, per_sample=True).cpu().numpy()
    for b in range(4):
        want = OP.sample_bilinear(imgs[b], v[b], u[b])
        assert np.array_equal(got_u8[b], want.astype(np.uint8)), b
        assert np.array_equal(got_f32[b], want.astype(np.float32), equal_nan=True), b
        assert np.array_equal(got_mask[b], OP.sample_mask(masks[b], v[b], u[b], 7)), b
        assert np.array_equal(got_depth[b], _nearest_f32(depths[b], v[b], u[b], 2.5)), b
    assert 0.1 < (got_mask == 7).mean() < 0.9 and (got_depth == 2.5).any()  # outside the image: the background value
    assert len({got_u8[b].tobytes() for b in range(4)}) == 4  # every sample read its own table


# ------------------------------------------------------------------ 6. projectors
def _check_projectors(P, DD, cal, nside, base_pix, rotate_pole, frames, rotations):
    imgs, masks, depths = frames
    d_imgs, d_masks, d_depths = dev(imgs), dev(masks), dev(depths)
    proj = P.HPProjector(cal, nside, base_pix, rotate_pole=rotate_pole, s2_bkgd_class=7)
    dproj = DD.HPDepthProjector(cal, nside, base_pix, rotate_pole=rotate_pole, s2_bkgd_class=3)
    u, v = P.rotated_coords(nside, base_pix, cal, rotations, rotate_pole=rotate_pole)
    u, v = u.cpu().numpy(), v.cpu().numpy()
    hp_img, hp_mask = proj(d_imgs, d_masks, rotations=rotations)
    f_img, f_depth = dproj.proj(d_imgs, d_depths, rotations=rotations)
    assert torch.equal(proj(d_imgs, rotations=dev(np.asarray(rotations))), hp_img)  # a device tensor, no masks
    npix = base_pix * nside * nside
    assert hp_img.shape == f_img.shape == (len(imgs), 3, npix) and hp_mask.shape == f_depth.shape == (len(imgs), npix)
    assert hp_img.dtype == hp_mask.dtype == torch.uint8 and f_img.dtype == f_depth.dtype == torch.float32
    hp_img, hp_mask, f_img, f_depth = (t.cpu().numpy() for t in (hp_img, hp_mask, f_img, f_depth))
    for b in range(len(imgs)):
        want = OP.sample_bilinear(imgs[b], v[b], u[b])
        assert np.array_equal(hp_img[b], want.astype(np.uint8)), b
        assert np.array_equal(f_img[b], want.astype(np.float32), equal_nan=True), b
        assert np.array_equal(hp_mask[b], OP.sample_mask(masks[b], v[b], u[b], 7)), b
        assert np.array_equal(f_depth[b], _nearest_f32(depths[b], v[b], u[b], 3.0)), b
    # rotations=None is the table path: what the unchanged call returns
    plain_img, plain_mask = proj(d_imgs, d_masks)
    none_img, none_mask = proj(d_imgs, d_masks, rotations=None)
    assert torch.equal(plain_img, none_img) and torch.equal(plain_mask, none_mask)
    assert torch.equal(plain_img, P.sample_bilinear_u8(d_imgs, proj.v, proj.u))
    plain_f, plain_d = dproj.proj(d_imgs, d_depths)
    none_f, none_d = dproj.proj(d_imgs, d_depths, rotations=None)
    assert torch.equal(plain_f.view(torch.int32), none_f.view(torch.int32)) and torch.equal(plain_d, none_d)
    return hp_img, hp_mask, plain_img.cpu().numpy()


@pytest.mark.parametrize("rotate_pole", [False, True])
def test_projectors_with_rotations(P, DD, rotate_pole):
    a = P.random_rotations(4, 5.0, flip=0.5, generator=torch.Generator().manual_seed(5))
    hp_img, hp_mask, plain = _check_projectors(P, DD, calibrations()["mvl_96x128"], 16, 8, rotate_pole, _frames(4, 4, 96, 128), a)
    assert (hp_img != plain).mean() > 0.15 and (hp_img > 0).mean() > 0.2  # rotated, and the camera still sees the grid


def test_projectors_with_rotations_at_full_size(P, DD):
    """966 x 1280 frames, nside 256, 8 base pixels, batch 3, a constant region so that the truncation case (c vs c - 1) is there."""
    imgs, masks, depths = _frames(5, 3, 966, 1280)
    imgs[1, :, 300:600, 400:900] = 117
    a = P.random_rotations(3, 5.0, flip=0.5, generator=torch.Generator().manual_seed(9))
    hp_img, _, _ = _check_projectors(P, DD, calibrations()["fv_966x1280"], 256, 8, True, (imgs, masks, depths), a)
    assert (hp_img[1] == 117).any() and (hp_img[1] == 116).any()


# ------------------------------------------------------------------ 7. graph capture
def test_rotations_change_between_graph_replays(P):
    cal, nside = calibrations()["mvl_96x128"], 16
    imgs = dev(_frames(6, 4, 96, 128)[0])
    first = P.random_rotations(4, 5.0, flip=0.5, generator=torch.Generator().manual_seed(1))
    second = P.random_rotations(4, 5.0, flip=0.5, generator=torch.Generator().manual_seed(2)).cuda()
    rot = first.cuda()

    def step():
        u, v = P.rotated_coords(nside, 8, cal, rot)
        return P.sample_bilinear_u8(imgs, v, u, per_sample=True)

    eager_first = step().clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    replay_first = out.clone()
    rot.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    replay_second = out.clone()
    eager_second = step()
    assert torch.equal(replay_first, eager_first)
    assert torch.equal(replay_second, eager_second)
    assert not torch.equal(replay_second, replay_first)
