"""Surround view, the parts that need no GPU: `hs_surround_to_hp_host` (the inline function the kernel runs, in a host loop)
against a float64 numpy model written here from the conventions of include/healswin.h, one camera against the reference's own
labels (tests/golden/projection.npz), the invariants of the fusion, `SurroundProjector.matrices`, `SurroundBackProjector`'s
tables, and every refusal.  The kernel is checked bit for bit against the host entry point in test_gpu_surround.py, which uses the
helpers of this file.

The model shares nothing with the code under test: the pixel centres come from the host tables (`projection.hp_grid`), the angles
from np.arctan2, everything else is plain float64 numpy.  Both sides evaluate the same formulas at directions that differ by
rounding (about 1e-15 rad, 1e-13 px at these sizes), so every DECISION of the model (does a camera see the pixel, which camera
wins, which image pixel is nearest) is the code's except where the model's own margin is below TIE = 1e-9: such pixels are near
ties, found from the model alone, and there the outputs must still be one of the model's candidates.

Tolerances outside near ties.
  camera, labels, depth words   equal
  frames u8     |out - model| <= 0.5 + 1e-6: the model's un-rounded value, moved by rint by at most 0.5
  frames f32    the model's value cast to float32, or one of its two neighbouring floats
Near ties may be at most 1 % of the covered pixels of a case and the covered pixels at least a quarter of the map: conditions on
the inputs, met with room to spare by the seeds chosen here (the shares are printed; with these seeds no near tie occurs at all).
Rotations are generic (seeded QR factors), never a symmetry of the grid: those are what the bit-for-bit comparison on the GPU
covers."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_erp import bits, generic_matrices
from tests.test_projection import GOLD, calibrations

TIE, MAX_TIES, MIN_COVERED = 1e-9, 1e-2, 0.25
BKGD, FILL = 200, -3.5  # values the random planes do not hold
BLENDS = {"winner": 0, "feather": 1}


@pytest.fixture(scope="module")
def S():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import surround
    return surround


def rig_cals(hw, n_cam, seed):
    """n_cam calibrations of one image size with generic extrinsic quaternions: the optics of the golden calibration of that
    size (PROJ_CALS, scaled WoodScape lenses), the offsets and the aspect ratio varied per camera"""
    base = {(60, 80): "rv_60x80", (96, 128): "mvl_96x128"}.get(tuple(hw), "rv_60x80")
    intr = calibrations()[base]["intrinsic"]
    scale = hw[1] / float(intr["width"])
    rng = np.random.default_rng(seed)
    names = ("FV", "RV", "MVL", "MVR")
    cals = []
    for c in range(n_cam):
        i = dict(intr, height=float(hw[0]), width=float(hw[1]), cx_offset=float(rng.uniform(-1.5, 1.5)), cy_offset=float(rng.uniform(-1.5, 1.5)),
                 aspect_ratio=float(rng.uniform(0.998, 1.002)))
        for o in range(1, int(intr["poly_order"]) + 1):
            i["k" + str(o)] = float(intr["k" + str(o)]) * scale
        q = rng.normal(size=4)
        cals.append(dict(name=names[c % 4], intrinsic=i, extrinsic=dict(quaternion=list(q / np.linalg.norm(q)))))
    return cals


def planes(seed, batch, n_cam, height, width, channels=3):
    """random bytes, float frames, class ids 0 .. 9, depths with inf, NaN and the 1000 m background among them, per camera"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (batch, n_cam, channels, height, width), dtype=np.uint8)
    fimg = rng.normal(0.0, 3.0, (batch, n_cam, channels, height, width)).astype(np.float32)
    lab = rng.integers(0, 10, (batch, n_cam, height, width), dtype=np.uint8)
    dep = rng.uniform(0.2, 400, (batch, n_cam, height, width)).astype(np.float32)
    dep[rng.random(dep.shape) < 0.1] = 1000.0
    dep[rng.random(dep.shape) < 0.05] = np.inf
    dep[rng.random(dep.shape) < 0.05] = np.nan
    return img, fimg, lab, dep


def rig_matrices(S, cals, rotations, frame=None):
    """M [B, K, 3, 3] as SurroundProjector forms it, on the host"""
    return S.SurroundProjector(cals, 4, frame=frame, device="cpu").matrices(rotations, None if rotations is not None else 1).numpy()


# ------------------------------------------------------------------ the numpy model
class Model:
    """Per (sample, camera, pixel) of a rig: coordinates, weights and every decision's margin; then the outputs and the near ties."""

    def __init__(self, cals, nside, base_pix, mats, max_theta_deg, edge_feather, present=None):
        from heal_swin_amd import projection as P
        theta, phi = P.hp_grid(nside, base_pix)
        g = np.stack((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)), -1)
        mats = np.asarray(mats, dtype=np.float64)
        self.batch, self.n_cam, self.npix = mats.shape[0], mats.shape[1], g.shape[0]
        intr = [c["intrinsic"] for c in cals]
        self.h, self.w = int(intr[0]["height"]), int(intr[0]["width"])
        h, w = float(self.h), float(self.w)
        mt = np.pi * (np.broadcast_to(np.asarray(max_theta_deg, dtype=np.float64), (self.n_cam,)) / 180.0)
        here = np.ones((self.batch, self.n_cam), bool) if present is None else np.asarray(present).astype(bool)
        shape = (self.batch, self.n_cam, self.npix)
        self.u, self.v, self.wgt = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        self.counts, self.near = np.zeros(shape, bool), np.zeros(shape, bool)
        with np.errstate(all="ignore"):
            for b in range(self.batch):
                for c in range(self.n_cam):
                    d = g @ mats[b, c].T
                    ok = np.isfinite(d).all(-1) & here[b, c]
                    d = np.where(ok[:, None], d, 1.0)
                    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
                    th = np.arctan2(r, d[:, 2])
                    cphi, sphi = np.where(r == 0, 1.0, d[:, 0] / r), np.where(r == 0, 0.0, d[:, 1] / r)
                    rho, tp = np.zeros_like(th), np.ones_like(th)
                    for o in range(1, int(intr[c]["poly_order"]) + 1):
                        tp = tp * th
                        rho = rho + float(intr[c]["k" + str(o)]) * tp
                    u = rho * cphi + intr[c]["cx_offset"] + w / 2.0 - 0.5
                    v = rho * sphi * intr[c]["aspect_ratio"] + intr[c]["cy_offset"] + h / 2.0 - 0.5
                    edges = np.stack((u + 0.5, w - 0.5 - u, v + 0.5, h - 0.5 - v))
                    in_theta = th <= mt[c]
                    seen = ok & in_theta & (u >= -0.5) & (u < w - 0.5) & (v >= -0.5) & (v < h - 0.5)
                    m = edges.min(0)
                    e = np.minimum(1.0, m / edge_feather) if edge_feather > 0 else np.ones_like(m)
                    wgt = (1.0 - th / mt[c]) * e
                    self.counts[b, c] = seen & (wgt > 0)
                    self.wgt[b, c] = np.where(self.counts[b, c], wgt, 0.0)
                    self.u[b, c], self.v[b, c] = np.where(seen, u, 0.0), np.where(seen, v, 0.0)
                    # does the camera see the pixel: max_theta - theta, and inside it the four edge distances, against 0
                    self.near[b, c] = ok & ((np.abs(mt[c] - th) < TIE) | (in_theta & (np.abs(edges) < TIE).any(0)))
        order = np.sort(self.wgt, axis=1)
        self.covered = self.counts.any(1)
        self.winner = np.where(self.covered, np.argmax(self.wgt, axis=1), 255).astype(np.uint8)  # the first maximum: the lowest index
        second = order[:, -2] if self.n_cam > 1 else np.zeros_like(order[:, -1])
        take = lambda t: np.take_along_axis(t, np.minimum(self.winner, self.n_cam - 1).astype(np.int64)[:, None], 1)[:, 0]  # noqa: E731
        uw, vw = take(self.u), take(self.v)
        half = (np.abs(uw + 0.5 - np.rint(uw + 0.5)) < TIE) | (np.abs(vw + 0.5 - np.rint(vw + 0.5)) < TIE)
        # near ties: a seeing decision of any camera, best minus second-best weight, the winner's nearest pick
        self.tie = self.near.any(1) | (self.covered & ((order[:, -1] - second < TIE) | half))

    def shares(self):
        return self.tie.sum() / max(self.covered.sum(), 1), self.covered.mean()

    def _at(self, plane, rows, cols):
        """plane [B, K, (C,) H, W] at (rows, cols) [B, K, n] -> [B, K, (C,) n]"""
        b, k = np.arange(self.batch)[:, None, None], np.arange(self.n_cam)[None, :, None]
        rows, cols = np.clip(rows, 0, self.h - 1).astype(np.int64), np.clip(cols, 0, self.w - 1).astype(np.int64)
        return plane[b, k, rows, cols] if plane.ndim == 4 else np.moveaxis(plane[b, k, :, rows, cols], -1, 2)

    def values(self, img):
        """per camera the bilinear value float64 [B, K, C, n]: rows and columns clamp"""
        f = img.astype(np.float64)
        i0, j0 = np.floor(self.v), np.floor(self.u)
        fy, fx = (self.v - i0)[:, :, None], (self.u - j0)[:, :, None]
        return ((1 - fy) * ((1 - fx) * self._at(f, i0, j0) + fx * self._at(f, i0, j0 + 1))
                + fy * ((1 - fx) * self._at(f, i0 + 1, j0) + fx * self._at(f, i0 + 1, j0 + 1)))

    def frame(self, img, blend):
        """un-rounded frame values float64 [B, C, n] (NaN where uncovered) and the per-camera values behind them"""
        val = self.values(img)
        if blend == "winner":
            out = np.take_along_axis(val, np.minimum(self.winner, self.n_cam - 1).astype(np.int64)[:, None, None], 1)[:, 0]
        else:
            num, den = np.zeros(val[:, 0].shape), np.zeros((self.batch, 1, self.npix))
            for c in range(self.n_cam):  # ascending c
                num = num + np.where(self.counts[:, c, None], self.wgt[:, c, None] * val[:, c], 0.0)
                den = den + self.wgt[:, c, None]
            with np.errstate(all="ignore"):
                out = num / den
        return np.where(self.covered[:, None], out, np.nan), val

    def nearest(self, plane, fill):
        """the winner's nearest image pixel of plane [B, K, H, W] -> [B, n], and per camera [B, K, n]"""
        per = self._at(plane, np.rint(self.v), np.rint(self.u))
        won = np.take_along_axis(per, np.minimum(self.winner, self.n_cam - 1).astype(np.int64)[:, None], 1)[:, 0]
        return np.where(self.covered, won, fill), per

    def candidates(self, plane, fill):
        """[B, n, K * 4 + 1]: what a near tie may return: any camera's pixel at either rounding of u and v, or the fill value"""
        eps = 2 * TIE
        cand = [self._at(plane, np.rint(self.v + dv), np.rint(self.u + du)) for dv in (-eps, eps) for du in (-eps, eps)]
        return np.concatenate([np.moveaxis(c, 1, 2) for c in cand] + [np.full((self.batch, self.npix, 1), fill, dtype=plane.dtype)], -1)


def f32_neighbours(want, got):
    """got equals float32(want) or one of its neighbouring floats; NaN where want is NaN"""
    w32 = want.astype(np.float32)
    lo, hi = np.nextafter(w32, np.float32(-np.inf)), np.nextafter(w32, np.float32(np.inf))
    return (np.isnan(want) & np.isnan(got)) | (got == w32) | (got == lo) | (got == hi)


def compare(S, cals, nside, base_pix, mats, data, blend, feather, present, max_theta_deg=95.0, what=""):
    """every output of the host entry point against the model; returns (near-tie share, covered share)"""
    img, fimg, lab, dep = data
    kw = dict(base_pix=base_pix, blend=blend, max_theta_deg=max_theta_deg, edge_feather=feather, s2_bkgd_class=BKGD, depth_fill=FILL,
              present=present)
    m = Model(cals, nside, base_pix, mats, max_theta_deg, feather, present)
    ties, covered = m.shares()
    print(f"{what}: near ties {m.tie.sum()} of {m.covered.sum()} covered pixels ({100 * ties:.3f} %), covered {100 * covered:.1f} % of the map")
    assert ties <= MAX_TIES and covered >= MIN_COVERED
    o_img, o_lab, o_dep, o_cam = S.surround_to_hp_host(cals, nside, mats, img, lab, dep, return_camera=True, **kw)
    o_fimg = S.surround_to_hp_host(cals, nside, mats, fimg, **kw)
    npix = base_pix * nside * nside
    assert o_img.dtype == np.uint8 and o_fimg.dtype == np.float32 and o_img.shape == o_fimg.shape == (len(mats), img.shape[2], npix)
    assert o_lab.dtype == o_cam.dtype == np.uint8 and o_dep.dtype == np.float32 and o_lab.shape == o_dep.shape == o_cam.shape == (len(mats), npix)
    clear = ~m.tie
    want_lab, per_lab = m.nearest(lab, BKGD)
    want_dep, per_dep = m.nearest(bits(dep), bits(np.float32(FILL))[()])
    assert np.array_equal(o_cam[clear], m.winner[clear])
    assert np.array_equal(o_lab[clear], want_lab[clear]) and np.array_equal(bits(o_dep)[clear], want_dep[clear])
    want_u8, val_u8 = m.frame(img, blend)
    want_f32, val_f32 = m.frame(fimg, blend)
    sel = np.broadcast_to(clear[:, None], want_u8.shape)
    err = np.abs(o_img.astype(np.float64) - np.where(np.isnan(want_u8), 0.0, want_u8))
    print(f"{what}: max |byte - model value| outside near ties {err[sel].max():.6f}")
    assert err[sel].max() <= 0.5 + 1e-6
    assert f32_neighbours(want_f32, o_fimg)[sel].all()
    # inside near ties: still one of the model's candidates
    if m.tie.any():
        t = m.tie
        assert ((o_cam[t][:, None] == np.arange(m.n_cam)) | (o_cam[t][:, None] == 255)).any(-1).all()
        assert (m.candidates(lab, BKGD)[t] == o_lab[t][:, None]).any(-1).all()
        assert (m.candidates(bits(dep), bits(np.float32(FILL))[()])[t] == bits(o_dep)[t][:, None]).any(-1).all()
        for out, want, val, tol in ((o_img.astype(np.float64), want_u8, val_u8, 0.5 + 1e-6), (o_fimg.astype(np.float64), want_f32, val_f32, 1e-5)):
            cand = np.concatenate((np.moveaxis(val, 1, -1), want[..., None], np.zeros_like(want)[..., None]), -1)  # [B, C, n, K + 2]
            close = (np.abs(out[..., None] - cand) <= tol + 1e-6 * np.abs(cand)).any(-1) | np.isnan(out)
            assert close[np.broadcast_to(t[:, None], close.shape)].all()
    return ties, covered


@functools.lru_cache(maxsize=None)
def rig_case(n_cam, hw, nside=8, base_pix=12, batch=3):
    """(cals, generic rotations [batch, 3, 3], planes): shared and left unchanged"""
    cals = rig_cals(hw, n_cam, 40 + n_cam)
    return cals, generic_matrices(7 * n_cam + hw[0], 2)[:batch], planes(3 * n_cam + hw[1], batch, n_cam, *hw)


# ------------------------------------------------------------------ 1. the host entry point against the model
@pytest.mark.parametrize("n_cam,hw", [(1, (60, 80)), (3, (96, 128)), (4, (60, 80))])
def test_host_entry_matches_the_numpy_model(S, n_cam, hw):
    cals, rot, data = rig_case(n_cam, hw)
    mats = rig_matrices(S, cals, rot)
    assert mats.shape == (3, n_cam, 3, 3)
    dropped = None
    if n_cam > 1:  # sample 1 without camera 0, sample 2 without the last one
        dropped = np.ones((3, n_cam), dtype=bool)
        dropped[1, 0] = dropped[2, -1] = False
    for blend in BLENDS:
        for feather in (0.0, 6.0):
            for present in ((None,) if dropped is None else (None, dropped)):
                compare(S, cals, 8, 12, mats, data, blend, feather, present,
                        what=f"K = {n_cam}, {hw}, {blend}, feather {feather}, {'all present' if present is None else 'a camera dropped'}")
    # a plane does not depend on which others are given, nor on the camera plane being asked for
    img, _, lab, dep = data
    kw = dict(blend="feather", edge_feather=6.0, present=dropped, s2_bkgd_class=BKGD, depth_fill=FILL)
    o_img, o_lab, o_dep, o_cam = S.surround_to_hp_host(cals, 8, mats, img, lab, dep, return_camera=True, **kw)
    assert np.array_equal(o_img, S.surround_to_hp_host(cals, 8, mats, img, **kw))
    assert np.array_equal(o_lab, S.surround_to_hp_host(cals, 8, mats, masks=lab, **kw))
    one = S.surround_to_hp_host(cals, 8, mats, depth=dep, return_camera=True, **kw)
    assert np.array_equal(bits(o_dep), bits(one[0])) and np.array_equal(o_cam, one[1])
    assert np.isnan(o_dep).any() and np.isinf(o_dep).any()
    part = S.surround_to_hp_host(cals, 8, mats, img, lab, dep, base_pix=8, return_camera=True, **kw)  # fewer base pixels are the first ones
    for f, p in zip((o_img, o_lab, bits(o_dep), o_cam), part):
        assert np.array_equal(p if p.dtype != np.float32 else bits(p), f[..., :512])


def test_per_camera_max_theta(S):
    cals, rot, data = rig_case(3, (96, 128))
    compare(S, cals, 8, 12, rig_matrices(S, cals, rot), data, "feather", 6.0, None, max_theta_deg=(95.0, 70.0, 110.0), what="max_theta per camera")


# ------------------------------------------------------------------ 2. one camera against the reference's own labels
@pytest.mark.parametrize("tag", ["mvl_96x128/n16_bp8_plain", "rv_60x80/n32_bp8_plain"])
def test_single_camera_reproduces_the_reference_labels(S, tag):
    from heal_swin_amd import projection as P
    g = np.load(GOLD)
    cal = calibrations()[tag.split("/")[0]]
    nside = int(tag.split("/")[1].split("_")[0][1:])
    mask, u, v, want = g[tag + "/mask"], g[tag + "/u"], g[tag + "/v"], g[tag + "/hp_mask"]
    h, w = mask.shape
    mats = rig_matrices(S, [cal], None, frame=P._camera_rotation(cal))
    assert np.abs(mats[0, 0] - np.eye(3)).max() <= 1e-15  # R^T R: the identity to rounding
    got = S.surround_to_hp_host([cal], nside, mats, masks=mask[None, None], base_pix=8, blend="winner", max_theta_deg=180.0, edge_feather=0.0,
                                s2_bkgd_class=3)
    assert got.shape == (1, want.size)

    def near(x, *marks):  # within 1e-9 of a half-integer or of a bound
        return (np.abs(x + 0.5 - np.rint(x + 0.5)) <= 1e-9) | np.any([np.abs(x - m) <= 1e-9 for m in marks], 0)

    excluded = near(u, -0.5, w - 0.5) | near(v, -0.5, h - 0.5)
    print(f"{tag}: {excluded.sum()} of {excluded.size} pixels excluded, {(want != 3).sum()} inside the image")
    assert excluded.mean() < 1e-3 and (want != 3).sum() > 100
    assert np.array_equal(got[0][~excluded], want[~excluded])


# ------------------------------------------------------------------ 3. invariants
def constant_planes(batch, n_cam, hw):
    """camera c's frame is 10 (c + 1) everywhere, its labels c + 1, its depth c + 1"""
    level = np.arange(1, n_cam + 1, dtype=np.uint8)
    img = np.broadcast_to((10 * level)[None, :, None, None, None], (batch, n_cam, 2) + tuple(hw)).copy()
    lab = np.broadcast_to(level[None, :, None, None], (batch, n_cam) + tuple(hw)).copy()
    return img, lab, lab.astype(np.float32)


@pytest.mark.parametrize("feather", [0.0, 6.0])
def test_the_winner_owns_labels_depth_and_the_winner_frame(S, feather):
    cals, rot, _ = rig_case(4, (60, 80))
    mats = rig_matrices(S, cals, rot)
    img, lab, dep = constant_planes(3, 4, (60, 80))
    kw = dict(edge_feather=feather, s2_bkgd_class=0, depth_fill=0.0, return_camera=True)
    w_img, w_lab, w_dep, cam = S.surround_to_hp_host(cals, 8, mats, img, lab, dep, blend="winner", **kw)
    covered = cam != 255
    assert covered.mean() >= MIN_COVERED and set(np.unique(cam[covered])) == {0, 1, 2, 3}
    assert np.array_equal(w_lab[covered], cam[covered] + 1) and (w_lab[~covered] == 0).all()
    assert np.array_equal(w_dep[covered], (cam[covered] + 1).astype(np.float32))
    assert np.array_equal(w_img, np.broadcast_to(np.where(covered, 10 * (cam + 1), 0)[:, None], w_img.shape))
    # the feathered frame lies between the smallest and the largest value of the counting cameras
    m = Model(cals, 8, 12, mats, 95.0, feather)
    f_img, f_lab, _, f_cam = S.surround_to_hp_host(cals, 8, mats, img, lab, dep, blend="feather", **kw)
    assert np.array_equal(f_cam, cam) and np.array_equal(f_lab, w_lab)  # the blend moves the frame only
    level = 10.0 * np.arange(1, 5)[None, :, None]
    lo, hi = np.where(m.counts, level, np.inf).min(1), np.where(m.counts, level, -np.inf).max(1)
    clear = ~m.tie & covered
    assert ((f_img[:, 0] >= lo - 0.5) & (f_img[:, 0] <= hi + 0.5))[clear].all()
    several = (m.counts.sum(1) > 1) & clear
    assert several.mean() > 0.05 and (f_img[:, 0][several] != w_img[:, 0][several]).any()  # and it does blend


def test_an_empty_sample_and_a_non_finite_matrix(S):
    cals, rot, (img, fimg, lab, dep) = rig_case(3, (96, 128))
    mats = rig_matrices(S, cals, rot)
    kw = dict(blend="feather", edge_feather=6.0, s2_bkgd_class=BKGD, depth_fill=FILL, return_camera=True)
    ref = S.surround_to_hp_host(cals, 8, mats, img, lab, dep, **kw)
    present = np.ones((3, 3), dtype=np.uint8)
    present[1] = 0  # sample 1 has no camera at all
    o_img, o_lab, o_dep, o_cam = S.surround_to_hp_host(cals, 8, mats, img, lab, dep, present=present, **kw)
    assert (o_img[1] == 0).all() and (o_lab[1] == BKGD).all() and (bits(o_dep[1]) == bits(np.float32(FILL))).all() and (o_cam[1] == 255).all()
    assert np.isnan(S.surround_to_hp_host(cals, 8, mats, fimg, present=present, **dict(kw, return_camera=False))[1]).all()
    for b in (0, 2):  # its neighbours are projected as ever
        assert all(np.array_equal(bits(o[b]) if o.dtype == np.float32 else o[b], bits(r[b]) if r.dtype == np.float32 else r[b])
                   for o, r in zip((o_img, o_lab, o_dep, o_cam), ref))
    # a NaN (or an inf) in one camera's matrix removes that camera only: the same as dropping it
    for bad_value in (np.nan, np.inf):
        bad = mats.copy()
        bad[2, 1, 1, 2] = bad_value
        drop = np.ones((3, 3), dtype=bool)
        drop[2, 1] = False
        got = S.surround_to_hp_host(cals, 8, bad, img, lab, dep, **kw)
        want = S.surround_to_hp_host(cals, 8, mats, img, lab, dep, present=drop, **kw)
        assert all(np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b) for a, b in zip(got, want))
        assert (got[3][2] != 1).all() and (ref[3][2] == 1).any() and (got[3][2] != 255).mean() >= MIN_COVERED


def test_exchanging_two_cameras_permutes_the_camera_plane_only(S):
    cals, rot, (img, fimg, lab, dep) = rig_case(4, (60, 80))
    mats = rig_matrices(S, cals, rot)
    perm = [2, 1, 0, 3]  # cameras 0 and 2 change places, with their images
    cals_p, mats_p = [cals[c] for c in perm], rig_matrices(S, [cals[c] for c in perm], rot)
    assert np.array_equal(mats_p, mats[:, perm])
    m = Model(cals, 8, 12, mats, 95.0, 6.0)
    kw = dict(edge_feather=6.0, s2_bkgd_class=BKGD, depth_fill=FILL, return_camera=True)
    a = S.surround_to_hp_host(cals, 8, mats, img, lab, dep, blend="winner", **kw)
    b = S.surround_to_hp_host(cals_p, 8, mats_p, img[:, perm], lab[:, perm], dep[:, perm], blend="winner", **kw)
    keep = ~m.tie  # a weight tie goes to the lower index, which the exchange changes
    assert m.tie.mean() <= MAX_TIES
    lut = np.full(256, 255, dtype=np.uint8)
    lut[:4] = perm  # the permutation is its own inverse
    assert np.array_equal(lut[b[3]][keep], a[3][keep]) and (b[3] != a[3]).any()
    assert np.array_equal(a[0][np.broadcast_to(keep[:, None], a[0].shape)], b[0][np.broadcast_to(keep[:, None], a[0].shape)])
    assert np.array_equal(a[1][keep], b[1][keep]) and np.array_equal(bits(a[2])[keep], bits(b[2])[keep])
    # the feathered sum runs in the other order: equal to rounding
    fa = S.surround_to_hp_host(cals, 8, mats, fimg, blend="feather", edge_feather=6.0)
    fb = S.surround_to_hp_host(cals_p, 8, mats_p, fimg[:, perm], blend="feather", edge_feather=6.0)
    assert np.array_equal(np.isnan(fa), np.isnan(fb)) and np.allclose(fa, fb, rtol=1e-6, atol=1e-6, equal_nan=True)


def symmetric_rig():
    """(cals, M [1, 4, 3, 3]): four cameras a quarter turn apart about the vehicle's z axis, equal intrinsics without offsets, exact
    matrices: pixels halfway between two optical axes have equal weights to the last bit"""
    cal = rig_cals((60, 80), 1, 0)[0]
    cal["intrinsic"].update(cx_offset=0.0, cy_offset=0.0, aspect_ratio=1.0)
    m0, rz = np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]]), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    return [cal] * 4, np.stack([m0 @ np.linalg.matrix_power(rz.T, c) for c in range(4)])[None] + 0.0


@pytest.mark.parametrize("nside", [4, 16])
def test_exact_weight_ties_go_to_the_lowest_index(S, nside):
    cals, mats = symmetric_rig()
    _, _, lab, _ = planes(5, 1, 4, 60, 80)
    perm = [3, 2, 1, 0]
    lut = np.full(256, 255, dtype=np.uint8)
    lut[:4] = perm
    cam = S.surround_to_hp_host(cals, nside, mats, masks=lab, blend="winner", edge_feather=0.0, return_camera=True)[1]
    turned = lut[S.surround_to_hp_host(cals, nside, mats[:, perm], masks=lab[:, perm], blend="winner", edge_feather=0.0, return_camera=True)[1]]
    ties = turned != cam  # with the cameras in the other order the other camera of an exact tie wins
    print(f"nside {nside}: {ties.sum()} exact ties, won by cameras {np.bincount(cam[ties], minlength=4)[:4]}")
    assert ties.sum() >= 4 and (cam[ties] < turned[ties]).all()


# ------------------------------------------------------------------ 4. the matrices
def test_matrices_are_camera_transposed_frame_augmentation(S):
    from heal_swin_amd import projection as P
    cals = rig_cals((60, 80), 4, 5)
    frame = generic_matrices(11, 1)[0]
    a = generic_matrices(12, 3)
    for f in (None, frame):
        proj = S.SurroundProjector(cals, 8, frame=f, device="cpu")
        want = np.stack([[P._camera_rotation(c).T @ (np.eye(3) if f is None else f) @ ab for c in cals] for ab in a])
        got = proj.matrices(a)
        assert got.dtype == torch.float64 and tuple(got.shape) == (6, 4, 3, 3) and np.abs(got.numpy() - want).max() <= 1e-15
        assert np.abs(proj.matrices(torch.from_numpy(a)).numpy() - want).max() <= 1e-15
        none = proj.matrices(None, 2).numpy()
        assert none.shape == (2, 4, 3, 3) and np.abs(none - np.stack([[P._camera_rotation(c).T @ (np.eye(3) if f is None else f) for c in cals]] * 2)).max() <= 1e-15
    assert proj.n_cameras == 4 and proj.npix == 768


# ------------------------------------------------------------------ 5. the back projector
@pytest.mark.parametrize("key,nside", [("rv_60x80", 8), ("mvl_96x128", 16)])
def test_back_projector_reads_each_pixels_own_direction(S, key, nside):
    from heal_swin_amd import evaluation as EV
    from heal_swin_amd import projection as P
    cal = calibrations()[key]
    h, w = int(cal["intrinsic"]["height"]), int(cal["intrinsic"]["width"])
    frame = generic_matrices(21, 1)[0]  # orthogonal
    for f, base_pix in ((None, 12), (frame, 12), (frame, 8)):
        back = S.SurroundBackProjector(cal, nside, base_pix=base_pix, frame=f, s2_bkgd_class=3, device="cpu")
        assert isinstance(back, EV.HPBackProjector) and back.shape == (h, w) and back.n_out == h * w and back.npix == base_pix * nside * nside
        assert back.nearest.dtype == back.idx.dtype == torch.int32 and back.wgt.dtype == torch.float64 and back.s2_bkgd_class == 3
        # the direction of every image pixel, turned by hand: camera frame -> vehicle frame (R_c) -> sphere's frame (F^T)
        u, v = EV.get_uv_from_hw(h, w, 1.0)
        theta, phi = EV.project_img_points_to_s2(u, v, cal)
        k = np.stack((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)), -1)
        turn = (np.eye(3) if f is None else f).T @ P._camera_rotation(cal)
        d = np.einsum("ij,hwj->hwi", turn, k)
        nearest, pix, wgt = EV.hp_nearest_pix_idcs(nside, np.arctan2(np.hypot(d[..., 0], d[..., 1]), d[..., 2]), np.arctan2(d[..., 1], d[..., 0]))
        rounding = np.sort(wgt, 0)[-1] - np.sort(wgt, 0)[-2] < 1e-9  # two pixels of equal weight: the rounding of d decides
        assert rounding.mean() < 1e-3
        assert np.array_equal(back.nearest.numpy()[~rounding], nearest[~rounding])
        assert np.array_equal(back.valid.numpy(), back.nearest.numpy() < back.npix) and back.valid.any()
        # and the way round: a sphere painted with its own pixel indices reads back, at every valid image pixel, the pixel of that direction
        own = np.arange(back.npix)
        valid = back.valid.numpy() & ~rounding
        assert np.array_equal(own[back.nearest.numpy()[valid]], nearest[valid])
    assert not S.SurroundBackProjector(cal, nside, base_pix=8, frame=frame, device="cpu").valid.all()


def test_back_projector_undoes_the_projector(S):
    """a camera's label image, projected by the rig and read back through that camera's back projector, is itself wherever that
    camera won (image pixels are several HEALPix pixels apart at this size, so the round trip lands in the same image pixel)"""
    cals = rig_cals((60, 80), 3, 9)
    nside = 64
    lab = (np.arange(60 * 80).reshape(60, 80) // 7 % 251).astype(np.uint8)
    labs = np.stack([lab, lab[::-1], lab[:, ::-1]])[None]
    mats = rig_matrices(S, cals, None)
    hp, cam = S.surround_to_hp_host(cals, nside, mats, masks=labs, blend="winner", edge_feather=0.0, s2_bkgd_class=255, return_camera=True)
    for c in range(3):
        back = S.SurroundBackProjector(cals[c], nside, device="cpu")
        nearest = back.nearest.numpy()
        mine = cam[0][nearest] == c
        assert mine.mean() > 0.2
        agree = hp[0][nearest][mine] == labs[0, c][mine]
        print(f"camera {c}: {mine.sum()} image pixels won, {agree.mean() * 100:.2f} % read their own label back")
        assert agree.mean() > 0.97  # the rest sit on a label boundary within one HEALPix pixel


# ------------------------------------------------------------------ 6. refusals
def test_every_refusal_of_the_c_abi_leaves_the_outputs_untouched(S):
    """Every refusal is HS_ERR_INVALID_ARG (1), decided on the host before anything is launched or written: the pointers name
    host memory no kernel could read, and the guard pattern of the outputs survives."""
    from heal_swin_amd._lib import HS_F32, HS_U8, lib

    buf = (ctypes.c_ubyte * (1 << 17))(*([0xA5] * (1 << 17)))
    base = ctypes.addressof(buf)
    at = lambda off: ctypes.c_void_p(base + off)  # noqa: E731
    # nside 4, 8 base pixels, batch 2, 2 cameras, 3 channels, 5 x 7: inputs of 420 / 140 / 560 bytes, outputs of 768 / 256 / 1024 / 256
    img, img_out, lab, lab_out, dep, dep_out, cam_out, rot, here = at(0), at(4096), at(8192), at(12288), at(16384), at(20480), at(24576), at(32768), at(40960)
    cals = rig_cals((5, 7), 2, 1)

    def rig(**kw):
        r = S._rig(cals, "feather", 95.0, 2.0)
        for k, val in kw.items():
            if k in ("n_cameras", "edge_feather", "blend"):
                setattr(r, k, val)
            elif k == "max_theta":
                r.max_theta[1] = val
            else:
                setattr(r.cam[1], k, val)
        return r

    def call(fn, nside=4, npix=128, rig=rig(), rot=rot, present=here, batch=2, height=5, width=7, frame=img, kind=HS_U8, channels=3,
             frame_out=img_out, labels=lab, labels_out=lab_out, background=0, depth=dep, depth_out=dep_out, fill=0.0, camera=cam_out):
        args = (nside, npix, rig, rot, present, batch, height, width, frame, kind, channels, frame_out, labels, labels_out, background, depth,
                depth_out, fill, camera)
        return fn(*args, None) if fn is lib.hs_surround_to_hp else fn(*args)

    none = dict(frame=None, frame_out=None, labels=None, labels_out=None, depth=None, depth_out=None)
    refused = (dict(nside=3), dict(nside=0), dict(nside=-4), dict(nside=16384, npix=12 * 16384 * 16384), dict(npix=0), dict(npix=-16), dict(npix=13 * 16),
               dict(npix=100), dict(npix=8), dict(batch=0), dict(batch=-3), dict(batch=65536), dict(rig=rig(n_cameras=0)), dict(rig=rig(n_cameras=9)),
               dict(rig=rig(n_cameras=-1)), dict(rig=rig(poly_order=0)), dict(rig=rig(poly_order=9)), dict(rig=rig(width=8)), dict(rig=rig(height=4)),
               dict(height=6), dict(width=6), dict(rig=rig(max_theta=0.0)), dict(rig=rig(max_theta=-1.0)), dict(rig=rig(max_theta=3.1415926535897936)),
               dict(rig=rig(max_theta=float("nan"))), dict(rig=rig(max_theta=float("inf"))), dict(rig=rig(edge_feather=-1e-9)),
               dict(rig=rig(edge_feather=float("nan"))), dict(rig=rig(edge_feather=float("inf"))), dict(rig=rig(blend=2)), dict(rig=rig(blend=-1)),
               dict(channels=0), dict(channels=17), dict(kind=HS_F32 + 1), dict(kind=9), dict(frame=None), dict(frame_out=None), dict(labels=None),
               dict(labels_out=None), dict(depth=None), dict(depth_out=None), dict(none), dict(none, camera=cam_out),
               dict(frame_out=img), dict(labels_out=lab), dict(depth_out=dep), dict(camera=lab), dict(frame_out=at(400)), dict(frame=at(4096 + 700)),
               dict(labels_out=dep), dict(depth_out=at(8192 + 64)), dict(frame_out=at(8192 - 700)), dict(labels_out=at(32768 + 100)),
               dict(camera=at(32768 + 280)), dict(camera=at(40960 + 3)), dict(depth_out=at(40960 - 1020)), dict(kind=HS_F32, frame_out=at(16384 - 3000)),
               dict(background=-1), dict(background=256), dict(rot=None), dict(rig=None))
    big = rig()  # height width >= 2^31 (Python refuses to build such a rig)
    for c in range(2):
        big.cam[c].height = big.cam[c].width = 46341
    refused += (dict(rig=big, height=46341, width=46341, **none), dict(rig=big, height=46341, width=46341, labels=lab, labels_out=lab_out,
                                                                      **{k: None for k in ("frame", "frame_out", "depth", "depth_out")}))
    for fn in (lib.hs_surround_to_hp, lib.hs_surround_to_hp_host):
        for kw in refused:
            assert call(fn, **kw) == 1, (fn.__name__, kw)
            assert lib.hs_last_error()
    assert bytes(buf) == b"\xa5" * (1 << 17)
    # the smallest call passes: one pixel, one camera with a 1 x 1 image that the pole looks into
    cal = rig_cals((1, 1), 1, 3)
    cal[0]["intrinsic"].update(cx_offset=0.0, cy_offset=0.0)
    one = S.surround_to_hp_host(cal, 1, np.eye(3)[None, None], masks=np.full((1, 1, 1, 1), 9, dtype=np.uint8), base_pix=1, max_theta_deg=180.0,
                                edge_feather=0.0, s2_bkgd_class=4)
    assert one.shape == (1, 1) and one[0, 0] in (4, 9)


def test_python_argument_checks(S):
    """Everything is checked before anything touches the device, so the refusals need none."""
    cals = rig_cals((5, 7), 2, 1)
    order9 = [cals[0], dict(cals[1], intrinsic=dict(cals[1]["intrinsic"], poly_order=9, **{f"k{i}": 0.0 for i in range(5, 10)}))]
    other = [cals[0], dict(cals[1], intrinsic=dict(cals[1]["intrinsic"], width=8.0))]
    for kw in (dict(nside=3), dict(nside=0), dict(nside=16384), dict(base_pix=0), dict(base_pix=13), dict(s2_bkgd_class=256), dict(s2_bkgd_class=-1),
               dict(cal_infos=[]), dict(cal_infos=cals * 5), dict(cal_infos=order9), dict(cal_infos=other), dict(frame=np.eye(4)),
               dict(frame=np.full((3, 3), np.nan)), dict(blend="mean"), dict(blend=1), dict(max_theta_deg=0.0), dict(max_theta_deg=-5.0),
               dict(max_theta_deg=180.1), dict(max_theta_deg=float("nan")), dict(max_theta_deg=(90.0, 95.0, 95.0)), dict(max_theta_deg=(90.0, 0.0)),
               dict(edge_feather=-1.0), dict(edge_feather=float("nan")), dict(edge_feather=float("inf")), dict(used_size=(46341, 46341))):
        with pytest.raises(ValueError):
            S.SurroundProjector(**dict(dict(cal_infos=cals, nside=4, device="cpu"), **kw))
    assert S.SurroundProjector(other, 4, used_size=(5, 7), device="cpu").n_cameras == 2  # used_size gives the rig its one size
    with pytest.raises(ValueError):
        S.SurroundBackProjector(cals[0], 3, device="cpu")
    with pytest.raises(ValueError):
        S.SurroundBackProjector(cals[0], 4, frame=np.eye(2), device="cpu")
    proj = S.SurroundProjector(cals, 4, max_theta_deg=(90.0, 180.0))  # names the device without touching it
    assert proj.npix == 192 and proj.depth_fill == 0.0 and S.SurroundProjector(cals, 4, s2_bkgd_class=7, device="cpu").depth_fill == 7.0
    a = generic_matrices(3, 1)
    img, mask, depth = torch.zeros(2, 2, 3, 5, 7, dtype=torch.uint8), torch.zeros(2, 2, 5, 7, dtype=torch.uint8), torch.zeros(2, 2, 5, 7)
    with pytest.raises(ValueError, match="at least one"):
        proj(rotations=a)
    for kw, err in ((dict(imgs=img.double()), TypeError), (dict(imgs=img.long()), TypeError), (dict(masks=mask.long()), TypeError),
                    (dict(depth=depth.double()), TypeError), (dict(depth=mask), TypeError), (dict(imgs=img, masks=mask[..., :4]), ValueError),
                    (dict(imgs=img, depth=depth[:1]), ValueError), (dict(imgs=img[None]), ValueError), (dict(masks=mask[0, 0]), ValueError),
                    (dict(imgs=torch.zeros(2, 2, 17, 5, 7, dtype=torch.uint8)), ValueError), (dict(imgs=torch.zeros(2, 2, 0, 5, 7, dtype=torch.uint8)), ValueError),
                    (dict(imgs=img[0], masks=mask), ValueError), (dict(imgs=img[:, :1]), ValueError), (dict(masks=torch.zeros(2, 3, 5, 7, dtype=torch.uint8)), ValueError),
                    (dict(masks=torch.zeros(2, 2, 7, 5, dtype=torch.uint8)), ValueError), (dict(imgs=img, rotations=a[:1]), ValueError),
                    (dict(imgs=img, rotations=np.eye(3)), ValueError), (dict(imgs=img, present=np.ones((2, 3), bool)), ValueError),
                    (dict(imgs=img, present=np.ones((3, 2), bool)), ValueError), (dict(imgs=img, present=np.ones((2, 2), np.float32)), TypeError),
                    (dict(imgs=img, present=torch.ones(2, 2, dtype=torch.int64)), TypeError)):
        with pytest.raises(err):
            proj(**kw)
    for kw in (dict(imgs=img), dict(imgs=img.float()), dict(masks=mask), dict(depth=depth), dict(imgs=img, masks=mask, depth=depth, present=np.ones((2, 2), bool))):
        with pytest.raises(RuntimeError, match="GPU tensor"):  # well-formed calls still need the device: there is no CPU path
            proj(**kw)
    m = rig_matrices(S, cals, a)
    for args, kw in (((cals, 4, m, img.numpy()[0]), {}), ((cals, 4, m[:1], img.numpy()), {}), ((cals, 4, m[:, :1], img.numpy()), {}), ((cals, 4, m[0], img.numpy()), {}),
                     ((cals, 4, m), {}), ((cals, 4, m, img.numpy()), dict(present=np.ones((2, 3), bool))), ((cals, 4, m, img.numpy()), dict(blend="both")),
                     ((cals, 4, m, img.numpy()), dict(base_pix=13)), ((cals, 5, m, img.numpy()), {})):
        with pytest.raises(ValueError):
            S.surround_to_hp_host(*args, **kw)
    with pytest.raises(TypeError):
        S.surround_to_hp_host(cals, 4, m, img.numpy().astype(np.int32))
