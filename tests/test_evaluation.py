"""Host side of heal_swin_amd.evaluation (no GPU): the back-projection geometry against the reference's own outputs
(tests/golden/backprojection.npz, made by make_golden_backprojection.py), healpy's get_interp_weights against a
restatement built on the oracle's pixel centres, and the metric formulas on a hand-computed confusion matrix."""
import math

import numpy as np
import pytest
import torch

from _golden import load


@pytest.fixture(scope="module")
def E():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import evaluation
    return evaluation


def _cals():
    from tests.test_projection import calibrations  # the three WoodScape-like calibrations of the fixtures, read as data
    return calibrations()


# ------------------------------------------------------------------ image plane -> S^2 against the reference
def test_get_uv_from_hw_bit_equal(E):
    z = load("backprojection")
    fv = _cals()["fv_966x1280"]["intrinsic"]
    names = sorted({k.split("/")[1] for k in z.files if k.startswith("uv/")})
    assert names == ["float", "int", "tuple"]
    for name in names:
        raw, kind = z[f"uv/{name}/res"], str(z[f"uv/{name}/kind"])
        res = {"float": lambda r: float(r[0]), "int": lambda r: int(r[0]), "tuple": lambda r: tuple(int(x) for x in r)}[kind](raw)
        u, v = E.get_uv_from_hw(fv["height"], fv["width"], res)
        assert np.array_equal(u, z[f"uv/{name}/u"]) and np.array_equal(v, z[f"uv/{name}/v"]), name
    # the int branch keeps the long side at full size: int(1280 * 40) // 40
    assert E.get_uv_from_hw(966, 1280, 40)[0].shape == (40, 1280)
    with pytest.raises(TypeError):
        E.get_uv_from_hw(966, 1280, "full")


@pytest.mark.parametrize("key", ["fv_966x1280", "mvl_96x128", "rv_60x80"])
@pytest.mark.parametrize("rot", ["plain", "rot"])
def test_project_img_points_to_s2_matches_reference(E, key, rot):
    z = load("backprojection")
    cal = _cals()[key]
    intr = cal["intrinsic"]
    cases = [("small", tuple(int(x) for x in z[f"s2/{key}/small_{rot}/res"]), None)]
    if key == "fv_966x1280":
        cases.append(("full", 1.0, int(z[f"s2/{key}/full_{rot}/step"])))
    for name, res, step in cases:
        u, v = E.get_uv_from_hw(intr["height"], intr["width"], res)
        theta, phi = E.project_img_points_to_s2(u, v, cal, rot == "rot")
        if step:
            theta, phi = theta[::step, ::step], phi[::step, ::step]
        ref_t, ref_p = z[f"s2/{key}/{name}_{rot}/theta"], z[f"s2/{key}/{name}_{rot}/phi"]
        assert theta.shape == ref_t.shape
        assert np.abs(theta - ref_t).max() <= 1e-6, (name, np.abs(theta - ref_t).max())
        if rot == "plain":
            assert np.array_equal(phi, ref_p), name
            assert phi.min() >= 0 and phi.max() < 2 * np.pi
        else:
            assert np.abs(phi - ref_p).max() <= 1e-6, (name, np.abs(phi - ref_p).max())


# ------------------------------------------------------------------ get_interp_weights
class _RingTable:
    """Ring layout read off the oracle's pixel centres: first pixel, pixel count and centre colatitude of every ring, and
    the longitude of every ring pixel (oracle.healpix.pix2ang_ring), nothing from closed-form ring formulas."""

    def __init__(self, nside):
        from oracle.healpix import pix2ang_ring

        self.nside, self.npix = nside, 12 * nside * nside
        self.theta, self.phi = pix2ang_ring(nside, np.arange(self.npix))
        starts = np.flatnonzero(np.r_[True, self.theta[1:] != self.theta[:-1]])
        assert len(starts) == 4 * nside - 1
        self.start = {r + 1: int(s) for r, s in enumerate(starts)}
        ends = np.r_[starts[1:], self.npix]
        self.count = {r + 1: int(e - s) for r, (s, e) in enumerate(zip(starts, ends))}

    def ring(self, r):
        sp = self.start[r]
        return sp, self.count[r], float(self.theta[sp])


def _fmodulo(v, m):
    if v >= 0:
        return v if v < m else math.fmod(v, m)
    t = math.fmod(v, m) + m
    return 0.0 if t == m else t


def _interp_ref(tab, theta, phi):
    """HEALPix get_interpol restated on the oracle's ring table; returns RING indices and weights [4]."""
    from oracle.healpix import ring2nest

    ns = tab.nside
    phi = _fmodulo(phi, 2 * math.pi)
    z = math.cos(theta)
    if abs(z) <= 2.0 / 3.0:  # ring_above: which two rings bracket theta (the decision rule itself is HEALPix's)
        ir1 = int(ns * (2 - 1.5 * z))
    else:
        r = int(ns * math.sqrt(3 * (1 - abs(z))))
        ir1 = r if z > 0 else 4 * ns - r - 1
    ir2 = ir1 + 1
    pix, wgt, th = [0] * 4, [0.0] * 4, [0.0, 0.0]

    def bracket(ring, slot):
        sp, nr, th_r = tab.ring(ring)
        dphi = 2 * math.pi / nr
        phase0 = float(tab.phi[sp])  # 0 or dphi / 2: the ring's phase shift
        shift = 0.5 if phase0 > 0.25 * dphi else 0.0
        t = phi / dphi - shift
        i1 = int(t) - 1 if t < 0 else int(t)
        ph1 = float(tab.phi[sp + (i1 % nr)]) + (2 * math.pi if i1 >= nr else 0.0) - (2 * math.pi if i1 < 0 else 0.0)
        w1 = (phi - ph1) / dphi
        pix[slot], pix[slot + 1] = sp + i1 % nr, sp + (i1 + 1) % nr
        wgt[slot], wgt[slot + 1] = 1 - w1, w1
        th[slot // 2] = th_r

    if ir1 > 0:
        bracket(ir1, 0)
    if ir2 < 4 * ns:
        bracket(ir2, 2)
    if ir1 == 0:
        wt = theta / th[1]
        fac = (1 - wt) * 0.25
        wgt = [fac, fac, wgt[2] * wt + fac, wgt[3] * wt + fac]
        pix[0], pix[1] = (pix[2] + 2) & 3, (pix[3] + 2) & 3
    elif ir2 == 4 * ns:
        wt = (theta - th[0]) / (math.pi - th[0])
        fac = wt * 0.25
        wgt = [wgt[0] * (1 - wt) + fac, wgt[1] * (1 - wt) + fac, fac, fac]
        pix[2], pix[3] = (pix[0] + 2) % 4 + tab.npix - 4, (pix[1] + 2) % 4 + tab.npix - 4
    else:
        wt = (theta - th[0]) / (th[1] - th[0])
        wgt = [wgt[0] * (1 - wt), wgt[1] * (1 - wt), wgt[2] * wt, wgt[3] * wt]
    return ring2nest(ns, np.array(pix)), np.array(wgt)


def _directions(tab, rng):
    ns = tab.nside
    two3 = math.acos(2.0 / 3.0)
    thetas = [0.0, math.pi, two3, math.pi - two3, math.nextafter(two3, 0), math.nextafter(two3, 4),
              math.acos(-2.0 / 3.0), 1e-9, math.pi - 1e-9, 0.5 * tab.ring(1)[2], math.pi - 0.5 * tab.ring(1)[2], math.pi / 2]
    rings = range(1, 4 * ns) if ns <= 16 else sorted({1, 2, ns - 1, ns, ns + 1, 2 * ns, 3 * ns - 1, 3 * ns, 3 * ns + 1, 4 * ns - 1,
                                                      *rng.integers(1, 4 * ns, 24).tolist()})
    thetas += [tab.ring(r)[2] for r in rings]  # exact ring centres
    phis = [0.0, math.nextafter(2 * math.pi, 0), 2 * math.pi, -1e-12, -0.3, -3.0, -2 * math.pi + 0.01, -7.0, 7.0, math.pi / 4, 1.234]
    out = [(t, p) for t in thetas for p in phis]
    for r in list(rings)[:: max(1, len(rings) // 8)]:  # exact pixel centres of some rings
        sp, nr, th = tab.ring(r)
        out += [(th, float(tab.phi[sp + j])) for j in range(0, nr, max(1, nr // 7))]
    out += list(zip(np.arccos(rng.uniform(-1, 1, 200)).tolist(), rng.uniform(-2 * np.pi, 4 * np.pi, 200).tolist()))
    return np.array(out)


@pytest.mark.parametrize("nside", [1, 2, 4, 16, 256])
def test_interp_weights_match_restatement(E, nside):
    from oracle.healpix import nest2ring

    tab = _RingTable(nside)
    d = _directions(tab, np.random.default_rng(nside))
    pix, wgt = E.get_interp_weights(nside, d[:, 0], d[:, 1])
    assert pix.shape == (4, len(d)) and wgt.shape == (4, len(d))
    for k, (t, p) in enumerate(d):
        ref_pix, ref_w = _interp_ref(tab, t, p)
        assert np.array_equal(pix[:, k], ref_pix), (nside, t, p, nest2ring(nside, pix[:, k]), nest2ring(nside, ref_pix))
        assert np.abs(wgt[:, k] - ref_w).max() <= 1e-12, (nside, t, p, wgt[:, k], ref_w)
    assert np.abs(wgt.sum(0) - 1).max() <= 1e-12
    assert wgt.min() >= -1e-12 and wgt.max() <= 1 + 1e-12  # HEALPix's own rounding at pixel centres: w1 = -1e-15
    assert pix.min() >= 0 and pix.max() < 12 * nside * nside


@pytest.mark.parametrize("nside", [1, 2, 4, 16])
def test_pixel_centre_gets_full_weight(E, nside):
    from oracle.healpix import pix2ang_nest

    ipix = np.arange(12 * nside * nside)
    theta, phi = pix2ang_nest(nside, ipix)
    pix, wgt = E.get_interp_weights(nside, theta, phi)
    own = np.where(pix == ipix[None], wgt, 0.0).sum(0)
    assert np.abs(own - 1).max() <= 1e-9
    nearest, _, _ = E.hp_nearest_pix_idcs(nside, theta, phi)
    assert np.array_equal(nearest, ipix)


def test_interp_weights_known_answer(E):
    """nside 1, centre of RING pixel 0 (theta = acos(2/3), phi = pi/4): ring 1 brackets it at its own pixel 0 (and 1 with
    weight 0), ring 2 at pixels 4, 5; theta sits on ring 1, so everything goes to pixel 0."""
    from heal_swin_amd import _lib

    pix, wgt = E.get_interp_weights(1, np.array([math.acos(2.0 / 3.0)]), np.array([math.pi / 4]))
    assert _lib.nest2ring(1, pix[:, 0]).tolist() == [0, 1, 4, 5]
    assert np.allclose(wgt[:, 0], [1, 0, 0, 0], rtol=0, atol=1e-15)


def test_interp_weights_reject_bad_input(E):
    for theta in (-1e-3, math.pi + 1e-3, float("nan")):
        with pytest.raises(AssertionError, match="theta"):
            E.get_interp_weights(4, np.array([0.5, theta]), np.array([0.1, 0.2]))
    with pytest.raises(AssertionError):
        E.get_interp_weights(4, np.array([0.5]), np.array([float("inf")]))
    for nside in (0, 3, -4):
        with pytest.raises(AssertionError, match="nside"):
            E.get_interp_weights(nside, np.array([0.5]), np.array([0.1]))
    with pytest.raises(ValueError):
        E.get_interp_weights(4, np.zeros(3), np.zeros(4))


# ------------------------------------------------------------------ metrics from the matrix
def test_metric_formulas_hand_computed(E):
    """rows = target, columns = prediction:
            pred 0  1  2
        t0 [     5, 1, 0]
        t1 [     2, 3, 1]
        t2 [     0, 0, 0]      class 2 never occurs, never predicted: union 0 -> absent_score
    IoU_0 = 5 / (6 + 7 - 5) = 5/8, IoU_1 = 3 / (6 + 4 - 3) = 3/7, IoU_2 = 0 / (0 + 1 - 0) = 0 (predicted once);
    acc = 8 / 12; acc(ignore 0) = 3 / 6."""
    m = E.SegConfusion(3, device="cpu")
    m.confmat.copy_(torch.tensor([[5, 1, 0], [2, 3, 1], [0, 0, 0]]))
    assert torch.equal(m.iou(), torch.tensor([5 / 8, 3 / 7, 0.0], dtype=torch.float32))
    assert m.accuracy().item() == pytest.approx(8 / 12, abs=1e-7)
    assert m.accuracy(ignore_index=0).item() == pytest.approx(3 / 6, abs=1e-7)
    m.confmat.copy_(torch.tensor([[5, 1, 0], [2, 3, 0], [0, 0, 0]]))
    iou = m.iou(absent_score=float("nan"))
    assert iou[:2].tolist() == pytest.approx([5 / 8, 3 / 6]) and math.isnan(iou[2].item())  # class 2 now absent everywhere
    assert m.iou()[2].item() == 0.0
    m.reset()
    assert int(m.confmat.abs().sum()) == 0
    with pytest.raises(ValueError):
        E.SegConfusion(65, device="cpu")


@pytest.mark.parametrize("rot", ["plain", "rot"])
def test_nearest_table_from_reference_theta_differs_only_at_near_ties(E, rot):
    """The nearest-pixel table at nside 256 from this library's (theta, phi) and from the reference's (the fixture's
    subsampled full-size FV grid): a pixel may differ only where its two largest weights are within 1e-3 of each other."""
    import conftest

    z = load("backprojection")
    cal = _cals()["fv_966x1280"]
    step = int(z[f"s2/fv_966x1280/full_{rot}/step"])
    u, v = E.get_uv_from_hw(966, 1280, 1.0)
    theta, phi = E.project_img_points_to_s2(u, v, cal, rot == "rot")
    ours, _, _ = E.hp_nearest_pix_idcs(256, theta[::step, ::step], phi[::step, ::step])
    ref, _, wgt = E.hp_nearest_pix_idcs(256, z[f"s2/fv_966x1280/full_{rot}/theta"], z[f"s2/fv_966x1280/full_{rot}/phi"])
    differ = ours != ref
    top2 = np.sort(wgt, axis=0)[-2:]
    assert np.all((top2[1] - top2[0])[differ] <= 1e-3)
    conftest.NOTES.append(f"nearest table, FV 966x1280 every {step}th pixel, nside 256, {rot}: {int(differ.sum())} of {differ.size} "
                          "pixels differ between this library's theta and the reference's")
