"""heal_swin_amd.depth_evaluation, host side: the extrinsic rotation, the direction tables and the used_size angles against
the reference's own outputs (tests/golden/depth_eval.npz, made by make_golden_depth_eval.py), and a numpy restatement of
the depth metrics against the reference metric classes' values.  No GPU needed."""
import math

import numpy as np
import pytest

from _golden import load


@pytest.fixture(scope="module")
def D():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import depth_evaluation
    return depth_evaluation


def _cal(key):
    from tests.test_projection import calibrations
    return calibrations()[key]


def _ulps(a, b):
    """Distance in fp32 ulps of b from a (both fp32)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


# ------------------------------------------------------------------ metrics restated in numpy (the kernel's semantics)
def metrics_ref(pred, target, total_mean, ranges, use_logvar):
    """Per-element values in the inputs' type (fp32), every sum in float64: what hs_depth_metrics computes."""
    p = pred[:, 0].reshape(-1) if pred.ndim == target.ndim + 1 else pred.reshape(-1)
    t = target.reshape(-1)
    f64 = np.float64
    with np.errstate(all="ignore"):
        sel = np.isfinite(p) & np.isfinite(t)
        d = p[sel].astype(f64) - t[sel].astype(f64)
        n = sel.sum()
        tm = f64(np.float32(total_mean))
        out = {"mse": (d * d).sum() / n, "mean_pred_dist": p[sel].astype(f64).sum() / n,
               "RelSE": (d * d).sum() / ((tm - t[sel]) ** 2).sum(), "RelAE": np.abs(d).sum() / np.abs(tm - t[sel]).sum()}
        ip = p.dtype.type(1) / (p.dtype.type(0.001) * p)  # each in its own type, as the reference's tensors
        it = t.dtype.type(1) / (t.dtype.type(0.001) * t)
        s = np.isfinite(ip) & np.isfinite(it)
        out["iRMSE"] = math.sqrt(((ip[s].astype(f64) - it[s]) ** 2).sum() / s.sum())
        s = sel & (p > 0) & (t > 0)
        dl = np.log(t[s]).astype(f64) - np.log(p[s])
        out["SILogE"] = (dl * dl).sum() / s.sum() - dl.sum() ** 2 / s.sum() ** 2
        for name, (lo, hi) in ranges.items():
            r = sel & (np.float32(lo) <= t) & (t < np.float32(hi))
            e = p[r].astype(f64) - t[r]
            out[name] = (e * e).sum() / r.sum() if r.sum() else 0.0
        if use_logvar:
            lv = pred[:, 1].reshape(-1)
            s = ~np.isnan(t) & (t != np.inf)
            out["mean_std"] = np.sqrt(np.exp(lv[s])).astype(f64).sum() / s.sum()
            stds = np.sqrt(np.exp(pred[:, 1].reshape(pred.shape[0], -1)))
            srt = np.sort(stds, axis=1)
            out["median_std"] = srt[:, (srt.shape[1] - 1) // 2].astype(f64).mean()  # torch's lower median
    return out


GOLDEN_RANGES = {"mse_range_000_005": (0, 5), "mse_range_020_100": (20, 100), "mse_range_005_300": (5, 300),
                 "mse_range_500_600": (500, 600), "range_hi_tuple": (-np.inf, 10), "range_hi_scalar": (-np.inf, 50.0)}


@pytest.mark.parametrize("tag", ["hp", "img"])
def test_metric_restatement_matches_reference(tag):
    g = load("depth_eval")
    pred, target = g[f"metrics/{tag}/pred"], g[f"metrics/{tag}/target"]
    half = pred.shape[0] // 2
    got = metrics_ref(pred, target, float(g["metrics/total_mean"]), GOLDEN_RANGES, True)
    for name, v in got.items():
        want = float(g[f"metrics/{tag}/{name}"])
        assert v == pytest.approx(want, rel=1e-5, abs=0), (tag, name, v, want)
    assert half >= 1


def test_range_names_and_bounds(D):
    names = D.range_names([(0, 5), (20, 100), (5, 300), (500, 600)])
    assert names == ["mse_range_000_005", "mse_range_020_100", "mse_range_005_300", "mse_range_500_600"]
    assert D.range_names([(10,)]) == ["mse_range__neg_inf_10"]
    assert D._range_bounds((10,)) == (-math.inf, 10.0)
    assert D._range_bounds(50.0) == (-math.inf, 50.0)
    assert D._range_bounds((100, 20)) == (20.0, 100.0)
    with pytest.raises(ValueError):
        D._range_bounds((1, 2, 3))


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize("key", ["fv_966x1280", "mvl_96x128", "rv_60x80"])
def test_extrinsic_rotation_matches_scipy(D, key):
    r = D.extrinsic_rotation(_cal(key))
    np.testing.assert_allclose(r, load("depth_eval")[f"rot/{key}"], rtol=0, atol=1e-15)


def _hp_cases(g):
    return sorted({k.rsplit("/", 1)[0] for k in g.files if k.startswith("hp/")})


def test_hp_direction_table_gives_reference_points(D):
    g = load("depth_eval")
    cases = _hp_cases(g)
    assert len(cases) == 3
    for tag in cases:
        _, key, ns = tag.split("/")
        nside, bp = (int(x) for x in ns[1:].split("_bp"))
        theta, phi = D.hp_ray_angles(nside, bp)
        dirs = D.directions(theta, phi, D.extrinsic_rotation(_cal(key)))
        depth, keep = g[tag + "/depth"], g[tag + "/keep"]
        np.testing.assert_array_equal(np.isfinite(depth), keep)  # NaN / inf dropped, 1000 and 0 kept by the plain rule
        pts = (depth[keep].astype(np.float64) * dirs[:, keep]).T.astype(np.float32)
        ref = g[tag + "/points"]
        assert pts.shape == ref.shape
        u = _ulps(ref, pts)
        assert (u <= 1).all() or (np.abs(pts - ref) <= 1e-14 * np.abs(depth[keep])[:, None] + (u <= 1)).all(), (tag, u.max())


@pytest.mark.parametrize("key", ["mvl_96x128", "rv_60x80"])
@pytest.mark.parametrize("rot", ["plain", "rot"])
def test_image_ray_angles_with_used_size(D, key, rot):
    g = load("depth_eval")
    tag = f"img/{key}/{rot}"
    h, w = g[tag + "/depth"].shape
    theta, phi = D.image_ray_angles(_cal(key), h, w, rot == "rot")
    np.testing.assert_allclose(theta, g[tag + "/theta"], rtol=0, atol=1e-6)
    dphi = np.angle(np.exp(1j * (phi - g[tag + "/phi"])))
    assert np.abs(dphi).max() <= 1e-6 * 4
    # the image is a downscaled frame: without the rescale the angles would be far off
    from heal_swin_amd.evaluation import get_uv_from_hw, project_img_points_to_s2
    u, v = get_uv_from_hw(h, w, (h, w))
    theta0, _ = project_img_points_to_s2(u, v, _cal(key), rot == "rot")
    assert np.abs(theta0 - g[tag + "/theta"]).max() > 1e-2


def test_used_size_none_is_todays_behaviour():
    from heal_swin_amd.evaluation import get_uv_from_hw, project_img_points_to_s2
    cal = _cal("rv_60x80")
    u, v = get_uv_from_hw(60, 80, 1.0)
    a = project_img_points_to_s2(u, v, cal, True)
    b = project_img_points_to_s2(u, v, cal, True, used_size=(60, 80))
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("key", ["mvl_96x128", "rv_60x80"])
@pytest.mark.parametrize("rot", ["plain", "rot"])
def test_image_points_match_reference(D, key, rot):
    """fp32(d * R u) on the host against the reference's clouds: |d| 1e-6 (the theta solver) plus one ulp."""
    g = load("depth_eval")
    tag = f"img/{key}/{rot}"
    depth, keep = g[tag + "/depth"], g[tag + "/keep"]
    h, w = depth.shape
    theta, phi = D.image_ray_angles(_cal(key), h, w, rot == "rot")
    dirs = D.directions(theta, phi, D.extrinsic_rotation(_cal(key)))
    k = keep.reshape(-1)
    np.testing.assert_array_equal(np.isfinite(depth.reshape(-1)), k)
    d = depth.reshape(-1)[k].astype(np.float64)
    pts = (d * dirs[:, k]).T.astype(np.float32)
    ref = g[tag + "/points"]
    tol = np.abs(d)[:, None] * 1e-6 + np.spacing(np.abs(ref))
    assert (np.abs(pts.astype(np.float64) - ref) <= tol).all()


def test_background_values(D):
    assert D._background_values((float("nan"), float("inf"))).size == 0
    np.testing.assert_array_equal(D._background_values((float("nan"), float("inf"), 1000)), np.array([1000], np.float32))
    with pytest.raises(ValueError):
        D._background_values((1, 2, 3, 4, 5))
