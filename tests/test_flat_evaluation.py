"""heal_swin_amd.flat_evaluation, host side: the flat-to-HEALPix tables against the reference's own sampled index images
(tests/golden/flat_eval.npz, made by make_golden_flat_eval.py), the row layout, the bilinear taps against torch's interpolate, a
numpy restatement of the projected depth and its metrics against the reference's values, and argument validation.  No GPU
needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _flat_cases import FLAT_MODEL_CASES
from _golden import load
from test_depth_evaluation import _cal, metrics_ref

# golden case -> (calibration, flat model case whose patch size and tile the rows layout takes, or None: image layout only)
CASES = {"identity": ("rv_60x80", None), "resize_pad_plain": ("mvl_96x128", "b_w8_p2_cos_v2"),
         "resize_pad_rot": ("mvl_96x128", "b_w8_p2_cos_v2"), "bp12": ("rv_60x80", "a_w4_p2_v1")}
DEPTH_CASES = ["resize_pad_plain", "resize_pad_rot"]
TAP_EPS = 4 * 2.0 ** -24  # four fp32 products and three adds, each within 2^-24 of max |tap| (the weights sum to at most 1)


@pytest.fixture(scope="module")
def FE():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import flat_evaluation
    return flat_evaluation


def meta(name):
    nside, bp, rot, h, w, oh, ow, left, top, right, bottom, bkgd = (int(x) for x in load("flat_eval")[name + "/meta"])
    return dict(nside=nside, base_pix=bp, rotate_pole=bool(rot), model_size=(h, w), orig_size=(oh, ow) if oh else None,
                padding=(left, top, right, bottom), s2_bkgd_class=bkgd)


def model_layout(name):
    """(patch_size, tile in tokens) of the case's flat model."""
    _, _, kw = FLAT_MODEL_CASES[CASES[name][1]]
    return kw["patch_size"], kw["window_size"] * 2 ** (len(kw["depths"]) - 1)


def projector(FE, name, layout="image", interpolation="nearest", device="cpu"):
    kw = meta(name)
    if layout == "rows":
        kw["patch_size"], kw["tile"] = model_layout(name)
    return FE.FlatToHPProjector(_cal(CASES[name][0]), kw.pop("nside"), layout=layout, interpolation=interpolation, device=device, **kw)


def undo_transforms(x, m, mode):
    """The torch composition the table replaces: slice, then interpolate (tensor [..., H, W] float)."""
    left, top, right, bottom = m["padding"]
    h, w = x.shape[-2:]
    x = x[..., top:h - bottom, left:w - right]
    if m["orig_size"] is None:
        return x
    lead = x.shape[:-2]
    y = F.interpolate(x.reshape(1, -1, *x.shape[-2:]), size=list(m["orig_size"]), mode=mode,
                      **({} if mode == "nearest" else {"align_corners": False}))
    return y.reshape(*lead, *m["orig_size"])


def bilinear_numpy(p, src):
    """What hs_flat_depth_to_hp computes from the tables: src fp32 [B, n_src] -> ([B, Npix], per-pixel max |tap|)."""
    idx, wgt = p.idx_host.astype(np.int64), p.wgt_host
    ok = (idx < src.shape[1]).all(0)
    taps = src[:, np.where(ok, idx, 0)]  # [B, 4, Npix]
    with np.errstate(all="ignore"):
        val = wgt[0] * (wgt[2] * taps[:, 0] + wgt[3] * taps[:, 1]) + wgt[1] * (wgt[2] * taps[:, 2] + wgt[3] * taps[:, 3])
    return np.where(ok, val, np.nan).astype(np.float32), np.abs(taps).max(1)


# ------------------------------------------------------------------ the tables
@pytest.mark.parametrize("name", list(CASES))
def test_tables_equal_reference(FE, name):
    g, m = load("flat_eval"), meta(name)
    table = g[name + "/table"]
    p = projector(FE, name)
    n_src = m["model_size"][0] * m["model_size"][1]
    assert p.npix == n_src and p.n_out == table.size == m["base_pix"] * m["nside"] ** 2 and p.shape == (table.size,)
    # the case pins something: enough covered and uncovered pixels, and no coordinate near a rounding boundary, so that exact
    # equality can be asked of every pixel (the rotated (u, v) agree with the reference's to 1e-10 px)
    covered = table >= 0
    assert covered.mean() >= 0.30 and (~covered).mean() >= 0.10
    tag = f"{CASES[name][0]}/n{m['nside']}_bp{m['base_pix']}_{'rot' if m['rotate_pole'] else 'plain'}"
    for uv in (load("projection")[tag + "/u"], load("projection")[tag + "/v"], p.u, p.v):
        fin = np.isfinite(uv)
        assert np.abs(np.abs(uv[fin] - np.floor(uv[fin])) - 0.5).min() > 1e-6
    np.testing.assert_array_equal(p.covered_host, covered)
    np.testing.assert_array_equal(p.covered.numpy(), covered)
    np.testing.assert_array_equal(p.nearest_host[covered], table[covered])
    assert (p.nearest_host[~covered] >= n_src).all() and p.nearest_host.dtype == np.int32
    np.testing.assert_array_equal(p.nearest.numpy(), p.nearest_host)
    # the table reproduces the reference's sample_mask of the class ids, background included
    ids = g[name + "/ids"].reshape(2, -1)
    got = np.where(covered, ids[:, np.where(covered, p.nearest_host, 0)], m["s2_bkgd_class"])
    np.testing.assert_array_equal(got, g[name + "/hp_labels"])


def test_orig_size_defaults_to_the_calibration(FE):
    cal = _cal("mvl_96x128")
    kw = dict(model_size=(64, 64), padding=(0, 8, 0, 8), device="cpu")
    a, b = FE.FlatToHPProjector(cal, 16, **kw), FE.FlatToHPProjector(cal, 16, orig_size=(96, 128), **kw)
    assert a.orig_size == (96, 128)
    np.testing.assert_array_equal(a.nearest_host, b.nearest_host)


@pytest.mark.parametrize("name", [n for n, (_, model) in CASES.items() if model])
def test_rows_layout_is_image_through_the_row_permutation(FE, name):
    img, rows = projector(FE, name), projector(FE, name, layout="rows")
    (h, w), (ps, tile) = img.model_size, model_layout(name)
    perm = FE.pixel_rows(h, w, ps, tile)
    assert sorted(perm.tolist()) == list(range(h * w))
    cov = img.covered_host
    np.testing.assert_array_equal(rows.nearest_host[cov], perm[img.nearest_host[cov]])
    assert (rows.nearest_host[~cov] >= h * w).all()
    # the p x p children of a token are consecutive rows, child (kh, kw) at kh * p + kw, and tokens follow the tiled Z order
    grid = perm.reshape(h // ps, ps, w // ps, ps)
    np.testing.assert_array_equal(grid - grid[:, :1, :, :1], np.broadcast_to((np.arange(ps)[:, None] * ps + np.arange(ps))[None, :, None, :],
                                                                              grid.shape))
    from heal_swin_amd._lib import flat_zorder
    np.testing.assert_array_equal(grid[:, 0, :, 0].reshape(-1) // (ps * ps), flat_zorder(h // ps, w // ps, tile)[0])
    bil_i, bil_r = projector(FE, name, interpolation="bilinear"), projector(FE, name, layout="rows", interpolation="bilinear")
    np.testing.assert_array_equal(bil_r.idx_host[:, cov], perm[bil_i.idx_host[:, cov]])
    np.testing.assert_array_equal(bil_r.wgt_host, bil_i.wgt_host)


@pytest.mark.parametrize("sizes", [((48, 64), (96, 128)), ((32, 48), (60, 80)), ((60, 80), (32, 48)), ((13, 17), (31, 29)),
                                   ((640, 768), (966, 1280))])
def test_bilinear_taps_reproduce_interpolate(FE, sizes):
    (h, w), (oh, ow) = sizes
    img = np.random.default_rng(h * w).uniform(-300, 300, (h, w)).astype(np.float32)
    ref = F.interpolate(torch.from_numpy(img)[None, None], size=[oh, ow], mode="bilinear", align_corners=False)[0, 0].numpy()
    y0, y1, h0, h1 = FE.resize_linear_taps(h, oh)
    x0, x1, w0, w1 = FE.resize_linear_taps(w, ow)
    for a in (h0, h1, w0, w1):
        assert a.dtype == np.float32 and a.min() >= 0 and a.max() <= 1
    t = np.stack([img[y0][:, x0], img[y0][:, x1], img[y1][:, x0], img[y1][:, x1]])
    got = h0[:, None] * (w0[None] * t[0] + w1[None] * t[1]) + h1[:, None] * (w0[None] * t[2] + w1[None] * t[3])
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref) / (TAP_EPS * np.abs(t).max(0))
    print("worst error over the bound:", err.max())
    assert err.max() <= 1.0


def test_nearest_source_is_torchs(FE):
    for (h, w), (oh, ow) in (((48, 64), (96, 128)), ((60, 80), (32, 48)), ((13, 17), (31, 29))):
        img = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (h, w)).astype(np.float32))
        src = FE.resize_nearest_source((h, w), (oh, ow))
        assert torch.equal(F.interpolate(img[None, None], size=[oh, ow], mode="nearest")[0, 0], img.reshape(-1)[torch.from_numpy(src)])


# ------------------------------------------------------------------ depth, restated from the tables in numpy
@pytest.mark.parametrize("name", DEPTH_CASES)
def test_projected_depth_from_the_tables_matches_reference(FE, name):
    g = load("flat_eval")
    pred, target = g[name + "/depth/pred"], g[name + "/depth/target"]
    src = pred[:, 0].reshape(2, -1)
    p = projector(FE, name)
    cov = p.covered_host
    near = np.where(cov, src[:, np.where(cov, p.nearest_host, 0)], np.float32(np.nan))
    want = g[name + "/depth/nearest/hp"]
    assert np.isnan(want).any() and np.isinf(want).any() and (want[np.isfinite(want)] <= 0).any()
    np.testing.assert_array_equal(near.view(np.uint32)[:, cov], want.view(np.uint32)[:, cov])
    np.testing.assert_array_equal(np.isnan(near), np.isnan(want))
    pb = projector(FE, name, interpolation="bilinear")
    got, tap = bilinear_numpy(pb, src)
    want = g[name + "/depth/bilinear/hp"]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    np.testing.assert_array_equal(got[inf], want[inf])
    fin = np.isfinite(want)
    assert fin.mean() > 0.2
    assert (np.abs(got[fin].astype(np.float64) - want[fin]) <= TAP_EPS * tap[fin]).all()
    # the restated metrics on the reference's projected maps against the reference metric classes
    for mode, hp in (("nearest", near), ("bilinear", got)):
        ref = metrics_ref(hp, target, float(g["total_mean"]), {}, False)
        for k in ("mse", "SILogE", "iRMSE", "RelAE", "RelSE"):
            assert ref[k] == pytest.approx(float(g[f"{name}/depth/{mode}/{k}"]), rel=1e-5, abs=0), (mode, k)


def test_bilinear_identity_uses_the_nearest_table(FE):
    p = projector(FE, "identity", interpolation="bilinear")
    assert p.idx is None and p.wgt is None
    np.testing.assert_array_equal(p.nearest_host, projector(FE, "identity").nearest_host)


# ------------------------------------------------------------------ coverage of the image plane
@pytest.mark.parametrize("name", ["resize_pad_plain", "resize_pad_rot"])
def test_flat_coverage_table(FE, name):
    from heal_swin_amd.evaluation import HPBackProjector
    m, cal = meta(name), _cal(CASES[name][0])
    h, w = m["model_size"]
    valid = HPBackProjector(cal, m["nside"], base_pix=m["base_pix"], output_resolution=(h, w), rotate_pole=m["rotate_pole"],
                            device="cpu").valid.numpy()
    assert 0.05 < valid.mean() < 0.95
    c = FE.FlatCoverage(cal, m["nside"], m["base_pix"], m["rotate_pole"], (h, w), device="cpu")
    assert c.shape == (h, w) and c.n_out == c.npix == h * w
    np.testing.assert_array_equal(c.valid.numpy(), valid)
    near = c.nearest.numpy()
    np.testing.assert_array_equal(near[valid.reshape(-1)], np.arange(h * w)[valid.reshape(-1)])
    assert (near[~valid.reshape(-1)] >= h * w).all()
    ps, tile = model_layout(name)
    r = FE.FlatCoverage(cal, m["nside"], m["base_pix"], m["rotate_pole"], (h, w), layout="rows", patch_size=ps, tile=tile, device="cpu")
    np.testing.assert_array_equal(r.nearest.numpy()[valid.reshape(-1)], FE.pixel_rows(h, w, ps, tile)[valid.reshape(-1)])
    assert (r.nearest.numpy()[~valid.reshape(-1)] >= h * w).all()


# ------------------------------------------------------------------ arguments
def test_argument_validation(FE):
    cal = _cal("mvl_96x128")
    with pytest.raises(ValueError, match="model_size"):
        FE.FlatToHPProjector(cal, 16, device="cpu")
    with pytest.raises(ValueError, match="leaves nothing"):
        FE.FlatToHPProjector(cal, 16, model_size=(64, 64), padding=(0, 32, 0, 32), device="cpu")
    with pytest.raises(ValueError, match="leaves nothing"):
        FE.FlatToHPProjector(cal, 16, model_size=(64, 64), padding=(40, 0, 30, 0), device="cpu")
    with pytest.raises(ValueError, match="padding"):
        FE.FlatToHPProjector(cal, 16, model_size=(64, 64), padding=(0, -1, 0, 0), device="cpu")
    with pytest.raises(ValueError, match="interpolation"):
        FE.FlatToHPProjector(cal, 16, model_size=(64, 64), interpolation="bicubic", device="cpu")
    with pytest.raises(ValueError, match="layout"):
        FE.FlatToHPProjector(cal, 16, model_size=(64, 64), layout="nhwc", device="cpu")
    with pytest.raises(ValueError, match="patch_size and tile"):
        FE.FlatToHPProjector(cal, 16, model_size=(64, 64), layout="rows", device="cpu")
    with pytest.raises(ValueError, match="does not divide"):  # sizes that do not match the model's tiling
        FE.FlatToHPProjector(cal, 16, model_size=(64, 48), layout="rows", patch_size=2, tile=32, device="cpu")
    with pytest.raises(ValueError, match="uint8"):
        FE.FlatToHPProjector(cal, 16, model_size=(64, 64), s2_bkgd_class=256, device="cpu")

    class Model:  # what for_model reads of a SwinTransformerSys
        class data_spec:
            dim_in = (64, 64)

        class config:
            patch_size = [2, 2]

        tile = 32

    p = FE.FlatToHPProjector.for_model(Model, cal, 16, padding=(0, 8, 0, 8), device="cpu")
    assert (p.layout, p.model_size, p.patch_size, p.tile) == ("rows", (64, 64), 2, 32)
    with pytest.raises(ValueError, match="does not match the model"):
        FE.FlatToHPProjector.for_model(Model, cal, 16, model_size=(48, 64), device="cpu")
    with pytest.raises(ValueError, match="does not match the model"):
        FE.FlatToHPProjector.for_model(Model, cal, 16, patch_size=4, device="cpu")


def test_labels_need_the_nearest_table_and_a_gpu(FE):
    cal = _cal("mvl_96x128")
    kw = dict(model_size=(64, 64), padding=(0, 8, 0, 8), device="cpu")
    logits = torch.zeros(1, 5, 64, 64)
    bil = FE.FlatToHPProjector(cal, 16, interpolation="bilinear", **kw)
    with pytest.raises(ValueError, match="cannot be interpolated"):
        bil.labels(logits)
    with pytest.raises(ValueError, match="cannot be interpolated"):
        bil.nearest
    p = FE.FlatToHPProjector(cal, 16, **kw)
    for call in (lambda: p.labels(logits), lambda: p.depth(logits), lambda: p.logits(logits)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
