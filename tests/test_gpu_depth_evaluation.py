"""heal_swin_amd.depth_evaluation on the GPU (csrc/depth_eval.hip): point clouds against the reference's own clouds, exact
Chamfer nearest neighbours against a float64 brute force (ties, ragged batches, empty clouds, split counts, full size), the
depth metrics against the reference's values and a float64 torch restatement, and the depth back-projection bit-exact."""
import numpy as np
import pytest
import torch

from _golden import load
from test_depth_evaluation import _cal, _ulps, metrics_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def D():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import depth_evaluation
    return depth_evaluation


# ------------------------------------------------------------------ point clouds
def _hp_tags(g):
    return sorted({k.rsplit("/", 1)[0] for k in g.files if k.startswith("hp/")})


def test_hp_points_match_reference(D):
    g = load("depth_eval")
    for tag in _hp_tags(g):
        _, key, ns = tag.split("/")
        nside, bp = (int(x) for x in ns[1:].split("_bp"))
        geo = D.HPDepthGeometry(_cal(key), nside, bp, device=DEV)
        depth = g[tag + "/depth"]
        pts, off = geo.points(torch.from_numpy(depth).to(DEV))
        ref = g[tag + "/points"]
        assert off.tolist() == [0, ref.shape[0]]
        got = pts[: ref.shape[0]].cpu().numpy()
        u = _ulps(ref, got)
        small = np.abs(got.astype(np.float64) - ref) <= 1e-14 * np.abs(depth[g[tag + "/keep"]])[:, None]
        assert ((u <= 1) | small).all(), (tag, u.max())
        # the writers' mask_background: 1000 is background too
        pts2, off2 = geo.points(torch.from_numpy(depth).to(DEV), background=(float("nan"), float("inf"), 1000))
        keep = np.isfinite(depth) & (depth != 1000)
        assert off2.tolist() == [0, int(keep.sum())]


@pytest.mark.parametrize("key", ["mvl_96x128", "rv_60x80"])
@pytest.mark.parametrize("rot", ["plain", "rot"])
def test_image_points_match_reference(D, key, rot):
    g = load("depth_eval")
    tag = f"img/{key}/{rot}"
    depth = g[tag + "/depth"]
    h, w = depth.shape
    geo = D.ImageDepthGeometry(_cal(key), h, w, rot == "rot", device=DEV)
    # strided input: every other column of a wider buffer
    buf = torch.full((h, 2 * w), 7.0, device=DEV)
    buf[:, ::2] = torch.from_numpy(depth).to(DEV)
    pts, off = geo.points(buf[:, ::2])
    ref = g[tag + "/points"]
    assert off.tolist() == [0, ref.shape[0]]
    got = pts[: ref.shape[0]].cpu().numpy().astype(np.float64)
    d = depth[g[tag + "/keep"]].astype(np.float64)
    assert (np.abs(got - ref) <= np.abs(d)[:, None] * 1e-6 + np.spacing(np.abs(ref))).all()


def test_points_batch_foreground_bf16(D):
    geo = D.HPDepthGeometry(_cal("rv_60x80"), 16, 8, device=DEV)
    rng = np.random.default_rng(1)
    depth = rng.uniform(1, 100, (3, geo.n)).astype(np.float32)
    depth[rng.random(depth.shape) < 0.2] = np.nan
    depth[1] = np.nan  # an empty cloud in the middle
    fg = rng.random(depth.shape) < 0.7
    t = torch.from_numpy(depth).to(DEV).bfloat16()
    pts, off = geo.points(t, foreground=torch.from_numpy(fg).to(DEV))
    dref = t.float().cpu().numpy()
    o = [0]
    for b in range(3):
        keep = np.isfinite(dref[b]) & fg[b]
        want = (dref[b][keep].astype(np.float64) * geo.dir_host[:, keep]).T.astype(np.float32)
        o.append(o[-1] + want.shape[0])
        np.testing.assert_array_equal(pts[o[-2]: o[-1]].cpu().numpy(), want)
    assert off.tolist() == o


# ------------------------------------------------------------------ Chamfer
def brute(a, b):
    """float64 brute force on the fp32 coordinates: (dist_a, dist_b)."""
    A, B = torch.as_tensor(a, device=DEV).double(), torch.as_tensor(b, device=DEV).double()
    da = torch.full((A.shape[0],), float("inf"), dtype=torch.float64, device=DEV)
    db = torch.full((B.shape[0],), float("inf"), dtype=torch.float64, device=DEV)
    for i in range(0, A.shape[0], 4096):
        d = ((A[i:i + 4096, None, :] - B[None, :, :]) ** 2).sum(-1)
        da[i:i + 4096] = d.min(1).values
        db = torch.minimum(db, d.min(0).values)
    return da, db


def _check_nn(a, b, da, db, ia=None, ib=None):
    ra, rb = brute(a, b)
    for got, ref in ((da, ra), (db, rb)):
        assert torch.all((got.double() - ref).abs() <= 5e-7 * ref + 1e-30), (got.double() - ref).abs().max().item()
    if ia is not None:
        A, B = a.double(), b.double()
        att = ((A - B[ia]) ** 2).sum(-1)
        assert torch.all((att - ra).abs() <= 5e-7 * ra + 1e-30)
        att = ((B - A[ib]) ** 2).sum(-1)
        assert torch.all((att - rb).abs() <= 5e-7 * rb + 1e-30)


@pytest.mark.parametrize("na,nb", [(1, 1), (1, 700), (700, 1), (2049, 513), (5000, 3001), (20000, 17)])
def test_chamfer_against_brute_force(D, na, nb):
    g = torch.Generator(device=DEV).manual_seed(na * 7 + nb)
    a = torch.randn(na, 3, device=DEV, generator=g) * 50 + 100
    b = torch.randn(nb, 3, device=DEV, generator=g) * 50 + 100
    da, db, ia, ib = D.chamfer_nn(a, b, return_idx=True)
    _check_nn(a, b, da, db, ia, ib)
    da2, db2 = D.chamfer_nn(a, b)
    assert torch.equal(da, da2) and torch.equal(db, db2)


def test_chamfer_ties_and_duplicates(D):
    # b holds every point twice, and a's points sit exactly between pairs of b's points at integer coordinates
    b = torch.tensor([[0, 0, 0], [2, 0, 0], [0, 0, 0], [2, 0, 0], [5, 5, 5]], dtype=torch.float32, device=DEV)
    a = torch.tensor([[1, 0, 0], [0, 0, 0], [5, 5, 5], [2, 0, 0]], dtype=torch.float32, device=DEV)
    da, db, ia, ib = D.chamfer_nn(a, b, return_idx=True)
    assert da.tolist() == [1.0, 0.0, 0.0, 0.0]
    assert ia.tolist() == [0, 0, 4, 1]  # (1,0,0): b0, b1, b2, b3 all at 1: the lowest index
    assert db.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0]
    assert ib.tolist() == [1, 3, 1, 3, 2]
    # ties across tiles and splits: 3000 copies of one point
    b = torch.zeros(3000, 3, device=DEV)
    a = torch.ones(5, 3, device=DEV)
    for s in (1, 2, 5):
        da, _, ia, ib = D.chamfer_nn(a, b, return_idx=True, splits=s)
        assert ia.tolist() == [0] * 5 and da.tolist() == [3.0] * 5
        assert ib.tolist() == [0] * 3000


def test_chamfer_ragged_batch_and_empty(D):
    g = torch.Generator(device=DEV).manual_seed(3)
    sizes_a, sizes_b = [700, 0, 1, 3000, 5], [900, 40, 0, 2500, 1]
    a = torch.randn(sum(sizes_a) + 11, 3, device=DEV, generator=g) * 10  # spare rows past the last cloud
    b = torch.randn(sum(sizes_b), 3, device=DEV, generator=g) * 10
    oa = torch.tensor(np.concatenate([[0], np.cumsum(sizes_a)]), device=DEV)
    ob = torch.tensor(np.concatenate([[0], np.cumsum(sizes_b)]), device=DEV)
    da, db, ia, ib, term = D.chamfer_nn(a, b, oa, ob, return_idx=True, return_term=True)
    t = term.cpu()
    for s in range(5):
        a0, a1, b0, b1 = oa[s].item(), oa[s + 1].item(), ob[s].item(), ob[s + 1].item()
        if a1 > a0 and b1 > b0:
            _check_nn(a[a0:a1], b[b0:b1], da[a0:a1], db[b0:b1], ia[a0:a1], ib[b0:b1])
            want = da[a0:a1].double().mean() + db[b0:b1].double().mean()
            assert t[s].item() == pytest.approx(want.item(), rel=1e-12)
        else:
            assert torch.isnan(t[s])
            assert torch.isnan(da[a0:a1]).all() and torch.isnan(db[b0:b1]).all()
            assert (ia[a0:a1] == -1).all() and (ib[b0:b1] == -1).all()
    assert torch.isnan(da[oa[-1]:]).all()


def test_chamfer_deterministic_across_launches_and_splits(D):
    g = torch.Generator(device=DEV).manual_seed(5)
    a = (torch.randn(9000, 3, device=DEV, generator=g) * 3).round()  # coarse grid: many exact ties
    b = (torch.randn(12000, 3, device=DEV, generator=g) * 3).round()
    ref = D.chamfer_nn(a, b, return_idx=True, splits=1)
    for s in (0, 0, 2, 3, 7, 24):
        got = D.chamfer_nn(a, b, return_idx=True, splits=s)
        for x, y in zip(ref, got):
            assert torch.equal(x, y)
    _check_nn(a, b, *ref)


def test_chamfer_full_size(D):
    """nside 256 / 8 base pixels against the 966 x 1280 image cloud, checked on 8192 random queries per direction."""
    cal = _cal("fv_966x1280")
    hp = D.HPDepthGeometry(cal, 256, 8, device=DEV)
    img = D.ImageDepthGeometry(cal, 966, 1280, False, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    dh = torch.rand(1, hp.n, device=DEV, generator=g) * 80 + 1
    di = torch.rand(1, 966, 1280, device=DEV, generator=g) * 80 + 1
    di[0, :100] = float("nan")
    pa, oa = hp.points(dh)
    pb, ob = img.points(di)
    na, nb = oa[1].item(), ob[1].item()
    assert na == hp.n and nb == 966 * 1280 - 100 * 1280
    da, db, ia, ib = D.chamfer_nn(pa, pb, oa, ob, return_idx=True, max_points=(hp.n, img.n))
    da2, db2 = D.chamfer_nn(pa, pb, oa, ob, max_points=(hp.n, img.n))
    for x, y in ((da, da2), (db, db2)):  # the spare rows past the image cloud read NaN in both
        torch.testing.assert_close(x, y, rtol=0, atol=0, equal_nan=True)
    assert torch.isnan(db[nb:]).all() and not torch.isnan(db[:nb]).any()
    A, B = pa[:na].double(), pb[:nb].double()
    for Q, T, dist, idx in ((A, B, da, ia), (B, A, db, ib)):
        sel = torch.randperm(Q.shape[0], generator=torch.Generator().manual_seed(2))[:8192].to(DEV)
        ref = torch.full((8192,), float("inf"), dtype=torch.float64, device=DEV)
        qs = Q[sel]
        for j in range(0, T.shape[0], 8192):
            d = ((qs[:, None, :] - T[None, j:j + 8192, :]) ** 2).sum(-1)
            ref = torch.minimum(ref, d.min(1).values)
        assert torch.all((dist[sel].double() - ref).abs() <= 5e-7 * ref + 1e-30)
        att = ((Q[sel] - T[idx[sel]]) ** 2).sum(-1)
        assert torch.all((att - ref).abs() <= 5e-7 * ref + 1e-30)


def test_chamfer_distance_metric(D):
    cal = _cal("rv_60x80")
    hp = D.HPDepthGeometry(cal, 16, 8, device=DEV)
    img = D.ImageDepthGeometry(cal, 30, 40, True, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(9)
    pred = torch.rand(3, 2, hp.n, device=DEV, generator=g) * 50 + 1
    target = torch.rand(3, 30, 40, device=DEV, generator=g) * 50 + 1
    target[2] = float("nan")  # empty target cloud: NaN term
    m = D.ChamferDistance(device=DEV)
    m.update(pred[:2], target[:2], hp, img)
    terms = []
    for s in range(2):
        pa, oa = hp.points(pred[s, 0])
        pb, ob = img.points(target[s])
        da, db = D.chamfer_nn(pa[: oa[1]], pb[: ob[1]])
        terms.append(da.double().mean() + db.double().mean())
    assert m.compute().item() == pytest.approx(sum(terms).item() / 2, rel=1e-12)
    m.update(pred[2:], target[2:], hp, img)
    assert torch.isnan(m.compute())


# ------------------------------------------------------------------ metrics
def _torch_ref(pred, target, total_mean, ranges, use_logvar):
    """float64 torch restatement on the device (fp32 transforms in fp32, as the kernel)."""
    return metrics_ref(pred.cpu().numpy(), target.cpu().numpy(), total_mean, ranges, use_logvar)


@pytest.mark.parametrize("tag", ["hp", "img"])
def test_metrics_match_reference(D, tag):
    g = load("depth_eval")
    pred = torch.from_numpy(g[f"metrics/{tag}/pred"]).to(DEV)
    target = torch.from_numpy(g[f"metrics/{tag}/target"]).to(DEV)
    ranges = [(0, 5), (20, 100), (5, 300), (500, 600), (10,), 50.0]
    m = D.DepthMetrics(total_mean=float(g["metrics/total_mean"]), distance_ranges=ranges, use_logvar=True, device=DEV)
    half = pred.shape[0] // 2
    m.update(pred[:half], target[:half])
    m.update(pred[half:], target[half:])
    got = m.compute()
    names = dict(zip(D.range_names(ranges), ["mse_range_000_005", "mse_range_020_100", "mse_range_005_300", "mse_range_500_600",
                                             "range_hi_tuple", "range_hi_scalar"]))
    for k, v in got.items():
        want = float(g[f"metrics/{tag}/{names.get(k, k)}"])
        assert v == pytest.approx(want, rel=1e-5, abs=0), (k, v, want)
    ref = _torch_ref(pred, target, float(g["metrics/total_mean"]), dict(zip(D.range_names(ranges), [D._range_bounds(r) for r in ranges])), True)
    for k, v in got.items():
        rel = 1e-6 if k in ("iRMSE", "SILogE", "mean_std", "median_std") else 1e-9
        assert v == pytest.approx(ref[k], rel=rel, abs=0), (k, v, ref[k])


def test_metrics_bf16_strided_model_output(D):
    """A depth model's own [B, 2, Npix] output in padded bf16 rows, and bit-identical sums across launches."""
    rng = np.random.default_rng(4)
    b, n = 3, 8 * 32 * 32
    buf = torch.from_numpy(rng.uniform(0.5, 90, (b, n, 4)).astype(np.float32)).to(DEV).bfloat16()
    pred = buf[:, :, :2].transpose(1, 2)  # [B, 2, Npix], stride_p 4
    target = torch.from_numpy(rng.uniform(0.5, 90, (b, n)).astype(np.float32)).to(DEV)
    target[0, :50] = float("inf")
    ms = [D.DepthMetrics(total_mean=30.0, distance_ranges=[(0, 40)], use_logvar=True, device=DEV) for _ in range(2)]
    for m in ms:
        m.update(pred, target)
    assert torch.equal(ms[0].state, ms[1].state)
    got = ms[0].compute()
    ref = _torch_ref(pred.float(), target, 30.0, {"mse_range_00_40": (0, 40)}, True)
    for k, v in got.items():
        rel = 1e-6 if k in ("iRMSE", "SILogE", "mean_std", "median_std") else 1e-9
        assert v == pytest.approx(ref[k], rel=rel, abs=0), (k, v, ref[k])


def test_backprojected_depth_metrics(D):
    """hs_backproject_depth bit-exact against get_interp_val with NaN completion, then DepthMetrics on the float64 image."""
    from heal_swin_amd.evaluation import HPBackProjector

    nside, bp = 16, 8
    p = HPBackProjector(_cal("rv_60x80"), nside, base_pix=bp, output_resolution=1.0, rotate_pole=True, device=DEV)
    rng = np.random.default_rng(6)
    vals = rng.uniform(1, 60, (2, 2, p.npix)).astype(np.float32)
    vals[0, 0, rng.integers(0, p.npix, 40)] = np.nan
    for dt in (torch.float32, torch.bfloat16):
        t = torch.from_numpy(vals).to(DEV).to(dt)
        out = p.depth(t, channel=0).cpu().numpy()
        idx, wgt = p.idx.cpu().numpy(), p.wgt.cpu().numpy()
        src = t.float().cpu().numpy()[:, 0]
        for i in range(2):
            full = np.full(12 * nside * nside, np.nan, dtype=np.float32)
            full[: p.npix] = src[i]
            m = full.astype(np.float64)[idx]
            want = ((m[0] * wgt[0] + m[1] * wgt[1]) + m[2] * wgt[2]) + m[3] * wgt[3]
            np.testing.assert_array_equal(out[i], want)
    # the fill rule on a hand-built table (pixel 0 inside the map, pixels 1 and 2 with one tap outside, of weight 0 and 0.25):
    # the map is completed with NaN, and 0 * NaN stays NaN
    from test_gpu_evaluation import hand_table_projector, hand_table_ref
    import heal_swin_amd.evaluation as E

    h = hand_table_projector(E)
    for dt in (torch.float32, torch.bfloat16):
        t = torch.from_numpy(rng.uniform(1, 60, (2, h.npix)).astype(np.float32)).to(DEV).to(dt)
        out = h.depth(t).cpu().numpy().reshape(2, 3)
        assert np.isfinite(out[:, 0]).all() and np.isnan(out[:, 1:]).all()
        np.testing.assert_array_equal(out, hand_table_ref(t.double().cpu().numpy(), h, np.nan))
    img = p.depth(torch.from_numpy(vals).to(DEV))
    assert torch.isnan(img).any() and torch.isfinite(img).any()
    target = torch.from_numpy(rng.uniform(1, 60, (2,) + p.shape).astype(np.float32)).to(DEV)
    m = D.DepthMetrics(total_mean=20.0, device=DEV)
    m.update(img, target)
    got = m.compute()
    ref = metrics_ref(img.cpu().numpy(), target.cpu().numpy(), 20.0, {}, False)
    for k, v in got.items():
        rel = 1e-6 if k in ("iRMSE", "SILogE") else 1e-9
        assert v == pytest.approx(ref[k], rel=rel, abs=0), (k, v, ref[k])
