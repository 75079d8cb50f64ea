"""heal_swin_amd.depth_data on the GPU (csrc/projection.hip, csrc/depth_data.hip): the depth sampling bit-equal to the
reference's, the target transforms of all 18 (transform, normalization, mask_background) combinations forward, inverse and as dataset preparation, the
streaming dataset statistics against a numpy restatement of compute_depth_stats.py, and the whole depth data path feeding
forward_depth_loss and DepthMetrics."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from _golden import load
from test_depth_evaluation import _cal
from test_gpu_evaluation import _free_port

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSFORMS = ["None", "log", "inv"]
NORMS = ["None", "standardize", "min-max"]


@pytest.fixture(scope="module")
def DD():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import depth_data
    return depth_data


# ------------------------------------------------------------------ sampling
def test_sampling_bit_equal_to_the_reference(DD):
    g = load("depth_data")
    tags = sorted({k.rsplit("/", 1)[0] for k in g.files if k.startswith("sample/")})
    assert len(tags) == 2
    for tag in tags:
        c = tag.replace("sample/", "coords/")
        u, v = g[c + "/u"], g[c + "/v"]
        img = torch.from_numpy(g[tag + "/img"]).to(DEV)
        depth = torch.from_numpy(g[tag + "/depth"]).to(DEV)
        hp_img = DD.sample_bilinear_f32(img, v, u)
        assert hp_img.dtype == torch.float32
        assert np.array_equal(hp_img.cpu().numpy(), g[tag + "/hp_img"], equal_nan=True), tag
        assert np.array_equal(DD.sample_depth(depth, v, u, 0).cpu().numpy(), g[tag + "/hp_mask"], equal_nan=True), tag
        # batched: every frame against the same table
        b_img = DD.sample_bilinear_f32(torch.stack([img, img.flip(1)]), v, u)
        assert np.array_equal(b_img[0].cpu().numpy(), g[tag + "/hp_img"], equal_nan=True)
    img, depth = torch.from_numpy(g["edge/img"]).to(DEV), torch.from_numpy(g["edge/depth"]).to(DEV)
    out = DD.sample_bilinear_f32(img, g["edge/rx"], g["edge/ry"]).cpu().numpy()
    assert np.isnan(g["edge/hp_img"]).any() and (g["edge/hp_img"] == 0).any()
    assert np.array_equal(out, g["edge/hp_img"], equal_nan=True)
    assert np.array_equal(DD.sample_depth(depth, g["edge/rx"], g["edge/ry"], 7.5).cpu().numpy(), g["edge/hp_mask"], equal_nan=True)


def _np_bilinear(img, rx, ry):
    """project_depth_on_s2.sample_bilinear restated (float64, numpy), for a full-size frame."""
    h, w = img.shape[1:]
    with np.errstate(invalid="ignore"):
        ix0, iy0, ix1, iy1 = np.floor(rx), np.floor(ry), np.ceil(rx), np.ceil(ry)

    def at(ix, iy):
        ok = (ix >= 0) & (ix < h) & (iy >= 0) & (iy < w)
        s = np.zeros((img.shape[0], rx.size))
        s[:, ok] = img[:, ix[ok].astype(np.int64), iy[ok].astype(np.int64)]
        return s

    fx1 = (ix1 - rx) * at(ix0, iy0) + (rx - ix0) * at(ix1, iy0)
    fx2 = (ix1 - rx) * at(ix0, iy1) + (rx - ix0) * at(ix1, iy1)
    return ((iy1 - ry) * fx1 + (ry - iy0) * fx2).astype(np.float32)


def _np_nearest(depth, rx, ry, bkgd):
    h, w = depth.shape
    with np.errstate(invalid="ignore"):
        x, y = np.around(rx), np.around(ry)
    ok = (x >= 0) & (x < h) & (y >= 0) & (y < w)
    out = np.full(rx.shape, bkgd, np.float32)
    out[ok] = depth[x[ok].astype(np.int64), y[ok].astype(np.int64)]
    return out


def test_full_size_projection(DD):
    """A 966 x 1280 frame and depth map -> nside 256, 8 base pixels, against the numpy restatement on the projector's table."""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (3, 966, 1280), dtype=np.uint8)
    depth = rng.uniform(0.2, 400, (966, 1280)).astype(np.float32)
    depth[rng.random(depth.shape) < 0.1] = 1000.0
    proj = DD.HPDepthProjector(_cal("fv_966x1280"), 256, 8, rotate_pole=True, s2_bkgd_class=0)
    hp_img, hp_mask = proj.proj(torch.from_numpy(img).to(DEV)[None], torch.from_numpy(depth).to(DEV)[None])
    assert hp_img.shape == (1, 3, 524288) and hp_mask.shape == (1, 524288)
    u, v = proj.u.cpu().numpy(), proj.v.cpu().numpy()
    assert np.array_equal(hp_img[0].cpu().numpy(), _np_bilinear(img, v, u), equal_nan=True)
    ref = _np_nearest(depth, v, u, 0.0)
    assert np.array_equal(hp_mask[0].cpu().numpy(), ref)
    assert (ref == 0).any() and (ref == 1000).any()  # both the outside and the background class are exercised


# ------------------------------------------------------------------ target transforms
def _check(out, ref, t, s, exact, tag):
    """Same positions of NaN, +inf, -inf and 0; elsewhere bit-equal (exact) or |d| <= 8 2^-24 max(|y|, |t| / s)."""
    out, ref = np.asarray(out, np.float32), np.asarray(ref, np.float32)
    for f in (np.isnan, np.isposinf, np.isneginf, lambda a: a == 0):
        assert np.array_equal(f(out), f(ref)), (tag, np.flatnonzero(f(out) != f(ref))[:8])
    fin = np.isfinite(ref) & (ref != 0)
    if exact:
        assert np.array_equal(out[fin], ref[fin]), tag
        return
    o, r = out[fin].astype(np.float64), ref[fin].astype(np.float64)
    tt = np.abs(np.asarray(t, np.float64)[fin]) / s
    bound = 8 * 2.0 ** -24 * np.maximum(np.abs(r), np.nan_to_num(tt, posinf=0.0))
    bad = np.abs(o - r) > bound
    assert not bad.any(), (tag, o[bad][:4], r[bad][:4])


def _scale(DD, T, N, M):
    s = DD.get_depth_data_stats(T, M)
    return {"None": 1.0, "standardize": float(np.float32(s.std)), "min-max": float(np.float32(s.max - s.min))}[N]


@pytest.mark.parametrize("T", TRANSFORMS)
def test_transforms_match_the_reference(DD, T):
    g = load("depth_data")
    x, z = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["z"]).to(DEV)
    for N in NORMS:
        for M in (False, True):
            tag = f"{T}/{N}/{int(M)}"
            s = _scale(DD, T, N, M)
            exact = T == "None" and N == "None"
            tr = DD.DepthTargetTransform(T, N, mask_background=M)
            _check(tr.transform_and_normalize(x).cpu(), g[f"fwd/{tag}"], g[f"fwd/{T}/None/{int(M)}"], s, exact, "fwd " + tag)
            _check(tr.unnormalize_and_retransform(z).cpu(), g[f"inv/{tag}"], g["z"], 1.0, exact, "inv " + tag)
            _check(tr.prepare(x).cpu(), g[f"prep_hp/{tag}"], g[f"prep_hp/{T}/None/{int(M)}"], s, exact, "prep_hp " + tag)
            flat = DD.DepthTargetTransform(T, N, mask_background=M, zero_is_background=False)
            _check(flat.prepare(x).cpu(), g[f"prep_flat/{tag}"], g[f"prep_flat/{T}/None/{int(M)}"], s, exact, "prep_flat " + tag)
            # strided rows (the scalar path): every other element of a [2, 2n] tensor, two rows
            xs = torch.stack([x, x]).repeat_interleave(2, dim=1)[:, ::2]
            ys = tr.transform_and_normalize(xs).cpu()
            for r in range(2):
                _check(ys[r], g[f"fwd/{tag}"], g[f"fwd/{T}/None/{int(M)}"], s, exact, "strided " + tag)


def test_in_place_on_the_model_output_channel(DD):
    g = load("depth_data")
    n = g["x"].size
    for odd in (False, True):  # n % 4 == 0: the 16-byte path; odd n: the scalar path
        m = n - 1 if odd else n
        out = torch.randn(2, 2, m, device=DEV)
        out[:, 0] = torch.from_numpy(g["x"][:m]).to(DEV)
        ch1 = out[:, 1].clone()
        tr = DD.DepthTargetTransform("log", "standardize", mask_background=True)
        res = tr.transform_and_normalize(out[:, 0], out=out[:, 0])
        assert res.data_ptr() == out.data_ptr()
        assert torch.equal(out[:, 1], ch1)
        for r in range(2):
            _check(out[r, 0].cpu(), g["fwd/log/standardize/1"][:m], g["fwd/log/None/1"][:m], _scale(DD, "log", "standardize", True),
                   False, f"in place odd={odd}")
        back = tr.unnormalize_and_retransform(out[:, 0], out=out[:, 0])
        assert back.data_ptr() == out.data_ptr() and torch.equal(out[:, 1], ch1)


# ------------------------------------------------------------------ dataset statistics
def _np_stats(arrays, transform, masking):
    """compute_depth_stats.py's arithmetic (log correctly rounded in float32, as the golden file)."""
    vals, fgs = [np.empty((0,))], [np.empty((0,), bool)]
    total = bkg = 0
    for a in arrays:
        a = np.asarray(a, np.float32).reshape(-1)
        bkg += int(np.count_nonzero(a == 1000))
        total += a.size
        keep = a[a != 1000] if masking else a
        with np.errstate(divide="ignore", invalid="ignore"):
            t = {"None": keep, "log": np.log(keep.astype(np.float64)).astype(np.float32), "inv": 1 / keep}[transform]
        vals.append(t)
        fgs.append(keep != 1000)
    d, fg = np.concatenate(vals), np.concatenate(fgs)
    with np.errstate(invalid="ignore"):
        return [np.amax(d), np.amin(d), np.mean(d), np.std(d), np.amax(d[fg]), total, bkg]


def _same(a, b, rel):
    a, b = float(a), float(b)
    if math.isnan(b) or math.isinf(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= rel * abs(b)


def _assert_stats(st, ref, tag, rel=1e-12):
    got = [st.max, st.min, st.mean, st.std, st.max_foreground, st.total_pixels, st.total_background]
    for i, name in enumerate(("max", "min", "mean", "std", "max_foreground", "total_pixels", "total_background")):
        r = rel if name in ("mean", "std") else 0.0
        assert _same(got[i], ref[i], r), (tag, name, got[i], ref[i])


@pytest.mark.parametrize("T", TRANSFORMS)
def test_statistics_match_the_golden(DD, T):
    g = load("depth_data")
    maps = torch.from_numpy(g["stats/maps"]).to(DEV)
    for M in (False, True):
        acc = DD.DepthStatsAccumulator(T, use_masking=M)
        acc.update(maps[0])
        acc.update(maps[1])
        _assert_stats(acc.compute(), g[f"stats/{T}/{int(M)}/two"], f"{T}/{M}/two")
        acc.update(maps[2])
        _assert_stats(acc.compute(), g[f"stats/{T}/{int(M)}/all"], f"{T}/{M}/all")
        acc.reset()
        acc.update(maps[0])
        acc.update(maps[1])
        _assert_stats(acc.compute(), g[f"stats/{T}/{int(M)}/two"], f"{T}/{M}/after reset")


def test_statistics_cancellation_and_split_updates(DD):
    rng = np.random.default_rng(5)
    a = (1000.0 + rng.choice([-1e-3, 1e-3], 3_000_001) + rng.normal(0, 2e-4, 3_000_001)).astype(np.float32)
    a = a[a != 1000]
    acc = DD.DepthStatsAccumulator()
    acc.update(torch.from_numpy(a).to(DEV))
    one = acc.compute()
    _assert_stats(one, _np_stats([a], "None", False), "cancellation")
    assert one.std > 5e-4
    acc2 = DD.DepthStatsAccumulator()
    k = 1_234_567
    acc2.update(torch.from_numpy(a[:k]).to(DEV))
    acc2.update(torch.from_numpy(a[k:]).to(DEV)[1:])  # an unaligned start: the scalar path
    acc2.update(torch.from_numpy(a[k:k + 1]).to(DEV))
    two = acc2.compute()
    for f in ("mean", "std"):
        assert _same(getattr(two, f), getattr(one, f), 1e-12), f
    assert (two.max, two.min, two.total_pixels) == (one.max, one.min, one.total_pixels)


def test_statistics_non_finite_inputs(DD):
    rng = np.random.default_rng(6)
    base = rng.uniform(0.5, 50, 5000).astype(np.float32)
    cases = {"posinf": [np.inf], "neginf": [-np.inf], "both": [np.inf, -np.inf], "nan": [np.nan], "zero": [0.0, 0.0],
             "negative": [-2.0], "background": [1000.0, 1000.0]}
    for name, extra in cases.items():
        a = base.copy()
        a[rng.choice(a.size, len(extra), replace=False)] = extra
        for T in TRANSFORMS:
            for M in (False, True):
                acc = DD.DepthStatsAccumulator(T, use_masking=M)
                acc.update(torch.from_numpy(a).to(DEV))
                _assert_stats(acc.compute(), _np_stats([a], T, M), f"{name}/{T}/{M}")
    acc = DD.DepthStatsAccumulator("log")
    acc.update(torch.tensor([0.0, 1.0, 2.0], device=DEV))
    st = acc.compute()
    assert st.min == -math.inf and st.mean == -math.inf and math.isnan(st.std)


def test_statistics_are_deterministic(DD):
    rng = np.random.default_rng(7)
    maps = [torch.from_numpy(rng.uniform(0.2, 999, (966, 1280)).astype(np.float32)).to(DEV) for _ in range(3)]
    states = []
    for _ in range(3):
        acc = DD.DepthStatsAccumulator("log", use_masking=True)
        for m in maps:
            acc.update(m)
        states.append(acc.state.cpu())
    assert torch.equal(states[0], states[1]) and torch.equal(states[0], states[2])


def _stats_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from heal_swin_amd.depth_data import DepthStatsAccumulator
    rng = np.random.default_rng(200 + rank)
    a = rng.uniform(0.2, 999, 100_000 + 777 * rank).astype(np.float32)
    a[rng.random(a.size) < 0.05] = 1000.0
    m = DepthStatsAccumulator("inv")
    m.update(torch.from_numpy(a).to(DEV))
    m.all_reduce()
    q.put((rank, a, m.state.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_statistics_all_reduce_two_ranks(DD):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_stats_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict((r, (a, s)) for r, a, s in (q.get(timeout=300) for _ in range(world)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert np.array_equal(res[0][1], res[1][1])  # every rank holds the same bits
    acc = DD.DepthStatsAccumulator("inv")
    acc.state.copy_(torch.from_numpy(res[0][1]))
    _assert_stats(acc.compute(), _np_stats([res[0][0], res[1][0]], "inv", False), "all_reduce")


# ------------------------------------------------------------------ the whole path
def test_depth_path_end_to_end(DD):
    """frame -> HEALPix sample -> target -> forward_depth_loss -> inverse -> DepthMetrics."""
    from heal_swin_amd import losses
    from heal_swin_amd.depth_evaluation import DepthMetrics
    from test_gpu_depth_loss import _hp_model

    m, _, _ = _hp_model(1)
    rng = np.random.default_rng(9)
    imgs = torch.from_numpy(rng.integers(0, 256, (2, 3, 96, 128), dtype=np.uint8)).to(DEV)
    depths = rng.uniform(0.3, 300, (2, 96, 128)).astype(np.float32)
    depths[rng.random(depths.shape) < 0.1] = 1000.0
    proj = DD.HPDepthProjector(_cal("mvl_96x128"), 32, 8)
    hp_img, hp_mask = proj.proj(imgs, torch.from_numpy(depths).to(DEV))
    assert hp_img.shape == (2, 3, 8 * 32 * 32) and hp_mask.dtype == torch.float32
    tr = DD.DepthTargetTransform("log", "standardize", mask_background=True)
    target = tr.prepare(hp_mask)
    assert torch.isinf(target).any() and torch.isfinite(target).any()
    loss = m.forward_depth_loss(hp_img, target, loss="l2")
    ref = losses.depth_loss(m(hp_img), target, loss="l2")
    loss, ref = float(loss.detach()), float(ref.detach())
    assert abs(loss - ref) <= 1e-5 * abs(ref), (loss, ref)
    # the inverse recovers the depths (0 and 1000 were the background: inf)
    back = tr.unnormalize_and_retransform(target)
    keep = (hp_mask != 0) & (hp_mask != 1000)
    assert torch.isinf(back[~keep]).all()
    assert torch.allclose(back[keep], hp_mask[keep], rtol=4e-6, atol=0)
    with torch.no_grad():
        out = m(hp_img)
    tr.unnormalize_and_retransform(out[:, 0], out=out[:, 0])
    metrics = DepthMetrics()
    metrics.update(out, back)
    res = metrics.compute()
    p, t = out[:, 0].double(), back.double()
    fin = torch.isfinite(p) & torch.isfinite(t)
    mse = float(((p - t)[fin] ** 2).mean())
    assert math.isfinite(res["mse"]) and abs(res["mse"] - mse) <= 1e-9 * mse
