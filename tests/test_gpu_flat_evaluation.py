"""heal_swin_amd.flat_evaluation on the GPU (csrc/flat_eval.hip and the segmentation kernels through the flat tables): projected
labels and depth bit-equal to the reference's sample_mask results (tests/golden/flat_eval.npz), the confusion matrix, the masked
image-plane IoU, the depth metrics against the reference metric classes and a float64 restatement, the flat model end to end
without NCHW logits, and the paper's size against the torch composition."""
import numpy as np
import pytest
import torch

from _flat_cases import PAPER_CFG
from _golden import load
from test_depth_evaluation import _cal, metrics_ref
from test_flat_evaluation import CASES, DEPTH_CASES, TAP_EPS, bilinear_numpy, meta, model_layout, projector, undo_transforms

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 5
SEG_LAYOUTS = [(n, lay) for n, (_, model) in CASES.items() for lay in (("image", "rows") if model else ("image",))]


@pytest.fixture(scope="module")
def FE():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import flat_evaluation
    return flat_evaluation


def _logits(ids, dtype, seed=0):
    """Logits [B, K, H, W] whose argmax is `ids` in fp32 and after rounding to bf16 (noise below 1, the winner at 2 or more)."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.rand((ids.shape[0], K) + tuple(ids.shape[1:]), generator=g)
    lg.scatter_(1, torch.from_numpy(ids.astype(np.int64))[:, None], 2.0, reduce="add")
    return lg.to(DEV).to(dtype)


def _as_rows(FE, nchw, name, pad_to=None):
    """An NCHW prediction as the flat model's head rows [B, H * W, C] (a [.., :C] view of padded rows when pad_to is given)."""
    b, c, h, w = nchw.shape
    perm = torch.from_numpy(FE.pixel_rows(h, w, *model_layout(name))).to(nchw.device)
    rows = torch.zeros((b, h * w, pad_to or c), dtype=nchw.dtype, device=nchw.device)
    rows[:, perm, :c] = nchw.flatten(2).transpose(1, 2)
    return rows[:, :, :c]


def _pred(FE, nchw, name, layout, pad_to=None):
    return nchw if layout == "image" else _as_rows(FE, nchw, name, pad_to)


def _compose(p, m, plane, mode, fill):
    """The torch composition: slice, interpolate, index at the rounded coordinates; plane float [B, H, W] -> [B, Npix]."""
    x = undo_transforms(plane, m, mode)
    oh, ow = x.shape[-2:]
    r = torch.from_numpy(np.around(p.v)).to(plane.device)
    c = torch.from_numpy(np.around(p.u)).to(plane.device)
    ok = (r >= 0) & (r < oh) & (c >= 0) & (c < ow)
    flat = x.flatten(1)[:, torch.where(ok, r * ow + c, 0).long()]
    return torch.where(ok, flat, torch.full_like(flat, fill))


# ------------------------------------------------------------------ segmentation
def test_pixel_rows_undo_flat_pixel_image(FE):
    from heal_swin_amd import ops
    for name in ("resize_pad_plain", "bp12"):
        h, w = meta(name)["model_size"]
        ps, tile = model_layout(name)
        rows = torch.arange(2 * h * w * 3, dtype=torch.float32, device=DEV).view(2, h * w, 3)
        img = ops.flat_pixel_image(rows, h, w, ps, tile)
        perm = torch.from_numpy(FE.pixel_rows(h, w, ps, tile)).to(DEV)
        assert torch.equal(img.flatten(2), rows[:, perm].transpose(1, 2))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,layout", SEG_LAYOUTS)
def test_labels_and_confusion_match_reference(FE, name, layout, dtype):
    from heal_swin_amd.evaluation import SegConfusion
    g = load("flat_eval")
    want = g[name + "/hp_labels"]
    p = projector(FE, name, layout=layout, device=DEV)
    pred = _pred(FE, _logits(g[name + "/ids"], dtype), name, layout, pad_to=8)
    got = p.labels(pred)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    ids = torch.from_numpy(g[name + "/ids"]).to(DEV)
    np.testing.assert_array_equal(p.labels(ids if layout == "image" else _as_rows(FE, ids[:, None], name)[:, :, 0]).cpu().numpy(), want)
    target = g[name + "/hp_target"]
    conf = SegConfusion(K, device=DEV)
    conf.update(p.logits(pred), torch.from_numpy(target).to(DEV), p)
    ref = np.bincount(target.reshape(-1).astype(np.int64) * K + want.reshape(-1), minlength=K * K).reshape(K, K)
    np.testing.assert_array_equal(conf.confmat.cpu().numpy(), ref)
    conf.update(p.logits(pred)[0], torch.from_numpy(target[0]).to(DEV), p)  # one sample without the batch axis
    ref = ref + np.bincount(target[0].astype(np.int64) * K + want[0], minlength=K * K).reshape(K, K)
    np.testing.assert_array_equal(conf.confmat.cpu().numpy(), ref)
    # the writer's numbers follow from the matrix
    inter, union = np.diag(ref), ref.sum(0) + ref.sum(1) - np.diag(ref)
    np.testing.assert_allclose(conf.iou().cpu().numpy(), (inter / union).astype(np.float32), rtol=1e-6)
    assert conf.accuracy().item() == pytest.approx(inter.sum() / ref.sum(), rel=1e-6)
    assert conf.accuracy(ignore_index=0).item() == pytest.approx(inter[1:].sum() / ref[1:].sum(), rel=1e-6)


@pytest.mark.parametrize("layout", ["image", "rows"])
def test_masked_image_plane_confusion(FE, layout):
    from heal_swin_amd.evaluation import SegConfusion
    name = "resize_pad_rot"
    g, m = load("flat_eval"), meta(name)
    kw = dict(zip(("patch_size", "tile"), model_layout(name))) if layout == "rows" else {}
    cov = FE.FlatCoverage(_cal(CASES[name][0]), m["nside"], m["base_pix"], m["rotate_pole"], m["model_size"], layout=layout, device=DEV, **kw)
    ids = g[name + "/ids"]
    target = np.random.default_rng(3).integers(0, K, ids.shape, dtype=np.uint8)
    valid = cov.valid_host
    assert 0.05 < valid.mean() < 0.95
    conf = SegConfusion(K, device=DEV)
    conf.update(cov.logits(_pred(FE, _logits(ids, torch.float32), name, layout, pad_to=8)), torch.from_numpy(target).to(DEV), cov, masked=True)
    ref = np.bincount(target[:, valid].reshape(-1).astype(np.int64) * K + ids[:, valid].reshape(-1), minlength=K * K).reshape(K, K)
    np.testing.assert_array_equal(conf.confmat.cpu().numpy(), ref)


# ------------------------------------------------------------------ depth
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", ["image", "rows"])
@pytest.mark.parametrize("f_out", [1, 2])
@pytest.mark.parametrize("name", DEPTH_CASES)
def test_projected_depth(FE, name, f_out, layout, dtype):
    g = load("flat_eval")
    nchw = torch.from_numpy(g[name + "/depth/pred"][:, :f_out]).to(DEV).to(dtype)
    pred = _pred(FE, nchw, name, layout, pad_to=4)
    src = nchw[:, 0].float().cpu().numpy().reshape(2, -1)
    p = projector(FE, name, layout=layout, device=DEV)
    got = p.depth(pred).cpu().numpy()
    if dtype == torch.float32:  # the reference's sample_mask, bit for bit, NaN positions included
        want = g[name + "/depth/nearest/hp"]
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    cov = p.covered_host
    img = projector(FE, name)  # bf16: the rounded values copied exactly
    np.testing.assert_array_equal(got.view(np.uint32)[:, cov], src[:, img.nearest_host[cov]].view(np.uint32))
    assert np.isnan(got[:, ~cov]).all()
    if f_out == 2:
        lv = nchw[:, 1].float().cpu().numpy().reshape(2, -1)
        np.testing.assert_array_equal(p.depth(pred, channel=1).cpu().numpy()[:, cov], lv[:, img.nearest_host[cov]])
    if layout == "image":
        np.testing.assert_array_equal(p.depth(nchw[:, 0]).cpu().numpy().view(np.uint32), got.view(np.uint32))
    pb = projector(FE, name, layout=layout, interpolation="bilinear", device=DEV)
    got = pb.depth(pred).cpu().numpy()
    mine, tap = bilinear_numpy(projector(FE, name, interpolation="bilinear"), src)
    np.testing.assert_array_equal(got.view(np.uint32)[~np.isnan(mine)], mine.view(np.uint32)[~np.isnan(mine)])  # fp32, no contraction
    np.testing.assert_array_equal(np.isnan(got), np.isnan(mine))
    if dtype == torch.float32:
        want = g[name + "/depth/bilinear/hp"]
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_array_equal(got[np.isinf(want)], want[np.isinf(want)])
        fin = np.isfinite(want)
        err = np.abs(got[fin].astype(np.float64) - want[fin]) / (TAP_EPS * tap[fin])
        print("bilinear: worst error over the tap bound", err.max())
        assert err.max() <= 1.0


@pytest.mark.parametrize("layout", ["image", "rows"])
@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("name", DEPTH_CASES)
def test_depth_metrics_match_reference(FE, name, mode, layout):
    from heal_swin_amd.depth_evaluation import DepthMetrics
    g = load("flat_eval")
    tm = float(g["total_mean"])
    nchw = torch.from_numpy(g[name + "/depth/pred"]).to(DEV)
    target = torch.from_numpy(g[name + "/depth/target"]).to(DEV)
    p = projector(FE, name, layout=layout, interpolation=mode, device=DEV)
    for f_out in (1, 2):
        pred = _pred(FE, nchw[:, :f_out], name, layout, pad_to=4)
        ms = [DepthMetrics(total_mean=tm, distance_ranges=[(0, 40)], device=DEV) for _ in range(3)]
        ms[0].update(pred, target, p)
        ms[1].update(pred, target, projector=p)
        assert torch.equal(ms[0].state, ms[1].state)  # two identical updates: bit-identical state
        hp = p.depth(pred)
        ms[2].update(hp, target)  # the projected map through the plain path: the same sums in the same order
        assert torch.equal(ms[0].state, ms[2].state)
        got = ms[0].compute()
        for k in ("mse", "SILogE", "iRMSE", "RelAE", "RelSE"):  # the reference metric classes (fp32 sums)
            want = float(g[f"{name}/depth/{mode}/{k}"])
            print(name, mode, layout, f_out, k, got[k], want)
            assert got[k] == pytest.approx(want, rel=1e-5, abs=0), (k, got[k], want)
        ref = metrics_ref(hp.cpu().numpy(), target.cpu().numpy(), tm, {"mse_range_00_40": (0, 40)}, False)
        for k, v in got.items():
            rel = 1e-6 if k in ("iRMSE", "SILogE") else 1e-9
            assert v == pytest.approx(ref[k], rel=rel, abs=0), (k, v, ref[k])
    # two updates accumulate
    ms[0].update(pred, target, p)
    assert ms[0].compute()["mse"] == pytest.approx(got["mse"], rel=1e-12)


def test_depth_metrics_logvar_bf16_strided_target(FE):
    from heal_swin_amd.depth_evaluation import DepthMetrics
    name = "resize_pad_plain"
    g = load("flat_eval")
    nchw = torch.from_numpy(g[name + "/depth/pred"]).to(DEV).bfloat16()
    buf = torch.zeros((2, 2048, 2), device=DEV)
    buf[:, :, 0] = torch.from_numpy(g[name + "/depth/target"]).to(DEV)
    target = buf[:, :, 0]
    for mode in ("nearest", "bilinear"):
        p = projector(FE, name, layout="rows", interpolation=mode, device=DEV)
        pred = _as_rows(FE, nchw, name, pad_to=8)
        m = DepthMetrics(total_mean=30.0, use_logvar=True, device=DEV)
        m.update(pred, target, p)
        hp = torch.stack([p.depth(pred), p.depth(pred, channel=1)], 1)
        m2 = DepthMetrics(total_mean=30.0, use_logvar=True, device=DEV)
        m2.update(hp, target)
        assert torch.equal(m.state, m2.state) and torch.allclose(m.median, m2.median, rtol=0, atol=0, equal_nan=True)
        assert np.isfinite(m.compute()["mean_std"])
    with pytest.raises(ValueError, match="channels"):
        DepthMetrics(use_logvar=True, device=DEV).update(pred[:, :, :1], target, p)
    with pytest.raises(ValueError, match="target must be"):
        DepthMetrics(device=DEV).update(pred, target[:, :100], p)


# ------------------------------------------------------------------ the flat model end to end
@pytest.mark.parametrize("name", ["resize_pad_rot", "bp12"])
def test_model_rows_to_confusion_without_nchw_logits(FE, name):
    from heal_swin_amd.evaluation import SegConfusion
    from test_gpu_flat_swin import _model
    model = _model(CASES[name][1])[0].eval()
    m, cal = meta(name), _cal(CASES[name][0])
    h, w = m["model_size"]
    x = torch.randn((2, 3, h, w), generator=torch.Generator().manual_seed(5)).to(DEV)
    kw = {k: m[k] for k in ("base_pix", "rotate_pole", "orig_size", "padding", "s2_bkgd_class")}
    p = FE.FlatToHPProjector.for_model(model, cal, m["nside"], device=DEV, **kw)
    target = torch.from_numpy(load("flat_eval")[name + "/hp_target"]).to(DEV)
    with torch.no_grad():
        nchw = model(x)
        rows = model.forward_rows(x)
        assert tuple(rows.shape) == (2, h * w, K) and rows.dtype == torch.float32
        assert torch.equal(nchw.flatten(2), rows[:, torch.from_numpy(FE.pixel_rows(h, w, *model_layout(name))).to(DEV)].transpose(1, 2))
        labels = _compose(p, m, nchw.argmax(1).double(), "nearest", float(m["s2_bkgd_class"])).long()
        assert torch.equal(p.labels(rows).long(), labels)
        ref = torch.bincount(target.long().reshape(-1) * K + labels.reshape(-1), minlength=K * K).reshape(K, K)
        conf = SegConfusion(K, device=DEV)
        del nchw, rows
        torch.cuda.synchronize()
        model.forward_rows(x)  # allocator warm: the measured call reuses cached blocks
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        rows = model.forward_rows(x)
        conf.update(p.logits(rows), target, p)
        torch.cuda.synchronize()
        assert torch.equal(conf.confmat, ref)
        # what stays allocated is the head rows alone (16 floats per pixel at most): no [B, K, H, W] tensor next to them
        assert torch.cuda.memory_allocated() - before <= rows.untyped_storage().nbytes() + 4096
        assert p.logits(rows).untyped_storage().data_ptr() == rows.untyped_storage().data_ptr()


# ------------------------------------------------------------------ the paper's size
def test_paper_size_equals_torch_composition(FE):
    from heal_swin_amd.depth_evaluation import DepthMetrics
    from heal_swin_amd.evaluation import SegConfusion
    b, k, (h, w), nside = 8, 12, (640, 768), 256
    ps, tile = PAPER_CFG["patch_size"], PAPER_CFG["window_size"] * 2 ** (len(PAPER_CFG["depths"]) - 1)
    cal = _cal("fv_966x1280")
    m = dict(orig_size=(966, 1280), padding=(0, 0, 0, 0))
    g = torch.Generator(device=DEV).manual_seed(0)
    rows = torch.randn((b, h * w, 16), generator=g, device=DEV)[:, :, :k]
    perm = torch.from_numpy(FE.pixel_rows(h, w, ps, tile)).to(DEV)
    p = FE.FlatToHPProjector(cal, nside, model_size=(h, w), layout="rows", patch_size=ps, tile=tile, device=DEV)
    cov = p.covered_host.mean()
    assert 0.3 <= cov <= 0.9
    ids = rows.argmax(2)[:, perm].view(b, h, w)  # the NCHW argmax
    labels = _compose(p, m, ids.double(), "nearest", 0.0).long()
    assert torch.equal(p.labels(rows).long(), labels)
    target = torch.randint(0, k, (b, p.n_out), generator=g, device=DEV).to(torch.uint8)
    conf = SegConfusion(k, device=DEV)
    conf.update(p.logits(rows), target, p)
    assert torch.equal(conf.confmat, torch.bincount(target.long().reshape(-1) * k + labels.reshape(-1), minlength=k * k).reshape(k, k))
    # depth: channel 0 of the same rows as a depth map
    depth = rows[:, :, 0]
    plane = depth[:, perm].view(b, h, w)
    want = _compose(p, m, plane, "nearest", float("nan"))
    got = p.depth(depth)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(want)], want[~torch.isnan(want)])
    pb = FE.FlatToHPProjector(cal, nside, model_size=(h, w), layout="rows", patch_size=ps, tile=tile, interpolation="bilinear", device=DEV)
    want = _compose(pb, m, plane, "bilinear", float("nan"))  # torch's GPU bilinear kernel: its own weights, so a looser bound
    got = pb.depth(depth)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    fin = ~torch.isnan(want)
    assert (got[fin] - want[fin]).abs().max().item() <= 1e-3 * plane.abs().max().item()
    dtarget = torch.rand((b, p.n_out), generator=g, device=DEV) * 50 + 0.5
    m1, m2 = DepthMetrics(total_mean=20.0, device=DEV), DepthMetrics(total_mean=20.0, device=DEV)
    m1.update(depth, dtarget, pb)
    m2.update(got, dtarget)
    assert torch.equal(m1.state, m2.state)
