"""heal_swin_amd.evaluation on the GPU: the back-projection and confusion-matrix kernels (csrc/evaluation.hip) bit-exact
against numpy restatements of the reference's project_hp_mask_back / project_hp_img_back (healpy get_interp_val) and of
torchmetrics' bincount, on hand-made inputs, on a model's own output and at full size (966 x 1280, nside 256)."""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


@pytest.fixture(scope="module")
def E():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import evaluation
    return evaluation


def _cal(key):
    from tests.test_projection import calibrations
    return calibrations()[key]


# ------------------------------------------------------------------ numpy restatements
def argmax_ref(logits):
    """torch.max(logits, 1)'s index on float32 [B, K, N] (np.argmax: first maximum, the first NaN wins)."""
    return np.argmax(logits, axis=1)


def masks_ref(pred_labels, nearest, nside, base_pix, bkgd):
    """project_hp_mask_back: labels completed to 12 base pixels with s2_bkgd_class, then read at the nearest pixel."""
    b, npix = pred_labels.shape
    full = np.full((b, 12 * nside * nside), bkgd, dtype=np.uint8)
    full[:, :npix] = pred_labels
    return full[:, nearest]


def images_ref(hp_img, pix, wgt, nside):
    """project_hp_img_back: np.sum(m[p] * w, 0) per plane, the map completed with 255.0."""
    b, c, npix = hp_img.shape
    out = np.empty((b, c) + pix.shape[1:], dtype=np.float64)
    for i in range(b):
        for ch in range(c):
            m = np.full(12 * nside * nside, 255.0)
            m[:npix] = hp_img[i, ch]
            out[i, ch] = np.sum(m[pix] * wgt, 0)
    return out


def conf_ref(target, pred, k):
    return np.bincount(target.astype(np.int64).reshape(-1) * k + pred.astype(np.int64).reshape(-1), minlength=k * k).reshape(k, k)


def _logits(rng, b, k, npix, dtype, pad=None):
    """Small-integer logits (many ties) with NaNs sprinkled in; pad: the model's padded native rows viewed as [B, K, Npix]."""
    x = rng.integers(-3, 4, (b, npix, pad or k)).astype(np.float32)
    nan = rng.random((b, npix, pad or k)) < 0.01
    x[nan] = np.nan
    t = torch.from_numpy(x).to(DEV).to(dtype)
    view = t[:, :, :k].transpose(1, 2) if pad else t.transpose(1, 2).contiguous()
    return view, view.float().cpu().numpy()


def hand_table_projector(E):
    """An HPBackProjector over 16 HEALPix pixels with a hand-built table of 3 output pixels: pixel 0 interpolates from four
    pixels of the map, pixel 1 has one tap outside [0, npix) (the first index past the map) with weight 0, pixel 2 one
    (a negative index) with weight 0.25.  What a tap outside reads is the fill rule of each method."""
    p = E.HPBackProjector.__new__(E.HPBackProjector)
    p.nside, p.base_pix, p.s2_bkgd_class, p.device, p.shape = 4, 1, 0, torch.device(DEV, torch.cuda.current_device()), (1, 3)
    idx = np.array([[3, 16, 7], [5, 1, -1], [9, 2, 0], [14, 4, 12]], dtype=np.int32).reshape(4, 1, 3)
    wgt = np.array([[0.5, 0.0, 0.375], [0.125, 0.5, 0.25], [0.25, 0.25, 0.125], [0.125, 0.25, 0.25]]).reshape(4, 1, 3)
    p.idx, p.wgt = torch.from_numpy(idx).to(DEV), torch.from_numpy(wgt).to(DEV)
    return p


def hand_table_ref(values, p, fill):
    """((v0 w0 + v1 w1) + v2 w2) + v3 w3 per output pixel of float64 maps [n, npix] completed with `fill` outside."""
    idx, w = p.idx.cpu().numpy().reshape(4, 3), p.wgt.cpu().numpy().reshape(4, 3)
    inside = (idx >= 0) & (idx < p.npix)
    v = np.where(inside, values[:, np.where(inside, idx, 0)], fill)
    return ((v[:, 0] * w[0] + v[:, 1] * w[1]) + v[:, 2] * w[2]) + v[:, 3] * w[3]


# ------------------------------------------------------------------ kernels against the restatements
@pytest.fixture(scope="module")
def small_proj(E):
    """rv_60x80 at nside 16: the frame sees part of the sphere, some pixels land outside the 8 base pixels."""
    p = E.HPBackProjector(_cal("rv_60x80"), 16, base_pix=8, output_resolution=1.0, rotate_pole=True, s2_bkgd_class=3, device=DEV)
    assert p.shape == (60, 80)
    return p


def test_tables_and_valid_mask(E, small_proj):
    p = small_proj
    u, v = E.get_uv_from_hw(60, 80, 1.0)
    theta, phi = E.project_img_points_to_s2(u, v, _cal("rv_60x80"), True)
    nearest, pix, wgt = E.hp_nearest_pix_idcs(16, theta, phi)
    assert np.array_equal(p.nearest.cpu().numpy(), nearest) and np.array_equal(p.idx.cpu().numpy(), pix)
    assert np.array_equal(p.wgt.cpu().numpy(), wgt)
    # HPMaskedIoU.get_mask: back-project an all-zero map with background 1, keep the zeros
    full = np.ones(12 * 16 * 16, dtype=np.uint8)
    full[: p.npix] = 0
    assert np.array_equal(p.valid.cpu().numpy(), full[nearest] == 0)
    assert 0 < int(p.valid.sum()) < p.n_out, "the case should exercise both covered and uncovered pixels"


def test_backproject_labels(E, small_proj):
    rng = np.random.default_rng(0)
    p = small_proj
    lab = rng.integers(0, 20, (3, p.npix), dtype=np.uint8)
    out = p.masks(torch.from_numpy(lab).to(DEV))
    assert out.dtype == torch.uint8 and out.shape == (3, 60, 80)
    assert np.array_equal(out.cpu().numpy(), masks_ref(lab, p.nearest.cpu().numpy(), 16, 8, 3))
    # a strided label view (every other image of a batch) and a single map
    lab6 = torch.from_numpy(rng.integers(0, 20, (6, p.npix), dtype=np.uint8)).to(DEV)
    assert torch.equal(p.masks(lab6[::2]), p.masks(lab6[::2].contiguous()))
    assert torch.equal(p.masks(lab6[1]), p.masks(lab6[1:2]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pad", [None, 16])
def test_backproject_argmax_of_logits(E, small_proj, dtype, pad):
    rng = np.random.default_rng(1)
    p = small_proj
    view, ref_logits = _logits(rng, 2, 10, p.npix, dtype, pad)
    assert torch.isnan(view).any()
    out = p.masks(view).cpu().numpy()
    pred = argmax_ref(ref_logits)
    assert np.array_equal(pred, torch.max(view.float(), 1)[1].cpu().numpy())  # the restatement is torch.max's rule
    assert np.array_equal(out, masks_ref(pred.astype(np.uint8), p.nearest.cpu().numpy(), 16, 8, 3))


def test_backproject_image_bit_exact(E, small_proj):
    rng = np.random.default_rng(2)
    p = small_proj
    img = rng.integers(0, 256, (2, 3, p.npix), dtype=np.uint8)
    out = p.images(torch.from_numpy(img).to(DEV))
    assert out.dtype == torch.float64 and out.shape == (2, 3, 60, 80)
    ref = images_ref(img, p.idx.cpu().numpy().astype(np.int64), p.wgt.cpu().numpy(), 16)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert torch.equal(p.images(torch.from_numpy(img[1]).to(DEV)), out[1])
    # the fill rule on the hand-built table: a tap outside the map reads 255.0, so it adds exactly 255.0 * its weight
    h = hand_table_projector(E)
    img = np.concatenate([np.zeros((1, h.npix), dtype=np.uint8), rng.integers(0, 256, (2, h.npix), dtype=np.uint8)])
    out = h.images(torch.from_numpy(img).to(DEV)).cpu().numpy().reshape(3, 3)
    assert out[0].tolist() == [0.0, 255.0 * 0.0, 255.0 * 0.25]
    assert np.array_equal(out, hand_table_ref(img.astype(np.float64), h, 255.0))


# ------------------------------------------------------------------ confusion matrix
@pytest.mark.parametrize("k", [10, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_confusion_hp_domain_from_logits(E, k, dtype):
    rng = np.random.default_rng(k)
    npix = 8 * 32 * 32
    view, ref_logits = _logits(rng, 3, k, npix, dtype, pad=k + (-k) % 16 + (4 if k == 64 else 0))
    tgt = rng.integers(0, k, (3, npix), dtype=np.uint8)
    m = E.SegConfusion(k, device=DEV)
    m.update(view, torch.from_numpy(tgt).to(DEV))
    ref = conf_ref(tgt, argmax_ref(ref_logits), k)
    assert np.array_equal(m.confmat.cpu().numpy(), ref)
    m.update(view, torch.from_numpy(tgt).to(DEV))  # accumulates
    assert np.array_equal(m.confmat.cpu().numpy(), 2 * ref)


def test_confusion_labels_and_one_class(E):
    rng = np.random.default_rng(5)
    n = 8 * 128 * 128
    m = E.SegConfusion(10, device=DEV)
    pred = rng.integers(0, 10, (4, n), dtype=np.uint8)
    tgt = rng.integers(0, 10, (4, n), dtype=np.uint8)
    m.update(torch.from_numpy(pred).to(DEV), torch.from_numpy(tgt).to(DEV))
    assert np.array_equal(m.confmat.cpu().numpy(), conf_ref(tgt, pred, 10))
    # one class everywhere: every lane of every wave adds into one bin (the contention case)
    m.reset()
    ones = torch.full((4, n), 7, dtype=torch.uint8, device=DEV)
    m.update(ones, ones)
    ref = np.zeros((10, 10), dtype=np.int64)
    ref[7, 7] = 4 * n
    assert np.array_equal(m.confmat.cpu().numpy(), ref)
    # mostly one class with a sprinkle of others (the skewed distribution of a segmentation)
    m.reset()
    p2 = np.where(rng.random((4, n)) < 0.97, 0, pred).astype(np.uint8)
    t2 = np.where(rng.random((4, n)) < 0.97, 0, tgt).astype(np.uint8)
    m.update(torch.from_numpy(p2).to(DEV), torch.from_numpy(t2).to(DEV))
    assert np.array_equal(m.confmat.cpu().numpy(), conf_ref(t2, p2, 10))


def test_confusion_raises_on_out_of_range(E):
    m = E.SegConfusion(5, device=DEV)
    pred = torch.zeros((2, 100), dtype=torch.uint8, device=DEV)
    tgt = torch.zeros((2, 100), dtype=torch.uint8, device=DEV)
    tgt[1, 17] = 5
    with pytest.raises(ValueError, match="target"):
        m.update(pred, tgt)
    with pytest.raises(ValueError, match="target"):
        m.iou()
    m.reset()
    pred[0, 3] = 9
    with pytest.raises(ValueError, match="predicted"):
        m.update(pred, torch.zeros_like(tgt))
    m.reset()
    with pytest.raises(ValueError):
        m.update(torch.zeros((1, 5, 100), device=DEV), torch.zeros((1, 100), dtype=torch.uint8, device=DEV)[:, :99])


# hand: (classes, prediction kind) through a hand-built nearest table of 65 image pixels, one full wave and one lane, whose
# pixels 0 and 64 are uncovered: with masked=True the first lane of both waves has nothing to count, and in the second wave
# no other lane has either (the contract of the waves' aggregated add, csrc/hs_histogram.h: wave_count_lead)
HAND_TABLES = [pytest.param(masked, (k, kind), id=f"{masked}-hand65-k{k}-{kind}")
               for masked in (False, True) for k in (1, 3, 64) for kind in ("labels", "f32", "bf16")]


def _hand_table_case(rng, k, kind):
    npix, n_out = 100, 65
    nearest = rng.integers(0, npix, n_out).astype(np.int32)
    nearest[[0, 64]] = npix
    p = types.SimpleNamespace(nearest=torch.from_numpy(nearest).to(DEV), n_out=n_out, npix=npix, shape=(n_out,), s2_bkgd_class=k - 1,
                              valid=torch.from_numpy(nearest < npix).to(DEV))
    if kind == "labels":
        lab = rng.integers(0, k, (3, npix), dtype=np.uint8)
        return p, torch.from_numpy(lab).to(DEV), lab
    view, ref_logits = _logits(rng, 3, k, npix, torch.float32 if kind == "f32" else torch.bfloat16)
    return p, view, argmax_ref(ref_logits).astype(np.uint8)


@pytest.mark.parametrize("masked,hand", [pytest.param(False, None, id="False"), pytest.param(True, None, id="True")] + HAND_TABLES)
def test_confusion_image_plane(E, small_proj, masked, hand):
    rng = np.random.default_rng(6)
    if hand is not None:
        k, kind = hand
        p, pred, labels = _hand_table_case(rng, k, kind)
        tgt = torch.from_numpy(rng.integers(0, k, (3, p.n_out), dtype=np.uint8)).to(DEV)
        m = E.SegConfusion(k, device=DEV)
        m.update(pred, tgt, projector=p, masked=masked)
        back = torch.from_numpy(np.concatenate([labels, np.full((3, 1), k - 1, dtype=np.uint8)], 1)).to(DEV)[:, p.nearest.long()]
        keep = p.valid.expand_as(tgt) if masked else torch.ones_like(tgt, dtype=torch.bool)
        ref = torch.bincount(tgt[keep].long() * k + back[keep].long(), minlength=k * k).reshape(k, k)
        assert int(ref.sum()) == 3 * (63 if masked else 65) and torch.equal(m.confmat, ref)
        return
    p = small_proj
    k = 12
    view, ref_logits = _logits(rng, 3, k, p.npix, torch.float32, pad=16)
    tgt = rng.integers(0, k, (3,) + p.shape, dtype=np.uint8)
    m = E.SegConfusion(k, device=DEV)
    m.update(view, torch.from_numpy(tgt).to(DEV), projector=p, masked=masked)
    back = masks_ref(argmax_ref(ref_logits).astype(np.uint8), p.nearest.cpu().numpy(), 16, 8, p.s2_bkgd_class)
    if masked:
        valid = p.valid.cpu().numpy()
        ref = conf_ref(tgt[:, valid], back[:, valid], k)
    else:
        ref = conf_ref(tgt, back, k)
    assert np.array_equal(m.confmat.cpu().numpy(), ref)


def test_confusion_mixed_cameras(E):
    rng = np.random.default_rng(7)
    projs = [E.HPBackProjector(_cal(key), 16, output_resolution=(24, 32), rotate_pole=True, device=DEV) for key in ("mvl_96x128", "rv_60x80")]
    lab = rng.integers(0, 6, (5, projs[0].npix), dtype=np.uint8)
    tgt = rng.integers(0, 6, (5, 24, 32), dtype=np.uint8)
    cams = [0, 1, 1, 0, 0]
    m = E.SegConfusion(6, device=DEV)
    m.update(torch.from_numpy(lab).to(DEV), torch.from_numpy(tgt).to(DEV), projector=projs, camera=cams)
    ref = sum(conf_ref(tgt[i], masks_ref(lab[i:i + 1], projs[c].nearest.cpu().numpy(), 16, 8, 0), 6) for i, c in enumerate(cams))
    assert np.array_equal(m.confmat.cpu().numpy(), ref)


# ------------------------------------------------------------------ end to end on a model's output
def test_end_to_end_model_to_metrics(E):
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys

    nside, bp, k = 64, 8, 10
    cfg = dict(patch_size=4, window_size=64, shift_size=32, shift_strategy="nest_roll", rel_pos_bias="flat", embed_dim=96,
               depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], drop_path_rate=0.0)  # HEAL-SWIN-T
    spec = dict(dim_in=bp * nside * nside, f_in=3, f_out=k, base_pix=bp, class_names=[])
    torch.manual_seed(3)
    model = SwinHPTransformerSys(SwinHPTransformerConfig(**cfg), DataSpec(**spec)).to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    x = torch.randint(0, 256, (2, 3, spec["dim_in"]), generator=g).float().to(DEV)
    y = torch.randint(0, k, (2, spec["dim_in"]), generator=g).to(torch.uint8).to(DEV)
    with torch.no_grad():
        logits = model(x)
    assert logits.shape == (2, k, spec["dim_in"])
    preds = torch.max(logits, 1)[1]
    m = E.SegConfusion(k, device=DEV)
    m.update(logits, y)
    ref = torch.bincount(y.long().reshape(-1) * k + preds.reshape(-1), minlength=k * k).reshape(k, k)
    assert torch.equal(m.confmat, ref)
    # image plane: the reference's back-projected metrics on a quarter-size FV frame
    p = E.HPBackProjector(_cal("fv_966x1280"), nside, base_pix=bp, output_resolution=0.25, device=DEV)
    tgt = torch.randint(0, k, (2,) + p.shape, generator=g).to(torch.uint8).to(DEV)
    full = torch.cat([preds, torch.zeros((2, 4 * nside * nside), dtype=preds.dtype, device=DEV)], 1)
    back = full.index_select(1, p.nearest.reshape(-1).long()).reshape((2,) + p.shape)
    assert torch.equal(p.masks(logits).long(), back)
    for masked in (False, True):
        m.reset()
        m.update(logits, tgt, projector=p, masked=masked)
        sel = p.valid.expand_as(tgt) if masked else torch.ones_like(tgt, dtype=torch.bool)
        ref = torch.bincount(tgt.long()[sel] * k + back[sel], minlength=k * k).reshape(k, k)
        assert torch.equal(m.confmat, ref)
    iou = m.iou()
    assert iou.shape == (k,) and torch.isfinite(iou).all()


# ------------------------------------------------------------------ full size
def test_full_size_fv_nside256(E):
    rng = np.random.default_rng(8)
    nside, bp = 256, 8
    p = E.HPBackProjector(_cal("fv_966x1280"), nside, base_pix=bp, device=DEV)
    assert p.shape == (966, 1280)
    nearest = p.nearest.cpu().numpy()
    lab = rng.integers(0, 10, (2, p.npix), dtype=np.uint8)
    assert np.array_equal(p.masks(torch.from_numpy(lab).to(DEV)).cpu().numpy(), masks_ref(lab, nearest, nside, bp, 0))
    view, ref_logits = _logits(rng, 2, 10, p.npix, torch.float32, pad=16)
    assert np.array_equal(p.masks(view).cpu().numpy(), masks_ref(argmax_ref(ref_logits).astype(np.uint8), nearest, nside, bp, 0))
    img = rng.integers(0, 256, (1, 3, p.npix), dtype=np.uint8)
    out = p.images(torch.from_numpy(img).to(DEV)).cpu().numpy()
    assert np.array_equal(out, images_ref(img, p.idx.cpu().numpy().astype(np.int64), p.wgt.cpu().numpy(), nside))


# ------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from heal_swin_amd.evaluation import SegConfusion
    g = torch.Generator().manual_seed(100 + rank)
    pred = torch.randint(0, 7, (2, 4096), generator=g).to(torch.uint8).to(DEV)
    tgt = torch.randint(0, 7, (2, 4096), generator=g).to(torch.uint8).to(DEV)
    m = SegConfusion(7, device=DEV)
    m.update(pred, tgt)
    local = m.confmat.cpu().clone()
    m.all_reduce()
    q.put((rank, local.numpy(), m.confmat.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_two_ranks():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict((r, (a, b)) for r, a, b in (q.get(timeout=300) for _ in range(world)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    total = res[0][0] + res[1][0]
    assert not np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], total) and np.array_equal(res[1][1], total)
