"""The flat data path on the GPU (heal_swin_amd/flat_data.py, csrc/flat_data.hip): frames, masks and depth maps cropped, resized
and padded in one HIP pass each, as the reference's NCHW tensors or as the rows the flat model reads, against
tests/golden/flat_data.npz, torch's GPU calls and the existing layout ops.  The two bilinear rules are those of test_flat_data.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _golden import load
from test_flat_data import CONFIGS, check_fp32_rule, check_uint8_rule
from test_gpu_depth_data import NORMS, TRANSFORMS, _check, _scale

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = [((640, 768), (0, 0, 0, 0)), (512, (-19, 0, -19, 0))]  # 966 x 1280 -> 640 x 768 and -> 512 x 678 -> 512 x 640
PAPER = dict(patch_size=2, tile=64)  # p = 2, window 8, four stages: T = 8 * 2^3
TINY = dict(patch_size=2, tile=8)    # p = 2, window 4, two stages
TINY_CONFIGS = [((48, 80), (0, 0, 0, 0)), ((40, 70), (5, 4, 5, 4)), (None, (-8, 0, -8, 0))]  # 96 x 128 -> multiples of p T = 16


@pytest.fixture(scope="module")
def FD():
    import heal_swin_amd.flat_data as m
    return m


@pytest.fixture(scope="module")
def DD():
    import heal_swin_amd.depth_data as m
    return m


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def gpu_reference(x, t, mode):
    """Resize -> Pad of [B, C, H0, W0] with torch's GPU calls (no crop_green)."""
    if not t.identity:
        x = F.interpolate(x, size=list(t.resized), mode=mode, **(dict(align_corners=False) if mode == "bilinear" else {}))
    left, top, right, bottom = t.padding
    x = x[..., max(-top, 0):x.shape[-2] - max(-bottom, 0), max(-left, 0):x.shape[-1] - max(-right, 0)]
    return F.pad(x, [max(left, 0), max(right, 0), max(top, 0), max(bottom, 0)])


def full_inputs(batch=2, seed=0):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (batch, 3, 966, 1280), dtype=np.uint8)
    masks = rng.integers(0, 12, (batch, 966, 1280), dtype=np.uint8)
    depth = rng.uniform(0.2, 400.0, (batch, 966, 1280)).astype(np.float32)
    r = rng.random(depth.shape)
    depth[r < 0.08] = 1000.0
    depth[(r >= 0.08) & (r < 0.10)] = 0.0
    return frames, masks, depth


# ------------------------------------------------------------------ 1. nearest: bit-equal
def test_nearest_matches_the_golden(FD):
    g = load("flat_data")
    masks, depth = torch.from_numpy(g["masks"]).to(DEV), torch.from_numpy(g["depth"]).to(DEV)
    for name, (size, padding) in CONFIGS.items():
        t = FD.FlatFrameTransform((96, 128), size=size, padding=padding, device=DEV)
        assert np.array_equal(t.masks(masks).cpu().numpy(), g[f"{name}/masks"]), name
        assert np.array_equal(t.depth(depth).cpu().numpy().view(np.uint32), g[f"{name}/depth_nearest"].view(np.uint32)), name


@pytest.mark.parametrize("size,padding", FULL)
def test_nearest_full_size_matches_torch_on_the_gpu(FD, size, padding):
    _, masks, depth = full_inputs()
    masks, depth = torch.from_numpy(masks).to(DEV), torch.from_numpy(depth).to(DEV)
    depth[0, 5, 7], depth[1, 900, 1200] = float("nan"), float("inf")
    t = FD.FlatFrameTransform((966, 1280), size=size, padding=padding, device=DEV, **PAPER)
    ref_m = gpu_reference(masks[:, None].float(), t, "nearest")[:, 0].to(torch.uint8)
    ref_d = gpu_reference(depth[:, None], t, "nearest")[:, 0]
    out_m, out_d = t.masks(masks), t.depth(depth)
    assert out_m.shape == ref_m.shape == (2, *t.out_size)
    assert torch.equal(out_m, ref_m) and torch.equal(bits(out_d), bits(ref_d))
    from heal_swin_amd import ops
    assert torch.equal(t.masks(masks, layout="rows").rows, ops.flat_labels(ref_m, 2, 64))
    assert torch.equal(bits(t.depth(depth, layout="rows").rows), bits(ops.flat_depth_target(ref_d, 2, 64)))


# ------------------------------------------------------------------ 2. bilinear depth: 4 ulp of the exact value of the taps
@pytest.mark.parametrize("size,padding", FULL)
def test_bilinear_depth_full_size(FD, size, padding):
    depth = full_inputs(batch=1, seed=1)[2]
    t = FD.FlatFrameTransform((966, 1280), size=size, padding=padding, device=DEV)
    out = t.depth(torch.from_numpy(depth).to(DEV), interpolation="bilinear").cpu().numpy()
    check_fp32_rule(out, t.tables("bilinear"), depth, f"{size} {padding}")


def test_bilinear_depth_small_and_non_finite(FD):
    g = load("flat_data")
    depth = g["depth"].copy()
    depth[0, 10, 10], depth[1, 50, 60], depth[1, 80, 100] = np.inf, np.nan, -np.inf
    for name, (size, padding) in CONFIGS.items():
        t = FD.FlatFrameTransform((96, 128), size=size, padding=padding, device=DEV)
        tab = t.tables("bilinear")
        out = t.depth(torch.from_numpy(depth).to(DEV), interpolation="bilinear").cpu().numpy()
        host = tab.apply_host(depth)  # the same fp32 formula in numpy: IEEE arithmetic, bit for bit
        assert np.array_equal(np.isnan(out), np.isnan(host)), name
        keep = ~np.isnan(host)
        assert np.array_equal(out[keep].view(np.uint32), host[keep].view(np.uint32)), name
        check_fp32_rule(t.depth(torch.from_numpy(g["depth"]).to(DEV), interpolation="bilinear").cpu().numpy(), tab, g["depth"], name)


# ------------------------------------------------------------------ 3. uint8 frames
@pytest.mark.parametrize("size,padding", FULL)
def test_frames_full_size(FD, size, padding):
    frames = np.random.default_rng(0).integers(0, 256, (1, 3, 966, 1280), dtype=np.uint8)
    x = torch.from_numpy(frames).to(DEV)
    t = FD.FlatFrameTransform((966, 1280), size=size, padding=padding, device=DEV)
    out = t.frames(x)
    assert out.dtype == torch.uint8 and out.shape == (1, 3, *t.out_size)
    check_uint8_rule(out.cpu().numpy(), t.tables("bilinear"), frames, f"{size} {padding}", max_share=0.002)
    # torch's own GPU result obeys the rule against the same taps, and the two agree outside the tie window
    ref = torch.round(gpu_reference(x.float(), t, "bilinear")).to(torch.uint8)
    check_uint8_rule(ref.cpu().numpy(), t.tables("bilinear"), frames, f"torch {size} {padding}")


def test_frames_match_the_golden(FD):
    g = load("flat_data")
    for name, (size, padding) in CONFIGS.items():
        t = FD.FlatFrameTransform((96, 128), size=size, padding=padding, device=DEV)
        out = t.frames(torch.from_numpy(g["frames"]).to(DEV)).cpu().numpy()
        check_uint8_rule(out, t.tables("bilinear"), g["frames"], name)
        assert np.array_equal(out, t.tables("bilinear").apply_host(g["frames"])), name
        if t.identity:
            assert np.array_equal(out, g[f"{name}/frames"]), name


# ------------------------------------------------------------------ 4. rows == layout op of the image
def _rows_equal_layout_op(FD, t, frames, masks, depth, p, T):
    from heal_swin_amd import ops
    for dtype in (torch.float32, torch.bfloat16):
        rows = t.frames(frames, dtype=dtype, layout="rows")
        assert (rows.patch_size, rows.tile, rows.height, rows.width) == (p, T, *t.out_size)
        assert torch.equal(rows.rows, ops.flat_patch_rows(t.frames(frames), p, T, dtype))
    assert torch.equal(t.masks(masks, layout="rows").rows, ops.flat_labels(t.masks(masks), p, T))
    target = None
    for mode in ("nearest", "bilinear"):
        img, rows = t.depth(depth, mode, target), t.depth(depth, mode, target, layout="rows").rows
        assert torch.equal(bits(rows), bits(ops.flat_depth_target(img, p, T)))


@pytest.mark.parametrize("size,padding", TINY_CONFIGS)
def test_rows_equal_the_layout_op_tiny(FD, size, padding):
    g = load("flat_data")
    t = FD.FlatFrameTransform((96, 128), size=size, padding=padding, device=DEV, **TINY)
    _rows_equal_layout_op(FD, t, *(torch.from_numpy(g[k]).to(DEV) for k in ("frames", "masks", "depth")), 2, 8)


@pytest.mark.parametrize("size,padding", FULL)
def test_rows_equal_the_layout_op_paper_size(FD, size, padding):
    t = FD.FlatFrameTransform((966, 1280), size=size, padding=padding, device=DEV, **PAPER)
    _rows_equal_layout_op(FD, t, *(torch.from_numpy(a).to(DEV) for a in full_inputs()), 2, 64)


# ------------------------------------------------------------------ 5. the depth chain
def test_depth_chain(FD, DD):
    g = load("flat_data")
    size, padding = CONFIGS["pad_int"]
    depth = torch.from_numpy(g["depth"]).to(DEV)
    t = FD.FlatFrameTransform((96, 128), size=size, padding=padding, device=DEV)
    plain = t.depth(depth)
    assert (plain == 0).any() and (plain == 1000).any()
    t16 = FD.FlatFrameTransform((96, 128), size=(40, 70), padding=(5, 4, 5, 4), device=DEV, **TINY)
    for T in TRANSFORMS:
        for N in NORMS:
            for M in (False, True):
                tag = f"{T}/{N}/{int(M)}"
                tr = DD.DepthTargetTransform(T, N, mask_background=M, zero_is_background=False)
                for mode in ("nearest", "bilinear"):
                    out = t.depth(depth, mode, target=tr)
                    assert torch.equal(bits(out), bits(tr.prepare(t.depth(depth, mode).flatten(1)).view_as(out))), (tag, mode)
                    rows = t16.depth(depth, mode, target=tr, layout="rows").rows
                    assert torch.equal(bits(rows), bits(tr.prepare(t16.depth(depth, mode, layout="rows").rows))), (tag, mode)
                out = t.depth(depth, target=tr)[0].cpu().numpy()
                _check(out, g[f"chain/{tag}"], g[f"chain/{T}/None/{int(M)}"], _scale(DD, T, N, M), T == "None" and N == "None", tag)
    with pytest.raises(ValueError):
        t.depth(depth, target=DD.DepthTargetTransform("log", "standardize"))


# ------------------------------------------------------------------ 6. the model takes the rows
def _tiny_model(f_out):
    """64 x 64, p = 2, window 8 (64 tokens), head dim 32 at every stage, T = 32.  Bit-equal gradients between two calls need a
    backward that is itself reproducible: 64-token windows with head dim 32 take the MFMA attention kernels (fp32 and bf16), which
    reduce through a workspace in a fixed order; smaller windows take window_attn_generic.hip, whose relative-position-bias and
    cosine-scale gradients are float atomicAdd sums (the only float atomics on the training path), so two calls on the SAME
    NCHW tensors already differ there in the last bits."""
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_transformer import SwinTransformerConfig, SwinTransformerSys
    cfg = dict(window_size=8, patch_size=2, shift_size=2, depths=[2, 2, 2], num_heads=[1, 2, 4], embed_dim=32, use_cos_attn=True,
               use_v2_norm_placement=True, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0)
    torch.manual_seed(0)
    return SwinTransformerSys(SwinTransformerConfig(**cfg), DataSpec(dim_in=(64, 64), f_in=3, f_out=f_out, base_pix=None,
                                                                     class_names=[])).to(DEV)


def _loss_and_grads(m, call):
    m.zero_grad(set_to_none=True)
    loss = call()
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_model_takes_rows(FD, DD, dtype):
    g = load("flat_data")
    frames, masks, depth = (torch.from_numpy(g[k]).to(DEV) for k in ("frames", "masks", "depth"))
    for f_out in (5, 1):
        m = _tiny_model(f_out)
        m.compute_dtype = dtype
        t = FD.FlatFrameTransform.for_model(m, (96, 128), size=(56, 60), padding=(2, 4, 2, 4), device=DEV)
        assert t.out_size == (64, 64) and (t.patch_size, t.tile) == (2, 32)
        x_img, x_rows = t.frames(frames), t.frames(frames, dtype=dtype, layout="rows")
        if f_out == 5:
            masks5 = masks.clamp(max=4)
            m.forward_seg_loss(x_img, t.masks(masks5)).backward()  # warm-up: the GEMM tuner's first-call trials
            a = _loss_and_grads(m, lambda: m.forward_seg_loss(x_img, t.masks(masks5)))
            b = _loss_and_grads(m, lambda: m.forward_seg_loss(x_rows, t.masks(masks5, layout="rows")))
        else:
            tr = DD.DepthTargetTransform("log", "standardize", mask_background=True, zero_is_background=False)
            m.forward_depth_loss(x_img, t.depth(depth, "bilinear", tr), mask_background=True).backward()  # warm-up
            a = _loss_and_grads(m, lambda: m.forward_depth_loss(x_img, t.depth(depth, "bilinear", tr), mask_background=True))
            b = _loss_and_grads(m, lambda: m.forward_depth_loss(x_rows, t.depth(depth, "bilinear", tr, layout="rows"),
                                                                mask_background=True))
        assert torch.isfinite(a[0]) and torch.equal(a[0], b[0])
        assert a[1].keys() == b[1].keys() and len(a[1]) > 10
        for n in a[1]:
            assert torch.equal(a[1][n], b[1][n]), n
        with torch.no_grad():
            assert torch.equal(m(x_img), m(x_rows)) and torch.equal(m.forward_rows(x_img), m.forward_rows(x_rows))


def test_model_rejects_foreign_rows(FD):
    g = load("flat_data")
    frames, masks = torch.from_numpy(g["frames"]).to(DEV), torch.from_numpy(g["masks"]).to(DEV)
    m = _tiny_model(5)
    good = FD.FlatFrameTransform.for_model(m, (96, 128), size=(64, 64), device=DEV)
    for kw in (dict(size=(64, 64), patch_size=4, tile=16), dict(size=(64, 64), patch_size=2, tile=16),
               dict(size=(64, 128), patch_size=2, tile=32)):
        other = FD.FlatFrameTransform((96, 128), device=DEV, **kw)
        with pytest.raises(ValueError):
            m(other.frames(frames, layout="rows"))
        with pytest.raises(ValueError):
            m.forward_seg_loss(good.frames(frames, layout="rows"), other.masks(masks, layout="rows"))
    with pytest.raises(ValueError):
        FD.FlatFrameTransform.for_model(m, (96, 128), size=(64, 128), device=DEV)
    with pytest.raises(ValueError):
        FD.FlatFrameTransform.for_model(m, (96, 128), size=(64, 64), tile=4, device=DEV)
    m.compute_dtype = torch.float32
    with pytest.raises(TypeError):
        m(good.frames(frames, dtype=torch.bfloat16, layout="rows"))  # the model computes in fp32


# ------------------------------------------------------------------ 7. class distribution
def test_class_distribution(FD):
    rng = np.random.default_rng(5)
    batches = [rng.integers(0, 14, shape, dtype=np.uint8) for shape in ((3, 96, 128), (2, 50, 70), (1, 7, 9))]
    batches[1][0, :10] = 255
    num_classes = 10
    counts, numel = [0] * num_classes, 0
    for b in batches:  # data_stats.py:21-28
        for i in range(num_classes):
            counts[i] += int((b == i).sum())
        numel += b.size
    want = np.array([100 * c / numel for c in counts])
    got = FD.class_distribution([torch.from_numpy(b).to(DEV) for b in batches], num_classes)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(FD.class_distribution(torch.from_numpy(batches[0]), num_classes),
                          np.array([100 * int((batches[0] == i).sum()) / batches[0].size for i in range(num_classes)]))
    with pytest.raises(TypeError):
        FD.class_distribution([torch.zeros(4, dtype=torch.int64, device=DEV)], num_classes)


# ------------------------------------------------------------------ 8. strides, streams, dtypes
def test_strided_batches_streams_and_dtypes(FD):
    g = load("flat_data")
    frames, masks, depth = (torch.from_numpy(g[k]).to(DEV) for k in ("frames", "masks", "depth"))
    t = FD.FlatFrameTransform((96, 128), size=(40, 70), padding=(5, 4, 5, 4), device=DEV, **TINY)
    big = torch.zeros((4, 3, 96, 128), dtype=torch.uint8, device=DEV)
    big[::2] = frames
    assert not big[::2].is_contiguous() and torch.equal(t.frames(big[::2]), t.frames(frames))
    assert torch.equal(t.frames(big[::2], layout="rows").rows, t.frames(frames, layout="rows").rows)
    bigd = torch.zeros((5, 96, 128), device=DEV)
    bigd[1:3] = depth
    assert torch.equal(bits(t.depth(bigd[1:3], "bilinear")), bits(t.depth(depth, "bilinear")))
    odd = torch.zeros((2, 96, 129), dtype=torch.uint8, device=DEV)[:, :, 1:]  # rows not dense: copied once, same result
    odd.copy_(masks)
    assert torch.equal(t.masks(odd), t.masks(masks))
    assert torch.equal(t.masks(masks[0])[0], t.masks(masks)[0])  # one unbatched sample
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = t.depth(depth, "bilinear", layout="rows").rows
    s.synchronize()
    assert torch.equal(bits(side), bits(t.depth(depth, "bilinear", layout="rows").rows))
    with pytest.raises(TypeError):
        t.frames(frames.float())
    with pytest.raises(TypeError):
        t.masks(masks.long())
    with pytest.raises(TypeError):
        t.depth(depth.double())
    with pytest.raises(TypeError):
        t.frames(frames, dtype=torch.float16, layout="rows")
    with pytest.raises(ValueError):
        t.frames(frames[..., :64])
    with pytest.raises(RuntimeError):
        t.masks(masks.cpu())
    with pytest.raises(ValueError):
        FD.FlatFrameTransform((96, 128), size=(40, 70), device=DEV).masks(masks, layout="rows")  # no patch_size / tile
