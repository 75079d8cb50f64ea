"""Host side of the flat data path (heal_swin_amd/flat_data.py): the output-size rule and the per-axis crop / resize / pad tables,
against torch's CPU F.interpolate / F.pad (the calls torchvision 0.9's tensor path makes) and tests/golden/flat_data.npz.

Two rules for bilinear values (the kernel's, checked on the GPU in test_gpu_flat_data.py, and torch's CPU kernel's, checked here,
which pins the restated taps to torch):
  fp32    |out - exact| <= 4 ulp_fp32(max |tap|), exact = the float64 evaluation of the same taps: four products and three sums,
          each rounded once, weights in [0, 1]
  uint8   equal to round(exact) except where exact lies within 2^-12 of k + 0.5 (16 fp32 ulp at 255), where one level is allowed
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _golden import load

CONFIGS = {"pair": ((56, 72), (0, 0, 0, 0)), "pad_int": (40, (3, 5, 0, 2)), "mixed": ((60, 90), (-4, 2, 1, -3)),
           "crop_only": (None, (-8, 0, -8, 0))}
FULL_CONFIGS = {"seg": (False, (640, 768), (0, 0, 0, 0)), "depth": (False, 512, (-19, 0, -19, 0)),
                "green_int": (True, 512, (3, 5, 0, 2)), "green_mixed": (True, (640, 768), (-4, 2, 1, -3))}
PADDINGS = [(0, 0, 0, 0), (-19, 0, -19, 0), (3, 5, 0, 2), (-4, 2, 1, -3)]
TIE_WINDOW = 2.0 ** -12


@pytest.fixture(scope="module")
def FD():
    import heal_swin_amd.flat_data as m
    return m


def torch_reference(FD, img, size, padding, mode, crop_green):
    """CenterCrop -> Resize -> Pad of [B, C, H, W] with torch's CPU calls."""
    if crop_green:
        h, w = img.shape[-2:]
        top, left = int(round((h - 960) / 2.0)), int(round((w - 1280) / 2.0))
        img = img[..., top:top + 960, left:left + 1280]
    h, w = img.shape[-2:]
    oh, ow = (h, w) if size is None else FD.resize_output_size(h, w, size)
    if (oh, ow) != (h, w):
        x = img if img.is_floating_point() else img.float()
        x = F.interpolate(x, size=[oh, ow], mode=mode, **(dict(align_corners=False) if mode == "bilinear" else {}))
        img = x if img.is_floating_point() else torch.round(x).to(img.dtype)
    left, top, right, bottom = padding
    img = img[..., max(-top, 0):img.shape[-2] - max(-bottom, 0), max(-left, 0):img.shape[-1] - max(-right, 0)]
    return F.pad(img, [max(left, 0), max(right, 0), max(top, 0), max(bottom, 0)])


def check_fp32_rule(out, tables, src, tag):
    exact, scale = tables.apply_host(src, exact=True), tables.max_tap(src)
    bound = 4 * np.spacing(scale.astype(np.float32)).astype(np.float64)
    fin = np.isfinite(exact)
    err = np.abs(np.asarray(out, np.float64) - exact)
    assert np.array_equal(np.isnan(out), np.isnan(exact)), tag
    assert (err[fin] <= bound[fin]).all(), (tag, float((err[fin] / np.maximum(bound[fin], 1e-300)).max()) * 4)


def check_uint8_rule(out, tables, src, tag, max_share=None):
    exact = tables.apply_host(src, exact=True)
    want = np.rint(exact)
    near_tie = np.abs(exact - np.floor(exact) - 0.5) <= TIE_WINDOW
    diff = np.abs(np.asarray(out, np.int64) - want.astype(np.int64))
    assert (diff[~near_tie] == 0).all(), (tag, int((diff[~near_tie] != 0).sum()))
    assert (diff[near_tie] <= 1).all(), tag
    if max_share is not None:
        assert near_tie.mean() <= max_share, (tag, float(near_tie.mean()))


def test_resize_output_size(FD):
    assert FD.resize_output_size(966, 1280, 512) == (512, 678)
    assert FD.resize_output_size(966, 1280, (640, 768)) == (640, 768)
    assert FD.resize_output_size(966, 1280, [640, 768]) == (640, 768)
    assert FD.resize_output_size(512, 700, 512) == (512, 700)
    assert FD.resize_output_size(700, 512, 512) == (700, 512)
    assert FD.resize_output_size(1280, 966, 512) == (678, 512)
    assert FD.resize_output_size(966, 1280, [512]) == (512, 678)


def test_out_size_and_errors(FD):
    t = FD.FlatFrameTransform((966, 1280), size=512, padding=(-19, 0, -19, 0), device=None)
    assert t.resized == (512, 678) and t.out_size == (512, 640) and not t.identity
    t = FD.FlatFrameTransform((966, 1280), size=None, padding=(3, 5, 0, 2), crop_green=True, device=None)
    assert t.crop == (3, 0, 960, 1280) and t.out_size == (967, 1283) and t.identity
    assert t.tables("bilinear") is t.tables("nearest")  # an unchanged size: no arithmetic
    with pytest.raises(ValueError):
        FD.FlatFrameTransform((96, 128), crop_green=True, device=None)
    with pytest.raises(ValueError):
        FD.FlatFrameTransform((96, 128), padding=(-64, 0, -64, 0), device=None)
    with pytest.raises(ValueError):
        t.tables("bicubic")
    with pytest.raises(RuntimeError):
        t.masks(torch.zeros(1, 966, 1280, dtype=torch.uint8))


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("size", [None, (640, 768), 512])
@pytest.mark.parametrize("crop_green", [False, True])
def test_tables_against_torch(FD, crop_green, size, padding):
    rng = np.random.default_rng(3)
    tag = f"green={crop_green} size={size} padding={padding}"
    t = FD.FlatFrameTransform((966, 1280), size=size, padding=padding, crop_green=crop_green, device=None)
    depth = rng.uniform(0.2, 400.0, (1, 1, 966, 1280)).astype(np.float32)
    depth[rng.random(depth.shape) < 0.05] = 1000.0
    frame = rng.integers(0, 256, (1, 1, 966, 1280), dtype=np.uint8)
    near, bil = t.tables("nearest"), t.tables("bilinear")
    ref = torch_reference(FD, torch.from_numpy(depth), size, padding, "nearest", crop_green).numpy()
    assert ref.shape[-2:] == t.out_size, tag
    assert np.array_equal(near.apply_host(depth).view(np.uint32), ref.view(np.uint32)), tag
    ref = torch_reference(FD, torch.from_numpy(frame), size, padding, "nearest", crop_green).numpy()
    assert np.array_equal(near.apply_host(frame), ref), tag
    # bilinear: our fp32 formula and torch's CPU kernel both obey the two rules
    ref = torch_reference(FD, torch.from_numpy(depth), size, padding, "bilinear", crop_green).numpy()
    check_fp32_rule(ref, bil, depth, "torch " + tag)
    check_fp32_rule(bil.apply_host(depth), bil, depth, "tables " + tag)
    ref = torch_reference(FD, torch.from_numpy(frame), size, padding, "bilinear", crop_green).numpy()
    check_uint8_rule(ref, bil, frame, "torch " + tag)
    check_uint8_rule(bil.apply_host(frame), bil, frame, "tables " + tag)


def test_full_size_tables_match_the_golden(FD):
    g = load("flat_data")
    for name, (green, size, padding) in FULL_CONFIGS.items():
        t = FD.FlatFrameTransform((966, 1280), size=size, padding=padding, crop_green=green, device=None).tables("nearest")
        assert np.array_equal(t.row_idx[0], g[f"full/{name}/rows"]) and np.array_equal(t.col_idx[0], g[f"full/{name}/cols"]), name


def test_golden_reproduces_from_the_tables(FD):
    g = load("flat_data")
    for name, (size, padding) in CONFIGS.items():
        t = FD.FlatFrameTransform((96, 128), size=size, padding=padding, device=None)
        near, bil = t.tables("nearest"), t.tables("bilinear")
        assert np.array_equal(near.apply_host(g["masks"]), g[f"{name}/masks"]), name
        assert np.array_equal(near.apply_host(g["depth"]).view(np.uint32), g[f"{name}/depth_nearest"].view(np.uint32)), name
        check_fp32_rule(g[f"{name}/depth_bilinear"], bil, g["depth"], name)
        check_fp32_rule(bil.apply_host(g["depth"]), bil, g["depth"], name)
        check_uint8_rule(g[f"{name}/frames"], bil, g["frames"], name)
        check_uint8_rule(bil.apply_host(g["frames"]), bil, g["frames"], name)


def test_spans_cover_every_tile(FD):
    t = FD.FlatFrameTransform((966, 1280), size=512, padding=(-19, 0, -19, 0), device=None).tables("bilinear")
    sh, sw = t.spans(32, 32)
    for idx, span in ((t.row_idx, sh), (t.col_idx, sw)):
        for start in range(0, idx.shape[1], 32):
            part = idx[:, start:start + 32]
            assert part.max() - part[part >= 0].min() + 1 <= span


def test_rows_objects_are_checked_against_the_model(FD):
    import types

    model = types.SimpleNamespace(data_spec=types.SimpleNamespace(dim_in=(64, 64), f_in=3),
                                  config=types.SimpleNamespace(patch_size=[2, 2]), tile=8)
    rows = torch.zeros(1, 32 * 32, 16)
    assert FD.PatchRows(rows, 3, 64, 64, 2, 8).check_model(model) is rows
    for bad in (FD.PatchRows(rows, 3, 64, 64, 4, 8), FD.PatchRows(rows, 3, 64, 64, 2, 16), FD.PatchRows(rows, 3, 64, 128, 2, 8),
                FD.PatchRows(rows, 1, 64, 64, 2, 8), FD.PixelRows(rows, 32, 64, 2, 8)):
        with pytest.raises(ValueError):
            bad.check_model(model)
