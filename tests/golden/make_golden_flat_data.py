#!/usr/bin/env python3
"""Generate tests/golden/flat_data.npz: small inputs and the expected outputs of the flat data path (heal_swin_amd/flat_data.py).

Run in the build container only:   python tests/golden/make_golden_flat_data.py
Expected values come from torch's CPU calls that torchvision 0.9's tensor path makes (our reading of it: torchvision is not
installed), F.interpolate(mode="nearest" | "bilinear", align_corners=False), torch.round and F.pad, and, for the depth chain, from
the reference's own normalize_depth_data.normalize_data and depth_utils.mask_transform_fcn, imported as make_golden_depth_data.py
imports them (flat_depth_datasets.py:137-146 after the resize and padding).  Records, as plain arrays:
  frames uint8 [2, 3, 96, 128], masks uint8 [2, 96, 128], depth float32 [2, 96, 128] (1000s and 0s among the values)
  <cfg>/frames, <cfg>/masks, <cfg>/depth_nearest, <cfg>/depth_bilinear     the reference's tensors for the small configurations
                                           CONFIGS (size, padding)
  chain/<T>/<N>/<M>                        the flat dataset's target steps on pad_int/depth_nearest[0] (padded zeros and raw 1000s
                                           included), for every transform T, normalization N and mask_background M
  full/<cfg>/rows, full/<cfg>/cols         per-axis tables at full size (966 x 1280 frames, FULL_CONFIGS with crop_green): the
                                           source row / column of every output row / column, -1 where padded, read off
                                           F.pad(F.interpolate(index image, mode="nearest"))
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_depth_data import NORMS, TRANSFORMS, _depth_map, _import  # noqa: E402

# name -> (size, padding [left, top, right, bottom]) on 96 x 128 frames
CONFIGS = {
    "pair": ((56, 72), (0, 0, 0, 0)),
    "pad_int": (40, (3, 5, 0, 2)),        # 40 x 53 -> 47 x 56
    "mixed": ((60, 90), (-4, 2, 1, -3)),  # 60 x 90 -> 59 x 87
    "crop_only": (None, (-8, 0, -8, 0)),  # 96 x 112, no resize
}
# name -> (crop_green, size, padding) on 966 x 1280 frames
FULL_CONFIGS = {
    "seg": (False, (640, 768), (0, 0, 0, 0)),
    "depth": (False, 512, (-19, 0, -19, 0)),
    "green_int": (True, 512, (3, 5, 0, 2)),
    "green_mixed": (True, (640, 768), (-4, 2, 1, -3)),
}
CROP = (960, 1280)


def output_size(h, w, size):
    """torchvision 0.9 functional_tensor.resize's size rule."""
    if size is None:
        return h, w
    if not isinstance(size, int):
        return tuple(size)
    short, long = (w, h) if w <= h else (h, w)
    if short == size:
        return h, w
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def reference(img, size, padding, mode, crop_green=False):
    """CenterCrop -> Resize -> Pad of a [B, C, H, W] tensor with the torch calls torchvision's tensor path makes."""
    if crop_green:
        h, w = img.shape[-2:]
        top, left = int(round((h - CROP[0]) / 2.0)), int(round((w - CROP[1]) / 2.0))
        img = img[..., top:top + CROP[0], left:left + CROP[1]]
    h, w = img.shape[-2:]
    oh, ow = output_size(h, w, size)
    if (oh, ow) != (h, w):
        x = img if img.is_floating_point() else img.float()
        kw = dict(align_corners=False) if mode == "bilinear" else {}
        x = F.interpolate(x, size=[oh, ow], mode=mode, **kw)
        img = x if img.is_floating_point() else torch.round(x).to(img.dtype)
    left, top, right, bottom = padding
    img = img[..., max(-top, 0):img.shape[-2] - max(-bottom, 0), max(-left, 0):img.shape[-1] - max(-right, 0)]
    return F.pad(img, [max(left, 0), max(right, 0), max(top, 0), max(bottom, 0)], mode="constant", value=0)


def make(N, DU):
    rng = np.random.default_rng(20261016)
    out = {}
    frames = rng.integers(0, 256, (2, 3, 96, 128), dtype=np.uint8)
    frames[:, :, :20, :30] = 255
    masks = rng.integers(0, 12, (2, 96, 128), dtype=np.uint8)
    masks[0, 40:60, 50:90] = 255
    depth = _depth_map(rng, (2, 96, 128))
    out["frames"], out["masks"], out["depth"] = frames, masks, depth
    tf, tm, td = torch.from_numpy(frames), torch.from_numpy(masks)[:, None], torch.from_numpy(depth)[:, None]
    for name, (size, padding) in CONFIGS.items():
        out[f"{name}/frames"] = reference(tf, size, padding, "bilinear").numpy()
        out[f"{name}/masks"] = reference(tm, size, padding, "nearest")[:, 0].numpy()
        out[f"{name}/depth_nearest"] = reference(td, size, padding, "nearest")[:, 0].numpy()
        out[f"{name}/depth_bilinear"] = reference(td, size, padding, "bilinear")[:, 0].numpy()
    x = out["pad_int/depth_nearest"][0]
    assert (x == 0).any() and (x == 1000).any()
    for T in TRANSFORMS:
        for Nm in NORMS:
            for M in (False, True):
                stats = N.get_depth_data_stats(data_transform=T, mask_background=M)
                mask = torch.from_numpy(x.copy())  # flat_depth_datasets.py:137-146
                if M:
                    mask[mask == 1000] = float("inf")
                if T:
                    mask = DU.mask_transform_fcn(T)(mask)
                out[f"chain/{T}/{Nm}/{int(M)}"] = N.normalize_data(data=mask, data_stats=stats, norm_type=Nm).numpy()
    h, w = 966, 1280
    index = torch.arange(h * w, dtype=torch.float64).view(1, 1, h, w) + 1  # 0 is the padding value
    for name, (green, size, padding) in FULL_CONFIGS.items():
        res = reference(index, size, padding, "nearest", green)[0, 0].numpy().astype(np.int64) - 1
        rows, cols = res // w, res % w
        rows[res < 0], cols[res < 0] = -1, -1
        r, c = rows.max(axis=1), cols.max(axis=0)
        assert np.array_equal(np.where(res >= 0, r[:, None] * w + c[None, :], -1), res)  # separable
        out[f"full/{name}/rows"], out[f"full/{name}/cols"] = r.astype(np.int32), c.astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "flat_data.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(4)
    _, N, DU, _ = _import()
    make(N, DU)
