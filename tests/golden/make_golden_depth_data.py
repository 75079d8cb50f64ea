#!/usr/bin/env python3
"""Generate tests/golden/depth_data.npz from the REFERENCE's own depth data code (read-only, /root/reference).

Run in the build container only:   python tests/golden/make_golden_depth_data.py
Imports data/depth_estimation/project_depth_on_s2.py, normalize_depth_data.py, hp_depth_datasets.py and utils/depth_utils.py with
make_golden's import stubs plus throwaway module stubs set up at run time (torchvision, torchmetrics, chamfer_distance,
pytorch_lightning, the Woodscape base dataset and flat_depth_datasets, which needs torchvision).  Records, as plain arrays:
  coords/<case>/{theta, phi, u, v}         project_depth_s2_points_to_img (with and without used_size / rotate_pole); the grid
                                           (an input) is oracle/healpix.py's pix2ang_nest of the first base_pix nside^2 pixels
  sample/<case>/{img, depth, hp_img, hp_mask}   sample_bilinear(img, v, u).astype(float32), sample_mask(depth, v, u, bkgd)
  edge/{img, depth, rx, ry, hp_img, hp_mask}    the same on hand-made coordinates (integers, borders, .5, NaN, +-inf)
  x, z                                     the crafted transform inputs (raw depths; normalized predictions)
  fwd|inv|prep_hp|prep_flat/<T>/<N>/<M>    transform_and_normalize(x) / unnormalize_and_retransform(z) / the HEALPix dataset's
                                           __getitem__ on x / the flat dataset's steps on x, for every transform T, normalization
                                           N and mask_background M (the 18 combinations)
  stats/maps, stats/<T>/<M>/{...}          compute_depth_stats.py's arithmetic restated in numpy on three raw maps (the script
                                           reads files at module level); its float32 log is taken correctly rounded
                                           (fp32(log(double))), which numpy's SIMD float32 log is not on ~4 % of values
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import PROJ_CALS, _import_projection  # noqa: E402
from make_golden_depth_eval import _stub_modules  # noqa: E402

TRANSFORMS = ["None", "log", "inv"]
NORMS = ["None", "standardize", "min-max"]


def _import():
    _import_projection()
    import heal_swin.data.depth_estimation.normalize_depth_data as N  # only imports torch: the real module

    _stub_modules()
    import healpy

    healpy.pixelfunc.isnsideok = lambda nside: True
    pl = types.ModuleType("pytorch_lightning")
    pl.core = types.ModuleType("pytorch_lightning.core")
    pl.core.datamodule = types.ModuleType("pytorch_lightning.core.datamodule")
    pl.core.datamodule.LightningDataModule = object
    ws = types.ModuleType("heal_swin.data.woodscape_dataset")
    ws.WoodscapeDataset = torch.utils.data.Dataset
    for name, mod in (("pytorch_lightning", pl), ("pytorch_lightning.core", pl.core),
                      ("pytorch_lightning.core.datamodule", pl.core.datamodule), ("heal_swin.data.woodscape_dataset", ws)):
        sys.modules[name] = mod
    import heal_swin.data as D
    import heal_swin.data.depth_estimation as DE

    D.woodscape_dataset = ws
    DE.flat_depth_datasets = sys.modules["heal_swin.data.depth_estimation.flat_depth_datasets"]
    DE.normalize_depth_data = N
    import heal_swin.data.depth_estimation.project_depth_on_s2 as P
    import heal_swin.utils.depth_utils as DU

    DE.project_depth_on_s2 = P
    import heal_swin.data.depth_estimation.hp_depth_datasets as HD

    return P, N, DU, HD


def _depth_map(rng, shape):
    d = rng.uniform(0.2, 400.0, shape).astype(np.float32)
    r = rng.random(shape)
    d[r < 0.08] = 1000.0
    d[(r >= 0.08) & (r < 0.10)] = 0.0
    return d


def make(P, N, DU, HD):
    from oracle.healpix import pix2ang_nest

    rng = np.random.default_rng(20261016)
    out = {}
    # ---- coordinates and sampling
    for key, nside, bp, rotate, used in (("mvl_96x128", 16, 8, False, None), ("mvl_96x128", 16, 8, True, (48, 64)),
                                         ("rv_60x80", 8, 12, True, None), ("fv_966x1280", 8, 8, False, (483, 640))):
        cal = PROJ_CALS[key]
        theta, phi = pix2ang_nest(nside, np.arange(nside * nside * bp))
        tag = f"{key}/n{nside}_bp{bp}_{'rot' if rotate else 'plain'}_{'x'.join(map(str, used)) if used else 'cal'}"
        u, v = P.project_depth_s2_points_to_img(theta, phi, cal, rotate, used_size=used)
        out[f"coords/{tag}/theta"], out[f"coords/{tag}/phi"] = theta, phi
        out[f"coords/{tag}/u"], out[f"coords/{tag}/v"] = u, v
        if key == "mvl_96x128":
            H, W = used if used else (int(cal["intrinsic"]["height"]), int(cal["intrinsic"]["width"]))
            img = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
            img[:, : H // 3, : W // 3] = 200
            depth = _depth_map(rng, (H, W))
            out[f"sample/{tag}/img"], out[f"sample/{tag}/depth"] = img, depth
            out[f"sample/{tag}/hp_img"] = P.sample_bilinear(img, v, u).astype(np.float32)
            out[f"sample/{tag}/hp_mask"] = P.sample_mask(depth, v, u, 0)
    img = rng.integers(1, 256, (3, 7, 9), dtype=np.uint8)
    depth = _depth_map(rng, (7, 9))
    rx = np.array([0.0, 2.0, 2.5, 3.5, 6.0, 6.2, -0.3, -1.0, 5.999999, 1e9, -1e9, 0.5, 1.5, np.nan, 3.25, 6.5, 2.0, np.inf, 1.0])
    ry = np.array([0.0, 3.0, 0.5, 1.5, 8.0, 8.4, 0.4, 2.0, 7.999999, 1.0, 1.0, 8.5, -0.5, 1.0, np.nan, 7.5, 4.75, 1.0, -np.inf])
    with np.errstate(invalid="ignore"):
        out["edge/hp_img"] = P.sample_bilinear(img, rx, ry).astype(np.float32)
        out["edge/hp_mask"] = P.sample_mask(depth, rx, ry, 7.5)
    out["edge/img"], out["edge/depth"], out["edge/rx"], out["edge/ry"] = img, depth, rx, ry

    # ---- target transforms
    f32 = np.float32
    special = [0.0, -0.0, 1000.0, 1e-4, f32(1e-3), np.nextafter(f32(1e-3), f32(0)), -1.0, -5.5, np.inf, -np.inf, np.nan, 13.654291,
               3.408, 0.16296709, 999.94287, 1.0]
    x = np.concatenate([np.array(special, f32), np.logspace(-2.5, 3, 240).astype(f32), rng.uniform(0.2, 80, 120).astype(f32)])
    z = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 100.0, -100.0, 1e-4, -1e-4, 1e-3, 5.0, -3.0], f32),
                        rng.normal(0, 1.5, 240).astype(f32), rng.uniform(-0.2, 1.2, 120).astype(f32)])
    out["x"], out["z"] = x, z
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "s.npz")
    np.savez(path, hp_img=np.zeros((3, x.size), f32), hp_mask=x)
    for T in TRANSFORMS:
        for Nm in NORMS:
            for M in (False, True):
                stats = N.get_depth_data_stats(data_transform=T, mask_background=M)
                tag = f"{T}/{Nm}/{int(M)}"
                out[f"fwd/{tag}"] = DU.transform_and_normalize(torch.from_numpy(x.copy()), Nm, stats, T).numpy()
                out[f"inv/{tag}"] = DU.unnormalize_and_retransform(torch.from_numpy(z.copy()), Nm, stats, T).numpy()
                ds = types.SimpleNamespace(paths=[path], mask_background=M, data_transform=T, normalize_data=Nm, data_stats=stats)
                _, hp_mask = HD.WoodscapeHPDepthImagesDataset.__getitem__(ds, 0)
                out[f"prep_hp/{tag}"] = hp_mask.numpy()
                mask = torch.from_numpy(x.copy())  # flat_depth_datasets.py:139-146 after the resize and padding
                if M:
                    mask[mask == 1000] = float("inf")
                if T:
                    mask = DU.mask_transform_fcn(T)(mask)
                out[f"prep_flat/{tag}"] = N.normalize_data(data=mask, data_stats=stats, norm_type=Nm).numpy()

    # ---- statistics (compute_depth_stats.py restated; three maps, the last with zeros)
    maps = [_depth_map(rng, (48, 64)) for _ in range(3)]
    maps[0][maps[0] == 0] = 0.5
    maps[1][maps[1] == 0] = 0.25
    out["stats/maps"] = np.stack(maps)
    for T in TRANSFORMS:
        for M in (False, True):
            vals = []
            for m in maps:
                m = m.flatten()
                keep = m[m != 1000] if M else m
                with np.errstate(divide="ignore"):
                    if T == "log":
                        t = np.log(keep.astype(np.float64)).astype(np.float32)
                    elif T == "inv":
                        t = 1 / keep
                    else:
                        t = keep
                vals.append((t, keep != 1000))
            for name, sel in (("two", slice(0, 2)), ("all", slice(0, 3))):
                all_data = np.concatenate([np.empty((0,))] + [v for v, _ in vals[sel]])
                fg = np.concatenate([np.empty((0,), bool)] + [f for _, f in vals[sel]])
                n_maps = len(range(3)[sel])
                with np.errstate(invalid="ignore"):
                    res = [np.amax(all_data), np.amin(all_data), np.mean(all_data), np.std(all_data), np.amax(all_data[fg]),
                           n_maps * maps[0].size, sum(np.count_nonzero(m == 1000) for m in maps[sel])]
                out[f"stats/{T}/{int(M)}/{name}"] = np.array(res, np.float64)
    np.savez_compressed(os.path.join(HERE, "depth_data.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(4)
    make(*_import())
