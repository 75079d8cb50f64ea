#!/usr/bin/env python3
"""Generate tests/golden/flat_eval.npz from the REFERENCE's own projection and metric code (imported read-only, as make_golden.py).

Run in the build container only:   python tests/golden/make_golden_flat_eval.py
Same run-time stubs and PROJ_CALS as make_golden_depth_eval.py.  The reference's flat writers (evaluation/flat_pred_writers.py:
321-421, evaluation/flat_depth_pred_writers.py:128-253) un-pad and resize with torchvision's Pad and Resize, which is not
installed here; this script makes those two steps with the torch calls torchvision 0.9's tensor path makes, by our reading
(a slice, and torch.nn.functional.interpolate).  Everything after them is the reference's own code:
  project_on_s2.project_s2_points_to_img, project_on_s2.sample_mask (uint8), project_depth_on_s2.sample_mask (float32, NaN
  background) and custom_metrics' DepthMSE, ScaleInvariantLogError, DepthiRMSE, DepthRelAE, DepthRelSE.
Records, as plain arrays, per case <c>:
  <c>/meta                 nside, base_pix, rotate_pole, model H, W, orig H, W (0 0: no Resize), padding l t r b, background class
  <c>/table                int32 [Npix]: the model-plane pixel h * W + w each HEALPix pixel samples (an index image pushed through
                           the chain and the reference's sample_mask), -1 where sample_mask gave the background
  <c>/ids, <c>/hp_labels   uint8 class ids [B, H, W] of a flat prediction and the reference's sample_mask of them [B, Npix]
  <c>/hp_target            uint8 [B, Npix]
  <c>/depth/pred           fp32 [B, 2, H, W] with NaN / +-inf / <= 0 mixed in; <c>/depth/target fp32 [B, Npix], inf background
  <c>/depth/<mode>/hp      the reference's projected depth [B, Npix] for Resize nearest / bilinear
  <c>/depth/<mode>/<metric>  the reference metric classes' compute() after one update per sample
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import PROJ_CALS, _import_projection  # noqa: E402
from make_golden_depth_eval import _depth, _import_depth  # noqa: E402

# name: (calibration, nside, base_pix, rotate_pole, model (H, W), orig (H, W) or None, padding [l, t, r, b], background, depth)
CASES = {
    "identity": ("rv_60x80", 32, 8, False, (60, 80), None, (0, 0, 0, 0), 0, False),
    "resize_pad_plain": ("mvl_96x128", 16, 8, False, (64, 64), (96, 128), (0, 8, 0, 8), 0, True),
    "resize_pad_rot": ("mvl_96x128", 16, 8, True, (64, 64), (96, 128), (0, 8, 0, 8), 3, True),
    "bp12": ("rv_60x80", 8, 12, True, (32, 48), (60, 80), (0, 0, 0, 0), 0, False),
}
CLASSES = 5
TOTAL_MEAN = 37.25


def undo_transforms(x, orig, padding, mode):
    """Pad([-p for p in padding]) then Resize(orig, interpolation=mode) of a [H, W] tensor, as torchvision 0.9 does on tensors."""
    left, top, right, bottom = padding
    h, w = x.shape
    x = x[top:h - bottom, left:w - right]
    if orig is None:
        return x
    y = x[None, None].to(torch.float32 if x.dtype == torch.uint8 else x.dtype)
    y = F.interpolate(y, size=list(orig), mode=mode, **({} if mode == "nearest" else {"align_corners": False}))
    return y[0, 0].to(x.dtype)


def main():
    from oracle.healpix import pix2ang_nest

    _, CM = _import_depth()
    P = _import_projection()
    import heal_swin.data.depth_estimation.project_depth_on_s2 as PD

    rng = np.random.default_rng(20261016)
    out = {}
    for name, (key, nside, bp, rot, (h, w), orig, padding, bkgd, with_depth) in CASES.items():
        cal = PROJ_CALS[key]
        theta, phi = pix2ang_nest(nside, np.arange(nside * nside * bp))
        u, v = P.project_s2_points_to_img(theta, phi, cal, rot)
        out[name + "/meta"] = np.array([nside, bp, int(rot), h, w, *(orig or (0, 0)), *padding, bkgd], dtype=np.int64)
        index = torch.arange(h * w, dtype=torch.float32).view(h, w)
        table = PD.sample_mask(undo_transforms(index, orig, padding, "nearest").numpy(), v, u, s2_bkgd_class=float("nan"))
        out[name + "/table"] = np.where(np.isnan(table), -1, table).astype(np.int32)
        ids = rng.integers(0, CLASSES, (2, h, w), dtype=np.uint8)
        out[name + "/ids"] = ids
        out[name + "/hp_labels"] = np.stack([P.sample_mask(undo_transforms(torch.from_numpy(m), orig, padding, "nearest").numpy(), v, u,
                                                           s2_bkgd_class=bkgd) for m in ids])
        out[name + "/hp_target"] = rng.integers(0, CLASSES, (2, theta.size), dtype=np.uint8)
        if not with_depth:
            continue
        pred = np.stack([_depth(rng, (2, h, w)), rng.normal(0.5, 1.0, (2, h, w)).astype(np.float32)], 1)
        r = rng.random((2, h, w))
        pred[:, 0][r < 0.01] = -np.inf
        pred[:, 0][(r >= 0.01) & (r < 0.03)] = -3.0
        target = rng.uniform(0.5, 300.0, (2, theta.size)).astype(np.float32)
        target[:, np.isnan(table)] = np.inf
        target[rng.random(target.shape) < 0.03] = np.inf
        out[name + "/depth/pred"], out[name + "/depth/target"] = pred, target
        for mode in ("nearest", "bilinear"):
            hp = np.stack([PD.sample_mask(undo_transforms(torch.from_numpy(m), orig, padding, mode).numpy(), v, u,
                                          s2_bkgd_class=float("nan")) for m in pred[:, 0]])
            out[f"{name}/depth/{mode}/hp"] = hp
            ms = {"mse": CM.DepthMSE(), "SILogE": CM.ScaleInvariantLogError(), "iRMSE": CM.DepthiRMSE(),
                  "RelAE": CM.DepthRelAE(total_mean=TOTAL_MEAN), "RelSE": CM.DepthRelSE(total_mean=TOTAL_MEAN)}
            for k, m in ms.items():
                for b in range(hp.shape[0]):  # the writer updates once per sample; the metric classes read channel 0 of [1, 1, Npix]
                    m.update(torch.from_numpy(hp[b])[None, None].clone(), torch.from_numpy(target[b])[None].clone())
                out[f"{name}/depth/{mode}/{k}"] = np.asarray(float(m.compute()), dtype=np.float64)
    out["total_mean"] = np.array(TOTAL_MEAN)
    path = os.path.join(HERE, "flat_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
