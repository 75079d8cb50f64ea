#!/usr/bin/env python3
"""Generate tests/golden/depth_eval.npz from the REFERENCE's own depth evaluation code (read-only, /root/reference).

Run in the build container only:   python tests/golden/make_golden_depth_eval.py
Imports the reference's utils/depth_utils.py and evaluation/custom_metrics.py with make_golden's import stubs plus throwaway
module stubs, set up at run time, for torchvision, torchmetrics (a minimal Metric with add_state) and chamfer_distance;
healpy.pixelfunc.pix2ang / nside2npix are routed to oracle.healpix.  Records, as plain arrays:
  rot/<cal>                             Rotation.from_quat(quaternion).as_matrix() (scipy)
  hp/<cal>/n<nside>_bp<bp>/{depth, points, keep}   create_point_cloud_from_depth_mask(hp_data=True) of one depth map with
                                        NaN / inf / 1000 depths mixed in, and the kept set of ChamferDistance.update
  img/<cal>/<rot>/{depth, points, keep, theta, phi}   the same for image-plane data (get_ray_angles with used_size)
  metrics/<case>/{pred, target, <metric name>}   the reference metric classes' compute() after one or two updates
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import PROJ_CALS, _import_projection  # noqa: E402


def _stub_modules():
    tv = types.ModuleType("torchvision")
    tv.transforms = types.SimpleNamespace(InterpolationMode=types.SimpleNamespace(NEAREST=0, BILINEAR=1))
    tm = types.ModuleType("torchmetrics")

    class Metric:
        def __init__(self, compute_on_step=True, dist_sync_on_step=False, process_group=None, dist_sync_fn=None):
            pass

        def add_state(self, name, default, dist_reduce_fx=None):
            setattr(self, name, default.clone())

    tm.Metric, tm.IoU, tm.MetricCollection = Metric, object, dict
    cd = types.ModuleType("chamfer_distance")
    cd.ChamferDistance = lambda: None
    for name, mod in (("torchvision", tv), ("torchmetrics", tm), ("chamfer_distance", cd)):
        sys.modules[name] = mod
    for name in ("heal_swin.data.depth_estimation.flat_depth_datasets", "heal_swin.data.depth_estimation.normalize_depth_data"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["heal_swin.data.depth_estimation.normalize_depth_data"].DataStats = object  # annotations only


def _import_depth():
    from oracle import healpix as OH

    _import_projection()
    _stub_modules()
    import healpy

    healpy.pixelfunc.pix2ang = lambda nside, ipix, nest=False: (OH.pix2ang_nest if nest else OH.pix2ang_ring)(nside, ipix)
    healpy.pixelfunc.nside2npix = lambda nside: 12 * nside * nside
    healpy.nside2npix = healpy.pixelfunc.nside2npix
    import heal_swin.data.depth_estimation as DE

    DE.flat_depth_datasets = sys.modules["heal_swin.data.depth_estimation.flat_depth_datasets"]
    DE.normalize_depth_data = sys.modules["heal_swin.data.depth_estimation.normalize_depth_data"]
    import heal_swin.evaluation.custom_metrics as CM
    import heal_swin.utils.depth_utils as DU

    return DU, CM


def _depth(rng, shape):
    d = rng.uniform(0.5, 300.0, shape).astype(np.float32)
    r = rng.random(shape)
    d[r < 0.05] = np.nan
    d[(r >= 0.05) & (r < 0.08)] = np.inf
    d[(r >= 0.08) & (r < 0.10)] = 1000.0
    d[(r >= 0.10) & (r < 0.11)] = 0.0
    return d


def _cloud(DU, depth, cal, **kw):
    pc, _ = DU.create_point_cloud_from_depth_mask(data=torch.from_numpy(depth)[None], cal_info=cal, **kw)
    pc = pc[0]
    s = torch.sum(pc, dim=-1)
    keep = ~(s.isnan() | s.isinf())
    return pc[keep].float().numpy(), keep.numpy()


def _metric_values(CM, pred, target, ranges, total_mean):
    ms = {"mse": CM.DepthMSE(), "SILogE": CM.ScaleInvariantLogError(), "iRMSE": CM.DepthiRMSE(),
          "RelAE": CM.DepthRelAE(total_mean=total_mean), "RelSE": CM.DepthRelSE(total_mean=total_mean),
          "mean_pred_dist": CM.MeanPredDist()}
    if pred.shape[1] == 2:
        ms["mean_std"], ms["median_std"] = CM.MeanSTD(), CM.MeanSTDMedian()
    CM.add_distance_ranged_mse(ms, ranges)  # named (lo, hi) ranges; the (hi,) and scalar forms directly
    ms["range_hi_tuple"], ms["range_hi_scalar"] = CM.DepthRangeMSE(distance_range=(10,)), CM.DepthRangeMSE(distance_range=50.0)
    p, t = torch.from_numpy(pred), torch.from_numpy(target)
    half = p.shape[0] // 2
    out = {}
    for k, m in ms.items():
        for sl in (slice(0, half), slice(half, None)):  # two updates
            m.update(p[sl].clone(), t[sl].clone())
        out[k] = np.asarray(float(m.compute()), dtype=np.float64)
    return out


def main():
    DU, CM = _import_depth()
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(20261016)
    out = {}
    for key, cal in PROJ_CALS.items():
        out[f"rot/{key}"] = Rotation.from_quat(cal["extrinsic"]["quaternion"]).as_matrix()
    for key, nside, bp in (("fv_966x1280", 8, 8), ("mvl_96x128", 16, 8), ("rv_60x80", 8, 12)):
        depth = _depth(rng, (bp * nside * nside,))
        pts, keep = _cloud(DU, depth, PROJ_CALS[key], nside=nside, base_pix=bp, hp_data=True)
        tag = f"hp/{key}/n{nside}_bp{bp}"
        out[tag + "/depth"], out[tag + "/points"], out[tag + "/keep"] = depth, pts, keep
    for key, (h, w) in (("mvl_96x128", (24, 32)), ("rv_60x80", (30, 40))):
        for rot in (False, True):
            depth = _depth(rng, (h, w))
            pts, keep = _cloud(DU, depth, PROJ_CALS[key], hp_data=False, rotate_pole=rot)
            theta, phi = DU.get_ray_angles(torch.from_numpy(depth)[None], PROJ_CALS[key], hp_data=False, rotate_pole=rot)
            tag = f"img/{key}/{'rot' if rot else 'plain'}"
            out[tag + "/depth"], out[tag + "/points"], out[tag + "/keep"] = depth, pts, keep.reshape(h, w)
            out[tag + "/theta"], out[tag + "/phi"] = np.asarray(theta), np.asarray(phi)
    # metrics: HEALPix [B, 2, N] with the quirks (targets +inf / -inf / 0 / NaN, predictions 0 / negative / NaN / inf)
    ranges = [(0, 5), (20, 100), (5, 300), (500, 600)]
    for tag, shape in (("hp", (4, 2, 768)), ("img", (2, 2, 12, 16))):
        pred = np.stack([rng.uniform(0.5, 120.0, shape[:1] + shape[2:]), rng.normal(0.5, 1.0, shape[:1] + shape[2:])], 1).astype(np.float32)
        target = rng.uniform(0.5, 120.0, shape[:1] + shape[2:]).astype(np.float32)
        flat_p, flat_t = pred[:, 0].reshape(-1), target.reshape(-1)
        k = flat_t.size
        idx = rng.permutation(k)
        flat_t[idx[:10]] = np.inf
        flat_t[idx[10:15]] = -np.inf
        flat_t[idx[15:20]] = 0.0
        flat_t[idx[20:30]] = np.nan
        flat_p[idx[25:35]] = 0.0
        flat_p[idx[35:40]] = -3.0
        flat_p[idx[40:45]] = np.nan
        flat_p[idx[45:50]] = np.inf
        flat_t[idx[50:55]] = 5.0  # on a range bound
        pred[:, 0] = flat_p.reshape(pred[:, 0].shape)
        target = flat_t.reshape(target.shape)
        out[f"metrics/{tag}/pred"], out[f"metrics/{tag}/target"] = pred, target
        for name, v in _metric_values(CM, pred, target, ranges, 37.25).items():
            out[f"metrics/{tag}/{name}"] = v
    out["metrics/ranges"] = np.array([str(r) for r in ranges])
    out["metrics/total_mean"] = np.array(37.25)
    path = os.path.join(HERE, "depth_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
