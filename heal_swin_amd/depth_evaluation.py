"""Evaluation of depth predictions on the GPU: the depth model's validation metrics, the back-projected metric set and the
Chamfer distance between point clouds (the depth half of the reference's heal_swin/evaluation).  Mirrors the reference:

  extrinsic_rotation(cal_info)                 scipy Rotation.from_quat(quaternion).as_matrix() (scalar-last, normalised)
  get_ray_angles(...)                          utils/depth_utils.py:399-430
      HEALPix data                             pix2ang(nside, ipix, nest=True) of the first base_pix nside^2 pixels, with NO
                                               rotate_pole (the reference ignores it on this path; so does HPDepthGeometry)
      image-plane data                         project_depth_img_points_to_s2 (data/depth_estimation/project_depth_on_s2.py:
                                               177-257) at get_uv_from_hw(h, w, (h, w)): evaluation.project_img_points_to_s2
                                               with used_size=(h, w)
  HPDepthGeometry / ImageDepthGeometry.points  create_point_cloud_from_depth_mask (:465-539) + the kept set of
                                               ChamferDistance.update (evaluation/custom_metrics.py:539-561)   `hs_depth_points`
  chamfer_nn(a, b)                             the chamfer_distance extension (custom_metrics.py:569)          `hs_chamfer_nn`
  ChamferDistance                              custom_metrics.py:471-577; the writers' chamfer_distance* metrics
                                               (evaluation/hp_depth_pred_writers.py:734-1225)
  DepthMetrics                                 DepthMSE, DepthRelSE, DepthRelAE, DepthiRMSE, DepthRangeMSE, MeanSTD,
                                               MeanSTDMedian, MeanPredDist, ScaleInvariantLogError (custom_metrics.py:62-468)
                                               as the Lightning depth module (models_lightning/depth_estimation/
                                               model_lightning_depth_swin_hp.py:73-84) and the back-projected writer
                                               (hp_depth_pred_writers.py:377-535) use them                      `hs_depth_metrics`
  evaluation.HPBackProjector.depth(pred)       project_depth_hp_mask_back(..., s2_bkgd_class=nan) (:370-386)   `hs_backproject_depth`

The reference's back-projected set is DepthMetrics.update(projector.depth(pred), flat_target).  Depth values are read in place
through their strides, fp32 or bf16 (float64 for the back-projected predictions).  update() never waits for the device.

Left out: STDPredDist (custom_metrics.py:388-426; its compute() reads the misspelt self.num_sampels and cannot run) and
BlurredDepthMSE (needs torchvision's Gaussian blur).

Differences from the reference, by construction:
  * state is float64 sums (the reference keeps float32 sums); per-element values are formed in the reference's compute type
    (fp32, or float64 for float64 predictions), differences in float64 from the fp32 values.
  * a point is fp32(d * (R u)) with R u a float64 table, where the reference forms fp32(R (d u)) in float64: at most an ulp.
  * theta of an image point: a float64 Newton instead of newton_krylov (see evaluation.py), <= 1e-6 rad.
  * the Chamfer term is mean(dist_a) + mean(dist_b) in float64 (the reference's torch.mean is fp32).
  * MeanSTDMedian is the lower median of the fp32 standard deviations by an exact radix select (order_stats.row_median,
    `hs_select_rows`): torch.median's value bit for bit, with the rows split over the chip.  float64 standard deviations
    take torch.median.
"""
import math

import numpy as np
import torch

from ._lib import check, lib, np_ptr, ptr, stream_ptr
from ._sphere_args import _device_tensor, _kind_of
from .evaluation import _device, get_uv_from_hw, project_img_points_to_s2
from .order_stats import row_median
from .projection import _camera_rotation, hp_grid

MAX_BACKGROUND = 4
MAX_RANGES = 8
NSUMS = 29
(S_N, S_SE, S_AE, S_MEAN_SE, S_MEAN_AE, S_PRED, S_SIL_N, S_SIL_D, S_SIL_D2, S_INV_N, S_INV_SE, S_STD_N, S_STD,
 S_RANGE) = range(14)


# ------------------------------------------------------------------ host geometry (once per calibration)
def extrinsic_rotation(cal_info):
    """Rotation matrix of the extrinsic quaternion (x, y, z, w), as scipy's Rotation.from_quat(q).as_matrix()."""
    return _camera_rotation(cal_info)


def hp_ray_angles(nside, base_pix):
    """get_ray_angles(hp_data=True): pix2ang(nest) of pixels 0 .. base_pix nside^2 - 1 (no rotate_pole, as the reference)."""
    return hp_grid(nside, base_pix)


def image_ray_angles(cal_info, height, width, rotate_pole=False):
    """get_ray_angles(hp_data=False) of an height x width depth image of the camera's frame."""
    u, v = get_uv_from_hw(height, width, (int(height), int(width)))
    return project_img_points_to_s2(u, v, cal_info, rotate_pole, used_size=(int(height), int(width)))


def directions(theta, phi, rotation):
    """Rotated unit directions R (sin t cos p, sin t sin p, cos t), float64 [3, n]."""
    th, ph = np.asarray(theta, np.float64).reshape(-1), np.asarray(phi, np.float64).reshape(-1)
    u = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    return np.asarray(rotation, np.float64) @ u


def _background_values(background):
    """The finite background depths of a get_foreground_mask background tuple (NaN and +-inf are always dropped)."""
    vals = [float(b) for b in (background if isinstance(background, (tuple, list)) else (background,))]
    extra = sorted({v for v in vals if math.isfinite(v)})
    if len(extra) > MAX_BACKGROUND:
        raise ValueError(f"at most {MAX_BACKGROUND} finite background values")
    return np.asarray(extra, dtype=np.float32)


class _DepthGeometry:
    """The rotated direction table of one calibration, resident on the device; `shape` is the depth layout per sample."""

    def _init(self, theta, phi, cal_info, shape, device):
        self.device = _device(device)
        self.shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(self.shape))
        self.rotation = extrinsic_rotation(cal_info)
        self.dir_host = np.ascontiguousarray(directions(theta, phi, self.rotation))
        self.dir = torch.from_numpy(self.dir_host).to(self.device)

    def points(self, depth, foreground=None, background=(float("nan"), float("inf"))):
        """Point clouds of a batch of depth maps [B, *shape] (or one map [*shape]), fp32 / bf16, any strides.

        Returns (points fp32 [B * n, 3], offsets int64 [B + 1]), both on the device: sample b's kept points, in pixel order,
        are rows offsets[b] .. offsets[b + 1]; rows past offsets[B] are unused.  A pixel is kept when its depth is finite,
        is not one of the finite `background` values (the writers' mask_background uses (nan, inf, 1000)) and, if
        `foreground` (bool / uint8 [B, *shape] or [*shape]) is given, it is true there."""
        _device_tensor(depth, "depth", self.device, (torch.float32, torch.bfloat16))
        if tuple(depth.shape) == self.shape:
            depth = depth[None]
        if tuple(depth.shape[1:]) != self.shape:
            raise ValueError(f"depth must be [B, {', '.join(map(str, self.shape))}], got {tuple(depth.shape)}")
        b = depth.shape[0]
        if len(self.shape) == 1:
            width, sh, sw = self.n, 0, depth.stride(1)
        else:
            width, sh, sw = self.shape[1], depth.stride(1), depth.stride(2)
        fg, fg_sb = None, 0
        if foreground is not None:
            fg = foreground.to(self.device)
            if tuple(fg.shape) == self.shape:
                fg = fg[None].expand(b, *self.shape)
            if tuple(fg.shape) != (b,) + self.shape:
                raise ValueError(f"foreground must be [{b}, {', '.join(map(str, self.shape))}], got {tuple(foreground.shape)}")
            if fg.stride(0) == 0:
                fg = fg[:1].to(torch.uint8).contiguous()
            else:
                fg = fg.to(torch.uint8).contiguous()
                fg_sb = self.n
        bg = _background_values(background)
        ws = torch.empty(int(lib.hs_depth_points_workspace(b, self.n)), dtype=torch.uint8, device=self.device)
        pts = torch.empty((b * self.n, 3), dtype=torch.float32, device=self.device)
        offsets = torch.empty(b + 1, dtype=torch.int64, device=self.device)
        check(lib.hs_depth_points(ptr(depth), _kind_of(depth), b, self.n, width, depth.stride(0), sh, sw, ptr(fg), fg_sb,
                                  np_ptr(bg) if bg.size else None, int(bg.size),
                                  ptr(self.dir), ptr(ws), ptr(pts), ptr(offsets), stream_ptr(self.device)), "hs_depth_points")
        return pts, offsets


class HPDepthGeometry(_DepthGeometry):
    """Directions of the first base_pix nside^2 nested HEALPix pixels (depth data [B, Npix])."""

    def __init__(self, cal_info, nside, base_pix=8, device="cuda"):
        self.nside, self.base_pix = int(nside), int(base_pix)
        theta, phi = hp_ray_angles(self.nside, self.base_pix)
        self._init(theta, phi, cal_info, (self.base_pix * self.nside * self.nside,), device)


class ImageDepthGeometry(_DepthGeometry):
    """Directions of the pixels of an height x width depth image of the camera (depth data [B, H, W])."""

    def __init__(self, cal_info, height, width, rotate_pole=False, device="cuda"):
        theta, phi = image_ray_angles(cal_info, height, width, rotate_pole)
        self._init(theta, phi, cal_info, (int(height), int(width)), device)


# ------------------------------------------------------------------ Chamfer nearest neighbours
def _cloud(x, name, device):
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3:
        raise TypeError(f"{name} must be a float32 [N, 3] tensor")
    if x.device != device:
        raise TypeError(f"{name} must be on {device}")
    return x.contiguous()


def chamfer_nn(a, b, a_offsets=None, b_offsets=None, return_idx=False, splits=0, max_points=None, return_term=False):
    """Exact nearest neighbours between clouds a and b (fp32 [Na, 3], [Nb, 3]; with offsets int64 [B + 1] on the device,
    B ragged clouds each): dist_a[i] = min_j |a_i - b_j|^2 within the sample, dist_b likewise (fp32 from coordinate
    differences, lowest index on ties).  Returns (dist_a, dist_b) or (dist_a, dist_b, idx_a, idx_b) int64; return_term
    appends the per-sample term mean(dist_a) + mean(dist_b) (float64 [B], NaN if a cloud is empty).  Rows outside every
    cloud (past offsets[B]) and rows whose other cloud is empty read NaN / -1.  max_points = (bound a, bound b) on one
    sample's points (sizes the grid; default: all rows); splits: workgroups per query block along the targets (0: auto)."""
    dev = a.device if torch.is_tensor(a) else None
    a, b = _cloud(a, "a", dev), _cloud(b, "b", dev)
    if (a_offsets is None) != (b_offsets is None):
        raise ValueError("give offsets for both clouds or for neither")
    if a_offsets is None:
        a_offsets = torch.tensor([0, a.shape[0]], dtype=torch.int64, device=dev)
        b_offsets = torch.tensor([0, b.shape[0]], dtype=torch.int64, device=dev)
    for o in (a_offsets, b_offsets):
        if o.dtype != torch.int64 or o.dim() != 1 or o.device != dev:
            raise TypeError("offsets must be int64 [B + 1] tensors on the clouds' device")
    if a_offsets.shape != b_offsets.shape or a_offsets.shape[0] < 2:
        raise ValueError("a_offsets and b_offsets must both be [B + 1], B >= 1")
    batch = a_offsets.shape[0] - 1
    a_max, b_max = (a.shape[0], b.shape[0]) if max_points is None else (min(int(max_points[0]), a.shape[0]),
                                                                          min(int(max_points[1]), b.shape[0]))
    a_offsets, b_offsets = a_offsets.contiguous(), b_offsets.contiguous()
    ws = torch.empty(a.shape[0] + b.shape[0], dtype=torch.int64, device=dev)
    dist_a = torch.empty(a.shape[0], dtype=torch.float32, device=dev)
    dist_b = torch.empty(b.shape[0], dtype=torch.float32, device=dev)
    idx_a = torch.empty(a.shape[0], dtype=torch.int64, device=dev) if return_idx else None
    idx_b = torch.empty(b.shape[0], dtype=torch.int64, device=dev) if return_idx else None
    term = torch.empty(batch, dtype=torch.float64, device=dev) if return_term else None
    check(lib.hs_chamfer_nn(ptr(a), ptr(a_offsets), a.shape[0], a_max, ptr(b), ptr(b_offsets), b.shape[0], b_max, batch,
                            int(splits), ptr(ws), ptr(dist_a), ptr(dist_b), ptr(idx_a), ptr(idx_b), ptr(term),
                            stream_ptr(dev)), "hs_chamfer_nn")
    out = (dist_a, dist_b) + ((idx_a, idx_b) if return_idx else ())
    return out + (term,) if return_term else out


class ChamferDistance:
    """custom_metrics.ChamferDistance: every sample adds mean(dist_pred) + mean(dist_target) of its two point clouds;
    compute() is the sum over the number of samples (the writers call the reference's update once per sample).

    update(pred, target, pred_geometry, target_geometry, foreground=None, background=(nan, inf))
        pred: the model's output [B, C, *shape] (channel 0 is the depth) or [B, *shape]; target [B, *shape']; the
        geometries give each side's directions (HPDepthGeometry, or ImageDepthGeometry for the *_full_res metrics).
        foreground: a mask for both sides (same shapes), or a (pred_mask, target_mask) pair, either may be None."""

    def __init__(self, device="cuda"):
        self.device = _device(device)
        self.sum_chamfer = torch.zeros((), dtype=torch.float64, device=self.device)
        self.num_samples = torch.zeros((), dtype=torch.float64, device=self.device)

    def reset(self):
        self.sum_chamfer.zero_()
        self.num_samples.zero_()

    def update(self, pred, target, pred_geometry, target_geometry, foreground=None, background=(float("nan"), float("inf"))):
        if pred.dim() == len(pred_geometry.shape) + 2:
            pred = pred[:, 0]
        if isinstance(foreground, (tuple, list)):
            fg_p, fg_t = foreground
        else:
            fg_p = fg_t = foreground
        pa, oa = pred_geometry.points(pred, fg_p, background)
        pb, ob = target_geometry.points(target, fg_t, background)
        *_, term = chamfer_nn(pa, pb, oa, ob, max_points=(pred_geometry.n, target_geometry.n), return_term=True)
        self.sum_chamfer += term.sum()
        self.num_samples += term.numel()

    def compute(self):
        return self.sum_chamfer / self.num_samples

    def all_reduce(self, group=None):
        """Sum over ranks (torchmetrics' dist_reduce_fx='sum')."""
        import torch.distributed as dist

        state = torch.stack([self.sum_chamfer, self.num_samples])
        dist.all_reduce(state, op=dist.ReduceOp.SUM, group=group)
        self.sum_chamfer.copy_(state[0])
        self.num_samples.copy_(state[1])


# ------------------------------------------------------------------ error metrics
def _range_bounds(distance_range):
    """DepthRangeMSE's [min, max] of a range given as (hi,), a scalar hi (lo = -inf) or (lo, hi)."""
    if isinstance(distance_range, (tuple, list)):
        if len(distance_range) == 1:
            distance_range = distance_range[0]
        elif len(distance_range) == 2:
            return float(min(distance_range)), float(max(distance_range))
        else:
            raise ValueError(f"Range needs to be two numbers, got distance_range={distance_range}...")
    return float("-inf"), float(distance_range)


def range_names(distance_ranges):
    """The metric keys of add_distance_ranged_mse (custom_metrics.py:268-296)."""
    max_digits = max([len(str(x)) for x in np.array(distance_ranges, dtype=object).flatten()] or [0]) if distance_ranges else 0
    names = []
    for ran in distance_ranges:
        if isinstance(ran, (tuple, list)) and len(ran) == 2:
            names.append("mse_range_" + f"{str(ran[0]):0>{max_digits}}" + "_" + f"{str(ran[1]):0>{max_digits}}")
        elif isinstance(ran, (tuple, list)) and len(ran) == 1:
            names.append("mse_range_" + "_neg_inf_" + str(ran[0]))
        else:
            names.append("mse_range_" + "_neg_inf_" + str(ran))
    return names


class DepthMetrics:
    """Every depth error metric of the reference from one pass per batch (`hs_depth_metrics`).

    update(pred, target): pred [B, C, Npix] / [B, C, H, W] (channel 0 the mean, channel 1 the log variance) or, without a
    channel dimension, [B, Npix] / [B, H, W] (the back-projected float64 means); fp32, bf16 or float64, any strides.
    target [B, Npix] / [B, H, W].  update(pred, target, projector): a flat prediction scored on the sphere (see
    _update_projected).  compute() returns a dict keyed by the reference's metric names:
      mse, RelSE, RelAE (with total_mean), iRMSE, SILogE, mean_pred_dist, mse_range_* (distance_ranges, at most 8) and,
      with use_logvar, mean_std and median_std.
    total_mean and the range bounds are taken in fp32, as the reference's scalar-with-fp32-tensor arithmetic does."""

    def __init__(self, total_mean=None, distance_ranges=(), use_logvar=False, device="cuda"):
        self.device = _device(device)
        self.total_mean = None if total_mean is None else float(np.float32(total_mean))
        self.distance_ranges = list(distance_ranges)
        if len(self.distance_ranges) > MAX_RANGES:
            raise ValueError(f"at most {MAX_RANGES} distance ranges")
        bounds = [_range_bounds(r) for r in self.distance_ranges]
        self._ranges = np.asarray(bounds, dtype=np.float32).reshape(-1)
        self._names = range_names(self.distance_ranges)
        self.use_logvar = bool(use_logvar)
        self.state = torch.zeros(NSUMS, dtype=torch.float64, device=self.device)
        self.median = torch.zeros(2, dtype=torch.float64, device=self.device)  # (sum of per-sample medians, samples)

    def reset(self):
        self.state.zero_()
        self.median.zero_()

    def _rule_args(self, total):
        """What the two metric launches end with: the rule (use_logvar, total_mean, the ranges), a partial record per workgroup of
        a pass over `total` elements, the state and the stream."""
        partial = torch.empty(int(lib.hs_depth_metrics_partials(total)) * NSUMS, dtype=torch.float64, device=self.device)
        rng = self._ranges
        return (int(self.use_logvar), 0.0 if self.total_mean is None else self.total_mean, np_ptr(rng) if rng.size else None,
                len(self.distance_ranges), ptr(partial), ptr(self.state), stream_ptr(self.device))

    @staticmethod
    def _strides(t, spatial):
        """(width, stride_h, stride_w) of the trailing spatial dims of t."""
        if spatial == 1:
            return t.shape[-1], 0, t.stride(-1)
        return t.shape[-1], t.stride(-2), t.stride(-1)

    def _update_projected(self, pred, target, projector):
        """update() of a FLAT prediction sampled onto the sphere through a flat_evaluation.FlatToHPProjector
        (`hs_depth_metrics_gather`): target [B, Npix] fp32 / bf16, pred in the projector's layout, read in place; the
        projected map is not written.  The state is the one update(projector.depth(pred), target) gives, bit for bit."""
        _device_tensor(target, "target", self.device)
        pred, sb, sc, sp = projector._depth_args(pred, 2 if self.use_logvar else 1)
        if target.dim() != 2 or tuple(target.shape) != (pred.shape[0], projector.n_out):
            raise ValueError(f"target must be [{pred.shape[0]}, {projector.n_out}], got {tuple(target.shape)}")
        b, n = target.shape
        near, idx, wgt = projector._tables()
        check(lib.hs_depth_metrics_gather(ptr(pred), _kind_of(pred), b, projector.npix, sb, sc, sp, near, idx, wgt, n, ptr(target),
                                          _kind_of(target), target.stride(0), target.stride(1), *self._rule_args(b * n)),
              "hs_depth_metrics_gather")
        if self.use_logvar:  # MeanSTDMedian needs the projected log variance itself
            self._add_stds(torch.sqrt(torch.exp(projector.depth(pred, channel=1))))

    def update(self, pred, target, projector=None):
        if projector is not None:
            return self._update_projected(pred, target, projector)
        _device_tensor(pred, "pred", self.device)
        _device_tensor(target, "target", self.device)
        spatial = target.dim() - 1
        if spatial not in (1, 2):
            raise ValueError(f"target must be [B, Npix] or [B, H, W], got {tuple(target.shape)}")
        if pred.dim() == target.dim():
            if self.use_logvar:
                raise ValueError("use_logvar needs predictions with a channel dimension")
            sc = 0
        elif pred.dim() == target.dim() + 1:
            if pred.shape[1] < (2 if self.use_logvar else 1):
                raise ValueError(f"predictions have {pred.shape[1]} channels")
            sc = pred.stride(1)
        else:
            raise ValueError(f"pred {tuple(pred.shape)} does not match target {tuple(target.shape)}")
        if pred.shape[0] != target.shape[0] or pred.shape[-spatial:] != target.shape[-spatial:]:
            raise ValueError(f"pred {tuple(pred.shape)} does not match target {tuple(target.shape)}")
        b = target.shape[0]
        n = int(np.prod(target.shape[1:]))
        width, psh, psw = self._strides(pred, spatial)
        _, tsh, tsw = self._strides(target, spatial)
        check(lib.hs_depth_metrics(ptr(pred), _kind_of(pred, True), b, n, width, pred.stride(0), sc, psh, psw, ptr(target),
                                   _kind_of(target, True), target.stride(0), tsh, tsw, *self._rule_args(b * n)), "hs_depth_metrics")
        if self.use_logvar:  # MeanSTDMedian: the lower median per sample, on the device
            lv = pred[:, 1]
            self._add_stds(torch.sqrt(torch.exp(lv if lv.dtype == torch.float64 else lv.float())).reshape(b, -1))

    def _add_stds(self, stds):
        """stds [B, n]: one lower median per sample (torch.median's value: the select for fp32, torch.median itself for float64)."""
        if stds.dtype == torch.float32 and stds.shape[0] > 0:
            medians = row_median(stds if stds.stride(1) == 1 else stds.contiguous())
        else:
            medians = stds.median(1).values
        self.median[0] += medians.double().sum()
        self.median[1] += stds.shape[0]

    def add_median(self, log_var):
        """MeanSTDMedian's part of update() alone, for a caller whose kernel has already added the sums to `state` (the decoder
        tail's depth step): log_var fp32 [B, n], one lower median of sqrt(exp(.)) per sample."""
        self._add_stds(torch.sqrt(torch.exp(log_var.float())))

    def all_reduce(self, group=None):
        """Sum the states of all ranks (torchmetrics' dist_reduce_fx='sum')."""
        import torch.distributed as dist

        dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.median, op=dist.ReduceOp.SUM, group=group)

    def compute(self):
        """The metrics as Python floats (one device read)."""
        s = self.state.tolist()
        med = self.median.tolist()
        n = s[S_N]
        out = {"mse": s[S_SE] / n if n else math.nan}
        if self.total_mean is not None:
            out["RelSE"] = s[S_SE] / s[S_MEAN_SE] if s[S_MEAN_SE] else math.nan
            out["RelAE"] = s[S_AE] / s[S_MEAN_AE] if s[S_MEAN_AE] else math.nan
        out["iRMSE"] = math.sqrt(s[S_INV_SE] / s[S_INV_N]) if s[S_INV_N] else math.nan
        ns = s[S_SIL_N]
        out["SILogE"] = s[S_SIL_D2] / ns - s[S_SIL_D] ** 2 / ns ** 2 if ns else math.nan
        out["mean_pred_dist"] = s[S_PRED] / n if n else math.nan
        for r, name in enumerate(self._names):
            cnt, se = s[S_RANGE + 2 * r], s[S_RANGE + 2 * r + 1]
            out[name] = se / cnt if cnt else 0.0
        if self.use_logvar:
            out["mean_std"] = s[S_STD] / s[S_STD_N] if s[S_STD_N] else math.nan
            out["median_std"] = med[0] / med[1] if med[1] else math.nan
        return out
