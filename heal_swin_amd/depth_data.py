"""The depth data path on the GPU: fisheye frame and depth map -> HEALPix sample -> regression target -> (after the model)
depth in metres again, and the dataset statistics behind the normalization constants.  Mirrors the reference:

  project_depth_s2_points_to_img(theta, phi, cal_info, rotate_pole, used_size)
                                  data/depth_estimation/project_depth_on_s2.py:141-175 (projection.project_s2_points_to_img
                                  with used_size = (H, W) in place of the calibration's height and width)
  sample_bilinear_f32 / sample_depth   sample_bilinear(...).astype(np.float32) / sample_mask(depth, ...)  (:26-84)
                                  `hs_sample_bilinear_u8_f32` / `hs_sample_nearest_f32` (HIP, bit-exact; device tensors only)
  HPDepthProjector                project_depth_dataset_hp (:389-440) for the frames of one calibration
  write_depth_sample / HPDepthNpzDataset   the np.savez(hp_img=f32 [3, Npix], hp_mask=f32 [Npix]) samples and their reader
  DataStats / get_depth_data_stats     normalize_depth_data.py:6-130 (the six tables)
  DepthTargetTransform            hp_depth_datasets.py:90-107 (prepare), flat_depth_datasets.py:122-148 (prepare with
                                  zero_is_background=False), utils/depth_utils.py:140-170 (transform_and_normalize,
                                  unnormalize_and_retransform)                                              `hs_depth_target`
  DepthStatsAccumulator           compute_depth_stats.py's max / min / mean / std / counts           `hs_depth_stats_*`
  DepthHistogram                  its np.histogram(all_data, bins=1000) -> bin_counts, bin_edges      `hs_histogram_update`

Every transform is float32 with log / exp / 1/x formed in float64 and rounded once; the reference's torch calls on float32 agree
to an ulp or so.  Normalization is float32 (x - shift) / scale forward and x * scale + shift backward with shift / scale the
table's float32 mean / std (standardize) or min / max - min (min-max).  The statistics are float64 sums over float32 transformed
values as in the script (which concatenates float32 arrays into a float64 one).  Two differences: the script's float32 np.log
is not correctly rounded (numpy's SIMD log; about 4 % of values an ulp away from fp32(log(double))), and its max over
"non-background" values compares the TRANSFORMED values with 1000 -- here it is the max over values whose raw value is not 1000
(the same thing for the untransformed data, the case the script reports it for).
"""
import math
import os

import numpy as np
import torch

from ._lib import (HS_DEPTH_STATS_WORDS, HS_DT_1000_BKG, HS_DT_AFFINE, HS_DT_INV, HS_DT_INVERSE, HS_DT_LOG, HS_DT_NONE,
                   HS_DT_ZERO_BKG, HS_HISTOGRAM_MAX_BINS, check, lib, ptr, stream_ptr)
from ._sphere_args import _resolved
from .projection import _FisheyeProjector, _sample, _with_used_size, project_s2_points_to_img

IMG_KEY, MASK_KEY = "hp_img", "hp_mask"
TRANSFORMS = {None: HS_DT_NONE, "None": HS_DT_NONE, "log": HS_DT_LOG, "inv": HS_DT_INV}
NORMALIZATIONS = (None, "None", "standardize", "min-max")


# ------------------------------------------------------------------ projection
def project_depth_s2_points_to_img(theta, phi, cal_info, rotate_pole=False, used_size=None):
    """Float pixel coordinates (u along the width, v along the height) of spherical points; used_size = (height, width) of
    the image actually sampled replaces the calibration's size."""
    return project_s2_points_to_img(theta, phi, _with_used_size(cal_info, used_size), rotate_pole)


def sample_bilinear_f32(img, rx, ry, per_sample=False):
    """`sample_bilinear(img, rx, ry).astype(np.float32)`: img uint8 [C, H, W] or [B, C, H, W] on the GPU, rx along H, ry along
    W -> float32 [(B,) C, n]; NaN where a coordinate is not finite, 0 at integer coordinates (the reference's floor / ceil).
    per_sample=False: one coordinate table for the whole batch (rx, ry of any shape are flattened).  per_sample=True: rx, ry
    are [B, n] and sample b reads row b (`hs_sample_bilinear_u8_f32_per_sample`, the same kernel and arithmetic)."""
    return _sample("sample_bilinear_u8_f32", img, 4, torch.uint8, "img", rx, ry, per_sample, torch.float32)


def sample_depth(depth, rx, ry, background=0.0, per_sample=False):
    """`sample_mask(depth, rx, ry, background)`: depth float32 [H, W] or [B, H, W] on the GPU -> float32 [(B,) n], the nearest
    pixel's value (round half to even), `background` outside the image.  per_sample as in sample_bilinear_f32
    (`hs_sample_nearest_f32_per_sample`)."""
    return _sample("sample_nearest_f32", depth, 3, torch.float32, "depth", rx, ry, per_sample, torch.float32,
                   (float(np.float32(background)),))


class HPDepthProjector(_FisheyeProjector):
    """project_depth_dataset_hp for the frames of one camera: `proj(imgs, depths)` -> (hp_img float32 [B, 3, Npix], hp_mask
    float32 [B, Npix]) on the GPU.  The coordinate table is built once on the host and stays on the device.

    `proj(imgs, depths, rotations=A)` with A [B, 3, 3] (projection.random_rotations) is the augmented projection: one coordinate
    launch (projection.rotated_coords) plus the per-sample sampling launches; depth is still sampled nearest, and samples outside
    the image are 0 in the frame and `s2_bkgd_class` in the depth as without rotations.  `rotations=None` is the exact path: the
    resident table, the reference's bytes.  Identity rotations go through the device arithmetic and agree with it to coordinate
    rounding only (about 1e-12 px), not bit for bit."""

    _sample_frame, _sample_nearest = staticmethod(sample_bilinear_f32), staticmethod(sample_depth)

    def __init__(self, cal_info, nside, base_pix=8, rotate_pole=False, s2_bkgd_class=0, used_size=None, device="cuda"):
        super().__init__(cal_info, nside, base_pix, rotate_pole, float(s2_bkgd_class), used_size, device)

    def proj(self, imgs, depths=None, rotations=None):
        return self._proj(imgs, depths, rotations)

    __call__ = proj


# ------------------------------------------------------------------ samples on disk
def write_depth_sample(path, hp_img, hp_mask):
    """One sample in the reference's format (np.savez, hp_img float32 [3, Npix], hp_mask float32 [Npix])."""
    hp_img, hp_mask = np.asarray(hp_img), np.asarray(hp_mask)
    if hp_img.dtype != np.float32 or hp_img.ndim != 2:
        raise ValueError("hp_img is float32 [channels, Npix]")
    if hp_mask.dtype != np.float32 or hp_mask.ndim != 1 or hp_mask.shape[0] != hp_img.shape[1]:
        raise ValueError("hp_mask is float32 [Npix]")
    np.savez(path, **{IMG_KEY: hp_img, MASK_KEY: hp_mask})


class HPDepthNpzDataset(torch.utils.data.Dataset):
    """Directory of depth `.npz` samples; `ds[i]` returns the raw (hp_img, hp_mask) float32 arrays (the target is made on the
    GPU by DepthTargetTransform.prepare)."""

    def __init__(self, root):
        self.root = root
        self.file_names = sorted(f for f in os.listdir(root) if f.endswith(".npz"))
        self.names = [os.path.splitext(f)[0] for f in self.file_names]
        self.paths = [os.path.join(root, f) for f in self.file_names]

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, idx):
        data = np.load(self.paths[idx])
        return data[IMG_KEY], data[MASK_KEY]

    def get_item_by_name(self, name):
        return self[self.names.index(name)]


# ------------------------------------------------------------------ statistics tables
class DataStats:
    """normalize_depth_data.DataStats (max_foreground: compute_depth_stats.py's max over the non-background values)."""

    def __init__(self, name, max, min, mean, std, total_pixels=None, total_background=None, max_foreground=None):  # noqa: A002
        self.name, self.max, self.min, self.mean, self.std = name, max, min, mean, std
        self.total_pixels, self.total_background, self.max_foreground = total_pixels, total_background, max_foreground

    def __repr__(self):
        return (f"DataStats({self.name!r}, max={self.max!r}, min={self.min!r}, mean={self.mean!r}, std={self.std!r}, "
                f"total_pixels={self.total_pixels!r}, total_background={self.total_background!r})")


_TABLES = {
    (False, "log"): dict(name="Log depth data stats", max=6.907755374908447, min=-1.8142070770263672, mean=1.4544509182015166,
                         std=2.0786484162088192),
    (False, "inv"): dict(name="Inv depth data stats", max=6.136208534240723, min=0.001, mean=0.9910007833745446,
                         std=1.449026079271616, total_pixels=2997248000, total_background=120398457),
    (False, "None"): dict(name="Depth data stats", max=999.94287109375, min=0.16296708583831787, mean=53.27547067117465,
                          std=195.83201099547819, total_pixels=2997248000, total_background=120398457),
    (True, "log"): dict(name="Masked log depth data stats", max=6.907698154449463, min=-1.8142070770263672,
                        mean=1.226225759977343, std=1.7902344298584563),
    (True, "inv"): dict(name="Masked inv depth data stats", max=6.136208534240723, min=0.0010000570910051465,
                        mean=1.0324331088958505, std=1.4645187100900352, total_pixels=2997248000, total_background=120398457),
    (True, "None"): dict(name="Masked depth data stats", max=999.94287109375, min=0.16296708583831787, mean=13.654291032986958,
                         std=29.58008801108711, total_pixels=2876849543),
}


def _transform_name(data_transform):
    if data_transform not in TRANSFORMS:
        raise ValueError(f"data_transform must be one of None, 'None', 'log', 'inv', got {data_transform!r}")
    return "None" if data_transform is None else data_transform


def get_depth_data_stats(data_transform=None, mask_background=False):
    """The reference's SynWoodScape table for (data_transform, mask_background) (normalize_depth_data.py:112-130)."""
    return DataStats(**_TABLES[(bool(mask_background), _transform_name(data_transform))])


# ------------------------------------------------------------------ target transforms
def _rows(x, what):
    """(tensor [B, n] view, batch, n, stride_b, stride_p) of a float32 GPU tensor [B, n] or [n]."""
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise TypeError(f"{what} must be a float32 tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{what} must be a GPU tensor: the depth transforms run in the HIP kernel only (no CPU path)")
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2:
        raise ValueError(f"{what} must be [B, Npix] or [Npix], got {tuple(x.shape)}")
    if min(x.stride()) < 0:
        raise ValueError(f"{what} with negative strides is not supported")
    return x


class DepthTargetTransform:
    """The depth target's transform (None | 'log' | 'inv') and normalization (None | 'standardize' | 'min-max') with the table
    `data_stats` (default: get_depth_data_stats(data_transform, mask_background)), as one HIP pass each:

      prepare(depth)                      the dataset's __getitem__: 0 -> inf (HEALPix data; zero_is_background=False for the flat
                                          dataset), 1000 -> inf if mask_background, transform, normalize
      transform_and_normalize(x)          the Lightning module on outputs[:, 0] before the loss
      unnormalize_and_retransform(x)      before the metrics, on predictions and targets: back to depths in metres

    x: float32 [B, Npix] or [Npix] on the GPU, any non-negative strides (outputs[:, 0] of [B, C, Npix] works); out=None allocates
    the result, out=x works in place."""

    def __init__(self, data_transform=None, normalize_data=None, mask_background=False, data_stats=None, zero_is_background=True):
        self.data_transform = _transform_name(data_transform)
        if normalize_data not in NORMALIZATIONS:
            raise ValueError(f"normalize_data must be one of None, 'None', 'standardize', 'min-max', got {normalize_data!r}")
        self.normalize_data = "None" if normalize_data is None else normalize_data
        self.mask_background = bool(mask_background)
        self.zero_is_background = bool(zero_is_background)
        self.data_stats = get_depth_data_stats(self.data_transform, self.mask_background) if data_stats is None else data_stats
        self._transform = TRANSFORMS[self.data_transform]
        if self.normalize_data == "standardize":
            self._affine = (float(np.float32(self.data_stats.mean)), float(np.float32(self.data_stats.std)))
        elif self.normalize_data == "min-max":
            self._affine = (float(np.float32(self.data_stats.min)), float(np.float32(self.data_stats.max - self.data_stats.min)))
        else:
            self._affine = None

    def _run(self, x, out, flags):
        if out is None and torch.is_tensor(x):
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        x = _rows(x, "x")
        o = _rows(out, "out")
        if o.shape != x.shape or o.device != x.device:
            raise ValueError(f"out {tuple(o.shape)} does not match x {tuple(x.shape)}")
        shift, scale = self._affine if self._affine is not None else (0.0, 1.0)
        if self._affine is not None:
            flags |= HS_DT_AFFINE
        check(lib.hs_depth_target(ptr(x), x.stride(0), x.stride(1), ptr(o), o.stride(0), o.stride(1), x.shape[0], x.shape[1], flags,
                                  self._transform, shift, scale, stream_ptr(x.device)), "hs_depth_target")
        return out

    def inverse_op(self):
        """(flags, transform, shift, scale) of unnormalize_and_retransform as hs_depth_target takes them: what a kernel that applies
        the chain itself (the decoder tail's depth step, csrc/hs_depth_target.h) is given."""
        shift, scale = self._affine if self._affine is not None else (0.0, 1.0)
        return HS_DT_INVERSE | (HS_DT_AFFINE if self._affine is not None else 0), self._transform, shift, scale

    def prepare(self, depth, out=None):
        flags = (HS_DT_ZERO_BKG if self.zero_is_background else 0) | (HS_DT_1000_BKG if self.mask_background else 0)
        return self._run(depth, out, flags)

    def transform_and_normalize(self, x, out=None):
        return self._run(x, out, 0)

    def unnormalize_and_retransform(self, x, out=None):
        return self._run(x, out, HS_DT_INVERSE)


# ------------------------------------------------------------------ dataset statistics
(_TOTAL, _BKG, _VALUES, _FINITE, _POSINF, _NEGINF, _NAN, _FG_VALUES, _FG_POSINF, _FG_NAN) = range(10)
_NCOUNTS = 10


def _initial_state():
    d = np.array([0.0, 0.0, math.inf, -math.inf, -math.inf])  # mean, M2, min, max, foreground max
    return np.concatenate([np.zeros(_NCOUNTS, np.int64), d.view(np.int64)])


class DepthStatsAccumulator:
    """compute_depth_stats.py as a streaming reduction: update(depth) adds raw float32 depth maps (any shape) on the GPU;
    compute() -> DataStats(max, min, mean, std (ddof 0), total_pixels, total_background, max_foreground) with numpy's results on
    the same values (NaN / inf inputs included: e.g. a log of 0 gives min = mean = -inf, std = NaN).  data_transform None |
    'log' | 'inv' (a plain 1 / x, as the script); use_masking drops the background (raw 1000) values.  The state is
    deterministic (no float atomics): the same updates give bit-identical results."""

    def __init__(self, data_transform=None, use_masking=False, device="cuda"):
        self.data_transform = _transform_name(data_transform)
        self.use_masking = bool(use_masking)
        if torch.device(device).type != "cuda":
            raise RuntimeError("DepthStatsAccumulator runs on the GPU only (HIP kernels, no CPU path)")
        self.device = _resolved(device)
        self.state = torch.from_numpy(_initial_state()).to(self.device)

    def reset(self):
        self.state.copy_(torch.from_numpy(_initial_state()))

    def update(self, depth):
        if not torch.is_tensor(depth) or depth.dtype != torch.float32 or depth.device != self.device:
            raise TypeError(f"depth must be a float32 tensor on {self.device}")
        d = depth.contiguous().reshape(-1)
        partial = torch.empty(int(lib.hs_depth_stats_partials(d.numel())) * HS_DEPTH_STATS_WORDS, dtype=torch.int64,
                              device=self.device)
        check(lib.hs_depth_stats_update(ptr(d), d.numel(), TRANSFORMS[self.data_transform], int(self.use_masking), ptr(partial),
                                        ptr(self.state), stream_ptr(self.device)), "hs_depth_stats_update")

    def all_reduce(self, group=None):
        """Merge the states of all ranks, in rank order, into every rank's state (identical bits everywhere)."""
        import torch.distributed as dist

        world, rank = dist.get_world_size(group), dist.get_rank(group)
        states = torch.zeros((world, HS_DEPTH_STATS_WORDS), dtype=torch.int64, device=self.device)
        states[rank] = self.state
        dist.all_reduce(states, op=dist.ReduceOp.SUM, group=group)  # every row has one nonzero contributor: exact
        self.reset()
        check(lib.hs_depth_stats_merge(ptr(states), world, ptr(self.state), stream_ptr(self.device)), "hs_depth_stats_merge")

    def compute(self):
        s = self.state.cpu().numpy()
        c = [int(v) for v in s[:_NCOUNTS]]
        mean, m2, mn, mx, fg_mx = (float(v) for v in s[_NCOUNTS:].view(np.float64))
        nan, inf = math.nan, math.inf
        if c[_VALUES] == 0 or c[_NAN]:
            mx = mn = mean = std = nan
        else:
            mx = inf if c[_POSINF] else (mx if c[_FINITE] else -inf)
            mn = -inf if c[_NEGINF] else (mn if c[_FINITE] else inf)
            if c[_POSINF] and c[_NEGINF]:
                mean = nan
            elif c[_POSINF] or c[_NEGINF]:
                mean = inf if c[_POSINF] else -inf
            std = nan if c[_POSINF] or c[_NEGINF] else math.sqrt(m2 / c[_FINITE])
        if c[_FG_VALUES] == 0 or c[_FG_NAN]:
            fg_mx = nan
        elif c[_FG_POSINF]:
            fg_mx = inf
        name = f"depth data stats (data_transform={self.data_transform}, use_masking={self.use_masking})"
        return DataStats(name=name, max=mx, min=mn, mean=mean, std=std, total_pixels=c[_TOTAL], total_background=c[_BKG],
                         max_foreground=fg_mx)


class DepthHistogram:
    """compute_depth_stats.py's np.histogram(all_data, bins=1000) as a streaming count: update(depth) adds raw float32 depth
    maps (any shape) on the GPU; compute() -> (bin_counts int64 [bins], bin_edges float64 [bins + 1]), np.histogram's on the
    same values (the float32 transformed values as float64, as the script's concatenation makes them) with the same bins and
    range: NaN, +-inf and values outside the range are dropped, the last bin is closed.  The edges are numpy's own
    (np.histogram_bin_edges), so a degenerate range widens and an invalid one raises as numpy's does.  data_transform and
    use_masking as DepthStatsAccumulator.  The script's range is the data's (min, max): from_stats takes it from a first pass
    with the accumulator.  Integer counts: the same updates in any order give the same result."""

    def __init__(self, bins=1000, range=None, data_transform=None, use_masking=False, device="cuda"):  # noqa: A002
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)):
            raise TypeError(f"bins must be an integer (equal-width bins), got {type(bins).__name__}")
        if not 1 <= bins <= HS_HISTOGRAM_MAX_BINS:
            raise ValueError(f"bins must be in [1, {HS_HISTOGRAM_MAX_BINS}], got {bins}")
        if range is None:
            raise ValueError("range=(lo, hi) is required: a streaming histogram cannot take it from the data "
                             "(DepthHistogram.from_stats takes the accumulator's min and max)")
        lo, hi = (float(v) for v in range)
        self.bins, self.range = int(bins), (lo, hi)
        self.data_transform = _transform_name(data_transform)
        self.use_masking = bool(use_masking)
        self.bin_edges = np.histogram_bin_edges(np.empty(0, np.float64), self.bins, (lo, hi)).astype(np.float64, copy=False)
        if torch.device(device).type != "cuda":
            raise RuntimeError("DepthHistogram runs on the GPU only (HIP kernel, no CPU path)")
        self.device = _resolved(device)
        self._edges = torch.from_numpy(self.bin_edges).to(self.device)
        self.counts = torch.zeros(self.bins, dtype=torch.int64, device=self.device)

    @classmethod
    def from_stats(cls, stats, bins=1000, data_transform=None, use_masking=False, device="cuda"):
        """The histogram over [stats.min, stats.max] of a DataStats that DepthStatsAccumulator.compute() gave for the same data,
        transform and masking: np.histogram(all_data, bins) without a range."""
        return cls(bins, (stats.min, stats.max), data_transform, use_masking, device)

    def reset(self):
        self.counts.zero_()

    def update(self, depth):
        if not torch.is_tensor(depth) or depth.dtype != torch.float32 or depth.device != self.device:
            raise TypeError(f"depth must be a float32 tensor on {self.device}")
        d = depth.contiguous().reshape(-1)
        check(lib.hs_histogram_update(ptr(d), d.numel(), TRANSFORMS[self.data_transform], int(self.use_masking), ptr(self._edges),
                                      self.bins, ptr(self.counts), stream_ptr(self.device)), "hs_histogram_update")

    def all_reduce(self, group=None):
        """Sum the counts of all ranks."""
        import torch.distributed as dist

        dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)

    def compute(self):
        return self.counts.cpu().numpy(), self.bin_edges.copy()

    def save(self, path):
        """The script's np.savez(..., bin_counts=, bin_edges=)."""
        bin_counts, bin_edges = self.compute()
        np.savez(path, bin_counts=bin_counts, bin_edges=bin_edges)
