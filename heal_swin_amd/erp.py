"""Equirectangular panoramas (ERP, the lat/long image of 360-degree cameras, Stanford2D3D, Matterport, SUN360, rendered scenes,
weather and climate fields) to HEALPix and back: the data boundary of the full-sphere model (12 base pixels), as
`projection.HPProjector` / `evaluation.HPBackProjector` are for a calibrated fisheye camera.  No counterpart in the reference,
whose data covers at most 8 base pixels.

  erp_grid(height, width)                   (theta, phi) float64 [H, W] of the panorama's pixel centres
  erp_layout(lon_left, lon_increases_right) the 3x3 matrix L of a dataset's longitude convention
  ERPProjector                              `proj(imgs, masks, depth, rotations=A)`: frames (bilinear, optionally supersampled),
                                            labels and depth (nearest, copied) of a batch in one launch, no table written
                                                                                                   `hs_erp_to_hp`
  erp_to_hp_host(...)                       the same statements in a host loop (numpy), the kernel's oracle   `hs_erp_to_hp_host`
  ERPBackProjector                          an `HPBackProjector` whose image plane is the panorama: `.masks / .images / .depth`
                                            and `SegConfusion.update(pred, target, projector=...)` on the existing kernels

Convention (that of projection.rotated_coords): output pixel p of sample b shows the panorama at direction M_b g_p, g_p the centre
of nested pixel p.  In the kernel's own frame column j of a W-wide panorama is centred at longitude 2 pi (j + 0.5) / W and row i of
H at colatitude pi (i + 0.5) / H; columns wrap, rows clamp (nothing is interpolated across a pole).  A dataset with another
longitude origin or direction is described by L = erp_layout(...), and M_b = L A_b with A_b the augmentation
(`projection.random_rotations`, or any [B, 3, 3]; None is the identity).

The frame uses the proper bilinear weights (1 - f, f), NOT those of the reference's `sample_bilinear` (`ceil - r`, `r - floor`,
which return 0 at integer coordinates and are mirrored by `projection.sample_bilinear_u8` for the fisheye path): there is no
reference result to match here.
"""
import math

import numpy as np
import torch

from ._lib import HS_F32, HS_U8, check, lib, np_ptr, ptr, stream_ptr
from ._sphere_args import (MAX_CHANNELS, MAX_NSIDE, _any_given, _check_base_pix, _check_batch, _check_nside, _device_planes,  # noqa: F401
                           _dtype_name, _fills, _gather_planes, _matmul3, _results, _rotation_batch, _same_batch)
from .evaluation import HPBackProjector

_NAMES = ("imgs", "masks", "depth")


def erp_grid(height, width):
    """(theta, phi) float64 [H, W]: colatitude pi (i + 0.5) / H and longitude 2 pi (j + 0.5) / W of the pixel centres."""
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f"the panorama must be at least 1 x 1, got {height} x {width}")
    theta = math.pi * (np.arange(height, dtype=np.float64) + 0.5) / height
    phi = 2.0 * math.pi * (np.arange(width, dtype=np.float64) + 0.5) / width
    return np.broadcast_to(theta[:, None], (height, width)).copy(), np.broadcast_to(phi[None, :], (height, width)).copy()


def erp_layout(lon_left=0.0, lon_increases_right=True):
    """The float64 [3, 3] matrix L of a panorama whose column j is centred at longitude lon_left + 2 pi (j + 0.5) / W
    (lon_increases_right) or lon_left - 2 pi (j + 0.5) / W: L takes a direction of that frame to the kernel's own, in which the
    left edge is longitude 0 and longitude grows to the right.  L = Rz(-lon_left), times diag(1, -1, 1) from the left for the
    mirrored direction.  Pass it as `layout=` to ERPProjector and ERPBackProjector."""
    c, s = math.cos(float(lon_left)), math.sin(float(lon_left))
    m = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    if not lon_increases_right:
        m = np.diag([1.0, -1.0, 1.0]) @ m
    return m + 0.0  # no negative zeros


def _layout(layout):
    if layout is None:
        return None
    m = np.ascontiguousarray(layout, dtype=np.float64)
    if m.shape != (3, 3) or not np.isfinite(m).all():
        raise ValueError(f"layout must be a finite 3 x 3 matrix (erp_layout), got shape {m.shape}")
    return m


def _check_grid(nside, base_pix, supersample):
    supersample = int(supersample)
    if supersample not in (0, 1, 2):
        raise ValueError(f"supersample must be 0, 1 or 2, got {supersample}")
    return _check_nside(nside, supersample), _check_base_pix(base_pix), supersample


def _frame_kind(dtype):
    kind = {"uint8": HS_U8, "float32": HS_F32}.get(_dtype_name(dtype))
    if kind is None:
        raise TypeError(f"imgs must be uint8 or float32, got {dtype}")
    return kind


def _check_planes(planes, batch):
    """planes = [imgs, masks, depth] with batch dimensions (None where not given, not all of them): dtypes, one panorama size, the
    batch."""
    img, mask, depth = planes
    if img is not None:
        _frame_kind(img.dtype)
        if not 1 <= img.shape[1] <= MAX_CHANNELS:
            raise ValueError(f"imgs must have 1 .. {MAX_CHANNELS} channels, got {img.shape[1]}")
    if mask is not None and _dtype_name(mask.dtype) != "uint8":
        raise TypeError(f"masks must be uint8 class ids, got {mask.dtype}")
    if depth is not None and _dtype_name(depth.dtype) != "float32":
        raise TypeError(f"depth must be float32, got {depth.dtype}")
    sizes = {tuple(t.shape[-2:]) for t in planes if t is not None}
    if len(sizes) != 1:
        raise ValueError(f"imgs, masks and depth must share one panorama size, got {sorted(sizes)}")
    height, width = sizes.pop()
    if height < 1 or width < 1 or height * width >= 1 << 31:
        raise ValueError(f"the panorama must be at least 1 x 1 with height * width < 2^31, got {height} x {width}")
    _check_batch(batch)
    return height, width


class ERPProjector:
    """Equirectangular panoramas -> HEALPix: `proj(imgs, masks=None, depth=None, rotations=None)` returns `hp_img [B, C, Npix]`
    (uint8 or float32, as given), `hp_mask` uint8 [B, Npix] and `hp_depth` float32 [B, Npix] for whichever inputs are given (None
    ones are left out; a single result is returned as it is), in nested order on the first `base_pix` base pixels, ready for
    `SwinHPTransformerSys` and the losses.  imgs [(B,) C, H, W] (C <= 16), masks uint8 [(B,) H, W], depth float32 [(B,) H, W], all
    on the GPU.

    The frame is bilinear between panorama pixels with the proper weights (not the reference's `sample_bilinear`, which gives 0
    at integer coordinates); `supersample = s` averages it over the centres of each pixel's 4^s nested children (anti-aliasing:
    a 1024 x 2048 panorama has six times the pixels of nside 256).  Labels and depth take the nearest panorama pixel at the
    HEALPix pixel's own centre: classes never mix and depth values are copied bit for bit.  `rotations` [B, 3, 3] (what
    `projection.random_rotations` draws, a device tensor or a host array) are the per-sample augmentation; the matrix handed to
    the kernel is L A_b with L = `layout` (erp_layout).  A non-finite matrix gives 0 / NaN in the frame, `s2_bkgd_class` in the
    labels and `depth_fill` (default float(s2_bkgd_class), as HPRotator) in the depth.

    One launch of `hs_erp_to_hp`; L A_b is formed by elementwise sums on the device.  With `rotations` on the device nothing is
    read on the host and only the outputs (and the [B, 3, 3] matrix temporaries) are allocated: capturable."""

    def __init__(self, nside, base_pix=12, layout=None, s2_bkgd_class=0, supersample=0, device="cuda", depth_fill=None):
        self.nside, self.base_pix, self.supersample = _check_grid(nside, base_pix, supersample)
        self.s2_bkgd_class, self.depth_fill = _fills(s2_bkgd_class, depth_fill)
        self.device = torch.device(device)  # "cpu" serves `matrices` alone: `proj` takes GPU tensors only
        layout = _layout(layout)
        self._layout = None if layout is None else torch.from_numpy(layout).to(self.device)

    @property
    def npix(self):
        return self.base_pix * self.nside * self.nside

    def matrices(self, rotations, batch=None):
        """M_b = L A_b, float64 [B, 3, 3] on the device (A itself without a layout; `batch` identities for rotations=None)."""
        if rotations is None:
            m = torch.eye(3, dtype=torch.float64, device=self.device).expand(int(batch), 3, 3)
        else:
            m = _rotation_batch(rotations, self.device)
        if self._layout is not None:
            m = _matmul3(self._layout, m)  # L A_b
        return m.contiguous()

    def proj(self, imgs=None, masks=None, depth=None, rotations=None):
        planes, squeeze, batch = _gather_planes(((imgs, 4, None, _NAMES[0]), (masks, 3, None, _NAMES[1]), (depth, 3, None, _NAMES[2])))
        height, width = _check_planes(planes, batch)
        if rotations is not None and _rotation_batch(rotations).shape[0] != batch:
            raise ValueError(f"rotations holds {_rotation_batch(rotations).shape[0]} samples, the inputs {batch}")
        (img, mask, dep), outs = _device_planes(planes, _NAMES, self.device, "the projector", self.npix, 2,
                                                "the host loop is erp_to_hp_host")
        m = self.matrices(rotations, batch)
        channels = 0 if img is None else img.shape[1]
        check(lib.hs_erp_to_hp(self.nside, self.npix, ptr(m), batch, height, width, self.supersample, ptr(img),
                               HS_U8 if img is None else _frame_kind(img.dtype), channels, ptr(outs[0]), ptr(mask), ptr(outs[1]),
                               self.s2_bkgd_class, ptr(dep), ptr(outs[2]), self.depth_fill, stream_ptr(self.device)), "hs_erp_to_hp")
        return _results(outs, squeeze)

    __call__ = proj


def erp_to_hp_host(nside, rotations, imgs=None, masks=None, depth=None, base_pix=12, supersample=0, s2_bkgd_class=0, depth_fill=0.0):
    """ERPProjector.proj on the host (numpy arrays with their batch dimension; rotations [B, 3, 3] is the matrix M itself): the
    same inline function in a plain loop, equal to the kernel bit for bit (the geometry calls no math library, whose last bits
    differ between the device and the host).  Returns the outputs of the inputs given, a single one as it is."""
    nside, base_pix, supersample = _check_grid(nside, base_pix, supersample)
    m = np.ascontiguousarray(_rotation_batch(rotations).detach().cpu().numpy(), dtype=np.float64)
    planes = [None if t is None else np.ascontiguousarray(t) for t in (imgs, masks, depth)]
    _any_given(planes, _NAMES)
    for t, ndim, what in zip(planes, (4, 3, 3), _NAMES):
        if t is not None and t.ndim != ndim:
            raise ValueError(f"{what}: expected {ndim} dimensions, got {t.ndim}")
    _same_batch(planes, _NAMES, m.shape[0])
    height, width = _check_planes(planes, m.shape[0])
    img, mask, dep = planes
    npix = base_pix * nside * nside
    outs = [None if t is None else np.empty(t.shape[:-2] + (npix,), dtype=t.dtype) for t in planes]
    check(lib.hs_erp_to_hp_host(nside, npix, np_ptr(m), m.shape[0], height, width, supersample, np_ptr(img),
                                HS_U8 if img is None else _frame_kind(img.dtype), 0 if img is None else img.shape[1], np_ptr(outs[0]),
                                np_ptr(mask), np_ptr(outs[1]), int(s2_bkgd_class), np_ptr(dep), np_ptr(outs[2]), float(depth_fill)),
          "hs_erp_to_hp_host")
    return _results(outs, False)


class ERPBackProjector(HPBackProjector):
    """HEALPix predictions back onto a height x width panorama: an `HPBackProjector` in every attribute and method (`.nearest /
    .idx / .wgt / .valid / .shape / .npix / .n_out`, `.masks / .images / .depth`), built from the directions of the panorama's
    pixel centres instead of a fisheye calibration, so `SegConfusion.update(pred, erp_target, projector=back)` and the depth
    back-projection run unchanged on the existing kernels.  `layout` as for ERPProjector: pixel (i, j) looks along L^T k_ij, k_ij
    the direction of erp_grid's (theta, phi), which is where ERPProjector(layout=L) without rotations reads it from."""

    def __init__(self, height, width, nside, base_pix=12, layout=None, s2_bkgd_class=0, device="cuda"):
        theta, phi = erp_grid(height, width)
        layout = _layout(layout)
        if layout is not None:
            k = np.stack((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)), -1)
            w = k @ layout  # rows L^T k
            theta, phi = np.arctan2(np.hypot(w[..., 0], w[..., 1]), w[..., 2]), np.arctan2(w[..., 1], w[..., 0])
        self._set_tables(theta, phi, nside, base_pix, s2_bkgd_class, device)
