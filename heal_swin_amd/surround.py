"""Surround view: the frames of a rig of calibrated fisheye cameras fused onto one HEALPix sphere, and back.  WoodScape and
SynWoodScape record four fisheye cameras (FV, RV, MVL, MVR), each with an extrinsic quaternion in the vehicle frame
(`projection._EXT_REF` names them); together they see the whole sphere, which one camera (8 base pixels at the most) does not.
This is the data boundary of the full-sphere model (12 base pixels) for such frames, as `erp.ERPProjector` is for panoramas.
No counterpart in the reference, which projects one camera at a time, offline.

  SurroundProjector          `proj(imgs, masks, depth, rotations=A, present=P)`: the frames (bilinear, the winner's or feathered),
                             labels and depth (the winner's nearest pixel, copied) of a batch of rigs in one launch, no table
                             written                                                                        `hs_surround_to_hp`
  surround_to_hp_host(...)   the same statements in a host loop (numpy), the kernel's oracle           `hs_surround_to_hp_host`
  SurroundBackProjector      an `HPBackProjector` whose image plane is ONE camera of the rig: `.masks / .images / .depth` and
                             `SegConfusion.update(pred, target, projector=...)` score a surround prediction against that
                             camera's own ground truth on the existing kernels

Convention.  The sphere's frame is taken to the vehicle frame by F (`frame=`, None: the identity, the HEALPix pole is the
vehicle's z axis), the vehicle frame to camera c's by R_c^T (R_c = `projection._camera_rotation`, as `_pole_rotation` uses it), and
A_b is the per-sample augmentation (`projection.random_rotations`, or any [B, 3, 3]; a yaw about the vehicle's z is the natural
one): output pixel p of sample b is seen by camera c along M[b, c] g_p with M[b, c] = R_c^T F A_b, g_p the centre of nested pixel p.

Per camera (include/healswin.h has every statement): theta is the angle from the optical axis; beyond `max_theta_deg` the camera
does not see the pixel.  `max_theta_deg` is what keeps a calibration polynomial that is not monotonic from folding far directions
back into the image.  (u, v) are the WoodScape polynomial model's image coordinates; the pixel is seen iff its nearest image
pixel lies inside the image.  The weight is w = (1 - theta / max_theta) min(1, m / edge_feather), m the distance to the nearest
image border in pixels: it falls off away from the axis, where a fisheye lens is least sharp, and to zero at the border, so that
no seam shows.  A camera counts iff it is seen and w > 0; the winner is the counting camera of largest w (the lowest index among
equals).  blend="winner": the winner's bilinear value; blend="feather": the w-weighted mean of the counting cameras' values.
Labels and depth always come from the winner's nearest pixel: classes never mix and depth values are copied bit for bit.

Depth is each camera's own range.  The parallax between the cameras' centres is ignored: the rig is treated as one viewpoint
(WoodScape's cameras are 1 - 2 m apart, so objects nearer than a few metres show a seam that no projection onto one sphere can
avoid).  The frame uses the proper bilinear weights (1 - f, f) with rows and columns clamped to the image, as `erp`, not the
reference's `sample_bilinear`; the existing fisheye path (`HPProjector`) keeps its reference-parity weights and truncation.
"""
import math

import numpy as np
import torch

from ._lib import HS_U8, SurroundRig, check, lib, np_ptr, ptr, stream_ptr
from ._sphere_args import (MAX_CHANNELS, _any_given, _check_base_pix, _check_batch, _check_nside, _dtype_name, _fills, _gather_planes,
                           _matmul3, _on_device, _results, _rotation_batch, _same_batch)
from .erp import _frame_kind
from .evaluation import HPBackProjector, get_uv_from_hw, project_img_points_to_s2
from .projection import _camera_rotation, camera_record

MAX_CAMERAS = 8
_NAMES = ("imgs", "masks", "depth")
_BLENDS = {"winner": 0, "feather": 1}


def _frame_matrix(frame):
    if frame is None:
        return np.eye(3)
    m = np.ascontiguousarray(frame, dtype=np.float64)
    if m.shape != (3, 3) or not np.isfinite(m).all():
        raise ValueError(f"frame must be a finite 3 x 3 matrix (the sphere's frame to the vehicle frame), got shape {m.shape}")
    return m


def _rig(cal_infos, blend="feather", max_theta_deg=95.0, edge_feather=8.0, used_size=None):
    """The `hs_surround_rig` (ctypes) of 1 .. 8 calibrations, every value checked as the C ABI checks it."""
    cals = list(cal_infos)
    if not 1 <= len(cals) <= MAX_CAMERAS:
        raise ValueError(f"a rig has 1 .. {MAX_CAMERAS} cameras, got {len(cals)}")
    if blend not in _BLENDS:
        raise ValueError(f"blend must be 'winner' or 'feather', got {blend!r}")
    deg = np.asarray(max_theta_deg, dtype=np.float64)
    if deg.ndim > 1 or (deg.ndim == 1 and deg.shape[0] != len(cals)):
        raise ValueError(f"max_theta_deg must be a scalar or one value per camera ({len(cals)}), got shape {deg.shape}")
    theta = math.pi * (np.broadcast_to(deg, (len(cals),)) / 180.0)
    if not (np.isfinite(theta) & (theta > 0.0) & (theta <= math.pi)).all():
        raise ValueError(f"max_theta_deg must be in (0, 180], got {max_theta_deg}")
    edge_feather = float(edge_feather)
    if not (math.isfinite(edge_feather) and edge_feather >= 0.0):
        raise ValueError(f"edge_feather must be finite and >= 0 (pixels), got {edge_feather}")
    rig = SurroundRig()
    rig.n_cameras, rig.edge_feather, rig.blend = len(cals), edge_feather, _BLENDS[blend]
    for c, cal in enumerate(cals):
        rig.cam[c] = camera_record(cal, used_size)  # refuses a poly_order outside 1 .. 8
        rig.max_theta[c] = float(theta[c])
    sizes = {(rig.cam[c].height, rig.cam[c].width) for c in range(len(cals))}
    if len(sizes) != 1:
        raise ValueError(f"the cameras of a rig share one image size (used_size sets it), got {sorted(sizes)}")
    height, width = sizes.pop()
    if height < 1 or width < 1 or height * width >= 1 << 31:
        raise ValueError(f"the images must be at least 1 x 1 with height * width < 2^31, got {height} x {width}")
    return rig


def _check_planes(planes, batch, rig):
    """planes = [imgs [B, K, C, H, W], masks [B, K, H, W], depth [B, K, H, W]] (None where not given, not all of them): dtypes, the
    camera count, the rig's image size, the batch."""
    img, mask, depth = planes
    if img is not None:
        _frame_kind(img.dtype)
        if not 1 <= img.shape[2] <= MAX_CHANNELS:
            raise ValueError(f"imgs must have 1 .. {MAX_CHANNELS} channels, got {img.shape[2]}")
    if mask is not None and _dtype_name(mask.dtype) != "uint8":
        raise TypeError(f"masks must be uint8 class ids, got {mask.dtype}")
    if depth is not None and _dtype_name(depth.dtype) != "float32":
        raise TypeError(f"depth must be float32, got {depth.dtype}")
    height, width = rig.cam[0].height, rig.cam[0].width
    for t, what in zip(planes, _NAMES):
        if t is not None and t.shape[1] != rig.n_cameras:
            raise ValueError(f"{what} holds {t.shape[1]} cameras, the rig {rig.n_cameras}")
        if t is not None and tuple(t.shape[-2:]) != (height, width):
            raise ValueError(f"{what} is {t.shape[-2]} x {t.shape[-1]}, the rig's cameras {height} x {width}")
    _check_batch(batch)
    return height, width


def _check_present(present, batch, n_cameras):
    """present [B, K] bool / uint8 (tensor or array), checked without touching the device"""
    if _dtype_name(present.dtype) not in ("bool", "uint8"):
        raise TypeError(f"present must be bool or uint8, got {present.dtype}")
    if tuple(present.shape) != (batch, n_cameras):
        raise ValueError(f"present must be [batch, cameras] = [{batch}, {n_cameras}], got {tuple(present.shape)}")


def _out_shapes(planes, npix):
    return [None if t is None else (t.shape[0],) + ((t.shape[2],) if i == 0 else ()) + (npix,) for i, t in enumerate(planes)]


class SurroundProjector:
    """The frames of a rig of fisheye cameras -> one HEALPix sphere: `proj(imgs, masks=None, depth=None, rotations=None,
    present=None, return_camera=False)` returns `hp_img [B, C, Npix]` (uint8 or float32, as given), `hp_mask` uint8 [B, Npix] and
    `hp_depth` float32 [B, Npix] for whichever inputs are given, and `camera` uint8 [B, Npix] (the winner's index, 255 where no
    camera counts) last when asked for; a single result is returned as it is.  Nested order on the first `base_pix` base pixels,
    ready for `SwinHPTransformerSys` and the losses.  imgs [(B,) K, C, H, W] (C <= 16), masks uint8 [(B,) K, H, W], depth float32
    [(B,) K, H, W], all on the GPU, K the cameras of `cal_infos` (1 .. 8 WoodScape calibrations, one image size: `used_size` =
    (height, width) replaces the calibrations').

    `max_theta_deg`, a scalar or one value per camera, bounds the angle from the optical axis (95 degrees is half of WoodScape's
    190-degree lenses); it is what keeps a non-monotonic polynomial from folding far directions back into the image.
    `edge_feather` is the width in pixels over which the weight falls to zero at the image border.  `rotations` [B, 3, 3] (device
    tensor or host array) are the per-sample augmentation A_b, `present` [B, K] (bool / uint8) drops cameras per sample (camera
    dropout, or a sample with a missing camera).  A pixel that no camera counts for, and every pixel of a camera-less sample, is 0
    / NaN in the frame, `s2_bkgd_class` in the labels, `depth_fill` (default float(s2_bkgd_class)) in the depth.  A non-finite
    matrix removes its camera only.  Depth is each camera's own range: the parallax between the cameras' centres is ignored.

    One launch of `hs_surround_to_hp`; M[b, c] = R_c^T F A_b is formed by elementwise sums on the device.  With `rotations` and
    `present` on the device nothing is read on the host and only the outputs (and the [B, K, 3, 3] matrix temporaries) are
    allocated: capturable, after one eager call (the first call moves the K matrices R_c^T F to the device)."""

    def __init__(self, cal_infos, nside, base_pix=12, frame=None, blend="feather", max_theta_deg=95.0, edge_feather=8.0, s2_bkgd_class=0,
                 depth_fill=None, used_size=None, device="cuda"):
        self.nside, self.base_pix = _check_nside(nside), _check_base_pix(base_pix)
        self.s2_bkgd_class, self.depth_fill = _fills(s2_bkgd_class, depth_fill)
        cals = list(cal_infos)
        self._rig = _rig(cals, blend, max_theta_deg, edge_feather, used_size)
        f = _frame_matrix(frame)
        self.device = torch.device(device)  # "cpu" serves `matrices` alone: `proj` takes GPU tensors only
        # R_c^T F [K, 3, 3]; moved to the device by the first call, so that building a projector touches no device
        self._base_host, self._base_dev = torch.from_numpy(np.stack([_camera_rotation(c).T @ f for c in cals])), None

    @property
    def _base(self):
        if self._base_dev is None:
            self._base_dev = self._base_host.to(self.device)
        return self._base_dev

    @property
    def npix(self):
        return self.base_pix * self.nside * self.nside

    @property
    def n_cameras(self):
        return self._rig.n_cameras

    def matrices(self, rotations, batch=None):
        """M[b, c] = R_c^T F A_b, float64 [B, K, 3, 3] on the device (`batch` copies of R_c^T F for rotations=None)."""
        if rotations is None:
            return self._base.expand(int(batch), *self._base.shape).contiguous()
        a = _rotation_batch(rotations, self.device)
        return _matmul3(self._base[None], a[:, None]).contiguous()

    def proj(self, imgs=None, masks=None, depth=None, rotations=None, present=None, return_camera=False):
        planes, squeeze, batch = _gather_planes(((imgs, 5, None, _NAMES[0]), (masks, 4, None, _NAMES[1]), (depth, 4, None, _NAMES[2])))
        height, width = _check_planes(planes, batch, self._rig)
        if rotations is not None and _rotation_batch(rotations).shape[0] != batch:
            raise ValueError(f"rotations holds {_rotation_batch(rotations).shape[0]} samples, the inputs {batch}")
        if present is not None:
            if not torch.is_tensor(present):
                present = torch.from_numpy(np.ascontiguousarray(present))
            if squeeze and present.dim() == 1:
                present = present[None]
            _check_present(present, batch, self.n_cameras)
        img, mask, dep = _on_device(planes, _NAMES, self.device, "the projector", "the host loop is surround_to_hp_host")
        outs = [None if s is None else torch.empty(s, dtype=t.dtype, device=t.device) for s, t in zip(_out_shapes(planes, self.npix), planes)]
        cam = torch.empty((batch, self.npix), dtype=torch.uint8, device=self.device) if return_camera else None
        if present is not None:
            present = present.to(self.device).contiguous()
            present = present.view(torch.uint8) if present.dtype == torch.bool else present  # a bool is one byte, 0 or 1
        m = self.matrices(rotations, batch)
        check(lib.hs_surround_to_hp(self.nside, self.npix, self._rig, ptr(m), ptr(present), batch, height, width, ptr(img),
                                    HS_U8 if img is None else _frame_kind(img.dtype), 0 if img is None else img.shape[2], ptr(outs[0]),
                                    ptr(mask), ptr(outs[1]), self.s2_bkgd_class, ptr(dep), ptr(outs[2]), self.depth_fill, ptr(cam),
                                    stream_ptr(self.device)), "hs_surround_to_hp")
        return _results(outs + [cam], squeeze)

    __call__ = proj


def surround_to_hp_host(cal_infos, nside, matrices, imgs=None, masks=None, depth=None, present=None, base_pix=12, blend="feather",
                        max_theta_deg=95.0, edge_feather=8.0, s2_bkgd_class=0, depth_fill=0.0, used_size=None, return_camera=False):
    """SurroundProjector.proj on the host (numpy arrays with their batch dimension; matrices [B, K, 3, 3] is M itself, what
    `SurroundProjector.matrices` returns): the same inline function in a plain loop, equal to the kernel bit for bit (the geometry
    calls no math library).  Returns the outputs of the inputs given, `camera` last when asked for, a single one as it is."""
    nside, base_pix = _check_nside(nside), _check_base_pix(base_pix)
    rig = _rig(cal_infos, blend, max_theta_deg, edge_feather, used_size)
    m = np.ascontiguousarray(matrices.detach().cpu().numpy() if torch.is_tensor(matrices) else matrices, dtype=np.float64)
    if m.ndim != 4 or m.shape[1:] != (rig.n_cameras, 3, 3) or m.shape[0] < 1:
        raise ValueError(f"matrices must be [batch, {rig.n_cameras}, 3, 3] with batch >= 1, got {m.shape}")
    planes = [None if t is None else np.ascontiguousarray(t) for t in (imgs, masks, depth)]
    _any_given(planes, _NAMES)
    for t, ndim, what in zip(planes, (5, 4, 4), _NAMES):
        if t is not None and t.ndim != ndim:
            raise ValueError(f"{what}: expected {ndim} dimensions, got {t.ndim}")
    batch = m.shape[0]
    _same_batch(planes, _NAMES, batch)
    height, width = _check_planes(planes, batch, rig)
    if present is not None:
        present = np.ascontiguousarray(present)
        _check_present(present, batch, rig.n_cameras)
        present = present.view(np.uint8) if present.dtype == np.bool_ else present
    img, mask, dep = planes
    npix = base_pix * nside * nside
    outs = [None if s is None else np.empty(s, dtype=t.dtype) for s, t in zip(_out_shapes(planes, npix), planes)]
    cam = np.empty((batch, npix), dtype=np.uint8) if return_camera else None
    s2_bkgd_class, depth_fill = _fills(s2_bkgd_class, depth_fill)
    check(lib.hs_surround_to_hp_host(nside, npix, rig, np_ptr(m), np_ptr(present), batch, height, width, np_ptr(img),
                                     HS_U8 if img is None else _frame_kind(img.dtype), 0 if img is None else img.shape[2], np_ptr(outs[0]),
                                     np_ptr(mask), np_ptr(outs[1]), s2_bkgd_class, np_ptr(dep), np_ptr(outs[2]), depth_fill, np_ptr(cam)),
          "hs_surround_to_hp_host")
    return _results(outs + [cam], False)


class SurroundBackProjector(HPBackProjector):
    """HEALPix predictions of a surround sphere back onto the image of ONE camera of the rig: an `HPBackProjector` in every
    attribute and method (`.nearest / .idx / .wgt / .valid / .shape / .npix / .n_out`, `.masks / .images / .depth`), so
    `SegConfusion.update(pred, target, projector=back)` scores a surround prediction against that camera's own ground truth on
    the existing kernels.  Image pixel (u, v) (`get_uv_from_hw` of the calibration's size and `output_resolution`) looks along
    k = `project_img_points_to_s2(u, v, cal_info)` in the camera frame, that is along F^T R_c k in the sphere's frame, which is
    where SurroundProjector(frame=F) without rotations shows that camera (F orthogonal).  Built from the directions alone, as
    `HPBackProjector.from_angles` builds it."""

    def __init__(self, cal_info, nside, base_pix=12, frame=None, output_resolution=1.0, s2_bkgd_class=0, device="cuda"):
        intr = cal_info["intrinsic"]
        u, v = get_uv_from_hw(intr["height"], intr["width"], output_resolution)
        theta, phi = project_img_points_to_s2(u, v, cal_info)
        k = np.stack((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)), -1)
        w = k @ (_camera_rotation(cal_info).T @ _frame_matrix(frame))  # rows F^T R_c k
        theta, phi = np.arctan2(np.hypot(w[..., 0], w[..., 1]), w[..., 2]), np.arctan2(w[..., 1], w[..., 0])
        self._set_tables(theta, phi, _check_nside(nside), _check_base_pix(base_pix), s2_bkgd_class, device)
