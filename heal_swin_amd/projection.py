"""Fisheye image -> HEALPix projection on the GPU (second half): the step that produces the model's input
(`hp_img` uint8 [3, Npix], `hp_mask` uint8 [Npix], nested order on the first `base_pix` base pixels) from a calibrated
fisheye frame.  Mirrors heal_swin/data/segmentation/project_on_s2.py -- same function names, arguments and results:

  hp_grid(nside, base_pix)                          :347-354  pix2ang of the first base_pix * nside^2 nested pixels
                                                              (`hs_pix2ang_nest`, host C++; the reference calls healpy)
  rot_grid(theta, phi, cal_info, inv)               :108-136  grid rotated so that the camera axis is the pole
  project_s2_points_to_img(theta, phi, cal_info, rotate_pole)  :141-183  WoodScape polynomial fisheye model -> (u, v)
  sample_bilinear_u8(img, rx, ry) / sample_mask(mask, rx, ry, bkgd)      :38-80   `hs_sample_bilinear_u8` / `hs_sample_mask_u8`
                                                              (HIP, float64, bit-exact; device tensors only)
  HPProjector                                        :344-372  project_dataset_hp for one calibration: the coordinate table
                                                              is built once and stays on the GPU, every batch of frames is
                                                              two kernel launches
  random_rotations / camera_record / rotated_coords  (no counterpart: the reference projects offline and has no augmentation)
                                                              per-sample roll / tilt / mirror applied to the sampling
                                                              coordinates on the device (`hs_hp_rotated_coords`), sampled by
                                                              the same kernels with one coordinate row per sample
                                                              (`per_sample=True`, `HPProjector(...)(imgs, masks, rotations=A)`)

The coordinate table is host setup work done once per calibration (the reference caches it per calibration as well); it is
float64 numpy with the reference's expression order, so that (u, v) -- and with them every sampled byte -- equal the
reference's bit for bit.  The per-image work is on the GPU only: there is no CPU sampling path.
"""
import ctypes
import math

import numpy as np
import torch

from ._lib import FisheyeCamera, check, lib, np_ptr, ptr, stream_ptr
from ._sphere_args import _batched, _matmul3, _rotation_batch

_EXT_REF = {"FV": (1.0, 0.0, 0.0), "RV": (-1.0, 0.0, 0.0), "MVL": (0.0, 1.0, 0.0), "MVR": (0.0, -1.0, 0.0)}


def hp_grid(nside, base_pix=8):
    """(theta, phi) float64 of nested pixels 0 .. base_pix * nside^2 - 1."""
    n = int(nside) * int(nside) * int(base_pix)
    theta, phi = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
    check(lib.hs_pix2ang_nest(int(nside), 0, n, np_ptr(theta), np_ptr(phi)), "hs_pix2ang_nest")
    return theta, phi


def _camera_rotation(cal_info):
    x, y, z, w = np.asarray(cal_info["extrinsic"]["quaternion"], dtype=np.float64) / np.linalg.norm(cal_info["extrinsic"]["quaternion"])
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _pole_rotation(cal_info):
    """rot_grid's matrix R = Rz(phi_ref) Ry(theta_ref) (inv=False)."""
    axis = _camera_rotation(cal_info).T @ np.asarray(_EXT_REF[cal_info["name"]])
    phi_ref, theta_ref = np.arctan2(axis[1], axis[0]), np.arccos(axis[2])
    ct, st, cp, sp = np.cos(theta_ref), np.sin(theta_ref), np.cos(phi_ref), np.sin(phi_ref)
    return np.array([[cp, -sp, 0.0], [sp, cp, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[ct, 0.0, st], [0.0, 1.0, 0.0], [-st, 0.0, ct]])


def rot_grid(theta, phi, cal_info, inv=False):
    """The grid rotated by R = Rz(phi_ref) Ry(theta_ref), (theta_ref, phi_ref) the direction of the camera's reference axis
    (FV +x, RV -x, MVL +y, MVR -y of the vehicle frame) in camera coordinates; inv=True applies R^-1."""
    m = _pole_rotation(cal_info)
    if inv:
        m = m.T
    sin_t = np.sin(theta)
    xyz = np.stack(((np.cos(phi) * sin_t).reshape(-1), (np.sin(phi) * sin_t).reshape(-1), np.cos(theta).reshape(-1)), axis=-1) @ m.T
    with np.errstate(invalid="ignore"):
        return np.arccos(xyz[:, 2]).reshape(theta.shape), np.arctan2(xyz[:, 1], xyz[:, 0]).reshape(phi.shape)


def project_s2_points_to_img(theta, phi, cal_info, rotate_pole=False):
    """Float pixel coordinates (u along the width, v along the height) of spherical points."""
    if rotate_pole:
        theta, phi = rot_grid(theta, phi, cal_info, inv=False)
    intr = cal_info["intrinsic"]
    rho = 0
    for order in range(1, intr["poly_order"] + 1):
        rho += intr["k" + str(order)] * theta**order
    u = rho * np.cos(phi) + intr["cx_offset"] + int(intr["width"]) / 2 - 0.5
    v = rho * np.sin(phi) * intr["aspect_ratio"] + intr["cy_offset"] + int(intr["height"]) / 2 - 0.5
    return u, v


def _coords(r, device):
    if torch.is_tensor(r):
        return r.to(device=device, dtype=torch.float64).contiguous().reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(r, dtype=np.float64).reshape(-1)).to(device)


def _per_sample_count(src, ndim, rx, ry):
    """per_sample=True: rx, ry must be [B, n], B the batch of `src` (1 if it has no batch dimension); returns n.  Checked before
    anything touches the device."""
    sx, sy, shape = tuple(np.shape(rx)), tuple(np.shape(ry)), tuple(np.shape(src))
    batch = shape[0] if len(shape) == ndim else 1
    if sx != sy or len(sx) != 2 or sx[0] != batch:
        raise ValueError(f"per_sample=True: rx and ry must both be [batch, n] with batch = {batch}, got {sx} and {sy}")
    return sx[1]


def _sample(name, src, ndim, dtype, what, rx, ry, per_sample, out_dtype, background=()):
    """The four public samplers (two here, two in depth_data): src [(B,) ..., H, W] of `ndim` dimensions with its batch one, checked,
    then `hs_<name>` or `hs_<name>_per_sample` with `background` between n and the output -> out_dtype [(B,) ..., n]."""
    n = _per_sample_count(src, ndim, rx, ry) if per_sample else None
    src, squeeze = _batched(src, ndim, what, dtype)
    if n is None and int(np.prod(np.shape(rx))) != int(np.prod(np.shape(ry))):
        raise ValueError("rx and ry must have the same shape")
    if not src.is_cuda:
        raise RuntimeError(f"{what} must be a GPU tensor: the sampling runs in the HIP kernels only (no CPU path)")
    src = src.contiguous()
    rx, ry = _coords(rx, src.device), _coords(ry, src.device)
    n = rx.numel() if n is None else n
    out = torch.empty(src.shape[:-2] + (n,), dtype=out_dtype, device=src.device)
    fn = getattr(lib, f"hs_{name}_per_sample" if per_sample else f"hs_{name}")
    check(fn(ptr(src), *src.shape, ptr(rx), ptr(ry), n, *background, ptr(out), stream_ptr(src.device)), f"hs_{name}")
    return out[0] if squeeze else out


def sample_bilinear_u8(img, rx, ry, per_sample=False):
    """`sample_bilinear(img, rx, ry).astype(np.uint8)`: img uint8 [C, H, W] or [B, C, H, W] on the GPU, rx along H, ry along
    W (float64 arrays or tensors) -> uint8 [(B,) C, n].  per_sample=False: one coordinate table for the whole batch (rx, ry of
    any shape are flattened).  per_sample=True: rx, ry are [B, n] and sample b reads row b (`hs_sample_bilinear_u8_per_sample`,
    the same kernel and arithmetic)."""
    return _sample("sample_bilinear_u8", img, 4, torch.uint8, "img", rx, ry, per_sample, torch.uint8)


def sample_mask(mask, rx, ry, s2_bkgd_class=0, per_sample=False):
    """Nearest-pixel (round half to even) class ids: mask uint8 [H, W] or [B, H, W] on the GPU -> uint8 [(B,) n].  Classes
    never mix.  per_sample as in sample_bilinear_u8 (`hs_sample_mask_u8_per_sample`)."""
    return _sample("sample_mask_u8", mask, 3, torch.uint8, "mask", rx, ry, per_sample, torch.uint8, (int(s2_bkgd_class),))


# ------------------------------------------------------------------ per-sample rotation augmentation
def random_rotations(batch, max_tilt_deg=0.0, roll=True, flip=0.0, generator=None, device=None):
    """float64 [batch, 3, 3] augmentation matrices A = Rz(roll) T F for `rotations=`:
      roll  uniform in [0, 2 pi) about the optical axis (0 with roll=False),
      T     a rotation by an angle uniform in [0, max_tilt_deg] about a uniformly random axis in the xy plane (a camera tilt),
      F     diag(-1, 1, 1) with probability `flip` (the left-right mirror of the image), else the identity.
    Drawn on the host from `generator` (a torch.Generator; None: torch's default one), four numbers per sample whatever the
    options, then moved to `device`."""
    batch = int(batch)
    if batch < 0 or not 0.0 <= float(flip) <= 1.0 or float(max_tilt_deg) < 0.0:
        raise ValueError("random_rotations: batch >= 0, max_tilt_deg >= 0 and 0 <= flip <= 1 are required")
    r = torch.rand((batch, 4), dtype=torch.float64, generator=generator).numpy()
    a = 2.0 * math.pi * r[:, 0] if roll else np.zeros(batch)
    t, psi = math.radians(float(max_tilt_deg)) * r[:, 1], 2.0 * math.pi * r[:, 2]
    one, zero = np.ones(batch), np.zeros(batch)
    rz = np.stack([np.cos(a), -np.sin(a), zero, np.sin(a), np.cos(a), zero, zero, zero, one], -1).reshape(batch, 3, 3)
    # Rodrigues about (cos psi, sin psi, 0): I + sin t K + (1 - cos t) K^2
    x, y, st, vt = np.cos(psi), np.sin(psi), np.sin(t), 1.0 - np.cos(t)
    tilt = np.stack([1.0 - vt * y * y, vt * x * y, st * y,
                     vt * x * y, 1.0 - vt * x * x, -st * x,
                     -st * y, st * x, 1.0 - vt * (x * x + y * y)], -1).reshape(batch, 3, 3)
    out = np.matmul(rz, tilt)
    out[:, :, 0] = np.where((r[:, 3] < float(flip))[:, None], -out[:, :, 0], out[:, :, 0])  # (Rz T) F: the first column negated
    out = torch.from_numpy(out + 0.0)  # + 0.0: no negative zeros
    return out if device is None else out.to(device)


def camera_record(cal_info, used_size=None):
    """The `hs_fisheye_camera` of a calibration (ctypes, `_lib.FisheyeCamera`); used_size = (height, width) of the image actually
    sampled replaces the calibration's size, as in depth_data.project_depth_s2_points_to_img."""
    intr = cal_info["intrinsic"]
    order = int(intr["poly_order"])
    if not 1 <= order <= 8:
        raise ValueError(f"poly_order must be in [1, 8], got {order}")
    cam = FisheyeCamera()
    for i in range(order):
        cam.k[i] = float(intr["k" + str(i + 1)])
    cam.cx_offset, cam.cy_offset, cam.aspect_ratio = float(intr["cx_offset"]), float(intr["cy_offset"]), float(intr["aspect_ratio"])
    cam.poly_order = order
    cam.height, cam.width = (int(intr["height"]), int(intr["width"])) if used_size is None else (int(used_size[0]), int(used_size[1]))
    return cam


def _rotated_coords(nside, base_pix, cam, rotations, pole, device):
    """rotated_coords on prepared arguments: cam a FisheyeCamera, pole None or rot_grid's matrix as a float64 [3, 3] tensor on
    `device`.  No host synchronisation and, with `rotations` on the device, no copy: capturable."""
    device = torch.device(device)
    m = _rotation_batch(rotations, device)
    if pole is not None:
        m = _matmul3(m, pole)  # A_b R
    m = m.contiguous()
    batch, n = m.shape[0], int(nside) * int(nside) * int(base_pix)
    u = torch.empty((batch, n), dtype=torch.float64, device=device)
    v = torch.empty((batch, n), dtype=torch.float64, device=device)
    check(lib.hs_hp_rotated_coords(int(nside), 0, n, ctypes.byref(cam), ptr(m), batch, ptr(u), ptr(v), stream_ptr(device)),
          "hs_hp_rotated_coords")
    return u, v


def rotated_coords(nside, base_pix, cal_info, rotations, rotate_pole=False, used_size=None, device="cuda"):
    """(u, v) float64 [B, Npix] on the device: project_s2_points_to_img of hp_grid(nside, base_pix) for each of B samples, the
    grid's unit vectors multiplied by M_b = A_b R first (`hs_hp_rotated_coords`, one launch).  rotations = A [B, 3, 3], a
    device tensor or a host array (random_rotations); R is rot_grid's pole rotation (inv=False), the identity without
    rotate_pole.  The augmentation acts in the camera frame: roll is about the optical axis and keeps the image circle in
    place; output pixel p shows the camera-frame direction A_b R g_p, that is, the map shows the scene rotated by A_b^-1.  The
    product A_b R is formed on the device; nothing synchronises with the host.

    The pixel centres, the rotation and the camera model are evaluated in float64 on the device, so identity rotations agree
    with HPProjector's host-built table to rounding (about 1e-12 px), NOT bit for bit: the exact path is the table."""
    _rotation_batch(rotations)
    device = torch.device(device)
    pole = torch.from_numpy(_pole_rotation(cal_info)).to(device) if rotate_pole else None
    return _rotated_coords(nside, base_pix, camera_record(cal_info, used_size), rotations, pole, device)


def _with_used_size(cal_info, used_size):
    """cal_info with used_size = (height, width) of the image actually sampled in place of the calibration's size"""
    if used_size is None:
        return cal_info
    return dict(cal_info, intrinsic=dict(cal_info["intrinsic"], height=int(used_size[0]), width=int(used_size[1])))


class _FisheyeProjector:
    """What HPProjector and depth_data.HPDepthProjector share: the resident coordinate table of one calibration, the per-sample
    coordinates under `rotations`, and the two sampling launches.  A subclass names its frame and nearest samplers, the type of its
    background value and the keyword of its second plane."""

    _sample_frame = _sample_nearest = None

    def __init__(self, cal_info, nside, base_pix, rotate_pole, s2_bkgd_class, used_size, device):
        self.nside, self.base_pix, self.s2_bkgd_class = int(nside), int(base_pix), s2_bkgd_class
        theta, phi = hp_grid(self.nside, self.base_pix)
        u, v = project_s2_points_to_img(theta, phi, _with_used_size(cal_info, used_size), rotate_pole)
        self.device = torch.device(device)
        self.u, self.v = _coords(u, self.device), _coords(v, self.device)  # resident coordinate table: 16 B per pixel
        self._cam = camera_record(cal_info, used_size)
        self._pole = torch.from_numpy(_pole_rotation(cal_info)).to(self.device) if rotate_pole else None

    @property
    def npix(self):
        return self.u.numel()

    def _proj(self, imgs, nearest, rotations):
        if rotations is None:
            u, v, per_sample = self.u, self.v, False
        else:
            u, v = _rotated_coords(self.nside, self.base_pix, self._cam, rotations, self._pole, self.device)
            per_sample = True
        hp_img = self._sample_frame(imgs, v, u, per_sample)
        if nearest is None:
            return hp_img
        return hp_img, self._sample_nearest(nearest, v, u, self.s2_bkgd_class, per_sample)


class HPProjector(_FisheyeProjector):
    """project_dataset_hp for the frames of one camera: `proj(imgs, masks)` -> (hp_img uint8 [B, C, Npix], hp_mask uint8
    [B, Npix]) on the GPU, ready for `SwinHPTransformerSys.forward` and `seg_loss` (or `data.write_sample`).

    `proj(imgs, masks, rotations=A)` with A [B, 3, 3] (random_rotations) is the augmented projection: one coordinate launch
    (rotated_coords) plus the per-sample sampling launches; labels are still sampled nearest, so classes never mix, and samples
    outside the image are 0 in the frame and `s2_bkgd_class` in the labels as without rotations.  `rotations=None` is the exact
    path: the resident table, the reference's bytes.  Identity rotations go through the device arithmetic and agree with it to
    coordinate rounding only (about 1e-12 px), not bit for bit."""

    _sample_frame, _sample_nearest = staticmethod(sample_bilinear_u8), staticmethod(sample_mask)

    def __init__(self, cal_info, nside, base_pix=8, rotate_pole=False, s2_bkgd_class=0, device="cuda"):
        super().__init__(cal_info, nside, base_pix, rotate_pole, int(s2_bkgd_class), None, device)

    def proj(self, imgs, masks=None, rotations=None):
        return self._proj(imgs, masks, rotations)

    __call__ = proj
