"""Rotation of maps that already live on the sphere: augmentation for datasets that were projected once, offline, as the
reference's are (`hp_img` / `hp_mask` read from `.npz` files, heal_swin/data/segmentation/hp_datasets.py:92-98, and the HEALPix
depth maps of the depth datasets).  No frame is needed: the stored map is resampled on the device under each sample's own 3x3
matrix (no counterpart in the reference, which has no augmentation).

  rotated_interp(nside, rotations, first_pix, count)   healpy's get_interp_weights of the rotated pixel centres M_b g_p, per
                                                       (sample, pixel) on the device: (pix int32 [B, 4, n], wgt float64
                                                       [B, 4, n], nearest int32 [B, n])   `hs_hp_rotated_interp`
  rotated_interp_host(...)                             the same statements in a host loop (numpy), the device path's oracle
                                                                                          `hs_hp_rotated_interp_host`
  HPRotator                                            `rot(hp_img, hp_mask, hp_depth, rotations=A)`: frame (four-pixel
                                                       interpolation, rint), labels and depth (nearest pixel, copied) of a
                                                       batch in one launch, no table written   `hs_hp_rotate`

Convention (that of projection.rotated_coords): output pixel p of sample b shows the source map at direction M_b g_p.  For
`HPRotator`, A is what `projection.random_rotations` draws, in the camera frame, and M_b = R^T A_b R with R the pole rotation
of a dataset projected with rotate_pole (else the identity), so `rot(*proj(imgs, masks), rotations=A)` shows the scene of
`proj(imgs, masks, rotations=A)` -- at the cost of a second interpolation, which the projector's own augmentation avoids
whenever the frames are at hand.
"""
import numpy as np
import torch

from ._lib import check, lib, np_ptr, ptr, stream_ptr
from .projection import _pole_rotation, _rotation_batch

MAX_NSIDE = 8192  # 12 nside^2 nested indices as int32
MAX_CHANNELS = 16


def _check_grid(nside, first_pix, count, batch):
    nside, first_pix = int(nside), int(first_pix)
    if nside < 1 or nside & (nside - 1) or nside > MAX_NSIDE:
        raise ValueError(f"nside must be a power of two in [1, {MAX_NSIDE}], got {nside}")
    npix = 12 * nside * nside
    count = npix - first_pix if count is None else int(count)
    if first_pix < 0 or count < 0 or first_pix + count > npix:
        raise ValueError(f"pixels [{first_pix}, {first_pix + count}) outside [0, {npix}) for nside {nside}")
    if batch > 65535:
        raise ValueError(f"batch must be in [1, 65535], got {batch}")
    return nside, first_pix, count


def rotated_interp(nside, rotations, first_pix=0, count=None, device="cuda"):
    """(pix int32 [B, 4, count], wgt float64 [B, 4, count], nearest int32 [B, count]) on the device: HEALPix's get_interpol
    (healpy.get_interp_weights, nest=True) at the directions M_b g_p of the nested pixels first_pix .. first_pix + count - 1
    (count=None: up to 12 nside^2), and the pixel of largest weight (evaluation.hp_nearest_pix_idcs).  rotations [B, 3, 3], a
    device tensor or a host array; any real matrix is accepted, a non-finite one gives -1 / 0 / -1 for its sample.  One launch,
    nothing synchronises with the host."""
    batch = _rotation_batch(rotations).shape[0]
    nside, first_pix, count = _check_grid(nside, first_pix, count, batch)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"rotated_interp runs in the HIP kernel only, got device {device} (the host loop is rotated_interp_host)")
    m = _rotation_batch(rotations, device).contiguous()
    pix = torch.empty((batch, 4, count), dtype=torch.int32, device=device)
    wgt = torch.empty((batch, 4, count), dtype=torch.float64, device=device)
    nearest = torch.empty((batch, count), dtype=torch.int32, device=device)
    check(lib.hs_hp_rotated_interp(nside, first_pix, count, ptr(m), batch, ptr(pix), ptr(wgt), ptr(nearest), stream_ptr(device)),
          "hs_hp_rotated_interp")
    return pix, wgt, nearest


def rotated_interp_host(nside, rotations, first_pix=0, count=None):
    """rotated_interp on the host (numpy arrays): the same inline function in a plain loop."""
    m = _rotation_batch(rotations)
    m = np.ascontiguousarray(m.detach().cpu().numpy(), dtype=np.float64)
    batch = m.shape[0]
    nside, first_pix, count = _check_grid(nside, first_pix, count, batch)
    pix = np.empty((batch, 4, count), dtype=np.int32)
    wgt = np.empty((batch, 4, count), dtype=np.float64)
    nearest = np.empty((batch, count), dtype=np.int32)
    check(lib.hs_hp_rotated_interp_host(nside, first_pix, count, np_ptr(m), batch, np_ptr(pix), np_ptr(wgt), np_ptr(nearest)),
          "hs_hp_rotated_interp_host")
    return pix, wgt, nearest


def _plane(t, dtype, ndim, npix, what):
    """A map with its batch dimension, plus whether that was added: dtype, rank and pixel count, checked without touching the
    device."""
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if t.dtype != dtype:
        raise TypeError(f"{what} must be {dtype}, got {t.dtype}")
    lead = ndim - t.dim()
    if lead not in (0, 1):
        raise ValueError(f"{what}: expected {ndim - 1} or {ndim} dimensions, got {t.dim()}")
    if t.shape[-1] != npix:
        raise ValueError(f"{what} covers {t.shape[-1]} HEALPix pixels, expected {npix}")
    return (t[None] if lead else t), bool(lead)


class HPRotator:
    """Per-sample rotation of HEALPix-resident samples: `rot(hp_img, hp_mask, hp_depth, rotations=A)` returns the given maps
    (None ones are left out) rotated, in that order, dtypes and shapes as given -- hp_img uint8 [(B,) C, Npix] (C <= 16), hp_mask
    uint8 [(B,) Npix], hp_depth float32 [(B,) Npix] on the GPU, Npix = base_pix nside^2.

    A [B, 3, 3] is what projection.random_rotations draws, in the camera frame: `cal_info` and `rotate_pole=True` name the pole
    rotation R of a dataset that was projected with rotate_pole, and the maps are resampled under M_b = R^T A_b R
    (`rot.matrices(A)`).  The frame is interpolated between four pixels (rint, neighbours outside the `base_pix` base pixels read
    0); labels and depth take the pixel of largest weight (`s2_bkgd_class`, `depth_fill` outside), so classes never mix and depth
    values are copied bit for bit.  depth_fill defaults to float(s2_bkgd_class): what HPDepthProjector writes outside the image,
    and what DepthTargetTransform.prepare turns into inf.

    One launch of `hs_hp_rotate`; the matrices are formed by elementwise sums on the device.  With `rotations` on the device
    nothing is read on the host and only the outputs (and the [B, 3, 3] matrix temporaries) are allocated: capturable."""

    def __init__(self, nside, base_pix=8, cal_info=None, rotate_pole=False, s2_bkgd_class=0, depth_fill=None, device="cuda"):
        self.nside, _, _ = _check_grid(nside, 0, 0, 1)
        self.base_pix, self.s2_bkgd_class = int(base_pix), int(s2_bkgd_class)
        if not 1 <= self.base_pix <= 12:
            raise ValueError(f"base_pix must be in [1, 12], got {base_pix}")
        if not 0 <= self.s2_bkgd_class <= 255:
            raise ValueError(f"s2_bkgd_class must be in [0, 255] (uint8 labels), got {s2_bkgd_class}")
        if rotate_pole and cal_info is None:
            raise ValueError("rotate_pole=True needs the cal_info the dataset was projected with")
        self.depth_fill = float(s2_bkgd_class) if depth_fill is None else float(depth_fill)
        self.device = torch.device(device)  # "cpu" serves `matrices` alone: `rot` takes GPU tensors only
        self._pole = torch.from_numpy(_pole_rotation(cal_info)).to(self.device) if rotate_pole else None

    @property
    def npix(self):
        return self.base_pix * self.nside * self.nside

    def matrices(self, rotations):
        """M_b = R^T A_b R, float64 [B, 3, 3] on the device (A itself without rotate_pole)."""
        m = _rotation_batch(rotations, self.device)
        if self._pole is not None:
            m = (m[:, :, :, None] * self._pole[None, None, :, :]).sum(2)  # A_b R, elementwise: the same rounding on every device
            m = (self._pole.t()[None, :, :, None] * m[:, None, :, :]).sum(2)  # R^T (A_b R)
        return m.contiguous()

    def rot(self, hp_img=None, hp_mask=None, hp_depth=None, rotations=None):
        if rotations is None:
            raise ValueError("rotations=A [batch, 3, 3] is required (projection.random_rotations)")
        batch = _rotation_batch(rotations).shape[0]
        if hp_img is None and hp_mask is None and hp_depth is None:
            raise ValueError("give at least one of hp_img, hp_mask, hp_depth")
        planes, squeezes = [], set()
        for t, dtype, ndim, what in ((hp_img, torch.uint8, 3, "hp_img"), (hp_mask, torch.uint8, 2, "hp_mask"),
                                     (hp_depth, torch.float32, 2, "hp_depth")):
            if t is None:
                planes.append(None)
                continue
            t, squeeze = _plane(t, dtype, ndim, self.npix, what)
            if t.shape[0] != batch:
                raise ValueError(f"{what} holds {t.shape[0]} samples, rotations {batch}")
            planes.append(t)
            squeezes.add(squeeze)
        if len(squeezes) != 1:
            raise ValueError("either every map has a batch dimension or none has")
        if batch > 65535:
            raise ValueError(f"batch must be in [1, 65535], got {batch}")
        channels = 0 if planes[0] is None else planes[0].shape[1]
        if planes[0] is not None and not 1 <= channels <= MAX_CHANNELS:
            raise ValueError(f"hp_img must have 1 .. {MAX_CHANNELS} channels, got {channels}")
        for t, what in zip(planes, ("hp_img", "hp_mask", "hp_depth")):
            if t is not None and not t.is_cuda:
                raise RuntimeError(f"{what} must be a GPU tensor: the rotation runs in the HIP kernel only (no CPU path)")
            if t is not None and t.device != _resolved(self.device):
                raise RuntimeError(f"{what} is on {t.device}, the rotator on {self.device}")
        img, mask, depth = planes = [None if t is None else t.contiguous() for t in planes]
        m = self.matrices(rotations)
        outs = [None if t is None else torch.empty_like(t) for t in planes]
        check(lib.hs_hp_rotate(self.nside, self.npix, ptr(m), batch, ptr(img), channels, ptr(outs[0]), ptr(mask), ptr(outs[1]),
                               self.s2_bkgd_class, ptr(depth), ptr(outs[2]), self.depth_fill, stream_ptr(self.device)), "hs_hp_rotate")
        squeeze = squeezes.pop()
        res = tuple(o[0] if squeeze else o for o in outs if o is not None)
        return res[0] if len(res) == 1 else res

    __call__ = rot


def _resolved(device):
    return torch.device("cuda", torch.cuda.current_device()) if device.type == "cuda" and device.index is None else device
