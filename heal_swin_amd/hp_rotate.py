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
from ._sphere_args import (MAX_CHANNELS, MAX_NSIDE, _check_base_pix, _check_batch, _check_nside, _device_planes, _fills,  # noqa: F401
                           _gather_planes, _matmul3, _results, _rotation_batch)
from .projection import _pole_rotation


def _check_range(nside, first_pix, count, batch):
    nside, first_pix = _check_nside(nside), int(first_pix)
    npix = 12 * nside * nside
    count = npix - first_pix if count is None else int(count)
    if first_pix < 0 or count < 0 or first_pix + count > npix:
        raise ValueError(f"pixels [{first_pix}, {first_pix + count}) outside [0, {npix}) for nside {nside}")
    _check_batch(batch)
    return nside, first_pix, count


def rotated_interp(nside, rotations, first_pix=0, count=None, device="cuda"):
    """(pix int32 [B, 4, count], wgt float64 [B, 4, count], nearest int32 [B, count]) on the device: HEALPix's get_interpol
    (healpy.get_interp_weights, nest=True) at the directions M_b g_p of the nested pixels first_pix .. first_pix + count - 1
    (count=None: up to 12 nside^2), and the pixel of largest weight (evaluation.hp_nearest_pix_idcs).  rotations [B, 3, 3], a
    device tensor or a host array; any real matrix is accepted, a non-finite one gives -1 / 0 / -1 for its sample.  One launch,
    nothing synchronises with the host."""
    batch = _rotation_batch(rotations).shape[0]
    nside, first_pix, count = _check_range(nside, first_pix, count, batch)
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
    nside, first_pix, count = _check_range(nside, first_pix, count, batch)
    pix = np.empty((batch, 4, count), dtype=np.int32)
    wgt = np.empty((batch, 4, count), dtype=np.float64)
    nearest = np.empty((batch, count), dtype=np.int32)
    check(lib.hs_hp_rotated_interp_host(nside, first_pix, count, np_ptr(m), batch, np_ptr(pix), np_ptr(wgt), np_ptr(nearest)),
          "hs_hp_rotated_interp_host")
    return pix, wgt, nearest


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
        self.nside, self.base_pix = _check_nside(nside), _check_base_pix(base_pix)
        self.s2_bkgd_class, self.depth_fill = _fills(s2_bkgd_class, depth_fill)
        if rotate_pole and cal_info is None:
            raise ValueError("rotate_pole=True needs the cal_info the dataset was projected with")
        self.device = torch.device(device)  # "cpu" serves `matrices` alone: `rot` takes GPU tensors only
        self._pole = torch.from_numpy(_pole_rotation(cal_info)).to(self.device) if rotate_pole else None

    @property
    def npix(self):
        return self.base_pix * self.nside * self.nside

    def matrices(self, rotations):
        """M_b = R^T A_b R, float64 [B, 3, 3] on the device (A itself without rotate_pole)."""
        m = _rotation_batch(rotations, self.device)
        if self._pole is not None:
            m = _matmul3(self._pole.t(), _matmul3(m, self._pole))  # R^T (A_b R)
        return m.contiguous()

    def rot(self, hp_img=None, hp_mask=None, hp_depth=None, rotations=None):
        if rotations is None:
            raise ValueError("rotations=A [batch, 3, 3] is required (projection.random_rotations)")
        names = ("hp_img", "hp_mask", "hp_depth")
        planes, squeeze, batch = _gather_planes(((hp_img, 3, torch.uint8, names[0]), (hp_mask, 2, torch.uint8, names[1]),
                                                 (hp_depth, 2, torch.float32, names[2])), _rotation_batch(rotations).shape[0])
        for t, what in zip(planes, names):
            if t is not None and t.shape[-1] != self.npix:
                raise ValueError(f"{what} covers {t.shape[-1]} HEALPix pixels, expected {self.npix}")
        _check_batch(batch)
        channels = 0 if planes[0] is None else planes[0].shape[1]
        if planes[0] is not None and not 1 <= channels <= MAX_CHANNELS:
            raise ValueError(f"hp_img must have 1 .. {MAX_CHANNELS} channels, got {channels}")
        (img, mask, depth), outs = _device_planes(planes, names, self.device, "the rotator", self.npix, 1)
        m = self.matrices(rotations)
        check(lib.hs_hp_rotate(self.nside, self.npix, ptr(m), batch, ptr(img), channels, ptr(outs[0]), ptr(mask), ptr(outs[1]),
                               self.s2_bkgd_class, ptr(depth), ptr(outs[2]), self.depth_fill, stream_ptr(self.device)), "hs_hp_rotate")
        return _results(outs, squeeze)

    __call__ = rot

