"""Argument handling shared by the sphere data path (projection, depth_data, hp_rotate, erp, surround, hp_ensemble) and the evaluation
path (evaluation, depth_evaluation, flat_evaluation): plain functions, one copy of each.  Everything here refuses by shape,
dtype and value first and touches the device last, so a malformed call fails the same way with and without a GPU.
"""
import numpy as np
import torch

from ._lib import HS_F64, dtype_code

MAX_NSIDE = 8192  # 12 nside^2 nested indices as int32
MAX_CHANNELS = 16
MAX_BATCH = 65535  # the sample is the grid's y index


def _resolved(device):
    """torch.device(device), with the current device's index where "cuda" names none"""
    d = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d


def _rotation_batch(rotations, device=None):
    """rotations [B, 3, 3] (device tensor or host array) as a float64 tensor, on `device` if given; the shape is checked before
    anything touches the device."""
    shape = tuple(np.shape(rotations))
    if len(shape) != 3 or shape[1:] != (3, 3) or shape[0] < 1:
        raise ValueError(f"rotations must be [batch, 3, 3] with batch >= 1, got {shape}")
    if not torch.is_tensor(rotations):
        rotations = torch.from_numpy(np.ascontiguousarray(rotations, dtype=np.float64))
    return rotations if device is None else rotations.to(device=device, dtype=torch.float64)


def _matmul3(a, b):
    """a b for [..., 3, 3] operands that broadcast: elementwise products summed over the inner index, the same rounding on every
    device (a library matmul may fuse or reorder)."""
    return (a[..., :, :, None] * b[..., None, :, :]).sum(-2)


def _dtype_name(dtype):
    """'uint8', 'float32', ... of a torch or numpy dtype"""
    return str(dtype).replace("torch.", "")


def _batched(t, ndim, what, dtype=None):
    """`t` as a tensor with its batch dimension, plus whether that was added: dtype (where one is required) and rank, checked
    without touching the device."""
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{what} must be {_dtype_name(dtype)}, got {t.dtype}")
    lead = ndim - t.dim()
    if lead not in (0, 1):
        raise ValueError(f"{what}: expected {ndim - 1} or {ndim} dimensions, got {t.dim()}")
    return (t[None] if lead else t), bool(lead)


def _check_nside(nside, supersample=0):
    nside = int(nside)
    if nside < 1 or nside & (nside - 1) or nside << supersample > MAX_NSIDE:
        raise ValueError(f"nside must be a power of two with nside << supersample <= {MAX_NSIDE}, got {nside} << {supersample}"
                         if supersample else f"nside must be a power of two in [1, {MAX_NSIDE}], got {nside}")
    return nside


def _check_base_pix(base_pix):
    if not 1 <= int(base_pix) <= 12:
        raise ValueError(f"base_pix must be in [1, 12], got {base_pix}")
    return int(base_pix)


def _check_batch(batch):
    if not 1 <= batch <= MAX_BATCH:
        raise ValueError(f"batch must be in [1, {MAX_BATCH}], got {batch}")


def _label_class(s2_bkgd_class):
    """s2_bkgd_class as a uint8 label"""
    if not 0 <= int(s2_bkgd_class) <= 255:
        raise ValueError(f"s2_bkgd_class must be in [0, 255] (uint8 labels), got {s2_bkgd_class}")
    return int(s2_bkgd_class)


def _fills(s2_bkgd_class, depth_fill):
    """(s2_bkgd_class as a uint8 label, depth_fill with its default float(s2_bkgd_class): what HPDepthProjector writes outside the
    image)"""
    return _label_class(s2_bkgd_class), float(s2_bkgd_class) if depth_fill is None else float(depth_fill)


# ------------------------------------------------------------------ the tensors of the evaluation path
def _kind_of(t, allow_f64=False):
    """HS_F32 / HS_BF16 (HS_F64 where the entry point takes it) of a tensor's dtype; TypeError for any other"""
    return HS_F64 if allow_f64 and t.dtype == torch.float64 else dtype_code(t.dtype)


def _device_tensor(t, what, device, dtypes=None, error=TypeError):
    """Refuse what the evaluation kernels cannot read in place: anything but a GPU tensor on `device` (raised as `error`, the type
    callers of each public method catch), a dtype outside `dtypes` (TypeError), a negative stride (ValueError)."""
    if not torch.is_tensor(t) or t.device != device or not t.is_cuda:
        raise error(f"{what} must be a tensor on {device} (the evaluation kernels have no CPU path)")
    if dtypes is not None and t.dtype not in dtypes:
        raise TypeError(f"{what} must be {' / '.join(_dtype_name(d) for d in dtypes)}, got {t.dtype}")
    if t.dim() and min(t.stride()) < 0:
        raise ValueError(f"{what}: negative strides are not supported")


# ------------------------------------------------------------------ the planes of HPRotator.rot and ERPProjector.proj
def _any_given(planes, names):
    if all(t is None for t in planes):
        raise ValueError(f"give at least one of {', '.join(names)}")


def _same_batch(planes, names, batch):
    for t, what in zip(planes, names):
        if t is not None and t.shape[0] != batch:
            raise ValueError(f"{what} holds {t.shape[0]} samples, expected {batch}")


def _gather_planes(given, batch=None):
    """given = ((tensor or None, ndim, required dtype or None, name), ...) -> (planes with their batch dimension, None where not
    given; whether that dimension was added; the batch).  The planes agree on having a batch dimension and on the batch count
    (`batch` where the caller already has one, the rotations').  Nothing touches the device."""
    names = [what for _, _, _, what in given]
    _any_given([t for t, _, _, _ in given], names)
    planes, squeezes = [], set()
    for t, ndim, dtype, what in given:
        if t is not None:
            t, squeeze = _batched(t, ndim, what, dtype)
            squeezes.add(squeeze)
        planes.append(t)
    if len(squeezes) != 1:
        raise ValueError(f"either every one of {', '.join(names)} has a batch dimension or none has")
    batch = next(t.shape[0] for t in planes if t is not None) if batch is None else batch
    _same_batch(planes, names, batch)
    return planes, squeezes.pop(), batch


def _on_device(planes, names, device, owner, host_path="no CPU path"):
    """the planes, contiguous, after the device refusals: GPU tensors on `device` (that of `owner`, "the rotator")"""
    for t, what in zip(planes, names):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{what} must be a GPU tensor: {owner} runs in the HIP kernel only ({host_path})")
        if t is not None and t.device != _resolved(device):
            raise RuntimeError(f"{what} is on {t.device}, {owner} on {device}")
    return [None if t is None else t.contiguous() for t in planes]


def _device_planes(planes, names, device, owner, npix, src_dims, host_path="no CPU path"):
    """(the planes of _on_device; an output [..., npix] for each, its last `src_dims` dimensions replaced)"""
    planes = _on_device(planes, names, device, owner, host_path)
    return planes, [None if t is None else torch.empty(t.shape[:-src_dims] + (npix,), dtype=t.dtype, device=t.device) for t in planes]


def _results(outs, squeeze):
    """the outputs of the planes given, without the batch dimension that was added; a single one bare"""
    res = tuple(o[0] if squeeze else o for o in outs if o is not None)
    return res[0] if len(res) == 1 else res
