"""Rotation ensembles at evaluation: the test-time counterpart of the rotation augmentation (projection.random_rotations,
hp_rotate.HPRotator).  A sample is predicted under several rotations, every prediction is brought back to the unrotated grid,
the members are averaged there and the average is scored (no counterpart in the reference, which has no augmentation).

  HPRotationEnsemble.add(pred, rotations=A)     one member into the accumulators: `hs_hp_ensemble_add_seg` / `_add_depth`
  HPRotationEnsemble.finish()                   class ids uint8 [B, Npix] (and mean probabilities), or the depth mean fp32 [B, Npix]:
                                                `hs_hp_ensemble_finish_seg` / `_finish_depth`
  HPRotationEnsemble.run(model, hp_img, [A..])  rotate the frame, predict, add, for every A; then finish
  add_seg_host / add_depth_host                 the kernels' per-pixel functions in a host loop (numpy): their oracle

Convention.  `HPRotator.rot(hp_img, rotations=A)` shows at pixel q the scene at direction M g_q, M = `HPRotator.matrices(A)`.  A
prediction made on that frame is read, for the unrotated pixel p, at direction M^T g_p: the inverse of an orthogonal matrix is
its transpose, and M^T is what the kernel is given.  The four pixels around that direction that are covered by the base pixels,
valid (`valid_plane(A)`: the rotated input showed real scene there, not the fill outside the base pixels) and, for depth, finite,
contribute softmax(logits) (mode "prob") or the logits (mode "logit") or the depth with their interpolation weights; a pixel
whose weights sum to `min_weight` or less over all members gets `s2_bkgd_class` / NaN.
"""
import numpy as np
import torch

from ._lib import HS_BF16, HS_ENSEMBLE_LOGIT, HS_ENSEMBLE_PROB, HS_F32, HS_PRED_ROWS16, check, lib, np_ptr, ptr, stream_ptr
from ._sphere_args import _check_batch, _check_nside, _kind_of, _label_class, _resolved, _rotation_batch
from .evaluation import _pred_args
from .hp_rotate import HPRotator
from .projection import _pole_rotation

MAX_CLASSES = 16
MODES = {"prob": HS_ENSEMBLE_PROB, "logit": HS_ENSEMBLE_LOGIT}
ORTHOGONAL_TOL = 1e-9


def _kp(k):
    return -(-k // 4) * 4


def _host_mats(rot, batch):
    if rot is None:
        return None
    m = np.ascontiguousarray(_rotation_batch(rot).detach().cpu().numpy(), dtype=np.float64)
    if m.shape[0] != batch:
        raise ValueError(f"rot holds {m.shape[0]} matrices, the predictions {batch} samples")
    return m


def _host_pred(pred, ndim, npix):
    """(kind, element strides) of a host prediction: float32, or uint16 holding bfloat16 bits"""
    if pred.dtype not in (np.float32, np.uint16) or pred.ndim != ndim or pred.shape[-1] != npix:
        raise ValueError(f"pred must be float32 (or bfloat16 bits as uint16) with {ndim} dimensions and {npix} pixels, got {pred.dtype} "
                         f"{pred.shape}")
    return (HS_F32 if pred.dtype == np.float32 else HS_BF16), tuple(s // pred.itemsize for s in pred.strides)


def add_seg_host(nside, base_pix, pred, rot=None, valid=None, mode="prob", acc=None, wsum=None, accumulate=None, rows16=False):
    """`hs_hp_ensemble_add_seg_host`: pred a numpy array [B, K, Npix], float32 or uint16 (bfloat16 bits), any non-negative strides;
    rows16=True promises HS_PRED_ROWS16 rows.  rot = M^T [B, 3, 3] or None (the unrotated member), valid uint8 [B, Npix] or None.
    acc / wsum None: a first member (new arrays); else they are added to in place (stored into with accumulate=False).  Returns
    (acc float32 [B, Npix, KP], wsum float32 [B, Npix])."""
    nside = _check_nside(nside)
    npix = int(base_pix) * nside * nside
    kind, (sb, sk, sp) = _host_pred(pred, 3, npix)
    b, k, _ = pred.shape
    m = _host_mats(rot, b)
    if valid is not None:
        valid = np.ascontiguousarray(valid, dtype=np.uint8).reshape(b, npix)
    if acc is None:
        acc, wsum, accumulate = np.empty((b, npix, _kp(k)), dtype=np.float32), np.empty((b, npix), dtype=np.float32), False
    accumulate = True if accumulate is None else bool(accumulate)
    check(lib.hs_hp_ensemble_add_seg_host(nside, npix, np_ptr(m), b, np_ptr(pred), kind | (HS_PRED_ROWS16 if rows16 else 0), k, sb, sk, sp,
                                          np_ptr(valid), MODES[mode], int(accumulate), np_ptr(acc), np_ptr(wsum)),
          "hs_hp_ensemble_add_seg_host")
    return acc, wsum


def add_depth_host(nside, base_pix, pred, rot=None, valid=None, acc=None, wsum=None, accumulate=None):
    """`hs_hp_ensemble_add_depth_host`: pred numpy [B, Npix]; otherwise as add_seg_host.  Returns (acc, wsum) float32 [B, Npix]."""
    nside = _check_nside(nside)
    npix = int(base_pix) * nside * nside
    kind, (sb, sp) = _host_pred(pred, 2, npix)
    b = pred.shape[0]
    m = _host_mats(rot, b)
    if valid is not None:
        valid = np.ascontiguousarray(valid, dtype=np.uint8).reshape(b, npix)
    if acc is None:
        acc, wsum, accumulate = np.empty((b, npix), dtype=np.float32), np.empty((b, npix), dtype=np.float32), False
    accumulate = True if accumulate is None else bool(accumulate)
    check(lib.hs_hp_ensemble_add_depth_host(nside, npix, np_ptr(m), b, np_ptr(pred), kind, sb, sp, np_ptr(valid), int(accumulate),
                                            np_ptr(acc), np_ptr(wsum)), "hs_hp_ensemble_add_depth_host")
    return acc, wsum


class HPRotationEnsemble:
    """Average the predictions of one batch under several rotations on the unrotated HEALPix grid.

        ens = HPRotationEnsemble(nside, base_pix, cal_info=cal, rotate_pole=True, s2_bkgd_class=0)
        preds = ens.run(model, hp_img, [A1, A2, ...])                # uint8 [B, Npix] -> SegConfusion.update(preds, target)
    or, by hand,
        ens.add(model(hp_img))                                       # the unrotated member
        ens.add(model(rot(hp_img, rotations=A)), A, ens.valid_plane(A))
        preds, probs = ens.finish(return_probs=True); ens.reset()

    add(pred, rotations=A, valid=None, channel=None)
        pred fp32 / bf16 on the GPU, read in place through its strides (the model's padded head rows by 16-byte loads):
        [B, K, Npix] logits (K <= 16) add to the segmentation state; [B, Npix], or [B, C, Npix] with `channel=c`, add to the depth
        state.  One ensemble holds one of the two until reset().  A [B, 3, 3] is what random_rotations draws; a host array is
        refused unless |M M^T - I| <= 1e-9 for M = HPRotator.matrices(A) (the inverse is taken as the transpose); a device tensor is
        not looked at (no synchronisation).  rotations=None adds an unrotated member: weight 1 on the pixel itself.  valid uint8
        [B, Npix] in the rotated frame (valid_plane(A)).
    finish(return_probs=False)
        segmentation: preds uint8 [B, Npix], the first maximum of the accumulated values where the summed weight exceeds
        min_weight and s2_bkgd_class elsewhere; with return_probs also their weighted mean fp32 [B, K, Npix] (0 elsewhere).  Depth:
        the weighted mean fp32 [B, Npix], NaN elsewhere (DepthMetrics' background).  The state stays until reset().
    With `rotations` on the device, add and finish read nothing on the host and allocate only the outputs (the accumulators once
    per shape, the [B, 3, 3] temporaries of the matrices): capturable after one eager round."""

    def __init__(self, nside, base_pix=8, cal_info=None, rotate_pole=False, s2_bkgd_class=0, mode="prob", min_weight=1e-3, device="cuda"):
        self._rotator = HPRotator(nside, base_pix, cal_info=cal_info, rotate_pole=rotate_pole, s2_bkgd_class=0, device=device)
        self.nside, self.base_pix, self.device = self._rotator.nside, self._rotator.base_pix, self._rotator.device
        self.s2_bkgd_class = _label_class(s2_bkgd_class)
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
        self.mode, self.min_weight = mode, float(min_weight)
        if not 0.0 <= self.min_weight < float("inf"):
            raise ValueError(f"min_weight must be finite and >= 0, got {min_weight}")
        self._pole = _pole_rotation(cal_info) if rotate_pole else None  # host copy: the orthogonality check of host matrices
        self._acc = self._wsum = self._ones = None
        self.reset()

    @property
    def npix(self):
        return self.base_pix * self.nside * self.nside

    def reset(self):
        """Forget the members; the accumulators are kept for the next batch of the same shape (its first add overwrites them)."""
        self._task, self._members, self._shape = None, 0, None

    def _check_rotations(self, rotations, batch):
        shape = _rotation_batch(rotations).shape
        if shape[0] != batch:
            raise ValueError(f"rotations hold {shape[0]} matrices, the predictions {batch} samples")
        if torch.is_tensor(rotations) and rotations.is_cuda:
            return
        a = np.asarray(rotations.detach().numpy() if torch.is_tensor(rotations) else rotations, dtype=np.float64)
        m = a if self._pole is None else self._pole.T @ a @ self._pole
        err = np.abs(m @ m.transpose(0, 2, 1) - np.eye(3)).max()
        if not err <= ORTHOGONAL_TOL:  # a NaN fails
            raise ValueError(f"rotations must be orthogonal (the inverse is taken as the transpose): |M M^T - I| = {err:.3e} > {ORTHOGONAL_TOL}")

    def _check_device(self, t, what):
        if not t.is_cuda:
            raise RuntimeError(f"{what} must be a GPU tensor: the ensemble runs in the HIP kernels only (no CPU path)")
        if t.device != _resolved(self.device):
            raise RuntimeError(f"{what} is on {t.device}, the ensemble on {self.device}")

    def add(self, pred, rotations=None, valid=None, channel=None):
        if not torch.is_tensor(pred) or pred.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("pred must be a float32 / bfloat16 tensor: logits [B, K, Npix] or depth [B, Npix] / [B, C, Npix] with channel=")
        if pred.dim() not in (2, 3) or pred.shape[-1] != self.npix:
            raise ValueError(f"pred must be [B, K, {self.npix}] or [B, {self.npix}], got {tuple(pred.shape)}")
        if pred.dim() == 2 and channel is not None:
            raise ValueError("channel= needs predictions with a channel dimension [B, C, Npix]")
        task = "seg" if pred.dim() == 3 and channel is None else "depth"
        if task == "depth" and pred.dim() == 3:
            if not 0 <= int(channel) < pred.shape[1]:
                raise ValueError(f"channel {channel} outside the {pred.shape[1]} channels of pred")
            pred = pred[:, int(channel)]
        batch = pred.shape[0]
        _check_batch(batch)
        k = pred.shape[1] if task == "seg" else 0
        if task == "seg" and not 1 <= k <= MAX_CLASSES:
            raise ValueError(f"the ensemble kernels support 1 .. {MAX_CLASSES} classes, got {k}")
        if min(pred.stride()) < 0:
            raise ValueError("predictions with negative strides are not supported")
        if self._task is not None and self._task != task:
            raise ValueError(f"this ensemble holds {self._task} members: a call may not mix the two states (reset() first)")
        if self._shape is not None and self._shape != (batch, k):
            raise ValueError(f"this ensemble holds members of batch {self._shape[0]}" + (f", {self._shape[1]} classes" if k else "")
                             + f"; got batch {batch}" + (f", {k} classes" if k else ""))
        if rotations is not None:
            self._check_rotations(rotations, batch)
        if valid is not None:
            if not torch.is_tensor(valid) or valid.dtype != torch.uint8 or tuple(valid.shape) != (batch, self.npix):
                raise ValueError(f"valid must be a uint8 tensor [{batch}, {self.npix}] (valid_plane(A))")
        self._check_device(pred, "pred")
        if valid is not None:
            self._check_device(valid, "valid")
            valid = valid.contiguous()
        dev = pred.device
        mt = None if rotations is None else self._rotator.matrices(rotations).transpose(1, 2).contiguous()
        kp = _kp(k) if task == "seg" else 1
        want = (batch, self.npix, kp) if task == "seg" else (batch, self.npix)
        if self._acc is None or tuple(self._acc.shape) != want or self._acc.device != dev:
            self._acc = torch.empty(want, dtype=torch.float32, device=dev)
            self._wsum = torch.empty((batch, self.npix), dtype=torch.float32, device=dev)
        accumulate = int(self._members > 0)
        if task == "seg":
            kind, k, _, (sb, sk, sp), pred = _pred_args(pred, self.npix, dev)
            check(lib.hs_hp_ensemble_add_seg(self.nside, self.npix, ptr(mt), batch, ptr(pred), kind, k, sb, sk, sp, ptr(valid),
                                             MODES[self.mode], accumulate, ptr(self._acc), ptr(self._wsum), stream_ptr(dev)),
                  "hs_hp_ensemble_add_seg")
        else:
            check(lib.hs_hp_ensemble_add_depth(self.nside, self.npix, ptr(mt), batch, ptr(pred),
                                               _kind_of(pred), pred.stride(0), pred.stride(1), ptr(valid), accumulate, ptr(self._acc), ptr(self._wsum), stream_ptr(dev)),
                  "hs_hp_ensemble_add_depth")
        self._task, self._shape, self._members = task, (batch, k if task == "seg" else 0), self._members + 1

    def finish(self, return_probs=False):
        if not self._members:
            raise RuntimeError("finish() needs at least one add() since the last reset()")
        batch, k = self._shape
        dev = self._acc.device
        if self._task == "depth":
            if return_probs:
                raise ValueError("return_probs applies to the segmentation state")
            out = torch.empty((batch, self.npix), dtype=torch.float32, device=dev)
            check(lib.hs_hp_ensemble_finish_depth(self.npix, batch, ptr(self._acc), ptr(self._wsum), self.min_weight, ptr(out),
                                                  stream_ptr(dev)), "hs_hp_ensemble_finish_depth")
            return out
        preds = torch.empty((batch, self.npix), dtype=torch.uint8, device=dev)
        probs = torch.empty((batch, k, self.npix), dtype=torch.float32, device=dev) if return_probs else None
        sb, sk, sp = probs.stride() if return_probs else (0, 0, 0)
        check(lib.hs_hp_ensemble_finish_seg(self.npix, batch, k, ptr(self._acc), ptr(self._wsum), self.min_weight, self.s2_bkgd_class,
                                            ptr(preds), ptr(probs), sb, sk, sp, stream_ptr(dev)), "hs_hp_ensemble_finish_seg")
        return (preds, probs) if return_probs else preds

    def valid_plane(self, rotations):
        """uint8 [B, Npix] in the rotated frame: 1 where `HPRotator.rot(..., rotations=A)` showed a pixel of the map, 0 where it
        filled (the nearest source pixel lies outside the base pixels, or the matrix is not finite): an all-ones label map through
        the rotator."""
        batch = _rotation_batch(rotations).shape[0]
        if self._ones is None or self._ones.shape[0] != batch:
            self._ones = torch.ones((batch, self.npix), dtype=torch.uint8, device=self.device)
        return self._rotator.rot(hp_mask=self._ones, rotations=rotations)

    def run(self, model, hp_img, rotations_list, include_identity=True, channel=None, return_probs=False):
        """The ensemble of `model` on the frames hp_img uint8 [B, C, Npix] over the members of rotations_list (each A [B, 3, 3]),
        plus the unrotated one with include_identity: under no_grad, for every A the frame is rotated (HPRotator), predicted by
        model(frame) and added with valid_plane(A); then finish() and reset().  channel=c reads a depth head's channel c."""
        with torch.no_grad():
            self.reset()
            if include_identity:
                self.add(model(hp_img), channel=channel)
            for a in rotations_list:
                self.add(model(self._rotator.rot(hp_img, rotations=a)), a, self.valid_plane(a), channel=channel)
            out = self.finish(return_probs=return_probs)
            self.reset()
        return out
