"""Evaluation of HEALPix segmentation outputs on the GPU: metrics and back-projection onto the fisheye image plane, the
pipeline's other end (`projection.HPProjector` is its input side).  Mirrors the reference's names and results:

  get_uv_from_hw(height, width, output_resolution)   data/segmentation/project_on_s2.py:266-287  image-plane pixel grid
  project_img_points_to_s2(u, v, cal_info, rotate_pole)                                  :188-248  fisheye model inverted
  get_interp_weights(nside, theta, phi)               healpy.pixelfunc.get_interp_weights(..., nest=True)
                                                      (`hs_hp_interp_weights_nest`, host C++; the reference calls healpy)
  hp_nearest_pix_idcs(nside, theta, phi)              :83-105  the pixel of largest interpolation weight
  HPBackProjector                                     the tables of one calibration, resident on the GPU:
      .masks(pred)                                    project_hp_mask_back (:319-341)   `hs_backproject_labels`
      .images(hp_img)                                 project_hp_img_back (:302-316)    `hs_backproject_image`
      .depth(pred)                                    data/depth_estimation/project_depth_on_s2.py:370-386
                                                      (project_depth_hp_mask_back, NaN fill)  `hs_backproject_depth`
      .valid                                          evaluation/custom_metrics.py:48-53 (HPMaskedIoU.get_mask)
      .from_angles(theta, phi, nside, ...)            the same tables for any image plane given by its pixels' directions
                                                      (no counterpart; erp.ERPBackProjector's panorama)
  SegConfusion                                        the confusion matrix behind torchmetrics 0.3.2's IoU / Accuracy
                                                      (models_lightning/segmentation/model_lightning_swin_hp.py:47-55) and
                                                      the back-projected metrics (evaluation/hp_pred_writers.py:110-222,
                                                      :367-448), `hs_seg_confusion`

Predictions are the model's logits as it returns them ([B, K, Npix], fp32 or bf16, any strides: the padded native rows are
read in place) or uint8 class ids [B, Npix].  The per-batch work runs in the HIP kernels only; the tables are host work done
once per calibration (float64 numpy and C++, no scipy or healpy).

Differences from the reference, by construction:
  * theta of an image point: the reference solves rho(theta) = sum_i k_i theta^i at 100 radii with scipy's newton_krylov
    (default tolerance f_tol ~ 6e-6 on rho) and interpolates linearly between them; here the same 100 radii are solved with
    a float64 Newton iteration to convergence and interpolated with np.interp.  On the committed calibrations the two
    differ by at most ~3e-7 rad (tests/test_evaluation.py pins 1e-6); phi is computed identically.
  * get_interp_weights reduces phi to [0, 2 pi) with HEALPix's fmodulo before bracketing (healpy normalises its pointing
    before HEALPix's get_interpol; not checked against healpy itself, which is absent here).  rot_grid returns phi in
    (-pi, pi], so the rotated grids depend on that reduction.
"""
import numpy as np
import torch

from ._lib import HS_PRED_LABELS, HS_PRED_ROWS16, check, lib, np_ptr, ptr, stream_ptr
from ._sphere_args import _device_tensor, _kind_of, _label_class, _resolved as _device  # noqa: F401  (imported from here)
from .projection import rot_grid

MAX_CLASSES = 64


# ------------------------------------------------------------------ host geometry (once per calibration)
def get_uv_from_hw(height, width, output_resolution):
    """Image-plane pixel coordinates (u along the width, v along the height) as an 'xy' meshgrid.  output_resolution: a
    float scales both sides; an int sets the shorter side (and, as in the reference, the longer side becomes
    int(long * res) // res, i.e. keeps its full size); a tuple (height, width) sets both."""
    if isinstance(output_resolution, float):
        height_res, width_res = int(height * output_resolution), int(width * output_resolution)
    elif isinstance(output_resolution, int):
        if width <= height:
            width_res = output_resolution
            height_res = int(height * output_resolution) // width_res
        else:
            height_res = output_resolution
            width_res = int(width * output_resolution) // height_res
    elif isinstance(output_resolution, tuple):
        height_res, width_res = output_resolution[0], output_resolution[1]
    else:
        raise TypeError(f"output_resolution must be a float, an int or a (height, width) tuple, got {output_resolution!r}")
    u_range = np.linspace(0, width - 1, width_res)
    v_range = np.linspace(0, height - 1, height_res)
    return np.meshgrid(u_range, v_range, indexing="xy")


def _theta_of_rho(ks, rho):
    """Solve sum_i ks[i-1] theta^i = rho for every rho (float64 Newton from pi/2, the reference's starting point)."""
    theta = np.full(rho.shape, np.pi / 2)
    for _ in range(100):
        f, df = np.zeros_like(theta), np.zeros_like(theta)
        for k in ks[::-1]:  # Horner on theta * (k1 + k2 theta + ...)
            df = df * theta + f
            f = f * theta + k
        df = df * theta + f
        f = f * theta - rho
        step = f / df
        theta = theta - step
        if np.all(np.abs(step) <= 1e-15 * np.maximum(1.0, np.abs(theta))):
            break
    res = sum(k * theta ** (i + 1) for i, k in enumerate(ks)) - rho
    if not np.all(np.abs(res) <= 1e-9 * np.maximum(1.0, np.abs(rho))):
        raise RuntimeError(f"inverting the fisheye polynomial did not converge (residual {np.abs(res).max():.3e})")
    return theta


def project_img_points_to_s2(u, v, cal_info, rotate_pole=False, used_size=None):
    """(theta, phi) on S^2 of image points (u, v) of a calibrated fisheye camera: the inverse of
    projection.project_s2_points_to_img.  phi in [0, 2 pi) without rotation, in (-pi, pi] after rot_grid(inv=True).
    used_size = (h, w): (u, v) are coordinates of an h x w image of the camera's frame and are first rescaled to the
    calibration's size, u * W / w and v * H / h (the depth variant, data/depth_estimation/project_depth_on_s2.py:195-196)."""
    intr = cal_info["intrinsic"]
    width, height = int(intr["width"]), int(intr["height"])
    ks = [float(intr["k" + str(order)]) for order in range(1, intr["poly_order"] + 1)]
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if used_size is not None:
        u = u * width / int(used_size[1])
        v = v * height / int(used_size[0])
    x = u - intr["cx_offset"] - width / 2 + 0.5
    y = (v - intr["cy_offset"] - height / 2 + 0.5) / intr["aspect_ratio"]
    rho = np.sqrt(x**2 + y**2)
    phi = np.arctan2(y, x)
    phi = np.where(phi < 0, 2 * np.pi + phi, phi)
    rho_samples = np.linspace(0, rho.max(), 100)
    theta = np.interp(rho, rho_samples, _theta_of_rho(ks, rho_samples))
    if rotate_pole:
        theta, phi = rot_grid(theta, phi, cal_info, inv=True)
    return theta, phi


def get_interp_weights(nside, theta, phi):
    """healpy.pixelfunc.get_interp_weights(nside, theta, phi, nest=True): (pix int64 [4, *shape], wgt float64 [4, *shape])."""
    th = np.ascontiguousarray(theta, dtype=np.float64)
    ph = np.ascontiguousarray(phi, dtype=np.float64)
    if th.shape != ph.shape:
        raise ValueError(f"theta {th.shape} and phi {ph.shape} differ in shape")
    pix = np.empty((4,) + th.shape, dtype=np.int64)
    wgt = np.empty((4,) + th.shape, dtype=np.float64)
    check(lib.hs_hp_interp_weights_nest(int(nside), np_ptr(th), np_ptr(ph), th.size, np_ptr(pix), np_ptr(wgt)),
          "hs_hp_interp_weights_nest")
    return pix, wgt


def hp_nearest_pix_idcs(nside, theta, phi):
    """Nested index of the pixel with the largest interpolation weight (first maximum on ties, as np.argmax), plus the
    interpolation table it came from: (nearest [*shape], pix [4, *shape], wgt [4, *shape])."""
    pix, wgt = get_interp_weights(nside, theta, phi)
    nearest = np.take_along_axis(pix, np.argmax(wgt, axis=0)[None], axis=0)[0]
    return nearest, pix, wgt


# ------------------------------------------------------------------ device side
def _pred_args(pred, npix, device):
    """(pred_kind, n_classes, batch, (stride_b, stride_k, stride_p), tensor) of logits [B, K, Npix] or labels [B, Npix]."""
    _device_tensor(pred, "predictions", device, (torch.float32, torch.bfloat16, torch.uint8), RuntimeError)
    if pred.dtype == torch.uint8:
        if pred.dim() == 1:
            pred = pred[None]
        if pred.dim() != 2:
            raise ValueError(f"label predictions must be [B, Npix] uint8, got shape {tuple(pred.shape)}")
        kind, k, sb, sk, sp = HS_PRED_LABELS, None, pred.stride(0), 0, pred.stride(1)
    else:
        if pred.dim() == 2:
            pred = pred[None]
        if pred.dim() != 3:
            raise ValueError(f"logits must be [B, K, Npix], got shape {tuple(pred.shape)}")
        kind, k, sb, sk, sp = _kind_of(pred), pred.shape[1], *pred.stride()
        if not 1 <= k <= MAX_CLASSES:
            raise ValueError(f"the evaluation kernels support 1 .. {MAX_CLASSES} classes, got {k}")
    if pred.shape[-1] != npix:
        raise ValueError(f"predictions cover {pred.shape[-1]} HEALPix pixels, expected {npix}")
    if kind != HS_PRED_LABELS and _rows16(pred, k):
        kind |= HS_PRED_ROWS16
    return kind, k, pred.shape[0], (sb, sk, sp), pred


def _backproject_labels(pred, nearest, n_out, npix, background, out_shape, device):
    """`hs_backproject_labels`: class ids uint8 [B, *out_shape] of logits [B, K, npix] (argmax as torch.max(logits, 1)) or uint8
    labels [B, npix] read through nearest [n_out]; `background` where the table points outside [0, npix)."""
    kind, k, b, (sb, sk, sp), pred = _pred_args(pred, npix, device)
    out = torch.empty((b,) + tuple(out_shape), dtype=torch.uint8, device=device)
    check(lib.hs_backproject_labels(ptr(pred), kind, b, npix, k or 1, sb, sk, sp, ptr(nearest), n_out, background, ptr(out),
                                    stream_ptr(device)), "hs_backproject_labels")
    return out


def _rows16(logits, k):
    """True when every pixel's logits row [B, K, Npix][b, :, p] is contiguous, 16-byte aligned and padded so that reading it
    up to the next 16 bytes stays inside the row and inside the tensor's storage (the model's padded output rows)."""
    per = 16 // logits.element_size()
    width = -(-k // per) * per
    sb, sk, sp = logits.stride()
    if sk != 1 or sb % per or sp % per or sp < width or logits.data_ptr() % 16:
        return False
    b, _, n = logits.shape
    end = logits.storage_offset() + (b - 1) * sb + (n - 1) * sp + width
    return end * logits.element_size() <= logits.untyped_storage().nbytes()


class HPBackProjector:
    """The back-projection tables of one calibration, built once on the host and resident on the GPU.

    For every pixel of the image plane (`get_uv_from_hw(height, width, output_resolution)`, shape [H', W']):
      nearest  int32 [H', W']     nested index of the HEALPix pixel of largest interpolation weight
      idx, wgt int32 / float64 [4, H', W']   healpy's interpolation pixels and weights
      valid    bool [H', W']      nearest < base_pix nside^2: the pixel is covered by the model's base pixels (exactly
                                  HPMaskedIoU.get_mask, custom_metrics.py:48-53)
    """

    def __init__(self, cal_info, nside, base_pix=8, output_resolution=1.0, rotate_pole=False, s2_bkgd_class=0, device="cuda"):
        intr = cal_info["intrinsic"]
        u, v = get_uv_from_hw(intr["height"], intr["width"], output_resolution)
        theta, phi = project_img_points_to_s2(u, v, cal_info, rotate_pole)
        self._set_tables(theta, phi, nside, base_pix, s2_bkgd_class, device)

    @classmethod
    def from_angles(cls, theta, phi, nside, base_pix=8, s2_bkgd_class=0, device="cuda"):
        """The projector of any image plane given by the directions (theta, phi) [H', W'] of its pixels (erp.ERPBackProjector's
        panorama): the same tables from the same `hp_nearest_pix_idcs`, every method unchanged."""
        self = cls.__new__(cls)
        self._set_tables(theta, phi, nside, base_pix, s2_bkgd_class, device)
        return self

    def _set_tables(self, theta, phi, nside, base_pix, s2_bkgd_class, device):
        self.nside, self.base_pix, self.s2_bkgd_class = int(nside), int(base_pix), _label_class(s2_bkgd_class)
        theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
        if theta.ndim != 2 or theta.shape != phi.shape:
            raise ValueError(f"theta and phi must share one [H', W'] shape, got {theta.shape} and {phi.shape}")
        nearest, pix, wgt = hp_nearest_pix_idcs(self.nside, theta, phi)
        self.device = _device(device)
        self.shape = tuple(nearest.shape)
        self.nearest = torch.from_numpy(nearest.astype(np.int32)).to(self.device)
        self.idx = torch.from_numpy(pix.astype(np.int32)).to(self.device)
        self.wgt = torch.from_numpy(wgt).to(self.device)
        self.valid = self.nearest < self.npix

    @property
    def npix(self):
        """HEALPix pixels the model sees: base_pix * nside^2."""
        return self.base_pix * self.nside * self.nside

    @property
    def n_out(self):
        return self.shape[0] * self.shape[1]

    def masks(self, pred):
        """Back-projected class ids uint8 [B, H', W'] from logits [B, K, Npix] (argmax as torch.max(logits, 1)) or uint8
        labels [B, Npix]; pixels outside the model's base pixels get s2_bkgd_class."""
        return _backproject_labels(pred, self.nearest, self.n_out, self.npix, self.s2_bkgd_class, self.shape, self.device)

    def images(self, hp_img):
        """Bilinear back-projection of HEALPix images: uint8 [B, C, Npix] or [C, Npix] -> float64 [(B,) C, H', W'];
        pixels that interpolate from outside the model's base pixels read 255 there, as in the reference."""
        _device_tensor(hp_img, "hp_img", self.device, (torch.uint8,))
        if hp_img.dim() not in (2, 3) or hp_img.shape[-1] != self.npix:
            raise ValueError(f"hp_img must be [B, C, {self.npix}] or [C, {self.npix}], got {tuple(hp_img.shape)}")
        lead = hp_img.shape[:-1]
        src = hp_img.contiguous()
        out = torch.empty(lead + self.shape, dtype=torch.float64, device=self.device)
        check(lib.hs_backproject_image(ptr(src), int(np.prod(lead)), self.npix, ptr(self.idx), ptr(self.wgt), self.n_out, ptr(out),
                                       stream_ptr(self.device)), "hs_backproject_image")
        return out

    def depth(self, pred, channel=0):
        """Bilinear back-projection of HEALPix depth values: project_depth_hp_mask_back(..., s2_bkgd_class=nan)
        (data/depth_estimation/project_depth_on_s2.py:370-386).  pred: fp32 / bf16 [B, C, Npix] (channel `channel` is read
        in place, any strides) or [B, Npix] -> float64 [B, H', W'].  The map is completed with NaN outside the model's base
        pixels and NaN propagates from any of the four pixels, a weight-0 one included (0 * NaN in the reference's sum)."""
        _device_tensor(pred, "pred", self.device, (torch.float32, torch.bfloat16))
        if pred.dim() == 3:
            pred = pred[:, channel]
        if pred.dim() != 2 or pred.shape[-1] != self.npix:
            raise ValueError(f"pred must be [B, C, {self.npix}] or [B, {self.npix}], got {tuple(pred.shape)}")
        out = torch.empty((pred.shape[0],) + self.shape, dtype=torch.float64, device=self.device)
        check(lib.hs_backproject_depth(ptr(pred), _kind_of(pred), pred.shape[0], self.npix, pred.stride(0), pred.stride(1),
                                       ptr(self.idx), ptr(self.wgt), self.n_out, ptr(out), stream_ptr(self.device)),
              "hs_backproject_depth")
        return out


class SegConfusion:
    """Confusion matrix C [K, K] (int64, on the device; rows = target, columns = prediction, torchmetrics'
    bincount(target * K + pred)) with the metrics torchmetrics 0.3.2 derives from it.

    update(pred, target)                               HEALPix domain: target uint8 [B, Npix] (the training / validation
                                                       metric of model_lightning_swin_hp.py:47-55)
    update(pred, target, projector)                    image plane: the prediction back-projected through projector's
                                                       nearest table, target uint8 [B, H', W']; uncovered pixels count as
                                                       projector.s2_bkgd_class (the *_back_projected metrics)
    update(pred, target, projector, masked=True)       uncovered pixels skipped (back_projected_hp_masked_iou)
    update(proj.logits(pred), target, proj)            a FLAT prediction on the sphere or on its covered image pixels: proj a
                                                       flat_evaluation.FlatToHPProjector (target uint8 [B, Npix]) or
                                                       FlatCoverage (target [B, H, W], masked=True)
    update(pred, target, [p0, p1, ...], camera=cams)   a batch that mixes calibrations: cams[b] indexes the projector of
                                                       sample b; one launch per run of consecutive samples of one camera
                                                       (one per camera when the batch is grouped by camera)

    Targets >= K raise ValueError (torchmetrics raises on them too); the check reads a device counter, so it synchronises
    the stream: pass check=False to defer it to the next metric read.
    """

    def __init__(self, num_classes, device="cuda"):
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in [1, {MAX_CLASSES}], got {num_classes}")
        self.num_classes = int(num_classes)
        self.device = _device(device)
        self.confmat = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64, device=self.device)
        self._bad = torch.zeros(2, dtype=torch.int64, device=self.device)  # (targets >= K, label predictions >= K)

    def reset(self):
        self.confmat.zero_()
        self._bad.zero_()

    def _launch(self, pred, target, nearest, n_out, uncovered, npix):
        kind, k, b, (sb, sk, sp), pred = _pred_args(pred, npix, self.device)
        if k is not None and k != self.num_classes:
            raise ValueError(f"logits have {k} classes, the matrix {self.num_classes}")
        if target.numel() != b * (npix if nearest is None else n_out):
            raise ValueError(f"target {tuple(target.shape)} does not match {b} predictions of "
                             f"{npix if nearest is None else n_out} pixels")
        check(lib.hs_seg_confusion(ptr(pred), kind, b, npix, self.num_classes, sb, sk, sp, ptr(nearest), n_out, ptr(target),
                                   uncovered, ptr(self.confmat), ptr(self._bad), stream_ptr(self.device)), "hs_seg_confusion")

    def update(self, pred, target, projector=None, masked=False, camera=None, check=True):
        _device_tensor(target, "target (class ids)", self.device, (torch.uint8,))
        if torch.is_tensor(pred) and pred.dim() == (1 if pred.dtype == torch.uint8 else 2):
            pred = pred[None]
        if projector is None:
            if target.dim() == 1:
                target = target[None]
            self._launch(pred, target.contiguous(), None, 0, 0, target.shape[-1])
        else:
            projs = list(projector) if isinstance(projector, (list, tuple)) else [projector]
            if target.dim() == len(projs[0].shape):  # one sample of the projector's plane ([H', W'], or [Npix] on the sphere)
                target = target[None]
            b = target.shape[0]
            if camera is None:
                if len(projs) != 1:
                    raise ValueError("several projectors need `camera`, the projector index of every sample")
                cams = [0] * b
            else:
                cams = [int(c) for c in (camera.tolist() if torch.is_tensor(camera) else camera)]
                if len(cams) != b or min(cams) < 0 or max(cams) >= len(projs):
                    raise ValueError("camera must give a projector index for every sample")
            if pred.shape[0] != b:
                raise ValueError(f"{pred.shape[0]} predictions for {b} targets")
            start = 0
            for end in range(1, b + 1):
                if end == b or cams[end] != cams[start]:
                    p = projs[cams[start]]
                    if tuple(target.shape[1:]) != p.shape:
                        raise ValueError(f"targets are {tuple(target.shape[1:])}, the projector's image plane {p.shape}")
                    self._launch(pred[start:end], target[start:end].contiguous(), p.nearest, p.n_out,
                                 -1 if masked else p.s2_bkgd_class, p.npix)
                    start = end
        if check:
            self._check()

    def _check(self):
        bad_t, bad_p = self._bad.tolist()
        if bad_t:
            raise ValueError(f"{bad_t} target values >= num_classes = {self.num_classes}")
        if bad_p:
            raise ValueError(f"{bad_p} predicted class ids >= num_classes = {self.num_classes}")

    def all_reduce(self, group=None):
        """Sum the matrices of all ranks (torch.distributed), as torchmetrics' dist_reduce_fx='sum'."""
        import torch.distributed as dist

        dist.all_reduce(self.confmat, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self._bad, op=dist.ReduceOp.SUM, group=group)

    def iou(self, absent_score=0.0):
        """Per-class IoU (float32 [K]): diag / (row + col - diag); classes absent from target and prediction get
        absent_score (torchmetrics 0.3.2 IoU(reduction='none'); the reference's writers use absent_score=nan)."""
        self._check()
        inter = torch.diag(self.confmat)
        union = self.confmat.sum(0) + self.confmat.sum(1) - inter
        scores = inter.float() / union.float()
        scores[union == 0] = absent_score
        return scores

    def accuracy(self, ignore_index=None):
        """Micro-averaged accuracy (float32 scalar tensor): trace / total; with ignore_index = i, the pixels whose TARGET is i
        are dropped from both: sum_{c != i} C[c, c] / sum_{c != i} row_c.  This is our reading of torchmetrics 0.3.2's
        Accuracy(ignore_index=0) on class ids (the reference's acc_ignored)."""
        self._check()
        diag, rows = torch.diag(self.confmat), self.confmat.sum(1)
        if ignore_index is not None:
            keep = torch.arange(self.num_classes, device=self.device) != int(ignore_index)
            diag, rows = diag[keep], rows[keep]
        return diag.sum().float() / rows.sum().float()
