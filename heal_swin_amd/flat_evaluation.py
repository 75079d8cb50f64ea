"""The flat Swin-UNet baseline scored on the sphere: flat predictions (segmentation logits or depth) sampled onto the HEALPix
grid and compared with the HEALPix ground truth, the reference's `val_on_hp_projected` writers and `*_projected_to_hp` metrics,
and the flat prediction against the flat target on the image pixels the HEALPix grid covers (`hp_masked_iou`).  Mirrors:

  FlatToHPProjector                 the per-sample chain of WoodscapeFlatValOnHPProjectedPredictionWriter (evaluation/
                                    flat_pred_writers.py:321-421) and WoodscapeDepthFlatValOnHPProjectedPredictionWriter
                                    (evaluation/flat_depth_pred_writers.py:128-253) as ONE table per calibration:
                                      tv.transforms.Pad([-p for p in padding])       un-pad
                                      tv.transforms.Resize(orig_size, interpolation) nearest, or bilinear for depth
                                      project_s2_points_to_img(theta, phi, cal_info, rotate_pole) of the HEALPix pixels
                                      sample_mask(pred, v, u, s2_bkgd_class)         np.around, background outside the image
      .labels(pred)                 the projected class ids uint8 [B, Npix]              `hs_backproject_labels`
      .depth(pred)                  the projected depth fp32 [B, Npix], NaN background   `hs_flat_depth_to_hp`
      SegConfusion.update(projector.logits(pred), hp_target, projector)                  `hs_seg_confusion`
                                    Accuracy, Accuracy(ignore_index=0) and IoU of the writer follow from the matrix
      DepthMetrics.update(pred, hp_target, projector)                                    `hs_depth_metrics_gather`
                                    DepthMSE, SILogE, iRMSE, RelAE, RelSE without writing the projected map
  FlatCoverage                      HPMaskedIoU.get_mask (evaluation/custom_metrics.py:25-59) as a projector over the image
                                    plane itself: SegConfusion.update(coverage.logits(pred), flat_target, coverage, masked=True)
                                    is WoodscapeFlatHPMaskedIoUPredictionWriter (flat_pred_writers.py:253-318)

Predictions are read in place, fp32 or bf16: an NCHW map (`layout="image"`: logits [B, K, H, W], depth [B, C, H, W] or
[B, H, W], class ids uint8 [B, H, W]) or the head rows `SwinTransformerSys.forward_rows` returns (`layout="rows"`:
[B, H * W, f_out], pixels in tiled Z order over tokens with the p x p children of a token consecutive, what
ops.flat_pixel_image undoes), so that the NCHW logits need not be written at all.  The logits are argmaxed at the sampled
pixel only; argmax commutes with a nearest gather, so this equals the reference's chain on class ids.

The tables are host work done once per calibration (float64 numpy and integers).  torchvision is not installed where this was
written, so Resize and Pad themselves were not run: the tables are pinned to the torch calls that torchvision 0.9's tensor path
makes, by our reading of it (functional_tensor.py): a negative Pad is the slice img[..., top : H - bottom, left : W - right]
with padding = [left, top, right, bottom], and Resize(size=[h, w]) is torch.nn.functional.interpolate(img, size=[h, w],
mode="nearest") or (mode="bilinear", align_corners=False), without antialiasing.  The nearest table is built by pushing an
index image through that very interpolate call on the CPU, so torch's own rounding is the definition; the bilinear taps restate
torch's fp32 source-index arithmetic (area_pixel_compute_source_index) and are tested against interpolate.  When the un-padded
prediction already has orig_size, both modes are the identity, as the reference's orig_size=None, which skips the Resize (a
same-size bilinear interpolate would turn an infinite prediction into NaN: 0 * inf).
"""
import numpy as np
import torch
import torch.nn.functional as F

from ._lib import check, flat_zorder, lib, ptr, stream_ptr
from ._sphere_args import _device_tensor, _kind_of, _label_class
from .evaluation import HPBackProjector, _backproject_labels, _device
from .projection import hp_grid, project_s2_points_to_img


# ------------------------------------------------------------------ host tables (once per calibration)
def resize_nearest_source(src_size, dst_size):
    """int64 [h', w']: the flat index y * w + x of the source pixel that interpolate(mode="nearest") reads for every pixel of
    the resized image, found by resizing an index image with torch itself."""
    (h, w), (oh, ow) = (int(s) for s in src_size), (int(s) for s in dst_size)
    index = torch.arange(h * w, dtype=torch.float64).view(1, 1, h, w)
    return F.interpolate(index, size=[oh, ow], mode="nearest").view(oh, ow).numpy().astype(np.int64)


def resize_linear_taps(n_in, n_out):
    """The two source positions and fp32 weights of every output position of a 1-D linear resize with align_corners=False:
    (i0, i1 int64 [n_out], l0, l1 float32 [n_out]); out = l0 * in[i0] + l1 * in[i1].  torch's area_pixel_compute_source_index
    in fp32: src = scale * (dst + 0.5) - 0.5 with scale = fp32(n_in) / n_out, rounded ONCE (torch's CPU kernel contracts the
    expression into a fused multiply-add; rounding the product first moves weights by up to an ulp of src, 3e-5 at 768 rows),
    negative src clamped to 0, l1 = src - floor(src), l0 = 1 - l1."""
    n_in, n_out = int(n_in), int(n_out)
    scale = np.float64(np.float32(n_in) / np.float32(n_out))
    src = (scale * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5).astype(np.float32)  # exact in float64, one rounding
    src = np.where(src < 0, np.float32(0), src).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def pixel_rows(height, width, patch_size, tile):
    """int64 [H * W]: the row of pixel h * W + w in the flat model's head rows (tiled Z order over the tokens, tile side `tile`
    tokens, the p x p children of a token consecutive, child (kh, kw) at kh * p + kw): ops.flat_pixel_image's inverse."""
    h, w, p, t = int(height), int(width), int(patch_size), int(tile)
    if p < 1 or t < 1 or h % p or w % p or (h // p) % t or (w // p) % t:
        raise ValueError(f"a {h} x {w} image does not divide into tiles of {t} x {t} tokens of {p} x {p} pixels")
    z_of_rm, _ = flat_zorder(h // p, w // p, t)
    hh, ww = np.divmod(np.arange(h * w, dtype=np.int64), w)
    token = (hh // p) * (w // p) + ww // p
    return z_of_rm.astype(np.int64)[token] * (p * p) + (hh % p) * p + ww % p


def _layout_map(layout, height, width, patch_size, tile):
    if layout == "image":
        return None
    if layout != "rows":
        raise ValueError(f"layout must be 'image' or 'rows', got {layout!r}")
    if patch_size is None or tile is None:
        raise ValueError("layout='rows' needs the model's patch_size and tile (FlatToHPProjector.for_model fills them)")
    return pixel_rows(height, width, patch_size, tile)


class _FlatSource:
    """What both projectors share: the layout of the flat prediction and the views the kernels read it through."""

    def _init_source(self, model_size, layout, patch_size, tile, device):
        self.model_size = (int(model_size[0]), int(model_size[1]))
        if min(self.model_size) < 1:
            raise ValueError(f"model_size {self.model_size} is empty")
        self.layout = layout
        self.patch_size = None if patch_size is None else int(patch_size)
        self.tile = None if tile is None else int(tile)
        self._rows = _layout_map(layout, *self.model_size, patch_size, tile)
        self.device = _device(device)

    @property
    def npix(self):
        """Source pixels of one prediction, H * W (what SegConfusion bounds the table by)."""
        return self.model_size[0] * self.model_size[1]

    def _to_source(self, pixel):
        """Index into one prediction of model-plane pixel indices h * W + w."""
        return pixel if self._rows is None else self._rows[pixel]

    def logits(self, pred):
        """The prediction as SegConfusion and the label kernels read it: logits [B, K, n_src] (a view: NCHW logits flattened,
        or the head rows [B, n_src, K] permuted, whose 16-byte rows then take the fast loads) or class ids uint8 [B, n_src]."""
        h, w = self.model_size
        _device_tensor(pred, "predictions", self.device, (torch.float32, torch.bfloat16, torch.uint8), RuntimeError)
        ids = pred.dtype == torch.uint8
        if self.layout == "image":
            want = "[B, H, W]" if ids else "[B, K, H, W]"
            if pred.dim() != (3 if ids else 4) or tuple(pred.shape[-2:]) != (h, w):
                raise ValueError(f"layout='image' predictions must be {want} with H x W = {h} x {w}, got {tuple(pred.shape)}")
            return pred.flatten(-2)
        if pred.dim() != (2 if ids else 3) or pred.shape[1] != self.npix:
            raise ValueError(f"layout='rows' predictions must be [B, {self.npix}{'' if ids else ', K'}], got {tuple(pred.shape)}")
        return pred if ids else pred.permute(0, 2, 1)

    def _depth_args(self, pred, channels=1):
        """(pred, stride_b, stride_c, stride_p) of a depth prediction with at least `channels` channels (a channel-less one
        has one)."""
        h, w = self.model_size
        _device_tensor(pred, "pred", self.device, (torch.float32, torch.bfloat16), RuntimeError)
        if self.layout == "image":
            if pred.dim() not in (3, 4) or tuple(pred.shape[-2:]) != (h, w):
                raise ValueError(f"layout='image' predictions must be [B, C, H, W] or [B, H, W] with H x W = {h} x {w}, got "
                                 f"{tuple(pred.shape)}")
            if h > 1 and pred.stride(-2) != w * pred.stride(-1):
                pred = pred.contiguous()
            have, sc, sp = (pred.shape[1], pred.stride(1), pred.stride(-1)) if pred.dim() == 4 else (1, 0, pred.stride(-1))
        else:
            if pred.dim() not in (2, 3) or pred.shape[1] != self.npix:
                raise ValueError(f"layout='rows' predictions must be [B, {self.npix}, C] or [B, {self.npix}], got {tuple(pred.shape)}")
            have, sc, sp = (pred.shape[2], pred.stride(2), pred.stride(1)) if pred.dim() == 3 else (1, 0, pred.stride(1))
        if have < channels:
            raise ValueError(f"predictions have {have} channels, {channels} are needed")
        return pred, pred.stride(0), sc, sp


class FlatToHPProjector(_FlatSource):
    """The flat-to-HEALPix sampling tables of one calibration, built once on the host and resident on the device.

    For each of the n_out = base_pix * nside^2 nested HEALPix pixels, the pixel of a flat prediction of `model_size` that the
    reference's writers sample: project_s2_points_to_img -> np.around -> inside [0, orig_h) x [0, orig_w) or uncovered -> the
    inverse of Resize(orig_size) on the un-padded prediction -> + (top, left) of padding = [left, top, right, bottom] ->
    `layout`.  orig_size defaults to the calibration's (height, width).
      nearest   int32 [Npix]       the source pixel (interpolation="nearest"); a value >= npix where uncovered
      idx, wgt  int32 / float32 [4, Npix]   interpolation="bilinear" (depth only): taps (y0 x0, y0 x1, y1 x0, y1 x1) and
                                   weights (h0, h1, w0, w1); value = h0 (w0 p00 + w1 p01) + h1 (w0 p10 + w1 p11)
      covered   bool [Npix]
    It carries what SegConfusion.update reads from a projector: nearest, n_out, npix (source pixels H * W), shape = (Npix,)
    and s2_bkgd_class."""

    def __init__(self, cal_info, nside, base_pix=8, rotate_pole=False, model_size=None, orig_size=None, padding=(0, 0, 0, 0),
                 layout="image", patch_size=None, tile=None, s2_bkgd_class=0, interpolation="nearest", device="cuda"):
        self.nside, self.base_pix, self.rotate_pole = int(nside), int(base_pix), bool(rotate_pole)
        self.s2_bkgd_class = _label_class(s2_bkgd_class)
        if interpolation not in ("nearest", "bilinear"):
            raise ValueError(f"interpolation must be 'nearest' or 'bilinear', got {interpolation!r}")
        self.interpolation = interpolation
        intr = cal_info["intrinsic"]
        self.orig_size = (int(intr["height"]), int(intr["width"])) if orig_size is None else (int(orig_size[0]), int(orig_size[1]))
        if model_size is None:
            raise ValueError("model_size = (H, W) of the flat prediction is required")
        self._init_source(model_size, layout, patch_size, tile, device)
        self.padding = tuple(int(p) for p in padding)
        if len(self.padding) != 4 or min(self.padding) < 0:
            raise ValueError(f"padding must be [left, top, right, bottom] >= 0, got {padding}")
        left, top, right, bottom = self.padding
        height, width = self.model_size
        uh, uw = height - top - bottom, width - left - right
        if uh < 1 or uw < 1:
            raise ValueError(f"padding {list(self.padding)} leaves nothing of a {height} x {width} prediction")
        oh, ow = self.orig_size
        if oh < 1 or ow < 1:
            raise ValueError(f"orig_size {self.orig_size} is empty")

        theta, phi = hp_grid(self.nside, self.base_pix)
        u, v = project_s2_points_to_img(theta, phi, cal_info, self.rotate_pole)
        self.u, self.v = u, v
        with np.errstate(invalid="ignore"):
            r, c = np.around(v, 0), np.around(u, 0)  # sample_mask(pred, v, u, ...): rows from v, columns from u
            covered = (r >= 0) & (r < oh) & (c >= 0) & (c < ow)
        r, c = r[covered].astype(np.int64), c[covered].astype(np.int64)
        n, n_src = theta.shape[0], self.npix
        identity = (uh, uw) == (oh, ow)

        def source(y, x):  # un-padded pixel -> index into one prediction
            return self._to_source((y + top) * width + (x + left))

        nearest = np.full(n, n_src, dtype=np.int64)
        src = resize_nearest_source((uh, uw), (oh, ow))[r, c]
        nearest[covered] = source(src // uw, src % uw)
        self.covered_host, self.nearest_host = covered, nearest.astype(np.int32)
        self.idx_host = self.wgt_host = self.idx = self.wgt = None
        if interpolation == "bilinear" and not identity:
            y0, y1, h0, h1 = resize_linear_taps(uh, oh)
            x0, x1, w0, w1 = resize_linear_taps(uw, ow)
            idx = np.full((4, n), n_src, dtype=np.int64)
            wgt = np.zeros((4, n), dtype=np.float32)
            for m, (y, x) in enumerate(((y0, x0), (y0, x1), (y1, x0), (y1, x1))):
                idx[m, covered] = source(y[r], x[c])
            wgt[0, covered], wgt[1, covered], wgt[2, covered], wgt[3, covered] = h0[r], h1[r], w0[c], w1[c]
            self.idx_host, self.wgt_host = idx.astype(np.int32), wgt
            self.idx = torch.from_numpy(self.idx_host).to(self.device)
            self.wgt = torch.from_numpy(self.wgt_host).to(self.device)
        self._nearest = torch.from_numpy(self.nearest_host).to(self.device)
        self.covered = torch.from_numpy(covered).to(self.device)
        self.shape = (n,)

    @classmethod
    def for_model(cls, model, cal_info, nside, **kwargs):
        """The projector of a SwinTransformerSys' head rows (`model.forward_rows`): model_size, patch_size, tile and
        layout="rows" come from the model."""
        size = (int(model.data_spec.dim_in[0]), int(model.data_spec.dim_in[1]))
        given = kwargs.pop("model_size", None)
        if given is not None and (int(given[0]), int(given[1])) != size:
            raise ValueError(f"model_size {tuple(given)} does not match the model's input {size}")
        for key, value in (("patch_size", model.config.patch_size[0]), ("tile", model.tile), ("layout", "rows")):
            if kwargs.setdefault(key, value) != value:
                raise ValueError(f"{key}={kwargs[key]!r} does not match the model ({value!r})")
        return cls(cal_info, nside, model_size=size, **kwargs)

    @property
    def n_out(self):
        """HEALPix pixels: base_pix * nside^2."""
        return self.shape[0]

    @property
    def nearest(self):
        if self.interpolation != "nearest":
            raise ValueError("class ids cannot be interpolated: build the projector with interpolation='nearest' for labels")
        return self._nearest

    def labels(self, pred):
        """The projected class ids uint8 [B, Npix]: sample_mask(argmax, v, u, s2_bkgd_class) of the un-padded, resized
        prediction.  pred: logits (argmax as torch.max(logits, 1), taken at the sampled pixel only) or uint8 class ids, in the
        projector's layout."""
        nearest = self.nearest  # (refuses a bilinear projector before anything looks at pred)
        return _backproject_labels(self.logits(pred), nearest, self.n_out, self.npix, self.s2_bkgd_class, self.shape, self.device)

    def _tables(self):
        """(nearest, idx, wgt) pointers for the depth kernels: one of the two tables."""
        return (ptr(self._nearest), None, None) if self.idx is None else (None, ptr(self.idx), ptr(self.wgt))

    def depth(self, pred, channel=0):
        """The projected depth fp32 [B, Npix], NaN where uncovered: project_depth_on_s2.sample_mask(pred, v, u, nan) of the
        un-padded, resized channel `channel`.  Nearest values are copied bit for bit."""
        pred, sb, sc, sp = self._depth_args(pred, int(channel) + 1)
        if channel:
            pred = pred.select(1 if self.layout == "image" else 2, int(channel))
        out = torch.empty((pred.shape[0], self.n_out), dtype=torch.float32, device=self.device)
        near, idx, wgt = self._tables()
        check(lib.hs_flat_depth_to_hp(ptr(pred), _kind_of(pred), pred.shape[0], self.npix, sb, sp, near, idx, wgt, self.n_out, ptr(out),
                                      stream_ptr(self.device)), "hs_flat_depth_to_hp")
        return out


class FlatCoverage(_FlatSource):
    """HPMaskedIoU's mask as a projector over the image plane itself: shape = img_dims, n_out = npix = H * W, and nearest[i]
    is pixel i's own index (its row for layout="rows") where HPBackProjector(output_resolution=img_dims).valid holds, a value
    >= npix elsewhere.  SegConfusion.update(coverage.logits(pred), flat_target, coverage, masked=True) scores the flat
    prediction against the flat target on the covered pixels only."""

    def __init__(self, cal_info, nside, base_pix=8, rotate_pole=False, img_dims=None, layout="image", patch_size=None, tile=None,
                 s2_bkgd_class=0, device="cuda"):
        if img_dims is None:
            raise ValueError("img_dims = (H, W) of the flat prediction is required")
        self._init_source(img_dims, layout, patch_size, tile, device)
        self.nside, self.base_pix, self.s2_bkgd_class = int(nside), int(base_pix), int(s2_bkgd_class)
        back = HPBackProjector(cal_info, self.nside, base_pix=self.base_pix, output_resolution=self.model_size,
                               rotate_pole=rotate_pole, device="cpu")
        valid = back.valid.numpy().reshape(-1)
        nearest = np.where(valid, self._to_source(np.arange(self.npix, dtype=np.int64)), self.npix)
        self.valid_host, self.nearest_host = valid.reshape(self.model_size), nearest.astype(np.int32)
        self.nearest = torch.from_numpy(self.nearest_host).to(self.device)
        self.valid = torch.from_numpy(self.valid_host).to(self.device)
        self.shape = self.model_size

    @classmethod
    def for_model(cls, model, cal_info, nside, **kwargs):
        size = (int(model.data_spec.dim_in[0]), int(model.data_spec.dim_in[1]))
        return cls(cal_info, nside, img_dims=size, layout="rows", patch_size=model.config.patch_size[0], tile=model.tile, **kwargs)

    @property
    def n_out(self):
        return self.npix
