"""The flat data path on the GPU: a raw camera frame, class mask or depth map -> what the flat Swin-UNet
(`models_torch.swin_transformer.SwinTransformerSys`) reads.  Mirrors the reference's flat datasets, WoodscapeSemanticImagesDataset
(data/segmentation/flat_datasets.py:84-125) and WoodscapeDepthDataset (data/depth_estimation/flat_depth_datasets.py:69-147):

    CenterCrop((960, 1280)) if crop_green -> Resize(size) -> Pad(padding)      frames: bilinear on uint8; masks: nearest;
                                                                               depth: nearest or bilinear, then
    mask[mask == 1000] = inf (mask_background) -> log / inv -> standardize / min-max            (depth only)

  resize_output_size(h, w, size)    the output size of torchvision 0.9's Resize
  FlatFrameTransform                crop, resize and pad composed on the host into per-axis tables (both resizes are separable:
                                    O(H + W) entries), resident on the device
      .frames(x, dtype, layout)     uint8 [B, C, H0, W0] -> uint8 [B, C, H, W], or the patch rows ops.flat_patch_rows makes of it
      .masks(m, layout)             uint8 [B, H0, W0]    -> uint8 [B, H, W],    or the label rows ops.flat_labels makes of it
      .depth(d, interpolation, target, layout)
                                    fp32 [B, H0, W0]     -> fp32 [B, H, W],     or the target rows ops.flat_depth_target makes of
                                    it; `target` a depth_data.DepthTargetTransform(zero_is_background=False) applied in the pass
    one HIP launch each (`hs_flat_resize`), reading the raw batch in place; layout="rows" never writes the NCHW tensor
  PatchRows / PixelRows             the row tensors with the p, T, H, W they were made for: SwinTransformerSys.forward,
                                    forward_rows, forward_seg_loss and forward_depth_loss take them in place of the NCHW tensors
  class_distribution(masks, K)      data/segmentation/data_stats.py:14-36, exact integer counts on the device

torchvision is not installed where this was written, so Resize, Pad and CenterCrop themselves were not run: as
flat_evaluation.py states for its own tables, the rules here are our reading of torchvision 0.9's tensor path
(transforms/functional.py, functional_tensor.py): center_crop slices img[..., top : top + 960, left : left + 1280] with
top = int(round((h - 960) / 2.)); resize(size=int) sets the shorter side and gives the longer one int(size * long / short),
returning the image unchanged when the shorter side already equals size; resize(size=[h, w]) is
torch.nn.functional.interpolate(img, size=[h, w], mode="nearest") or (mode="bilinear", align_corners=False) on the image cast to
float32, rounded (torch.round, half to even) and cast back for uint8; pad with padding = [left, top, right, bottom] crops the
negative entries (img[..., -top : h + bottom, -left : w + right]) and then adds constant 0 for the positive ones.  The nearest
table is torch's own rounding (an index vector pushed through that interpolate call on the CPU); the bilinear taps are
flat_evaluation.resize_linear_taps.  Values are combined as h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11) in fp32
without contraction: within 4 ulp of the exact value of the same taps, as torch's CPU kernel is, not bit-equal to it.
"""
import numpy as np
import torch
import torch.nn.functional as F

from ._lib import (HS_BF16, HS_DT_1000_BKG, HS_DT_AFFINE, HS_DT_NONE, HS_F32, HS_FLAT_IMAGE, HS_FLAT_PATCH_ROWS, HS_FLAT_PIXEL_ROWS,
                   HS_U8, check, lib, ptr, stream_ptr)
from .evaluation import SegConfusion, _device
from .flat_evaluation import resize_linear_taps, resize_nearest_source

CROP_GREEN_SIZE = (960, 1280)  # flat_datasets.py: tv.transforms.CenterCrop((960, 1280))
_LDS_BYTES = 48 * 1024  # staging budget of one workgroup (the kernel takes up to 64 KiB)
_NO_CPU = "(the flat data kernels have no CPU path)"


# ------------------------------------------------------------------ host tables (once per source size and configuration)
def resize_output_size(height, width, size):
    """(h, w) after torchvision 0.9's Resize(size) of a height x width image.  A (h, w) pair is taken as it is (a one-element
    sequence counts as an int); an int sets the shorter side and the longer one becomes int(size * long / short); when the shorter
    side already equals size the image is returned unchanged.  Our reading of functional_tensor.resize: torchvision itself was not
    available to run."""
    height, width = int(height), int(width)
    if not isinstance(size, int):
        size = [int(s) for s in size]
        if len(size) == 2:
            return size[0], size[1]
        if len(size) != 1:
            raise ValueError(f"size must be an int or a (h, w) pair, got {size}")
        size = size[0]
    size = int(size)
    short, long = (width, height) if width <= height else (height, width)
    if short == size:
        return height, width
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if width <= height else (new_short, new_long)


def _nearest_axis(n_in, n_out, axis):
    """int64 [n_out]: the source index torch's interpolate(mode="nearest") reads along one axis of a 2-D resize."""
    shape = (1, 1, n_in, 1) if axis == 0 else (1, 1, 1, n_in)
    size = [n_out, 1] if axis == 0 else [1, n_out]
    index = torch.arange(n_in, dtype=torch.float64).view(shape)
    return F.interpolate(index, size=size, mode="nearest").reshape(n_out).numpy().astype(np.int64)


def _compose_axis(n_src, offset, n_crop, n_res, pad_lo, pad_hi, taps):
    """Crop [offset, offset + n_crop) -> resize to n_res (taps = (i0, i1, l0, l1) over the cropped axis) -> pad (negative: crop) as
    (idx int32 [2, n_out], wgt float32 [2, n_out]): source positions of the two taps, -1 where padding."""
    n_out = n_res + pad_lo + pad_hi
    if n_out < 1:
        raise ValueError(f"padding ({pad_lo}, {pad_hi}) leaves nothing of {n_res} resized pixels")
    i0, i1, l0, l1 = taps
    at = np.arange(n_out, dtype=np.int64) - pad_lo  # position in the resized axis
    inside = (at >= 0) & (at < n_res)
    idx = np.full((2, n_out), -1, dtype=np.int32)
    wgt = np.zeros((2, n_out), dtype=np.float32)
    idx[0, inside], idx[1, inside] = i0[at[inside]] + offset, i1[at[inside]] + offset
    wgt[0, inside], wgt[1, inside] = l0[at[inside]], l1[at[inside]]
    assert idx.max() < n_src and (idx[:, inside] >= offset).all() and idx[:, inside].max(initial=0) < offset + n_crop
    return idx, wgt


def _span(idx, tile):
    """The most source positions (last tap - first tap + 1) the outputs [k * tile, (k + 1) * tile) of one axis read, over k."""
    span = 0
    for start in range(0, idx.shape[1], tile):
        part = idx[:, start:start + tile]
        part = part[:, part[0] >= 0]
        if part.size:
            span = max(span, int(part.max()) - int(part.min()) + 1)
    return span


class _Tables:
    """The per-axis tables of one interpolation mode, on the host and on the device."""

    def __init__(self, rows, cols, bilinear, device):
        (self.row_idx, self.row_wgt), (self.col_idx, self.col_wgt) = rows, cols
        self.bilinear = bilinear
        if not bilinear:
            self.row_wgt = self.col_wgt = None
        self._dev = None if device is None else tuple(None if a is None else torch.from_numpy(a).to(device)
                                                      for a in (self.row_idx, self.row_wgt, self.col_idx, self.col_wgt))
        self._spans = {}

    def device_ptrs(self):
        return tuple(ptr(t) for t in self._dev)

    def spans(self, tile_h, tile_w):
        key = (tile_h, tile_w)
        if key not in self._spans:
            self._spans[key] = (_span(self.row_idx, tile_h), _span(self.col_idx, tile_w))
        return self._spans[key]

    def apply_host(self, img, exact=False):
        """The tables evaluated in numpy on img [..., H0, W0] (uint8 or float32): nearest copies; bilinear forms
        h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11) in float32 (uint8: then rounds half to even and casts), or with
        exact=True in float64 without the final rounding.  Padding is 0."""
        img = np.asarray(img)
        r0, r1, c0, c1 = self.row_idx[0], self.row_idx[1], self.col_idx[0], self.col_idx[1]
        valid = (r0 >= 0)[:, None] & (c0 >= 0)[None, :]
        ry0, ry1, cx0, cx1 = (np.maximum(a, 0) for a in (r0, r1, c0, c1))

        def tap(r, c):
            return img[..., r[:, None], c[None, :]]

        if not self.bilinear:
            return np.where(valid, tap(ry0, cx0), img.dtype.type(0))
        ft = np.float64 if exact else np.float32
        h0, h1 = self.row_wgt[0].astype(ft)[:, None], self.row_wgt[1].astype(ft)[:, None]
        w0, w1 = self.col_wgt[0].astype(ft)[None, :], self.col_wgt[1].astype(ft)[None, :]
        with np.errstate(invalid="ignore", over="ignore"):
            p00, p01, p10, p11 = (tap(r, c).astype(ft) for r, c in ((ry0, cx0), (ry0, cx1), (ry1, cx0), (ry1, cx1)))
            out = h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11)
        out = np.where(valid, out, ft(0))
        if exact or img.dtype != np.uint8:
            return out
        return np.rint(out).astype(np.uint8)

    def max_tap(self, img):
        """max |tap| per output pixel of a bilinear table (float64; 0 where padding): the scale of the rounding-error bound."""
        img = np.abs(np.asarray(img).astype(np.float64))
        valid = (self.row_idx[0] >= 0)[:, None] & (self.col_idx[0] >= 0)[None, :]
        rs, cs = [np.maximum(a, 0) for a in self.row_idx], [np.maximum(a, 0) for a in self.col_idx]
        m = np.zeros(img.shape[:-2] + valid.shape)
        for r in rs:
            for c in cs:
                m = np.maximum(m, img[..., r[:, None], c[None, :]])
        return np.where(valid, m, 0.0)


class PatchRows:
    """Patch rows [B, N0, K] (fp32 / bf16) of frames of H x W pixels, for a model with patch p and tile T: what
    ops.flat_patch_rows(image, p, T, dtype) returns, made by FlatFrameTransform.frames(layout="rows")."""

    def __init__(self, rows, channels, height, width, patch_size, tile):
        self.rows, self.channels = rows, None if channels is None else int(channels)
        self.height, self.width, self.patch_size, self.tile = int(height), int(width), int(patch_size), int(tile)

    kind = "patch rows"

    @property
    def device(self):
        return self.rows.device

    @property
    def is_cuda(self):
        return self.rows.is_cuda

    @property
    def dtype(self):
        return self.rows.dtype

    @property
    def batch(self):
        return self.rows.shape[0]

    def check_model(self, model):
        """Raise unless these rows were built for `model` (a SwinTransformerSys)."""
        want = (int(model.data_spec.dim_in[0]), int(model.data_spec.dim_in[1]), int(model.config.patch_size[0]), int(model.tile))
        have = (self.height, self.width, self.patch_size, self.tile)
        if have != want:
            raise ValueError(f"{self.kind} built for (H, W, patch, tile) = {have} do not fit the model's {want}")
        if self.channels is not None and self.channels != int(model.data_spec.f_in):
            raise ValueError(f"{self.kind} of {self.channels} channels do not fit the model's f_in = {model.data_spec.f_in}")
        return self.rows


class PixelRows(PatchRows):
    """Pixel rows [B, H * W] (uint8 labels or fp32 depth targets) in the order of the model's head rows: what ops.flat_labels /
    ops.flat_depth_target return, made by FlatFrameTransform.masks / .depth(layout="rows")."""

    kind = "pixel rows"

    def __init__(self, rows, height, width, patch_size, tile):
        super().__init__(rows, None, height, width, patch_size, tile)


class FlatFrameTransform:
    """CenterCrop (crop_green) -> Resize(size) -> Pad(padding) of frames of src_size = (H0, W0), composed once into per-axis
    tables on `device`.  size: None (no resize), an int (the shorter side) or (h, w); padding = [left, top, right, bottom], positive
    entries add constant 0, negative ones crop.  An unchanged size skips the resize (identity: values are copied, no arithmetic).
    `.out_size` is the (H, W) of the result, the data_spec.dim_in of the model that reads it.  patch_size and tile (of the model:
    for_model fills them) are needed for layout="rows" only.  device=None builds the host tables alone (`.tables(mode)`)."""

    def __init__(self, src_size, size=None, padding=(0, 0, 0, 0), crop_green=False, device="cuda", patch_size=None, tile=None):
        self.src_size = (int(src_size[0]), int(src_size[1]))
        h0, w0 = self.src_size
        if h0 < 1 or w0 < 1:
            raise ValueError(f"src_size {self.src_size} is empty")
        self.crop_green = bool(crop_green)
        if self.crop_green:
            ch, cw = CROP_GREEN_SIZE
            if h0 < ch or w0 < cw:
                raise ValueError(f"crop_green crops the centre {ch} x {cw}: a {h0} x {w0} frame is smaller")
            top, left = int(round((h0 - ch) / 2.0)), int(round((w0 - cw) / 2.0))
        else:
            (ch, cw), top, left = (h0, w0), 0, 0
        self.crop = (top, left, ch, cw)
        self.size = size if size is None or isinstance(size, int) else tuple(int(s) for s in size)
        self.resized = (ch, cw) if size is None else resize_output_size(ch, cw, size)
        if min(self.resized) < 1:
            raise ValueError(f"size {size} gives an empty image")
        self.identity = self.resized == (ch, cw)
        self.padding = tuple(int(p) for p in padding)
        if len(self.padding) != 4:
            raise ValueError(f"padding must be [left, top, right, bottom], got {padding}")
        pl, pt, pr, pb = self.padding
        self.out_size = (self.resized[0] + pt + pb, self.resized[1] + pl + pr)
        if min(self.out_size) < 1:
            raise ValueError(f"padding {list(self.padding)} leaves nothing of a {self.resized[0]} x {self.resized[1]} image")
        self.patch_size = None if patch_size is None else int(patch_size)
        self.tile = None if tile is None else int(tile)
        self.device = None if device is None else _device(device)
        self._tables = {}

    @classmethod
    def for_model(cls, model, src_size, **kwargs):
        """The transform that feeds `model` (a SwinTransformerSys): patch_size and tile come from the model, and .out_size must
        be the model's data_spec.dim_in."""
        for key, value in (("patch_size", int(model.config.patch_size[0])), ("tile", int(model.tile))):
            if kwargs.setdefault(key, value) != value:
                raise ValueError(f"{key}={kwargs[key]!r} does not match the model ({value!r})")
        self = cls(src_size, **kwargs)
        want = (int(model.data_spec.dim_in[0]), int(model.data_spec.dim_in[1]))
        if self.out_size != want:
            raise ValueError(f"the transform gives {self.out_size[0]} x {self.out_size[1]} frames, the model was built for "
                             f"data_spec.dim_in = {want}")
        return self

    def tables(self, interpolation):
        """The _Tables of "nearest" or "bilinear" (an unchanged size: the identity for both)."""
        if interpolation not in ("nearest", "bilinear"):
            raise ValueError(f"interpolation must be 'nearest' or 'bilinear', got {interpolation!r}")
        mode = "nearest" if self.identity else interpolation
        if mode not in self._tables:
            self._tables[mode] = self._build(mode)
        return self._tables[mode]

    def _build(self, mode):
        (h0, w0), (top, left, ch, cw), (rh, rw), (pl, pt, pr, pb) = self.src_size, self.crop, self.resized, self.padding
        if mode == "bilinear":
            taps_y, taps_x = resize_linear_taps(ch, rh), resize_linear_taps(cw, rw)
        else:
            ys, xs = (np.arange(ch), np.arange(cw)) if self.identity else (_nearest_axis(ch, rh, 0), _nearest_axis(cw, rw, 1))
            if not self.identity:  # torch's 2-D resize is the outer combination of the two 1-D ones
                assert np.array_equal(resize_nearest_source((ch, cw), (rh, rw)), ys[:, None] * cw + xs[None, :])
            one_y, one_x = np.ones(rh, np.float32), np.ones(rw, np.float32)
            taps_y, taps_x = (ys, ys, one_y, 0 * one_y), (xs, xs, one_x, 0 * one_x)
        return _Tables(_compose_axis(h0, top, ch, rh, pt, pb, taps_y), _compose_axis(w0, left, cw, rw, pl, pr, taps_x),
                       mode == "bilinear", self.device)

    # -------------------------------------------------------------- the device side (per batch)
    def _run(self, x, nch, tables, out_dtype, layout, target, what):
        if self.device is None or self.device.type != "cuda":
            raise RuntimeError(f"this FlatFrameTransform holds host tables only: build it with a GPU device {_NO_CPU}")
        if x.device != self.device:
            raise RuntimeError(f"{what} must be on the transform's device {self.device} {_NO_CPU}")
        if layout not in ("image", "rows"):
            raise ValueError(f"layout must be 'image' or 'rows', got {layout!r}")
        h0, w0 = self.src_size
        b = x.shape[0]
        if b < 1:
            raise ValueError(f"{what}: empty batch")
        if x.stride(0) < nch * h0 * w0 or not x[0].is_contiguous():  # any batch stride, dense images
            x = x.contiguous()
        src_code = HS_U8 if x.dtype == torch.uint8 else HS_F32
        out_code = {torch.uint8: HS_U8, torch.float32: HS_F32, torch.bfloat16: HS_BF16}[out_dtype]
        h, w = self.out_size
        p, t, ld = 0, 0, 0
        if layout == "image":
            code, shape = HS_FLAT_IMAGE, (b, nch, h, w)
            tiles = [(th, tw) for th, tw in ((16, 64), (8, 64), (8, 32), (4, 16), (2, 16), (1, 16))]
        else:
            p, t = self.patch_size, self.tile
            if p is None or t is None:
                raise ValueError("layout='rows' needs the model's patch_size and tile (FlatFrameTransform.for_model fills them)")
            if p < 1 or t < 1 or t & (t - 1) or h % (p * t) or w % (p * t):
                raise ValueError(f"a {h} x {w} frame does not divide into tiles of {t} x {t} tokens (a power of two) of {p} x {p} pixels")
            if out_dtype == torch.uint8 or x.dtype == torch.float32:
                code, ld, shape = HS_FLAT_PIXEL_ROWS, 1, (b, h * w)
            else:
                k = nch * p * p
                ld = k + (-k) % 8
                code, shape = HS_FLAT_PATCH_ROWS, (b, (h // p) * (w // p), ld)
            s, tiles = min(t, 16), []
            while s >= 1:
                tiles.append((s * p, s * p))
                s //= 2
            tiles = [tl for tl in tiles if tl[0] <= 256] or tiles[-1:]
        for th, tw in tiles:
            sh, sw = tables.spans(th, tw)
            if lib.hs_flat_resize_lds_bytes(nch, src_code, th, tw, sh, sw) <= _LDS_BYTES:
                break
        else:
            raise NotImplementedError(f"{what}: a {h0} x {w0} -> {self.resized[0]} x {self.resized[1]} resize reads a {sh} x {sw} "
                                      f"window for the smallest output tile ({th} x {tw}), more than the kernel stages")
        flags, transform, shift, scale = 0, HS_DT_NONE, 0.0, 1.0
        if target is not None:
            flags = HS_DT_1000_BKG if target.mask_background else 0
            transform = target._transform
            if target._affine is not None:
                flags |= HS_DT_AFFINE
                shift, scale = target._affine
        out = torch.empty(shape, dtype=out_dtype, device=self.device)
        ri, rw_, ci, cw_ = tables.device_ptrs()
        check(lib.hs_flat_resize(ptr(x), src_code, x.stride(0), b, nch, h0, w0, ri, rw_, ci, cw_, ptr(out), out_code, h, w, code, p, t, ld,
                                 th, tw, sh, sw, flags, transform, shift, scale, stream_ptr(self.device)), "hs_flat_resize")
        return out

    def _input(self, x, dtype, dims, what):
        h0, w0 = self.src_size
        if not torch.is_tensor(x) or x.dtype != dtype:
            raise TypeError(f"{what} must be a {str(dtype).replace('torch.', '')} tensor, got "
                            f"{x.dtype if torch.is_tensor(x) else type(x).__name__}")
        if x.dim() == dims - 1:
            x = x[None]
        if x.dim() != dims or tuple(x.shape[-2:]) != (h0, w0):
            raise ValueError(f"{what} must be [B, {'C, ' if dims == 4 else ''}{h0}, {w0}], got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError(f"{what} must be a GPU tensor {_NO_CPU}")
        return x

    def frames(self, x, dtype=torch.float32, layout="image"):
        """uint8 frames [B, C, H0, W0] -> layout="image": uint8 [B, C, H, W] (bilinear, rounded half to even, as torchvision's
        Resize of a uint8 tensor); layout="rows": PatchRows of [B, N0, K] in `dtype` (fp32 / bf16), the same uint8 values
        converted: ops.flat_patch_rows(image, p, T, dtype) bit for bit."""
        x = self._input(x, torch.uint8, 4, "frames")
        if layout == "rows" and dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"patch rows are float32 or bfloat16, got {dtype}")
        out = self._run(x, x.shape[1], self.tables("bilinear"), torch.uint8 if layout == "image" else dtype, layout, None, "frames")
        return out if layout == "image" else PatchRows(out, x.shape[1], *self.out_size, self.patch_size, self.tile)

    def masks(self, m, layout="image"):
        """uint8 class masks [B, H0, W0] -> layout="image": uint8 [B, H, W] (nearest, padding 0); layout="rows": PixelRows of
        uint8 [B, H * W]: ops.flat_labels(image, p, T) bit for bit."""
        m = self._input(m, torch.uint8, 3, "masks")
        out = self._run(m, 1, self.tables("nearest"), torch.uint8, layout, None, "masks")
        return out[:, 0] if layout == "image" else PixelRows(out, *self.out_size, self.patch_size, self.tile)

    def depth(self, d, interpolation="nearest", target=None, layout="image"):
        """fp32 depth maps [B, H0, W0] -> layout="image": fp32 [B, H, W]; layout="rows": PixelRows of fp32 [B, H * W]:
        ops.flat_depth_target(image, p, T) bit for bit.  Nearest values are copied bit for bit, bilinear ones are plain IEEE
        arithmetic (a non-finite tap propagates); padding is 0.  target: a DepthTargetTransform(zero_is_background=False), whose
        forward chain (1000 -> inf if mask_background, log / inv, normalization) is applied to the resized, padded value in the
        same pass: target.prepare(...) of the result without it, bit for bit (padded zeros included: log gives -inf)."""
        d = self._input(d, torch.float32, 3, "depth")
        if target is not None and target.zero_is_background:
            raise ValueError("the flat depth dataset does not turn 0 into inf (only the HEALPix dataset's s2_bkgd_class path does): "
                             "pass DepthTargetTransform(..., zero_is_background=False)")
        out = self._run(d, 1, self.tables(interpolation), torch.float32, layout, target, "depth")
        return out[:, 0] if layout == "image" else PixelRows(out, *self.out_size, self.patch_size, self.tile)


# ------------------------------------------------------------------ class statistics
def class_distribution(masks, num_classes, device="cuda"):
    """get_class_distribution (data/segmentation/data_stats.py:14-36): the percentage 100 * count_i / numel of every class id
    i < num_classes over `masks`, an iterable of uint8 tensors of class ids (any shape; moved to the device), as a float64 array
    [num_classes].  Ids >= num_classes count towards numel only.  The counts are exact integers, kept on the device (the
    diagonal of a SegConfusion fed the labels as prediction and target)."""
    conf = SegConfusion(num_classes, device=device)
    numel = 0
    for m in [masks] if torch.is_tensor(masks) else masks:
        if not torch.is_tensor(m) or m.dtype != torch.uint8:
            raise TypeError("masks must be uint8 tensors of class ids")
        if m.numel() == 0:
            continue
        m = m.to(conf.device).reshape(1, -1)
        conf.update(m, m, check=False)
        numel += m.numel()
    if numel == 0:
        raise ValueError("no pixels")
    counts = conf.confmat.diagonal().cpu().numpy().astype(np.int64)
    return 100 * counts.astype(np.float64) / numel
