"""Flat Swin-UNet (the paper's baseline on the undistorted fisheye image) on the MI355X-native hot path.

Keeps the public surface of the reference module `heal_swin/models_torch/swin_transformer.py` (class names, constructor
signatures, attribute paths and therefore state-dict keys, `forward` contract), and is built from the HEALPix modules of
swin_hp_transformer.py: a flat image whose side is a multiple of p * w * 2^(L-1) has the structure of a nested HEALPix map once
its tokens are stored in TILED Z ORDER (csrc/flat_tables.cpp):

  * the token grid is cut into T x T tiles, T = w * 2^(L-1), laid out row-major; each tile plays the part of a base pixel;
  * inside a tile the tokens follow a Morton order whose least-significant bit is the row bit.

Then every window of every stage is w^2 consecutive tokens, PatchMerging's concat order (0::2,0::2), (1::2,0::2), (0::2,1::2),
(1::2,1::2) is a plain view of 4 consecutive tokens, and a shifted block's roll + window partition is a row permutation with
region labels (`FlatShift`), which the HEALPix block's attention paths take as they are.  What is new is only at the image
boundary (csrc/flat_layout.hip): image -> patch rows, logits rows -> NCHW, labels -> pixel-row order.

Reference line numbers in comments refer to heal_swin/models_torch/swin_transformer.py.
"""
from dataclasses import dataclass, field
from typing import List, Literal, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, ops
from ..data_spec import DataSpec
from ..flat_data import PatchRows, PixelRows
from . import hp_shifting
from . import swin_hp_transformer as hp
from .swin_hp_transformer import DropPath, HSLayerNorm, HSLinear, Mlp, _make_norm  # noqa: F401  (reference names)

SUPPORTED_WINDOW_SIDES = (2, 4, 8, 16)  # w^2 in {4, 16, 64, 256}: the window sizes of the attention kernels


def _pair(v):
    if isinstance(v, int):
        return [v, v]
    v = list(v)
    return v * 2 if len(v) == 1 else v


def _check_window(ws, what):
    if ws[0] != ws[1]:
        raise NotImplementedError(f"{what} {ws[0]} x {ws[1]} is not square: only square windows are supported")
    if ws[0] not in SUPPORTED_WINDOW_SIDES:
        raise NotImplementedError(f"{what} side {ws[0]} is not supported: w^2 must be one of 4, 16, 64, 256")


class FlatShift:
    """The shifted block's roll by (-s, -s) + window partition (ref :364-378) and the reverse roll (:387-390) as ONE row permutation
    in tiled Z order, with the img_mask region label of every shifted position (ref :312-347).  Same interface as the HEALPix
    shifters: `tables(device)` -> (idx, inv, labels or None); the kernels gather through idx and scatter back through it."""

    def __init__(self, input_resolution, tile, window, shift, use_masking=True):
        self.input_resolution, self.tile, self.window, self.shift_size = tuple(input_resolution), tile, window, shift
        self.use_masking = use_masking
        Ht, Wt = self.input_resolution
        self._idx_np, self._inv_np, lab = _lib.build_flat_shift(Ht, Wt, tile, window, shift)
        self._labels_np = lab if use_masking else None
        self.shift_idcs = torch.from_numpy(self._idx_np.astype(np.int64))
        self.back_shift_idcs = torch.from_numpy(self._inv_np.astype(np.int64))
        self._dev = {}

    def tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(None if a is None else torch.from_numpy(a).to(device)
                                   for a in (self._idx_np, self._inv_np, self._labels_np))
        return self._dev[key]

    def get_mask(self):
        """The reference's dense [nW, w^2, w^2] attn_mask buffer (row-major windows and positions), or None without masking."""
        if not self.use_masking:
            return None
        Ht, Wt = self.input_resolution
        return torch.from_numpy(_lib.flat_attn_mask(Ht, Wt, self.window, self.shift_size))

    def shift(self, x):
        idx, inv, _ = self.tables(x.device)
        return ops.gather_rows(x, idx, inv, 0)

    def shift_back(self, x):
        idx, inv, _ = self.tables(x.device)
        return ops.gather_rows(x, inv, idx, 0)


class WindowAttention(hp.WindowAttention):
    """Window attention of a square w x w window (ref :78-217).  The reference's row-major `relative_position_index` buffer is kept
    for the state dict; the kernels read the same index with rows and columns in the in-window Z order."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0, use_cos_attn=False,
                 use_rel_pos_bias=True):
        ws = _pair(window_size)
        _check_window(ws, "window")
        super().__init__(dim, ws[0] * ws[1], num_heads, rel_pos_bias="flat", qkv_bias=qkv_bias, qk_scale=qk_scale,
                         attn_drop=attn_drop, proj_drop=proj_drop, use_cos_attn=use_cos_attn)
        self.use_rel_pos_bias = use_rel_pos_bias
        rm, z = _lib.flat_rel_pos_index(ws[0])
        self.relative_position_index = torch.from_numpy(rm)
        self._rel_idx32 = torch.from_numpy(z.astype(np.int32).reshape(-1))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)  # (the flat model initialises its table, ref :143)
        if not use_rel_pos_bias:  # the table stays a parameter and gets no gradient (ref :185-186)
            self.rel_pos_bias = None


class SwinTransformerBlock(hp.SwinTransformerBlock):
    """One (shifted-)window block on an H x W token grid in tiled Z order (ref :220-423).  `window_size` / `shift_size` hold the
    tokens per window and the shift of the HEALPix block (what its attention paths read); `window` / `shift` the reference's pairs."""

    def __init__(self, dim, input_resolution, num_heads, window_size=(4, 4), shift_size=-1, mlp_ratio=4.0, qkv_bias=True,
                 qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm, use_masking=True,
                 use_cos_attn=False, use_v2_norm_placement=False, use_rel_pos_bias=True, tile=None):
        nn.Module.__init__(self)
        ws = _pair(window_size)
        ss = [ws[0] // 2, ws[1] // 2] if shift_size == -1 else _pair(shift_size)
        H, W = input_resolution
        if H <= ws[0] or W <= ws[1]:  # one window over the whole grid, no shift (ref :272-278)
            ss, win = [0, 0], [H, W]
        else:
            win = list(ws)
        for i in range(2):
            assert 0 <= ss[i] < win[i], f"shift {ss[i]} must be in [0, window {win[i]}) in dimension {i}"
        _check_window(win, "window (after clamping to the resolution)")
        if ss[0] != ss[1]:
            # the reference rolls by shift[0] in both dimensions and back by (shift[0], shift[1]) (ref :365-390)
            raise NotImplementedError(f"shift {ss[0]} x {ss[1]} is not square: only equal shifts are supported")
        self.dim, self.input_resolution, self.num_heads, self.mlp_ratio = dim, tuple(input_resolution), num_heads, mlp_ratio
        self.use_v2_norm_placement = use_v2_norm_placement
        self.window, self.shift = win, ss
        self.window_size, self.shift_size = win[0] * win[1], ss[0]
        self.n_tokens = H * W
        tile = tile if tile is not None else win[0]
        # as in the reference the attention module is built with the UNclamped window (ref :290-300)
        self._build_branches(dim, WindowAttention(dim, ws, num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                                                  proj_drop=drop, use_cos_attn=use_cos_attn, use_rel_pos_bias=use_rel_pos_bias),
                             mlp_ratio, drop, drop_path, act_layer, norm_layer)
        self._set_shifter(FlatShift((H, W), tile, win[0], ss[0], use_masking) if ss[0] > 0 else hp_shifting.NoShift())

    def extra_repr(self):
        return (f"dim={self.dim}, input_resolution={self.input_resolution}, num_heads={self.num_heads}, "
                f"window_size={self.window}, shift_size={self.shift}, mlp_ratio={self.mlp_ratio}")


class PatchMerging(hp.PatchMerging):
    """2 x 2 tokens -> one (ref :426-473): in tiled Z order the reference's concat order x0, x1, x2, x3 is 4 consecutive tokens."""

    def __init__(self, input_resolution, dim, norm_layer=nn.LayerNorm):
        super().__init__(dim, dim_scale=2, norm_layer=norm_layer)
        self.input_resolution, self.patch_size = tuple(input_resolution), 4


class PatchExpand(nn.Module):
    """Linear(C -> 2C), each token -> 2 x 2 children of C/2, LayerNorm per child (ref :476-501).  The reference puts child (p1, p2)
    at channel block 2 p1 + p2; Z order wants p1 + 2 p2, so the product runs on the weight with blocks 1 and 2 exchanged (a row
    permutation inside the forward: the parameter and its gradient stay in the reference layout)."""

    def __init__(self, input_resolution, dim, dim_scale=2, norm_layer=nn.LayerNorm):
        super().__init__()
        self.input_resolution, self.dim = tuple(input_resolution), dim
        self.expand = HSLinear(dim, 2 * dim, bias=False) if dim_scale == 2 else nn.Identity()
        self.norm = _make_norm(norm_layer, dim // dim_scale)
        self.dim_scale = 4

    def forward(self, x):
        if isinstance(self.expand, nn.Identity):
            raise NotImplementedError("PatchExpand with dim_scale != 2")
        w = self.expand.weight
        n, k = w.shape
        wz = w.view(2, 2, n // 4, k).transpose(0, 1).reshape(n, k)  # block 2 p1 + p2 -> p1 + 2 p2
        x = ops.linear(x, wz)
        B, N, C = x.shape
        return self.norm(x.reshape(B, N * 4, C // 4))


class FinalPatchExpand_X4(hp.FinalPatchExpand_X4):
    """Linear(C -> p^2 C), p x p children per token, LayerNorm(C) (ref :504-535).  Child (p1, p2) is channel block p1 p + p2 as in the
    reference; the logits layout kernel puts it at pixel (p h + p1, p w + p2) (the reference's up_x4 view and permute)."""

    def __init__(self, input_resolution, patch_size, dim, norm_layer=nn.LayerNorm):
        ps = _pair(patch_size)
        super().__init__(ps[0] * ps[1], dim, norm_layer)
        self.input_resolution, self.patch_size, self.children_per_token = tuple(input_resolution), ps, ps[0] * ps[1]
        self.L = input_resolution[0] * input_resolution[1]

    def forward(self, x):
        x = self.expand(x)
        B, N, C = x.shape
        return self.norm(x.reshape(B, N * self.children_per_token, C // self.children_per_token))


class BasicLayer(hp._Stage):
    """Encoder stage: blocks + optional PatchMerging (ref :538-640)."""

    _resample = "downsample"

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, shift_size, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop=0.0, attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False,
                 use_masking=True, use_cos_attn=False, use_v2_norm_placement=False, use_rel_pos_bias=True, tile=None):
        super().__init__()
        self._build(SwinTransformerBlock, dim, tuple(input_resolution), depth, use_checkpoint, ([0, 0], shift_size), drop_path,
                    num_heads=num_heads, window_size=window_size, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop,
                    attn_drop=attn_drop, norm_layer=norm_layer, use_masking=use_masking, use_cos_attn=use_cos_attn,
                    use_v2_norm_placement=use_v2_norm_placement, use_rel_pos_bias=use_rel_pos_bias, tile=tile)
        self.downsample = downsample(input_resolution, dim=dim, norm_layer=norm_layer) if downsample is not None else None


class BasicLayer_up(hp._Stage):
    """Decoder stage: blocks + optional PatchExpand (ref :643-736)."""

    _resample = "upsample"

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, shift_size, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop=0.0, attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, upsample=None, use_checkpoint=False,
                 use_masking=True, use_cos_attn=False, use_v2_norm_placement=False, use_rel_pos_bias=True, tile=None):
        super().__init__()
        self._build(SwinTransformerBlock, dim, tuple(input_resolution), depth, use_checkpoint, ([0, 0], shift_size), drop_path,
                    num_heads=num_heads, window_size=window_size, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop,
                    attn_drop=attn_drop, norm_layer=norm_layer, use_masking=use_masking, use_cos_attn=use_cos_attn,
                    use_v2_norm_placement=use_v2_norm_placement, use_rel_pos_bias=use_rel_pos_bias, tile=tile)
        self.upsample = PatchExpand(input_resolution, dim=dim, dim_scale=2, norm_layer=norm_layer) if upsample is not None else None


class PatchEmbed(nn.Module):
    """p x p patches -> tokens (ref :739-793).  The Conv2d(k = s = p) parameters are kept; the image is laid out as patch rows in
    tiled Z order by one HIP kernel (features (c, kh, kw) as in the weight, zero-padded to a multiple of 8) and the conv is one
    Linear on them."""

    def __init__(self, config, data_spec, tile=None):
        super().__init__()
        self.config, self.data_spec = config, data_spec
        ps = _pair(config.patch_size)
        self.patches_resolution = [data_spec.dim_in[0] // ps[0], data_spec.dim_in[1] // ps[1]]
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.proj = nn.Conv2d(data_spec.f_in, config.embed_dim, kernel_size=ps, stride=ps)
        # reference quirk (:766-769): the config VALUE is stored, not an instance; only None is usable
        self.norm = config.patch_embed_norm_layer if config.patch_embed_norm_layer is not None else None
        self.tile = tile

    def forward(self, x, dtype=None):
        p = self.proj.kernel_size[0]
        if isinstance(x, PatchRows):  # the rows themselves (flat_data.FlatFrameTransform.frames(layout="rows")), checked by the model
            rows, C = x.rows, x.channels
        else:
            B, C, H, W = x.shape
            assert H == self.data_spec.dim_in[0] and W == self.data_spec.dim_in[1], \
                f"Input image size {H}*{W} doesn't match model ({self.data_spec.dim_in[0]}*{self.data_spec.dim_in[1]})."
            if dtype is None:
                dtype = x.dtype if x.dtype in (torch.float32, torch.bfloat16) else torch.float32
            rows = ops.flat_patch_rows(x, p, self.tile, dtype)  # B, N0, K (K = C p^2 padded to a multiple of 8)
        w = self.proj.weight.reshape(self.proj.weight.shape[0], C * p * p)
        pad = rows.shape[-1] - C * p * p
        if pad:
            w = F.pad(w, (0, pad))
        x = ops.linear(rows, w, self.proj.bias)
        return x if self.norm is None else self.norm(x)


@dataclass
class SwinTransformerConfig:
    """Same 23 fields and defaults as the reference config (ref :796-820)."""

    patch_size: Union[int, Tuple[int, int]] = (4, 4)
    window_size: Union[int, Tuple[int, int]] = (4, 4)
    shift_size: Union[int, Tuple[int, int]] = -1
    embed_dim: int = 96
    patch_embed_norm_layer: Optional[str] = None
    depths: List[int] = field(default_factory=lambda: [2, 2, 2, 2])
    num_heads: List[int] = field(default_factory=lambda: [3, 6, 12, 24])
    mlp_ratio: float = 4.0
    qkv_bias: bool = True
    qk_scale: Optional[float] = None
    use_cos_attn: bool = False
    drop_rate: float = 0.0
    attn_drop_rate: float = 0.0
    drop_path_rate: float = 0.1
    norm_layer: Literal[nn.LayerNorm] = nn.LayerNorm
    use_v2_norm_placement: bool = False
    ape: bool = False
    patch_norm: bool = True
    use_checkpoint: bool = False
    final_upsample: Literal["expand_first"] = "expand_first"
    use_masking: bool = True
    use_rel_pos_bias: bool = True
    dev_mode: bool = False


class SwinTransformerSys(hp.SwinHPTransformerSys):
    """Flat Swin-UNet: forward(x[B, f_in, H, W]) -> [B, f_out, H, W] fp32 logits (ref :823-1136).  Shares the HEALPix model's
    runtime machinery (compute dtype, bf16 parameter-cast cache, batched attention parameters) and its forward_seg_loss /
    forward_seg_step / forward_depth_loss / forward_depth_step, through the hooks _seg_labels, _depth_target, _as_image and _batch
    (the callers: models_lightning/segmentation/model_lightning_swin.py, training/loss_depth_regression.py).  Here labels are
    [B, H, W] integer class ids and target [B, H, W] depths -- or the flat_data.PixelRows FlatFrameTransform.masks / .depth(layout=
    "rows") made, x then usually being the PatchRows of .frames(layout="rows") -- and a step's preds come back as images: uint8
    [B, H, W] = self(x).argmax(1), fp32 [B, f_out, H, W] = self(x) with channel 0 in metres.  Neither the weighted / masked mean of
    a loss nor the confusion counts and metric sums depend on the pixel order (median_std is the median over the sample's pixels in
    either order), so in bf16 training the NCHW logits and the head rows are never written."""

    def __init__(self, config: SwinTransformerConfig, data_spec: DataSpec, **kwargs):
        nn.Module.__init__(self)
        self.config, self.data_spec = config, data_spec
        L = self.num_layers = len(config.depths)
        self.num_features = int(config.embed_dim * 2 ** (L - 1))
        self.num_features_up = int(config.embed_dim * 2)
        self.compute_dtype = kwargs.pop("compute_dtype", None)  # None: follow autocast, else the input dtype

        H, W = data_spec.dim_in[0], data_spec.dim_in[1]
        config.patch_size = _pair(config.patch_size)  # (the reference normalises the config in place, :862-876)
        config.window_size = _pair(config.window_size)
        ph, pw = config.patch_size
        wh, ww = config.window_size
        mf = 2 ** (L - 1)
        assert (H / (mf * ph * wh)) % 1 == 0, f"H={H} must be divisible by merge_factor*patch_height*window_height={mf}*{ph}*{wh}"
        assert (W / (mf * pw * ww)) % 1 == 0, f"W={W} must be divisible by merge_factor*patch_width*window_width={mf}*{pw}*{ww}"
        assert (H * W / (mf ** 2 * ph * pw)) % 1 == 0, f"H*W={H * W} must be divisible by merge_factor**2*patch_height*patch_width"
        if config.shift_size == -1:
            self.shift_size = (wh // 2, ww // 2)
        else:
            if isinstance(config.shift_size, int):
                config.shift_size = [config.shift_size, config.shift_size]
            self.shift_size = config.shift_size
        if ph != pw:
            raise NotImplementedError(f"patch {ph} x {pw} is not square: only square patches are supported")
        _check_window(config.window_size, "window")
        if self.shift_size[0] != self.shift_size[1]:
            raise NotImplementedError(f"shift {self.shift_size[0]} x {self.shift_size[1]} is not square: only equal shifts are supported")
        if config.final_upsample != "expand_first":
            raise NotImplementedError(f"final_upsample={config.final_upsample!r}: only 'expand_first' is supported")
        self.tile = wh * mf  # side of the Z-order tiles at stage 0 (a window at the last stage)
        self._image_layout = (H, W, ph, self.tile)  # what the layout kernels between image and pixel rows take

        self.patch_embed = PatchEmbed(config, data_spec=data_spec, tile=self.tile)
        num_patches = self.patch_embed.num_patches
        res = self.patches_resolution = self.patch_embed.patches_resolution
        if config.ape:
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, num_patches, config.embed_dim))
            nn.init.trunc_normal_(self.absolute_pos_embed, std=0.02)
            z_of_rm, rm_of_z = _lib.flat_zorder(res[0], res[1], self.tile)
            self._ape_np = (rm_of_z, z_of_rm)
            self._ape_dev = {}
        self.pos_drop = nn.Dropout(p=config.drop_rate)
        dpr = [v.item() for v in torch.linspace(0, config.drop_path_rate, sum(config.depths))]  # ref :936-938

        common = dict(window_size=config.window_size, shift_size=self.shift_size, mlp_ratio=config.mlp_ratio,
                      qkv_bias=config.qkv_bias, qk_scale=config.qk_scale, use_cos_attn=config.use_cos_attn, drop=config.drop_rate,
                      attn_drop=config.attn_drop_rate, norm_layer=config.norm_layer,
                      use_v2_norm_placement=config.use_v2_norm_placement, use_checkpoint=config.use_checkpoint,
                      use_masking=config.use_masking, use_rel_pos_bias=config.use_rel_pos_bias)
        self.layers = nn.ModuleList()
        for i in range(L):
            lo, hi = sum(config.depths[:i]), sum(config.depths[:i + 1])
            self.layers.append(BasicLayer(dim=int(config.embed_dim * 2 ** i), input_resolution=(res[0] // 2 ** i, res[1] // 2 ** i),
                                          depth=config.depths[i], num_heads=config.num_heads[i], drop_path=dpr[lo:hi],
                                          downsample=PatchMerging if i < L - 1 else None, tile=self.tile // 2 ** i, **common))
        self.layers_up = nn.ModuleList()
        self.concat_back_dim = nn.ModuleList()
        for i in range(L):
            down = L - 1 - i
            width, r = int(config.embed_dim * 2 ** down), (res[0] // 2 ** down, res[1] // 2 ** down)
            if i == 0:
                layer_up = PatchExpand(input_resolution=r, dim=width, dim_scale=2, norm_layer=config.norm_layer)
            else:
                lo, hi = sum(config.depths[:down]), sum(config.depths[:down + 1])
                layer_up = BasicLayer_up(dim=width, input_resolution=r, depth=config.depths[down], num_heads=config.num_heads[down],
                                         drop_path=dpr[lo:hi], upsample=PatchExpand if i < L - 1 else None, tile=self.tile // 2 ** down,
                                         **common)
            self.layers_up.append(layer_up)
            self.concat_back_dim.append(HSLinear(2 * width, width) if i > 0 else nn.Identity())
        if ops.COMP_RESIDUAL_LAST_STAGE and isinstance(self.layers_up[-1], BasicLayer_up):
            self.layers_up[-1].comp_residual = True  # as the HEALPix decoder's last stage (UnetDecoder)
        self.norm = _make_norm(config.norm_layer, self.num_features)
        self.norm_up = _make_norm(config.norm_layer, config.embed_dim)
        self.up = FinalPatchExpand_X4(input_resolution=(H // ph, W // pw), patch_size=config.patch_size, dim=config.embed_dim)
        self.output = nn.Conv2d(in_channels=config.embed_dim, out_channels=data_spec.f_out, kernel_size=1, bias=False)
        self.apply(self._init_weights)

    def _ape(self, device):
        key = str(device)
        if key not in self._ape_dev:
            self._ape_dev[key] = tuple(torch.from_numpy(a).to(device) for a in self._ape_np)
        return self._ape_dev[key]

    def forward_features(self, x, dtype=None):
        x = self.patch_embed(x, dtype)  # B, N0, C in tiled Z order
        if self.config.ape:  # the row-major embedding through the Z permutation (HIP row gather; its backward scatters back)
            rm_of_z, z_of_rm = self._ape(x.device)
            x = x + ops.gather_rows(self.absolute_pos_embed, rm_of_z, z_of_rm).to(x.dtype)
        x = self.pos_drop(x)
        x_downsample = []
        for k, layer in enumerate(self.layers):
            x_downsample.append(x)  # the INPUT of encoder stage k is the skip tensor (ref :1074-1076)
            x = layer(x)
            if self.config.dev_mode:
                print(f"forward_features after layer {k}: {x.size()}")
        return self.norm(x), x_downsample

    forward_up_features = hp.UnetDecoder.forward_up_features  # (ref :1093-1094: the same loop over this model's own layers_up)

    def _run(self, x, task=None):
        self._require_device(x)
        dt = self._activation_dtype(x)
        if isinstance(x, PatchRows):  # (before the scope: its _param_casts counts the forward, ops.note_forward)
            x.check_model(self)
            if x.dtype != dt:
                raise TypeError(f"the patch rows are {x.dtype}, the model computes in {dt}: make them with frames(x, dtype={dt})")
        with self._run_scope(dt):
            x, x_downsample = self.forward_features(x, dt)
            x = self.forward_up_features(x, x_downsample)
            return hp.decoder_tail(self.norm_up, self.up, self.output.weight, self.up.children_per_token, x, task)

    def forward(self, x):
        rows = self._run(x)  # B, Npix, f_out logits rows (children of a token consecutive)
        return ops.flat_pixel_image(rows.float(), *self._image_layout)

    def forward_rows(self, x):
        """The head rows forward() lays out as NCHW, as the decoder tail leaves them: [B, H * W, f_out] fp32 (the padded rows
        viewed in place), row = token * p^2 + kh * p + kw with the tokens in tiled Z order.  For consumers that read pixels
        through a table anyway (flat_evaluation.FlatToHPProjector.for_model / FlatCoverage.for_model: scoring on the sphere),
        so that the NCHW tensor is never written; ops.flat_pixel_image(rows, H, W, p, self.tile) is forward(x)."""
        return self._run(x)

    def _batch(self, x):
        return x.batch if isinstance(x, PatchRows) else x.shape[0]

    def _as_image(self, preds):
        """A step's predictions in the rows' pixel order, laid out as images by a HIP kernel: class ids uint8 [B, H * W] -> [B, H, W];
        fp32 [B, f_out, H * W] (any strides) -> [B, f_out, H, W], one channel at a time."""
        if preds is None:
            return None
        if preds.dtype == torch.uint8:
            return ops.flat_label_image(preds.contiguous(), *self._image_layout)
        return torch.cat([ops.flat_pixel_image(preds[:, c].contiguous().unsqueeze(2), *self._image_layout) for c in range(preds.shape[1])], 1)

    def _seg_labels(self, x, labels):
        """uint8 labels [B, H * W] in the logits rows' pixel order, on x's device, laid out by a HIP kernel (ids outside [0, 254]
        become 255, ignored)."""
        self._require_device(x)
        if self.data_spec.f_out > 255:
            raise NotImplementedError("the flat model's segmentation loss and step support at most 255 classes")
        if isinstance(labels, PixelRows):
            return self._pixel_rows(labels, x, torch.uint8, "labels")
        if labels.dtype not in (torch.uint8, torch.int32, torch.int64):
            labels = labels.long()
        return ops.flat_labels(labels.to(x.device), *self._image_layout[2:])

    def _depth_target(self, x, target):
        """The fp32 target [B, H * W] in the head rows' pixel order, on x's device, laid out by a HIP kernel (fp32 copied bit for bit:
        infinite and NaN depths survive)."""
        self._require_device(x)
        if isinstance(target, PixelRows):
            return self._pixel_rows(target, x, torch.float32, "target")
        assert tuple(target.shape) == (self._batch(x),) + tuple(self.data_spec.dim_in[:2]), "target [B, H, W]"
        return ops.flat_depth_target(target.to(device=x.device, dtype=torch.float32), *self._image_layout[2:])

    def _pixel_rows(self, rows, x, dtype, what):
        """The tensor of a PixelRows built for this model, on x's device, one row set per sample of x."""
        t = rows.check_model(self)
        if t.dtype != dtype or t.device != x.device or t.shape[0] != self._batch(x):
            raise ValueError(f"{what} rows must be {dtype} [{self._batch(x)}, H * W] on {x.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t
