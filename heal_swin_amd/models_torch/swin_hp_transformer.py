"""HEAL-SWIN-UNet on the MI355X-native hot path.

Keeps the public surface of the reference module `heal_swin/models_torch/swin_hp_transformer.py`
(class names, constructor signatures, attribute paths and therefore state-dict keys, `forward`
contracts) so that it can stand in for it under the reference's Lightning modules, while the
computation is organised differently:

  * per block there is ONE attention kernel call: shift -> window partition -> attention -> window reverse
    -> shift back are fused into `hs_window_attn_fwd/bwd`, which gathers rows of the un-shifted qkv tensor
    through the shifter's int32 table and scatters its output rows back through the same table
    (row permutations commute with the row-wise LayerNorm / Linear layers around it);
  * masks are per-pixel uint8 region labels, not [nW, Ws, Ws] tensors; the reference's `attn_mask` buffer
    only exists in `state_dict()` / is accepted by `load_state_dict()`;
  * all LayerNorms (block norms, PatchMerging's LN(4C) over 4 sibling pixels, PatchExpand's LN over each
    child row) run in the HIP row-LayerNorm kernel, with the v2-placement residual add fused in;
  * activations run in `compute_dtype` (fp32 or bf16; fp32 statistics/softmax/accumulation either way),
    parameters stay fp32.

Reference line numbers in comments refer to heal_swin/models_torch/swin_hp_transformer.py.
"""
import math
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import List, Literal, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint

from .. import _lib, ops
from ..data_spec import DataSpec
from . import hp_shifting

EMIT_REFERENCE_BUFFERS = True  # state_dict() carries the reference's `attn_mask` buffers (ref :306-308)


# ----------------------------------------------------------------------------- leaf layers
class HSLayerNorm(nn.LayerNorm):
    """nn.LayerNorm parameters, HIP kernel arithmetic (`hs_layernorm_fwd/bwd`)."""

    def forward(self, x, residual=None, row_scale=None, drop_p=0.0):
        assert self.elementwise_affine and len(self.normalized_shape) == 1 and abs(self.eps - 1e-5) < 1e-12
        return ops.layer_norm(x, self.weight, self.bias, residual, row_scale=row_scale, drop_p=drop_p)


def _make_norm(norm_layer, dim):
    return HSLayerNorm(dim) if norm_layer is nn.LayerNorm else norm_layer(dim)


class HSLinear(nn.Linear):
    """fp32 master weights; forward and input-gradient GEMMs in the activation dtype (library GEMM), weight and bias
    gradients by the HIP split-token kernel `hs_linear_wgrad` (ops.LinearFn)."""

    def forward(self, x):
        return ops.linear(x, self.weight, self.bias)

    def forward_passthrough(self, x):
        """(self(x), alias of x for a residual connection around the branch): see ops.LinearFn."""
        return ops.linear_passthrough(x, self.weight, self.bias)

    def forward_residual(self, x, residual):
        """self(x) + residual with the add in the product's epilogue."""
        return ops.linear_residual(x, self.weight, self.bias, residual)


class DropPath(nn.Module):
    """Stochastic depth per sample (the reference imports timm's; identity when p == 0 or in eval)."""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def sample_scale(self, batch, device):
        """Per-sample factor (0 or 1/keep) of one application, or None when inactive; the fused kernels take it as a [B] vector."""
        if self.drop_prob == 0.0 or not self.training:
            return None
        keep = 1.0 - self.drop_prob
        return torch.empty(batch, dtype=torch.float32, device=device).bernoulli_(keep).div_(keep)

    def forward(self, x):
        rs = self.sample_scale(x.shape[0], x.device)
        if rs is None:
            return x
        return x * rs.to(x.dtype).view((x.shape[0],) + (1,) * (x.dim() - 1))


def _exact_gelu(act):
    """The erf GELU the Mlp kernels compute (ops.mlp, ops.fused_mlp_block)?"""
    return isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "none"


class Mlp(nn.Module):
    """fc1 -> GELU(erf) -> drop -> fc2 -> drop (ref :21-44)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        self.fc1 = HSLinear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = HSLinear(hidden_features or in_features, out_features or in_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x, apply_out_drop=True, residual_alias=False, residual=None):
        """residual_alias: also return an alias of x whose gradient is folded into fc1's input-gradient GEMM.
        residual: added to the output inside fc2's epilogue (ops.RESID_EPILOGUE path; no output dropout then)."""
        if _exact_gelu(self.act) and x.dtype in (torch.bfloat16, torch.float32) and x.is_cuda:
            # one autograd node: GELU (+ hidden dropout) ride on the GEMM epilogues, masks regenerated in backward (ops.MlpFn)
            out = ops.mlp(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias,
                          drop_p=self.drop.p if self.training else 0.0, passthrough=residual_alias, residual=residual)
            y, x_res = out if residual_alias else (out, None)
        elif residual is not None:
            return self.fc2(self.drop(self.act(self.fc1(x)))) + residual
        else:
            x_res = None
            if residual_alias:
                h, x_res = self.fc1.forward_passthrough(x)
            else:
                h = self.fc1(x)
            y = self.fc2(self.drop(self.act(h)))
        y = self.drop(y) if apply_out_drop else y  # the caller fuses the output dropout into the next norm kernel
        return (y, x_res) if residual_alias else y


# ----------------------------------------------------------------------------- attention
def _labels_from_dense_mask(mask):
    """Recover per-position region labels from a {0, x} [nW, Ws, Ws] mask built by get_attn_mask_from_mask."""
    m = mask.detach().cpu()
    nW, Ws, _ = m.shape
    same = m == 0
    labels = same.to(torch.uint8).argmax(dim=2).to(torch.uint8)  # first position in the same region
    rebuilt = (labels[:, :, None] != labels[:, None, :]).to(m.dtype) * (-100)
    if not torch.equal(rebuilt.to(torch.float32), m.to(torch.float32)):
        raise NotImplementedError("WindowAttention mask is not a {0,-100} region mask; dense masks are not supported")
    return labels.reshape(-1).contiguous()


class WindowAttention(nn.Module):
    """Window multi-head self-attention with relative position bias (ref :47-174)."""

    def __init__(self, dim, window_size, num_heads, rel_pos_bias=None, qkv_bias=True, qk_scale=None,
                 attn_drop=0.0, proj_drop=0.0, use_cos_attn=False):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        self.use_cos_attn = use_cos_attn
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.rel_pos_bias = rel_pos_bias
        if use_cos_attn:  # ref :84-87
            self.logit_scale = nn.Parameter(torch.log(10 * torch.ones((num_heads, 1, 1))), requires_grad=True)
        if rel_pos_bias == "flat":  # ref :89-114; the table starts at zero (:92-96, :121)
            side = int(round(window_size ** 0.5))
            self.relative_position_bias_table = nn.Parameter(torch.zeros(((2 * side - 1) ** 2, num_heads)))
            rel = _lib.rel_pos_index(window_size)
            self.register_buffer("relative_position_index", torch.from_numpy(rel))
            self.register_buffer("_rel_idx32", torch.from_numpy(rel.astype(np.int32).reshape(-1)), persistent=False)
        self._scale_cache = None  # constant per-head scale tensor of the non-cosine variant, built once per device
        self.qkv = HSLinear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = HSLinear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def extra_repr(self):
        return f"dim={self.dim}, window_size={self.window_size}, num_heads={self.num_heads}"

    def head_scale(self):
        """Per-head multiplier of the raw scores: exp(min(logit_scale, ln 100)) (ref :144-147) or the qk scale."""
        if self.use_cos_attn:
            now = self.__dict__.get("_scale_now")  # made for all blocks at once by the model's forward (SwinHPTransformerSys._prefetch_attn_params)
            if now is not None:
                return now
            if self.logit_scale.is_cuda and self.logit_scale.dtype == torch.float32:
                return ops.cos_head_scale(self.logit_scale)  # one launch forward, one backward
            return torch.exp(torch.clamp(self.logit_scale, max=math.log(1.0 / 0.01))).reshape(-1)
        dev = self.qkv.weight.device
        if self._scale_cache is None or self._scale_cache.device != dev:
            self._scale_cache = torch.full((self.num_heads,), float(self.scale), dtype=torch.float32, device=dev)
        return self._scale_cache

    def bias(self):
        if self.rel_pos_bias is None:
            return None
        now = self.__dict__.get("_bias_now")  # made for all blocks at once by the model's forward
        if now is not None:
            return now
        return ops.RelPosBiasFn.apply(self.relative_position_bias_table, self._rel_idx32, self.window_size)

    def attend(self, x, window_size, idx, roll, labels, apply_proj_drop=True, residual_alias=False, residual=None):
        """x: [B, N, C] in natural order -> attention branch output [B, N, C] in natural order
        (residual_alias: also an alias of x whose gradient is folded into the qkv input-gradient GEMM)."""
        drop = self.attn_drop.p if self.training else 0.0  # dropout on the attention probabilities (ref :169), in-kernel
        if self.rel_pos_bias is not None and window_size != self.window_size:
            raise AssertionError("relative position bias needs input_resolution >= window_size")  # ref quirk :243-251
        x_res = None
        if self.fusable(x, window_size):
            # no-grad forward of a stage whose qkv weights fit the LDS: qkv -> attention -> proj in ONE kernel
            y = self.fused_module(x, window_size, idx, roll, labels)
            return (y, x) if residual_alias else y
        if residual is None and self.trainable_fused(x, window_size):
            # training forward of a stage whose qkv weights fit the LDS, branch without a norm in front (v2 placement): qkv ->
            # attention -> proj in ONE launch that also writes what the backward reads (ops.window_attn_module_train)
            return ops.window_attn_module_train(x, None, None, *self._module_args(window_size, idx, roll, labels),
                                                residual_alias=residual_alias)
        if residual_alias:
            qkv, x_res = self.qkv.forward_passthrough(x)
        else:
            qkv = self.qkv(x)
        o = ops.window_attn_core(qkv, *self._core_args(window_size, idx, roll, labels), attn_drop=drop)
        if residual is not None:  # x + proj(o) from the proj product's epilogue (ops.RESID_EPILOGUE; no proj dropout on this path)
            return self.proj.forward_residual(o, residual)
        y = self.proj(o)
        y = self.proj_drop(y) if apply_proj_drop else y  # the caller fuses proj_drop into the next norm kernel
        return (y, x_res) if residual_alias else y

    def _core_args(self, window_size, idx, roll, labels):
        """What ops.window_attn_core takes behind qkv: bias, score scale, the shift and the shape."""
        return self.bias(), self.head_scale(), idx, roll, labels, self.num_heads, window_size, self.use_cos_attn

    def _module_args(self, window_size, idx, roll, labels):
        """What both module kernels take behind x (and the norm in front): the two Linears' parameters, then the core's arguments."""
        return (self.qkv.weight, self.qkv.bias, self.proj.weight, self.proj.bias) + self._core_args(window_size, idx, roll, labels)

    def _module_fits(self, window_size):
        """What both forms of the module kernel ask beside their own ops.*_ok: nothing stochastic inside the branch, the bias table's window."""
        return (not (self.training and (self.attn_drop.p > 0 or self.proj_drop.p > 0)) and
                (self.rel_pos_bias is None or window_size == self.window_size))

    def fusable(self, x, window_size):
        """The one-launch inference kernel applies: no gradient wanted, supported shape, nothing stochastic switched on."""
        return ops.window_attn_module_ok(x, self.num_heads, window_size) and self._module_fits(window_size)

    def fused_module(self, x, window_size, idx, roll, labels, norm=None, residual=False):
        """[x +] proj(attention(qkv([norm](x)))) by `hs_window_attn_module_fwd` (inference only; ops.window_attn_module_ok)."""
        return ops.window_attn_module(x, *self._module_args(window_size, idx, roll, labels),
                                      ln_weight=None if norm is None else norm.weight, ln_bias=None if norm is None else norm.bias,
                                      residual=residual)

    def trainable_fused(self, x, window_size):
        """The one-launch TRAINING form applies (ops.window_attn_module_train_ok): gradients wanted, supported shape, nothing
        stochastic inside the branch."""
        return ops.window_attn_module_train_ok(x, self.num_heads, window_size) and self._module_fits(window_size)

    def fused_module_train(self, x, window_size, idx, roll, labels, norm, norm2=None):
        """x + proj(attention(qkv(norm(x)))) by `hs_window_attn_module_fwd_train`, differentiable (ops.window_attn_module_train);
        with norm2 the same launch also applies the block's second LayerNorm: returns (norm2(x1), x1)."""
        return ops.window_attn_module_train(x, norm.weight, norm.bias, *self._module_args(window_size, idx, roll, labels),
                                            norm2=None if norm2 is None else (norm2.weight, norm2.bias))

    def forward(self, x, mask=None):
        """Reference-compatible entry: x [num_windows*B, Ws, C], mask [nW, Ws, Ws] in {0,-100} or None."""
        B_, Ws, C = x.shape
        if mask is None:
            return self.attend(x.reshape(1, B_ * Ws, C), Ws, None, 0, None).reshape(B_, Ws, C)
        nW = mask.shape[0]
        labels = _labels_from_dense_mask(mask).to(x.device)
        return self.attend(x.reshape(B_ // nW, nW * Ws, C), Ws, None, 0, labels).reshape(B_, Ws, C)


class SwinTransformerBlock(nn.Module):
    """One (shifted-)window block (ref :193-340)."""

    def __init__(self, dim, input_resolution, base_pix, num_heads, window_size=4, shift_size=0, shift_strategy="nest_roll",
                 rel_pos_bias=None, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, use_v2_norm_placement=False, use_cos_attn=False):
        super().__init__()
        self.dim, self.input_resolution, self.num_heads = dim, input_resolution, num_heads
        self.window_size, self.shift_size, self.mlp_ratio = window_size, shift_size, mlp_ratio
        self.use_v2_norm_placement = use_v2_norm_placement
        self.n_tokens = input_resolution
        if input_resolution <= window_size:  # a single window: no partition, no shift (ref :243-246)
            self.shift_size, self.window_size = 0, input_resolution

        # as in the reference the attention module is built with the UNclamped window_size (ref :249-251)
        self._build_branches(dim, WindowAttention(dim, window_size=window_size, num_heads=num_heads, rel_pos_bias=rel_pos_bias,
                                                  qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop,
                                                  use_cos_attn=use_cos_attn),
                             mlp_ratio, drop, drop_path, act_layer, norm_layer)

        nside = math.sqrt(input_resolution // base_pix)
        assert nside % 1 == 0, "nside has to be an integer in every layer"
        nside = int(nside)
        if self.shift_size > 0:
            if shift_strategy == "nest_roll":
                shifter = hp_shifting.NestRollShift(self.shift_size, self.input_resolution, self.window_size)
            elif shift_strategy == "nest_grid_shift":
                shifter = hp_shifting.NestGridShift(nside, base_pix, self.window_size)
            elif shift_strategy == "ring_shift":
                shifter = hp_shifting.RingShift(nside, base_pix, self.window_size, self.shift_size)
            else:
                raise KeyError(shift_strategy)
        else:
            shifter = hp_shifting.NoShift()
        self._set_shifter(shifter)

    def _build_branches(self, dim, attn, mlp_ratio, drop, drop_path, act_layer, norm_layer):
        """norm1, attn, drop_path, norm2, mlp -- in the reference's registration order (state-dict key order)."""
        self.norm1 = _make_norm(norm_layer, dim)
        self.attn = attn
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = _make_norm(norm_layer, dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def _set_shifter(self, shifter):
        """The shift of a shifted block: any object with `tables(device)` -> (idx int32, inv int32, labels uint8 or None) and
        `get_mask()` (the reference's dense mask or None); NoShift for the others."""
        self.shifter = shifter
        self._is_roll = isinstance(self.shifter, hp_shifting.NestRollShift)
        self._shifted = self.shift_size > 0

        # reference keeps a dense [nW, Ws, Ws] `attn_mask` buffer in the state dict (:306-308); here it is
        # virtual: emitted by state_dict(), accepted (and dropped) by load_state_dict().
        self.register_buffer("attn_mask", None)
        self._register_state_dict_hook(SwinTransformerBlock._emit_attn_mask)
        self._register_load_state_dict_pre_hook(self._accept_attn_mask, with_module=False)

    @staticmethod
    def _emit_attn_mask(module, state_dict, prefix, local_metadata):
        if EMIT_REFERENCE_BUFFERS and module._shifted:
            mask = module.shifter.get_mask()
            if mask is not None:  # (a flat block without masking has none)
                state_dict[prefix + "attn_mask"] = mask

    def _accept_attn_mask(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        state_dict.pop(prefix + "attn_mask", None)

    def extra_repr(self):
        return (f"dim={self.dim}, input_resolution={self.input_resolution}, num_heads={self.num_heads}, "
                f"window_size={self.window_size}, shift_size={self.shift_size}, mlp_ratio={self.mlp_ratio}")

    def _shift_args(self, x):
        """(idx, roll, labels) of the block's shift as the attention kernels take it."""
        if not self._shifted:
            return None, 0, None
        idx, _, labels = self.shifter.tables(x.device)
        if self._is_roll:  # modular offset instead of a table
            return None, self.shift_size % x.shape[1], labels
        return idx, 0, labels

    def _attention_branch(self, x, apply_proj_drop=True, residual_alias=False, residual=None):
        return self.attn.attend(x, self.window_size, *self._shift_args(x), apply_proj_drop, residual_alias, residual)

    def _stochastic(self):
        """Any dropout / DropPath on the two residual branches active right now?"""
        return self.training and ((isinstance(self.drop_path, DropPath) and self.drop_path.drop_prob > 0) or
                                  self.attn.proj_drop.p > 0 or self.mlp.drop.p > 0)

    def _hs_norms(self):
        return isinstance(self.norm1, HSLayerNorm) and isinstance(self.norm2, HSLayerNorm)

    def _path_scale(self, x):
        """per-sample DropPath factor of one branch ([B] tensor) or None"""
        return self.drop_path.sample_scale(x.shape[0], x.device) if isinstance(self.drop_path, DropPath) else None

    def _fused_mlp(self, x1, post_norm=False):
        """x1 + mlp(norm2(x1)) -- post_norm (v2 placement): x1 + norm2(mlp(x1)) -- by the one-launch Mlp block kernel
        (ops.fused_mlp_block) where it applies: HIP norms, exact GELU, hidden = 4 C at C = 96 / 128, nothing stochastic on the
        branch; else None."""
        m = self.mlp
        if not (isinstance(self.norm2, HSLayerNorm) and isinstance(m.fc1, HSLinear) and isinstance(m.fc2, HSLinear) and
                _exact_gelu(m.act) and ops.fused_mlp_ok(x1, m.fc1.weight.shape[0]) and m.fc2.weight.shape[0] == self.dim):
            return None
        rs = self._path_scale(x1) if self.training else None
        dp = m.drop.p if self.training else 0.0
        # with either: Mlp.drop (both sites) and DropPath inside the launch, which the kernel has for the v2 placement
        if (rs is None and not dp) or ops.fused_mlp_stochastic_ok(x1, post_norm):
            return ops.fused_mlp_block(x1, self.norm2.weight, self.norm2.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias,
                                       post_norm=post_norm, row_scale=rs, drop_p=dp)
        return None

    def placement(self):
        """Where the block's norms sit and how its residual adds are made -- the one rule forward() and the stages' block loop go by:
        "v1" (norm in front of the branch, HIP norms): both adds deferred into the LayerNorm kernel that consumes the sum, or into
        a product's epilogue (forward_deferred); "v2" (norm behind the branch, HIP norms): the two `x + norm(branch)` results are the
        residual stream itself (forward_stream_v2 where the stream is compensated); None: foreign norm layers, the plain composition."""
        if not self._hs_norms():
            return None
        return "v2" if self.use_v2_norm_placement else "v1"

    def can_defer(self):
        """v1 placement with the HIP norms: both residual adds -- together with the dropout / DropPath on the added branch --
        ride on the LayerNorm kernel that consumes the sum."""
        return self.placement() == "v1"

    def forward_deferred(self, x, pending, x_lo=None, comp=None):
        """v1 block on the input `x (+ x_lo) + rs*drop(p)` for pending = (p, rs, drop_p) (or None); returns (x1, pending', x1_lo)
        with the block output = x1 (+ x1_lo) + rs'*drop(m) (ref :337-338 and :316 of the next block).  x_lo / x1_lo are the
        rounding remainders of the compensated residual stream (bf16 runs; None when off or not yet started)."""
        comp = (ops.COMP_RESIDUAL if comp is None else comp) and x.dtype == torch.bfloat16
        if self.attn.fusable(x, self.window_size) and not self._stochastic():
            # no-grad forward: x1 = xs + proj(attn(qkv(norm1(xs)))) is ONE launch (norm1 as the kernel's prologue, the
            # residual add as its epilogue), xs = x + previous block's MLP branch
            xs = self.resolve_pending(x, pending)
            x1 = self.attn.fused_module(xs, self.window_size, *self._shift_args(xs), norm=self.norm1, residual=True)
            return self._mlp_half(x1, alias=False)
        sites = self._resid_sites(x, x_lo, comp)
        if sites is not None and pending is None and self.attn.trainable_fused(x, self.window_size):
            # norm1 -> qkv -> attention -> proj -> residual add in ONE launch that also writes what the backward reads ... and, with
            # ops.FUSED_NORM2, the block's norm2 on the sum it has just formed
            out = self.attn.fused_module_train(x, self.window_size, *self._shift_args(x), self.norm1,
                                               norm2=self.norm2 if ops.FUSED_NORM2 else None)
            n2, x1 = out if ops.FUSED_NORM2 else (None, out)
            return self._mlp_half(x1, n2, sites[1])
        proj_site, fc2_site = sites or (None, None)
        xs, n1, xs_lo = self._norm1_step(x, pending, x_lo, comp)
        x1, n2, x1_lo = self._attention_half(xs, n1, proj_site, xs_lo, comp)
        return self._mlp_half(x1, n2, fc2_site, x1_lo)

    def _resid_sites(self, x, x_lo, comp):
        """(proj's, fc2's) ops.resid_site -- a residual add leaves its branch's last product's epilogue where that product runs on
        hs_gemm_nt anyway (the HBM-bound shapes of stages 0-1) and, fc2's, where it runs in the library (long K: stages 1-3); the
        norm behind it is then a plain LayerNorm whose second output is an alias of its input (the alias' gradient is added inside
        the LayerNorm backward kernel) -- or None where both adds stay in the norm kernels whatever the shapes: ops.RESID_EPILOGUE
        off, not bf16, a compensated stream, or dropout / DropPath on the branches, which only the norm kernel applies with the add."""
        if not (ops.RESID_EPILOGUE and x.dtype == torch.bfloat16 and not comp and x_lo is None and not self._stochastic()):
            return None
        C, rows = self.dim, x.numel() // self.dim
        return (ops.resid_site(C, C, x.dtype, m=rows, lib=False),
                ops.resid_site(C, self.mlp.fc1.weight.shape[0], x.dtype, m=rows))

    def _norm1_step(self, x, pending, x_lo=None, comp=False):
        """(xs, norm1(xs), xs_lo) for xs (+ xs_lo) = x (+ x_lo) + rs*drop(p), pending = (p, rs, drop_p) or None (xs is x)."""
        if pending is None:  # x feeds norm1 AND the residual add behind the branch: the alias keeps the two gradients in one kernel
            n1, xs = ops.layer_norm_passthrough(x, self.norm1.weight, self.norm1.bias)
            return xs, n1, x_lo
        t, rs, dp = pending
        if comp:
            return ops.add_layer_norm_stream(x, x_lo, t, self.norm1.weight, self.norm1.bias, row_scale=rs, drop_p=dp)
        xs, n1 = ops.add_layer_norm(x, t, self.norm1.weight, self.norm1.bias, row_scale=rs, drop_p=dp)
        return xs, n1, x_lo

    def _attention_half(self, xs, n1, site=None, xs_lo=None, comp=False):
        """(x1, n2, x1_lo) for x1 (+ x1_lo) = xs (+ xs_lo) + rs*drop(attention branch of n1): the add in proj's epilogue (site; n2 is
        then None, norm2 is the Mlp half's business), else in the norm2 kernel, which applies proj_drop and DropPath with it."""
        if site is not None:
            return self._attention_branch(n1, apply_proj_drop=False, residual=xs), None, None
        a = self._attention_branch(n1, apply_proj_drop=False)
        rs, dp = self._path_scale(xs), self.attn.proj_drop.p if self.training else 0.0
        if comp:
            return ops.add_layer_norm_stream(xs, xs_lo, a, self.norm2.weight, self.norm2.bias, row_scale=rs, drop_p=dp)
        x1, n2 = ops.add_layer_norm(xs, a, self.norm2.weight, self.norm2.bias, row_scale=rs, drop_p=dp)
        return x1, n2, None

    def _mlp_half(self, x1, n2=None, site=None, x1_lo=None, alias=True):
        """The v1 block's second half on x1 (+ x1_lo), n2 = norm2(x1) where the step before has made it: (x2, None, None) where the
        add rides in a launch of this block -- the fused Mlp block (norm2 -> fc1 -> GELU -> fc2 -> add in one), or fc2's epilogue
        (site) -- else (x1, the pending Mlp branch, x1_lo).  alias=False (the no-grad module path): norm2 as a plain LayerNorm."""
        if n2 is None:
            x2 = self._fused_mlp(x1)
            if x2 is not None:
                return x2, None, None
            n2, x1 = ops.layer_norm_passthrough(x1, self.norm2.weight, self.norm2.bias) if alias else (self.norm2(x1), x1)
        if site is not None:
            return self.mlp(n2, apply_out_drop=False, residual=x1), None, None
        m = self.mlp(n2, apply_out_drop=False)
        return x1, (m, self._path_scale(x1), self.mlp.drop.p if self.training else 0.0), x1_lo

    def forward_stream_v2(self, x, x_lo=None):
        """v2 block (ref :334-335) on the compensated stream x (+ x_lo); returns (x', x'_lo)."""
        return self._v2_block(x, x_lo, stream=True)

    def _v2_block(self, x, x_lo=None, stream=False):
        """ref :334-335: x + drop_path(norm(branch(x))) for both branches, each sum fused into its norm kernel; returns (x', x'_lo).
        stream: on the compensated stream x (+ x_lo), the sums by ops.layer_norm_stream, which also emits the remainder.
        The residual operand is the alias handed back by the branch's first Linear: its gradient is then added inside that
        Linear's input-gradient GEMM, not by a separate elementwise kernel."""
        train = self.training
        a, xr = self._attention_branch(x, apply_proj_drop=False, residual_alias=True)
        x, x_lo = self._v2_add_norm(self.norm1, a, xr, x_lo, stream, self.attn.proj_drop.p if train else 0.0)
        x2 = None if stream else self._fused_mlp(x, post_norm=True)  # x + norm2(mlp(x)) in one launch where the Mlp is HBM-bound (stage 0)
        if x2 is not None:
            return x2, None
        m, xr = self.mlp(x, apply_out_drop=False, residual_alias=True)
        return self._v2_add_norm(self.norm2, m, xr, x_lo, stream, self.mlp.drop.p if train else 0.0)

    def _v2_add_norm(self, norm, t, xr, x_lo, stream, drop_p):
        """(xr (+ x_lo) + rs*norm(drop(t)), its remainder or None): one norm kernel either way, but not the same call."""
        rs = self._path_scale(xr)
        if stream:
            return ops.layer_norm_stream(t, norm.weight, norm.bias, xr, res_lo=x_lo, row_scale=rs, drop_p=drop_p)
        return norm(t, residual=xr, row_scale=rs, drop_p=drop_p), None

    @staticmethod
    def resolve_pending(x, pending):
        """x + rs*drop(p): the standalone form of a deferred residual (end of a stage)."""
        if pending is None:
            return x
        t, rs, dp = pending
        vec = 8 if t.dtype == torch.bfloat16 else 4
        if (dp or rs is not None) and t.is_cuda and t.dtype in (torch.bfloat16, torch.float32) and (t.numel() // t.shape[0]) % vec == 0:
            return ops.residual_drop(x, t, rs, dp)  # dropout, DropPath and the add in one HIP pass
        if dp:
            t = F.dropout(t, dp, True)
        if rs is not None:
            t = t * rs.to(t.dtype).view(-1, 1, 1)
        return x + t

    def forward(self, x):
        B, N, C = x.shape
        assert N == self.n_tokens, f"expected {self.n_tokens} tokens, got {N}"
        place = self.placement()
        if place == "v1":
            return self.resolve_pending(*self.forward_deferred(x, None)[:2])
        if place == "v2":
            return self._v2_block(x)[0]
        if self.use_v2_norm_placement:  # foreign norm layers
            x = x + self.drop_path(self.norm1(self._attention_branch(x)))
            return x + self.drop_path(self.norm2(self.mlp(x)))
        # ref :315-316, :337-338
        x = x + self.drop_path(self._attention_branch(self.norm1(x)))
        return x + self.drop_path(self.mlp(self.norm2(x)))


# ----------------------------------------------------------------------------- resolution changes
class PatchMerging(nn.Module):
    """4 sibling pixels (consecutive in nested order) -> one token: view [B, N/4, 4C] -> LN(4C) -> Linear(4C -> 2C)
    (ref :364-395; the strided slices + cat there are exactly this view)."""

    def __init__(self, dim, dim_scale=2, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = HSLinear(4 * dim, dim_scale * dim, bias=False)
        self.norm = _make_norm(norm_layer, 4 * dim)

    def forward(self, x):
        B, N, C = x.shape
        assert N % 4 == 0, f"x size {N} is not divisible by 4 as necessary for patching."
        return self.reduction(self.norm(x.reshape(B, N // 4, 4 * C)))


class PatchExpand(nn.Module):
    """Linear(C -> 2C) then every token becomes 4 children of C/2 channels, LN over each child (ref :407-430)."""

    def __init__(self, dim, dim_scale=2, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.expand = HSLinear(dim, dim_scale * dim, bias=False) if dim_scale != 1 else nn.Identity()
        self.norm = _make_norm(norm_layer, dim * dim_scale // 4)

    def forward(self, x):
        x = self.expand(x)
        B, N, C = x.shape
        return self.norm(x.reshape(B, N * 4, C // 4))  # 'b n (p c) -> b (n p) c' is a view in nested order


class FinalPatchExpand_X4(nn.Module):
    """Linear(C -> p*C), p children per token, LN(C) (ref :433-452)."""

    def __init__(self, patch_size, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim, self.patch_size, self.output_dim = dim, patch_size, dim
        self.expand = HSLinear(dim, patch_size * dim, bias=False)
        self.norm = _make_norm(norm_layer, dim)

    def forward(self, x):
        x = self.expand(x)
        B, N, C = x.shape
        return self.norm(x.reshape(B, N * self.patch_size, C // self.patch_size))


# ----------------------------------------------------------------------------- stages
class _Stage(nn.Module):
    """What the four stage classes (encoder and decoder, HEALPix and flat) share: the constructor body, the block loop, forward."""

    _resample = None  # name of the attribute that holds the stage's PatchMerging / PatchExpand (or None)

    def _build(self, block_cls, dim, input_resolution, depth, use_checkpoint, shifts, drop_path, **block_kw):
        """The stage's attributes and its `depth` blocks of block_cls(**block_kw): even blocks with shifts[0] (none), odd ones with
        shifts[1] (ref :516); drop_path a rate or one per block."""
        self.dim, self.input_resolution, self.depth, self.use_checkpoint = dim, input_resolution, depth, use_checkpoint
        self.blocks = nn.ModuleList([
            block_cls(dim=dim, input_resolution=input_resolution, shift_size=shifts[i % 2],
                      drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path, **block_kw)
            for i in range(depth)
        ])

    def forward(self, x):
        x = self._run_blocks(x)
        resample = getattr(self, self._resample)
        return x if resample is None else resample(x)

    def _run_blocks(self, x):
        pending = None  # second residual branch of the previous block, added inside the next block's first LayerNorm
        x_lo = None     # rounding remainder of the residual stream (compensated bf16 stream, ops.COMP_RESIDUAL); dropped at the
        #                 end of the stage (one ordinary rounding): every tensor that leaves a stage is a plain activation
        for blk in self.blocks:
            place = None if self.use_checkpoint else blk.placement()  # (a checkpointed block runs whole, through its forward)
            if place == "v1":
                x, pending, x_lo = blk.forward_deferred(x, pending, x_lo, comp=self._comp())
            elif place == "v2" and self._comp() and x.dtype == torch.bfloat16 and x.is_cuda:
                x, x_lo = blk.forward_stream_v2(x, x_lo)
            else:
                x, pending, x_lo = SwinTransformerBlock.resolve_pending(x, pending), None, None
                x = checkpoint.checkpoint(blk, x, use_reentrant=False) if self.use_checkpoint else blk(x)
        return SwinTransformerBlock.resolve_pending(x, pending)

    comp_residual = None  # None: follow ops.COMP_RESIDUAL; True / False: this stage's own setting (see UnetDecoder)

    def _comp(self):
        return ops.COMP_RESIDUAL if self.comp_residual is None else bool(self.comp_residual)

    def extra_repr(self):
        return f"dim={self.dim}, input_resolution={self.input_resolution}, depth={self.depth}"


class BasicLayer(_Stage):
    """Encoder stage: blocks + optional PatchMerging (ref :455-547)."""

    _resample = "downsample"

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, base_pix, shift_size, shift_strategy, rel_pos_bias,
                 mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm,
                 downsample=None, use_checkpoint=False, use_v2_norm_placement=False, use_cos_attn=False):
        super().__init__()
        self._build(SwinTransformerBlock, dim, input_resolution, depth, use_checkpoint, (0, shift_size), drop_path,
                    base_pix=base_pix, num_heads=num_heads, window_size=window_size, shift_strategy=shift_strategy,
                    rel_pos_bias=rel_pos_bias, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                    norm_layer=norm_layer, use_v2_norm_placement=use_v2_norm_placement, use_cos_attn=use_cos_attn)
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None


class BasicLayer_up(_Stage):
    """Decoder stage: blocks + optional PatchExpand (ref :561-653)."""

    _resample = "upsample"

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, base_pix, shift_size, shift_strategy, rel_pos_bias,
                 mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm,
                 upsample=None, use_checkpoint=False, use_v2_norm_placement=False, use_cos_attn=False):
        super().__init__()
        self._build(SwinTransformerBlock, dim, input_resolution, depth, use_checkpoint, (0, shift_size), drop_path,
                    base_pix=base_pix, num_heads=num_heads, window_size=window_size, shift_strategy=shift_strategy,
                    rel_pos_bias=rel_pos_bias, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                    norm_layer=norm_layer, use_v2_norm_placement=use_v2_norm_placement, use_cos_attn=use_cos_attn)
        self.upsample = PatchExpand(dim=dim, dim_scale=2, norm_layer=norm_layer) if upsample is not None else None


class PatchEmbed(nn.Module):
    """`patch_size` consecutive nested pixels -> one token (ref :656-694).  The Conv1d(k = s = patch) parameters are kept
    (state-dict layout [C, f_in, patch]); the arithmetic is a per-patch linear map."""

    def __init__(self, config, data_spec):
        super().__init__()
        assert config.patch_size % 4 == 0, "required for valid nside in deeper layers"
        self.config, self.data_spec = config, data_spec
        self.num_patches = data_spec.dim_in // config.patch_size
        self.proj = nn.Conv1d(data_spec.f_in, config.embed_dim, kernel_size=config.patch_size, stride=config.patch_size)
        # reference quirk (:681-684): the config VALUE is stored, not an instance; only None is usable
        self.norm = config.patch_embed_norm_layer if config.patch_embed_norm_layer is not None else None

    def forward(self, x):
        B, C, N = x.shape
        assert N == self.data_spec.dim_in, f"Input image size ({N}) doesn't match model ({self.data_spec.dim_in})."
        P = self.config.patch_size
        patches = x.reshape(B, C, N // P, P).permute(0, 2, 1, 3).reshape(B, N // P, C * P)
        w = self.proj.weight.reshape(self.proj.weight.shape[0], C * P)
        if x.is_cuda and x.dtype == torch.bfloat16:
            # RGB x 4 pixels = 12 input features = 24-byte rows: zero-padded to 16 so that the product and, above all, its weight
            # gradient (a 128 x 12 output reduced over every token: 1.27 ms in the library, 0.09 ms in hs_linear_wgrad) run in
            # the HIP kernels (16-byte operand rows)
            pad = (-C * P) % 8
            if pad:
                patches, w = F.pad(patches, (0, pad)), F.pad(w, (0, pad))
            x = ops.linear(patches, w, self.proj.bias)
        else:
            x = F.linear(patches, w.to(x.dtype), self.proj.bias.to(x.dtype))
        return x if self.norm is None else self.norm(x)


def _stage_kw(config, data_spec):
    """What every stage of a model takes from its config; width, resolution, depth, heads, drop-path rates and resampling are its own."""
    return dict(window_size=config.window_size, base_pix=data_spec.base_pix, shift_size=config.shift_size,
                shift_strategy=config.shift_strategy, rel_pos_bias=config.rel_pos_bias, mlp_ratio=config.mlp_ratio,
                qkv_bias=config.qkv_bias, qk_scale=config.qk_scale, use_cos_attn=config.use_cos_attn, drop=config.drop_rate,
                attn_drop=config.attn_drop_rate, norm_layer=config.norm_layer, use_v2_norm_placement=config.use_v2_norm_placement,
                use_checkpoint=config.use_checkpoint)


class UnetDecoder(nn.Module):
    """Expanding path with skip connections (ref :704-791)."""

    def __init__(self, config, data_spec, dpr):
        super().__init__()
        self.config = config
        L = self.num_layers = len(config.depths)
        self.num_features = int(config.embed_dim * 2 ** (L - 1))
        num_patches = data_spec.dim_in // config.patch_size
        self.layers_up = nn.ModuleList()
        self.concat_back_dim = nn.ModuleList()
        for i_layer in range(L):
            down = L - 1 - i_layer
            width = int(config.embed_dim * 2 ** down)
            if i_layer == 0:
                self.concat_back_dim.append(nn.Identity())
                self.layers_up.append(PatchExpand(dim=width, dim_scale=2, norm_layer=config.norm_layer))
                continue
            self.concat_back_dim.append(HSLinear(2 * width, width))
            lo = sum(config.depths[:down])
            self.layers_up.append(BasicLayer_up(
                dim=width, input_resolution=num_patches // (4 ** down), depth=config.depths[down], num_heads=config.num_heads[down],
                drop_path=dpr[lo:lo + config.depths[down]], upsample=PatchExpand if down > 0 else None, **_stage_kw(config, data_spec)))
        if ops.COMP_RESIDUAL_LAST_STAGE and isinstance(self.layers_up[-1], BasicLayer_up):
            # the last decoder stage feeds the tail directly: its residual stream is carried as hi + lo (ops.COMP_RESIDUAL_LAST_STAGE)
            self.layers_up[-1].comp_residual = True
        self.up = FinalPatchExpand_X4(patch_size=config.patch_size, dim=config.embed_dim)
        self.output = nn.Conv1d(in_channels=config.embed_dim, out_channels=data_spec.f_out, kernel_size=1, bias=False)
        self.norm_up = _make_norm(config.norm_layer, config.embed_dim)

    def forward_up_features(self, x, x_downsample):
        """The expanding path (also the flat model's, which keeps layers_up / concat_back_dim on itself as its reference does)."""
        for inx, layer_up in enumerate(self.layers_up):
            if inx > 0:
                lin = self.concat_back_dim[inx]  # Linear(2c -> c) on cat([x, skip]) (ref :772-775), without the concat copy
                x = ops.concat_linear(x, x_downsample[self.num_layers - 1 - inx], lin.weight, lin.bias)
            x = layer_up(x)
            if self.config.dev_mode:
                print(f"feature shape after decoder layer {inx}: {x.size()}")
        return x

    def forward(self, x, x_downsample, task=None):
        """task: None for the logits, or the SegTask / DepthTask of decoder_tail, whose result is returned instead."""
        x = self.forward_up_features(x, x_downsample)
        w = self.output.weight  # 1x1 conv without bias (ref :756-761) as the [f_out, C] matrix it is (ops.LinearFn)
        out = decoder_tail(self.norm_up, self.up, w, self.up.patch_size, x, task)
        return out if task is not None else out.float().transpose(1, 2)  # B, f_out, Npix (fp32)


@dataclass
class SegTask:
    """decoder_tail's segmentation request: the weighted cross-entropy (class_weights f32 [f_out] or None) of the logits rows against
    labels [B, rows] in the rows' order (forward_seg_loss); with `step` the caller's whole shared_step (forward_seg_step): (loss,
    preds u8 [B, rows] or None), and the counts of (labels, preds) added to `confusion` (an evaluation.SegConfusion or None)."""

    labels: torch.Tensor
    class_weights: Optional[torch.Tensor] = None
    step: bool = False
    confusion: Optional[object] = None
    want_preds: bool = True

    def fused(self, xn2, up, w, xn_lo, B):
        """The result in one launch on norm_up's output xn2 [B * N0, C] (+ xn_lo), or None: not uint8 labels, a loss without gradient."""
        if self.labels.dtype != torch.uint8 or not (self.step or torch.is_grad_enabled()):
            return None
        args = (xn2, up.expand.weight, up.norm.weight, up.norm.bias, w, self.labels.contiguous(), self.class_weights, xn_lo)
        if not self.step:
            # training: expand -> LayerNorm -> head -> weighted CE in one forward kernel; the logits are never written
            return ops.expand_ln_head_ce(*args)
        # the caller's shared_step in one forward kernel: loss, class ids and confusion matrix; the logits are never written
        confmat, bad = (None, None) if self.confusion is None else (self.confusion.confmat, self.confusion._bad)
        loss, preds = ops.expand_ln_head_ce_step(*args, confmat, bad, self.want_preds)
        return loss, (None if preds is None else preds.view(B, -1))

    def from_rows(self, logits):
        """The same result composed from the written logits (the rows seen as [B, f_out, rows] fp32) by the standalone kernels."""
        from ..losses import seg_loss, seg_predictions
        loss = seg_loss(logits, self.labels, self.class_weights)
        if not self.step:
            return loss
        # the shared_step composed from the written rows: hs_seg_confusion reads them in place (and takes the argmax itself)
        if self.confusion is not None:
            self.confusion.update(logits.detach(), self.labels, check=False)
        return loss, (seg_predictions(logits.detach()).to(torch.uint8) if self.want_preds else None)


@dataclass
class DepthTask:
    """decoder_tail's depth request: the depth-regression loss (HS_DEPTH_* kind, huber delta) of the head rows against target f32
    [B, rows] in the rows' order (forward_depth_loss); with `step` the caller's whole shared_step (forward_depth_step): (loss, preds
    f32 [B, f_out, rows] or None: channel 0 in metres), and `metrics` (a depth_evaluation.DepthMetrics or None) updated on (preds,
    target in metres) through `transform` (a depth_data.DepthTargetTransform or None)."""

    target: torch.Tensor
    kind: int
    delta: float
    step: bool = False
    transform: Optional[object] = None
    metrics: Optional[object] = None
    want_preds: bool = True

    def fused(self, xn2, up, w, xn_lo, B):
        """As SegTask.fused; None: outside ops.expand_ln_head_depth_ok, a loss without gradient."""
        f_out = w.shape[0]
        if not ((self.step or torch.is_grad_enabled()) and
                ops.expand_ln_head_depth_ok(xn2, up.dim, up.expand.weight.shape[0] // up.dim, f_out, self.kind, self.delta)):
            return None
        args = (xn2, up.expand.weight, up.norm.weight, up.norm.bias, w, self.target, self.kind, self.delta, xn_lo)
        if not self.step:
            # training: expand -> LayerNorm -> head -> depth loss in one forward kernel; the head rows are never written
            return ops.expand_ln_head_depth(*args)
        # the depth caller's shared_step in one forward kernel: loss, metres and metric sums; the head rows are never written
        loss, preds = ops.expand_ln_head_depth_step(*args, self.transform, self.metrics, self.want_preds, batch=B)
        return loss, (None if preds is None else preds.view(f_out, B, -1).transpose(0, 1))

    def from_rows(self, pred):
        """The same result composed from the written head rows (seen as [B, f_out, rows] fp32) by the standalone kernels."""
        from ..losses import _DepthLossFn, depth_step_from_rows
        if self.step:
            return depth_step_from_rows(pred, self.target, self.kind, self.delta, self.transform, self.metrics, self.want_preds)
        return _DepthLossFn.apply(pred, self.target, self.kind, self.delta)


def decoder_tail(norm_up, up, w, children, x, task=None):
    """norm_up -> up (Linear C -> children * C, one LayerNorm(C) per child) -> 1x1 head w [f_out, C, ...] on the decoder output
    x [B, N0, C].  Returns the logits rows [B, N0 * children, f_out] (the children of a token consecutive; fp32, or the fallback's
    compute dtype), or with a task (SegTask, DepthTask: labels / target [B, N0 * children] in the same row order) what the task
    asks for instead: in one launch without the rows where the one-launch tail applies and the task can take it (task.fused), else
    composed from the rows by the standalone kernels (task.from_rows)."""
    f_out = w.shape[0]
    if (isinstance(up.norm, HSLayerNorm) and isinstance(up.expand, HSLinear) and up.expand.bias is None and
            ops.expand_ln_head_ok(x, up.dim, children, f_out)):
        # the whole tail in one forward kernel (hs_expand_ln_head_fwd): expand -> view -> LayerNorm -> head with fp32 statistics
        # on the expand product's accumulators; the [B, Npix, C] tensor is written once for the backward, or not at all
        xn_lo = None
        if isinstance(norm_up, HSLayerNorm):  # norm_up output as hi + lo: no rounding between norm_up and the logits
            xn, xn_lo = ops.layer_norm_hilo(x, norm_up.weight, norm_up.bias)
        else:
            xn = norm_up(x)
        B, N0, _ = xn.shape
        xn2 = xn.reshape(B * N0, up.dim)
        out = None if task is None else task.fused(xn2, up, w, xn_lo, B)
        if out is not None:
            return out
        lg = ops.expand_ln_head(xn2, up.expand.weight, up.norm.weight, up.norm.bias, w, xn_lo)
        rows = ops.pad_slice(lg.view(B, N0 * children, -1), f_out)
    elif isinstance(up.norm, HSLayerNorm) and ops.ln_head_ok(x, up.dim, f_out):
        # the tail's LayerNorm and the class head in one pass over the expanded rows (hs_ln_head_*): the normalised
        # [B, Npix, C] tensor is neither written nor kept for the backward
        x = up.expand(norm_up(x))  # B, N0, p * C: row (b, n) holds the p children of token n back to back
        B, N0, _ = x.shape
        x = ops.ln_head(x.reshape(B * N0 * children, up.dim), up.norm.weight, up.norm.bias, w)
        rows = ops.pad_slice(x.view(B, N0 * children, -1), f_out)
    else:
        x = up(norm_up(x))  # B, Npix, C
        if x.dtype == torch.bfloat16 and f_out % 8 and f_out > 8:
            # 12 classes: rows padded to 16 so that the input gradient (K = 12 -> 16) runs in hs_gemm_nt: 0.33 ms instead of the
            # library's 0.85 ms; the caller sees the [.., :f_out] view (the loss kernels read logits through their strides)
            rows = ops.pad_slice(ops.linear(x, F.pad(w.reshape(f_out, -1), (0, 0, 0, (-f_out) % 8))), f_out)
        else:
            rows = ops.linear(x, w)
    # logits leave the model in fp32 whatever the compute dtype (see ops.LnHeadFn)
    return rows if task is None else task.from_rows(rows.float().transpose(1, 2))


def check_step_confusion(confusion, f_out):
    """forward_seg_step's `confusion`: None or a SegConfusion of the model's class count."""
    if confusion is not None and getattr(confusion, "num_classes", None) != f_out:
        raise ValueError(f"confusion counts {getattr(confusion, 'num_classes', None)} classes, the model predicts {f_out}")


def check_depth_step_args(transform, metrics, f_out, device):
    """forward_depth_step's `transform` and `metrics`, checked on the host before any device work."""
    from ..depth_data import DepthTargetTransform
    from ..depth_evaluation import DepthMetrics
    if transform is not None and not isinstance(transform, DepthTargetTransform):
        raise TypeError(f"transform must be a depth_data.DepthTargetTransform or None, got {type(transform).__name__}")
    if metrics is None:
        return
    if not isinstance(metrics, DepthMetrics):
        raise TypeError(f"metrics must be a depth_evaluation.DepthMetrics or None, got {type(metrics).__name__}")
    if metrics.use_logvar and f_out < 2:
        raise ValueError(f"metrics.use_logvar needs a two-channel head (mean, log variance), the model predicts {f_out}")
    if metrics.state.device != torch.device(device):
        raise ValueError(f"metrics live on {metrics.state.device}, the input on {device}")


@dataclass
class SwinHPTransformerConfig:
    """Same 23 fields and defaults as the reference config (ref :794-818)."""

    patch_size: int = 4
    window_size: int = 4
    shift_size: int = 2
    shift_strategy: Literal["nest_roll", "nest_grid_shift", "ring_shift"] = "nest_roll"
    rel_pos_bias: Optional[Literal["flat"]] = None
    embed_dim: int = 96
    patch_embed_norm_layer: Optional[Literal[nn.LayerNorm]] = None
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
    dev_mode: bool = False
    decoder_class: Literal[UnetDecoder] = UnetDecoder


class SwinHPTransformerSys(nn.Module):
    """HEAL-SWIN-UNet: forward(x[B, f_in, Npix]) -> [B, f_out, Npix] (ref :821-955)."""

    def __init__(self, config: SwinHPTransformerConfig, data_spec: DataSpec, **kwargs):
        super().__init__()
        self.config, self.data_spec = config, data_spec
        L = self.num_layers = len(config.depths)
        self.num_features = int(config.embed_dim * 2 ** (L - 1))
        self.num_features_up = int(config.embed_dim * 2)
        self.compute_dtype = kwargs.pop("compute_dtype", None)  # None: follow autocast, else the input dtype

        self.patch_embed = PatchEmbed(config, data_spec=data_spec)
        num_patches = self.patch_embed.num_patches
        if config.ape:
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, num_patches, config.embed_dim))
            nn.init.trunc_normal_(self.absolute_pos_embed, std=0.02)
        self.pos_drop = nn.Dropout(p=config.drop_rate)
        dpr = [v.item() for v in torch.linspace(0, config.drop_path_rate, sum(config.depths))]  # ref :871-873

        self.layers = nn.ModuleList()
        for i in range(L):
            lo = sum(config.depths[:i])
            self.layers.append(BasicLayer(
                dim=int(config.embed_dim * 2 ** i), input_resolution=num_patches // (4 ** i), depth=config.depths[i],
                num_heads=config.num_heads[i], drop_path=dpr[lo:lo + config.depths[i]], downsample=PatchMerging if i < L - 1 else None,
                **_stage_kw(config, data_spec)))
        # a reference config object names the reference's own UnetDecoder class: use this package's counterpart
        decoder_cls = config.decoder_class
        if getattr(decoder_cls, "__name__", "") == "UnetDecoder":
            decoder_cls = UnetDecoder
        self.decoder = decoder_cls(config, data_spec, dpr)
        self.norm = _make_norm(config.norm_layer, self.num_features)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):  # ref :912-919 (Conv1d layers keep the torch default init)
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"absolute_pos_embed"}

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return {"relative_position_bias_table"}

    def _activation_dtype(self, x):
        if self.compute_dtype is not None:
            return self.compute_dtype
        if torch.is_autocast_enabled():
            return torch.get_autocast_gpu_dtype()
        return x.dtype if x.dtype in (torch.float32, torch.bfloat16) else torch.float32

    def _prefetch_attn_params(self):
        """The relative-position bias tiles and the cosine score scales of ALL blocks in one launch each (per window size), handed to
        the blocks for this forward; the backward scatters / differentiates them in one launch each as well."""
        sink = ops.RT.grad_sink
        if not ops.BATCH_ATTN_PARAMS or self.config.use_checkpoint or (sink is not None and getattr(sink, "world", 1) > 1):
            # (a checkpointed block recomputes its forward later, outside this call: it must see the same per-block tensors both times;
            # under data parallelism the batched backward would report every block's table gradient at the END of the pass, and no
            # gradient bucket could start its exchange before that: the per-block nodes keep the exchange overlapped with the backward)
            return
        mods = self.__dict__.get("_attn_mods")
        if mods is None:
            mods = self.__dict__["_attn_mods"] = [m for m in self.modules() if isinstance(m, WindowAttention)]
        by_ws = {}
        for m in mods:
            t = getattr(m, "relative_position_bias_table", None)
            if m.rel_pos_bias == "flat" and t is not None and t.is_cuda and t.dtype == torch.float32:
                by_ws.setdefault((m.window_size, t.shape[0]), []).append(m)
        for (ws, _), group in by_ws.items():
            if len(group) > 1:
                for m, b in zip(group, ops.rel_pos_bias_many(group[0]._rel_idx32, ws, [m.relative_position_bias_table for m in group])):
                    m.__dict__["_bias_now"] = b
        cos = [m for m in mods if m.use_cos_attn and m.logit_scale.is_cuda and m.logit_scale.dtype == torch.float32 and m.num_heads <= 64]
        if len(cos) > 1:
            for m, sc in zip(cos, ops.cos_head_scale_many([m.logit_scale for m in cos])):
                m.__dict__["_scale_now"] = sc

    def _clear_attn_params(self):
        for m in self.__dict__.get("_attn_mods") or ():
            m.__dict__.pop("_bias_now", None)
            m.__dict__.pop("_scale_now", None)

    def forward_features(self, x):
        x = self.patch_embed(x)
        if self.config.ape:
            x = x + self.absolute_pos_embed.to(x.dtype)
        x = self.pos_drop(x)
        x_downsample = []
        for k, layer in enumerate(self.layers):
            x_downsample.append(x)  # the INPUT of encoder stage k is the skip tensor (ref :939-941)
            x = layer(x)
            if self.config.dev_mode:
                print(f"feature shape after basic layer {k}: {x.size()}")
        return self.norm(x), x_downsample

    def _require_device(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__} (heal_swin_amd) runs only on an MI355X (HIP) device; there is no CPU path")

    @contextmanager
    def _run_scope(self, dt):
        """What every run of the model in compute dtype dt happens inside: the bf16 parameter copies as ops.RT.cast_cache, autocast
        off, the attention parameters of all blocks prefetched; restored and cleared on every way out."""
        prev, ops.RT.cast_cache = ops.RT.cast_cache, self._param_casts(dt)
        ops.RT.last_cast_cache = ops.RT.cast_cache
        try:
            with torch.autocast(device_type="cuda", enabled=False):
                self._prefetch_attn_params()
                yield
        finally:
            self._clear_attn_params()
            ops.RT.cast_cache = prev

    def _run(self, x, task=None):
        """The logits [B, f_out, Npix] of x, or what `task` (a SegTask / DepthTask in the decoder's row order) asks for instead."""
        self._require_device(x)
        dt = self._activation_dtype(x)
        with self._run_scope(dt):
            x, x_downsample = self.forward_features(x.to(dt))
            return self.decoder(x, x_downsample) if task is None else self.decoder(x, x_downsample, task)

    # Hooks of the forward_seg_* / forward_depth_* methods below; the flat model overrides them for its pixel order and images.
    def _batch(self, x):
        return x.shape[0]

    def _as_image(self, preds):
        """A step's predictions (or None) in the layout forward() gives: here the decoder's rows are the HEALPix pixels already."""
        return preds

    def _seg_labels(self, x, labels):
        """uint8 labels [B, Npix] in the decoder's row order, on x's device."""
        self._require_device(x)
        if labels.dtype != torch.uint8 and self.data_spec.f_out <= 255:
            # the kernels read one byte per pixel and ignore ids >= f_out.  A plain cast would WRAP (256 -> class 0, and
            # CrossEntropyLoss' ignore_index -100 -> 156): out-of-range ids are mapped to 255 (ignored) before narrowing
            labels = torch.where((labels < 0) | (labels > 254), 255, labels).to(torch.uint8)
        return labels

    def _class_weights(self, x, class_weights):
        return None if class_weights is None else class_weights.to(device=x.device, dtype=torch.float32).contiguous()

    def _depth_target(self, x, target):
        """The fp32 target [B, Npix] in the decoder's row order, on x's device."""
        self._require_device(x)
        assert target.shape == (self._batch(x), x.shape[-1]), "target [B, Npix]"
        return target.to(device=x.device, dtype=torch.float32).contiguous()

    def forward(self, x):
        return self._run(x)

    def forward_seg_loss(self, x, labels, class_weights=None):
        """nn.CrossEntropyLoss(weight=class_weights)(self(x), labels.long()) -- the segmentation caller's training step
        (models_lightning/segmentation/model_lightning_swin_hp.py:39-45, :104-111) -- as ONE call, so that the loss rides on the
        decoder tail's kernels: in bf16 training the [B, f_out, Npix] logits and their gradient are never written (SURVEY 8f N2;
        csrc/expand_ln_head.hip, csrc/ln_head.hip).  Where the fused tail does not apply (fp32, other widths, no gradient) this is
        exactly losses.seg_loss(self(x), labels, class_weights).  labels: [B, Npix] integer class ids."""
        return self._run(x, SegTask(self._seg_labels(x, labels), self._class_weights(x, class_weights)))

    def forward_seg_step(self, x, labels, class_weights=None, confusion=None, return_preds=True):
        """The segmentation caller's `shared_step` (models_lightning/segmentation/model_lightning_swin_hp.py:104-111) as ONE call:
            outputs = self(x); _, preds = torch.max(outputs, 1); loss = CrossEntropyLoss(weight)(outputs, labels.long());
            iou / acc / acc_ignored (preds, labels)
        -> (loss, preds): the loss of forward_seg_loss (bit for bit, same gradients), preds uint8 [B, Npix] (None with
        return_preds=False), and the (label, pred) counts added to `confusion` (an evaluation.SegConfusion; read its iou() /
        accuracy() when the metric is logged, all_reduce() it under data parallelism).  In bf16 all of it rides on ONE decoder-tail
        launch (`hs_expand_ln_head_ce_step_fwd`) that reads the labels and writes one byte per pixel, with a gradient (training)
        and without (validation): the logits are never written.  Elsewhere (fp32, other widths, > 16 classes) the same results are
        composed from the logits rows.  Labels >= f_out carry no weight and are not counted; the SegConfusion reports them at its
        next metric read (no synchronisation here, as update(..., check=False))."""
        check_step_confusion(confusion, self.data_spec.f_out)
        loss, preds = self._run(x, SegTask(self._seg_labels(x, labels), self._class_weights(x, class_weights), True, confusion, bool(return_preds)))
        return loss, self._as_image(preds)

    def forward_depth_loss(self, x, target, loss="l2", huber_delta=1.0, use_logvar=False, mask_background=False):
        """get_depth_loss(cfg)(self(x), target) -- the depth caller's training step (training/loss_depth_regression.py) -- as ONE
        call, so that the loss rides on the decoder tail's kernels: in bf16 training the [B, f_out, Npix] head rows and their
        gradient are never written (csrc/expand_ln_head.hip, csrc/ln_head.hip).  Where the fused tail does not apply (fp32, other
        widths, no gradient) this is losses.depth_loss(self(x), target, ...) on the standalone kernels.  target: [B, Npix] depths
        (pixels with an infinite target are masked out); `loss` may be a CommonDepthConfig-like object (use_logvar, loss,
        huber_delta) as get_depth_loss takes; `mask_background` is accepted and ignored, as in the reference."""
        from ..losses import check_depth_channels, depth_loss_spec
        kind, delta = depth_loss_spec(loss, huber_delta, use_logvar)
        check_depth_channels(kind, self.data_spec.f_out)
        return self._run(x, DepthTask(self._depth_target(x, target), kind, delta))

    def forward_depth_step(self, x, target, loss="l2", huber_delta=1.0, use_logvar=False, transform=None, metrics=None, return_preds=True,
                           mask_background=False):
        """The depth caller's `shared_step` (models_lightning/depth_estimation/model_lightning_depth_swin_hp.py:132-159) as ONE call:
            outputs = self(x); loss in the normalised space; unnormalize_and_retransform(outputs[:, 0]), (target);
            metrics.update(outputs, target)
        -> (loss, preds): the loss of forward_depth_loss (bit for bit, same gradients), preds fp32 [B, f_out, Npix] with channel 0 in
        metres and channel 1 the raw log variance (None with return_preds=False), and `metrics` (a depth_evaluation.DepthMetrics or
        None) updated on (preds, transform.unnormalize_and_retransform(target)).  target [B, Npix] is what the dataset delivers,
        transform.prepare(depth); transform is a depth_data.DepthTargetTransform or None (the identity); the other arguments as
        forward_depth_loss.  Where ops.expand_ln_head_depth_ok (bf16, C in {64, 96, 128}, a head the loss kind accepts) all of it
        is ONE decoder-tail launch (`hs_expand_ln_head_depth_step_fwd`) plus the one-workgroup merge of the metric records, with a
        gradient and without: the head rows are never written; median_std (metrics.use_logvar) takes the radix-select median of the written
        log variance (preds[:, 1], or 4 bytes per pixel of scratch).  Elsewhere the same results are composed from the head rows
        (losses.depth_step_from_rows).  No synchronisation with the host.
        Deviation from the reference (as forward_depth_loss): it takes the loss on transform_and_normalize(
        unnormalize_and_retransform(outputs[:, 0])), this takes it on outputs[:, 0]; the two agree to rounding wherever the
        prediction stays inside the transform's domain ('inv': metres >= 1e-3)."""
        from ..losses import check_depth_channels, depth_loss_spec
        kind, delta = depth_loss_spec(loss, huber_delta, use_logvar)
        check_depth_channels(kind, self.data_spec.f_out)
        check_depth_step_args(transform, metrics, self.data_spec.f_out, x.device)
        loss, preds = self._run(x, DepthTask(self._depth_target(x, target), kind, delta, True, transform, metrics, bool(return_preds)))
        return loss, self._as_image(preds)

    def _param_casts(self, dt):
        """bf16 copies of the Linear parameters, re-made in one multi-tensor kernel after each optimizer step (ops.ParamCastCache)."""
        ops.note_forward(torch.is_grad_enabled())
        if dt == torch.float32:
            return None
        cache = self.__dict__.get("_cast_cache")
        params = [p for m in self.modules() if isinstance(m, HSLinear) for p in (m.weight, m.bias) if p is not None]
        if (cache is None or cache.dtype != dt or len(cache.params) != len(params) or any(a is not b for a, b in zip(cache.params, params))
                or any(sh.device != p.device for sh, p in zip(cache.shadows[:1], params[:1]))):
            cache = ops.ParamCastCache(params, dt, shadow_of=self.__dict__.get("_shadow_provider"))  # (optim.FlatAdam)
            self.__dict__["_cast_cache"] = cache  # not a module attribute: stays out of state_dict / .to()
        cache.refresh(force=torch.is_grad_enabled())  # (fused optimizers do not bump parameter versions: see ops.ParamCastCache)
        return cache

    def invalidate_param_casts(self):
        """Force the bf16 parameter copies to be re-made at the next forward (needed only after in-place writes through
        `param.data`, which PyTorch's version counters do not see; see ops.ParamCastCache)."""
        cache = self.__dict__.get("_cast_cache")
        if cache is not None:
            cache.invalidate()
