"""Config / DataSpec of the flat Swin-UNet golden cases (tests/golden/flat_swin.npz, made by make_golden_flat_swin.py)."""

# name -> (image H, W, config overrides); drop rates are 0 everywhere
FLAT_MODEL_CASES = {
    # 2 stages, window 4, patch 2, scaled attention, v1 placement
    "a_w4_p2_v1": (32, 48, dict(window_size=4, patch_size=2, shift_size=2, depths=[2, 2], num_heads=[2, 4], embed_dim=16)),
    # 3 stages, window 8 (64 tokens), head dim 32: the MFMA and module-kernel paths; cosine attention, v2 placement.  At 64 x 64 the
    # last stage is 8 x 8 tokens: the reference clamps its window to the resolution (one window, no shift)
    "b_w8_p2_cos_v2": (64, 64, dict(window_size=8, patch_size=2, shift_size=2, depths=[2, 2, 2], num_heads=[1, 2, 4], embed_dim=32,
                                    use_cos_attn=True, use_v2_norm_placement=True)),
    # absolute position embedding, no shift mask, the default shift (-1: window // 2), one output channel (depth)
    "c_ape_nomask_depth": (32, 32, dict(window_size=4, patch_size=2, shift_size=-1, depths=[2, 2], num_heads=[2, 4], embed_dim=16,
                                        ape=True, use_masking=False, _f_out=1)),
    # patch 4
    "d_p4": (64, 64, dict(window_size=4, patch_size=4, shift_size=2, depths=[2, 2], num_heads=[2, 4], embed_dim=16)),
}

# (Ht, Wt, window side, shift) of the table cases
FLAT_TABLE_CASES = [(8, 12, 4, 2), (16, 24, 4, 1), (16, 16, 8, 2), (32, 48, 8, 4), (16, 32, 2, 1), (32, 32, 16, 8)]

# the paper's flat segmentation model (run_configs/segmentation/swin_*)
PAPER_CFG = dict(patch_size=2, window_size=8, shift_size=2, embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24],
                 use_cos_attn=True, use_v2_norm_placement=True, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0)
PAPER_SPEC = dict(dim_in=(640, 768), f_in=3, f_out=12, base_pix=None, class_names=[])


def flat_cfg_spec(name):
    H, W, kw = FLAT_MODEL_CASES[name]
    kw = dict(kw)
    f_out = kw.pop("_f_out", 5)
    cfg = dict(drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0)
    cfg.update(kw)
    return cfg, dict(dim_in=(H, W), f_in=3, f_out=f_out, base_pix=None, class_names=[])


def flat_weights(shapes, seed):
    """The golden models' parameters, regenerated from a seed instead of stored: {name: shape} -> {name: fp32 tensor}.  Linear
    and conv weights N(0, 0.02) as the reference's init, biases N(0, 0.02), LayerNorm weights 1 + N(0, 0.2) and biases N(0, 0.1),
    bias tables N(0, 0.3), cosine logit scales log(10) + N(0, 0.1), the absolute position embedding N(0, 0.02)."""
    import math

    import torch

    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in sorted(shapes):
        r = torch.randn(tuple(shapes[k]), generator=g, dtype=torch.float32)
        leaf = k.rsplit(".", 1)[-1]
        owner = k.rsplit(".", 2)[-2] if k.count(".") >= 1 else ""
        if leaf == "relative_position_bias_table":
            t = r * 0.3
        elif leaf == "logit_scale":
            t = math.log(10.0) + r * 0.1
        elif owner.startswith("norm") and leaf == "weight":
            t = 1.0 + r * 0.2
        elif owner.startswith("norm") and leaf == "bias":
            t = r * 0.1
        else:
            t = r * 0.02
        out[k] = t
    return out


def grad_sample(numel, seed=7, n=256):
    """Flat indices at which the large gradients of the golden cases are recorded."""
    import numpy as np

    return np.random.default_rng(seed + numel).choice(numel, size=min(n, numel), replace=False)


FULL_GRAD_MAX = 2048  # gradients up to this many elements are recorded whole, larger ones at grad_sample() + their L2 norm


def flat_dy(shape, seed):
    """The output gradient of a golden case, regenerated from its seed."""
    import torch

    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float32)
