"""ctypes binding of libhealswin.so (C ABI declared in include/healswin.h).

There is no fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libhealswin.so")

HS_F32, HS_BF16 = 0, 1
HS_F64 = 3
HS_PRED_LABELS, HS_PRED_ROWS16 = 2, 4
HS_ENSEMBLE_PROB, HS_ENSEMBLE_LOGIT = 0, 1
HS_ATTN_COSINE = 1
HS_ATTN_FORCE_VALU = 2
HS_ATTN_RESIDUAL = 4
HS_ATTN_OVERWRITE_GRADS = 8
HS_EPI_BIAS, HS_EPI_GELU, HS_EPI_DGELU, HS_EPI_RESID = 0, 1, 2, 3
HS_ACC_DEFER = 2
HS_MLP_NORM_AFTER = 16
HS_U8, HS_I32, HS_I64 = 8, 9, 10
HS_FLAT_PATCH_ROWS, HS_FLAT_PIXEL_ROWS, HS_FLAT_IMAGE = 0, 1, 2
HS_DEPTH_L1, HS_DEPTH_L2, HS_DEPTH_HUBER, HS_DEPTH_LOGVAR = 0, 1, 2, 3
HS_DT_NONE, HS_DT_LOG, HS_DT_INV = 0, 1, 2
HS_DT_ZERO_BKG, HS_DT_1000_BKG, HS_DT_AFFINE, HS_DT_INVERSE = 1, 2, 4, 8
HS_DEPTH_STATS_WORDS = 15
HS_HISTOGRAM_MAX_BINS = 4096

c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_uint = ctypes.c_uint
c_ptr = ctypes.c_void_p
c_float = ctypes.c_float


class WgradProblem(ctypes.Structure):
    """`hs_wgrad_problem` (include/healswin.h): one member of an hs_linear_wgrad_group call."""
    _fields_ = [("dy", c_ptr), ("x", c_ptr), ("dw", c_ptr), ("dbias", c_ptr), ("n_out", c_int), ("k_in", c_int), ("accumulate", c_int),
                ("gelu_x", c_int)]


def wgrad_problems(members):
    """ctypes array of hs_wgrad_problem from (dy, x, dw, dbias or None, n_out, k_in, accumulate, gelu_x) tuples of tensors / ints."""
    arr = (WgradProblem * len(members))()
    for q, (dy, x, dw, db, n_out, k_in, acc, gelu_x) in zip(arr, members):
        q.dy, q.x, q.dw, q.dbias = dy.data_ptr(), x.data_ptr(), dw.data_ptr(), (None if db is None else db.data_ptr())
        q.n_out, q.k_in, q.accumulate, q.gelu_x = int(n_out), int(k_in), int(acc), int(bool(gelu_x))
    return arr

class AdamGroup(ctypes.Structure):
    """`hs_adam_group` (include/healswin.h): the hyper-parameters of one parameter group of an hs_adam_step_groups call."""
    _fields_ = [("lr_dev", c_ptr), ("lr", c_float), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float),
                ("decoupled", ctypes.c_int32)]


def adam_groups(records):
    """ctypes array of hs_adam_group from (lr: float or 0-dim fp32 device tensor, beta1, beta2, eps, weight_decay, decoupled) tuples."""
    arr = (AdamGroup * len(records))()
    for q, (lr, b1, b2, eps, wd, decoupled) in zip(arr, records):
        on_device = hasattr(lr, "data_ptr")
        q.lr_dev, q.lr = (lr.data_ptr() if on_device else None), (0.0 if on_device else float(lr))
        q.beta1, q.beta2, q.eps, q.weight_decay, q.decoupled = float(b1), float(b2), float(eps), float(wd), int(bool(decoupled))
    return arr


class FisheyeCamera(ctypes.Structure):
    """`hs_fisheye_camera` (include/healswin.h): the polynomial fisheye model hs_hp_rotated_coords projects with."""
    _fields_ = [("k", ctypes.c_double * 8), ("cx_offset", ctypes.c_double), ("cy_offset", ctypes.c_double), ("aspect_ratio", ctypes.c_double),
                ("poly_order", c_int), ("width", c_int), ("height", c_int)]


class SurroundRig(ctypes.Structure):
    """`hs_surround_rig` (include/healswin.h): the cameras hs_surround_to_hp fuses, with their weights' parameters."""
    _fields_ = [("n_cameras", c_int), ("cam", FisheyeCamera * 8), ("max_theta", ctypes.c_double * 8), ("edge_feather", ctypes.c_double),
                ("blend", c_int)]


# name -> argtypes; every function returns int status unless listed in _OTHER_RESTYPE
_SIGNATURES = {
    "hs_nest2ring": [c_int, c_ptr, c_ptr, c_i64],
    "hs_ring2nest": [c_int, c_ptr, c_ptr, c_i64],
    "hs_nest_win_idcs": [c_int, c_ptr],
    "hs_rel_pos_index": [c_int, c_ptr],
    "hs_build_nest_roll_shift": [c_i64, c_int, c_int, c_ptr, c_ptr, c_ptr],
    "hs_build_nest_grid_shift": [c_int, c_int, c_int, c_ptr, c_ptr, c_ptr],
    "hs_build_ring_shift": [c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr],
    "hs_attn_mask_from_labels": [c_ptr, c_i64, c_int, c_ptr],
    "hs_flat_zorder": [c_int, c_int, c_int, c_ptr, c_ptr],
    "hs_build_flat_shift": [c_int, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr],
    "hs_flat_rel_pos_index": [c_int, c_ptr, c_ptr],
    "hs_flat_attn_mask": [c_int, c_int, c_int, c_int, c_ptr],
    "hs_flat_img_to_rows": [c_ptr, c_int, c_ptr, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_i64, c_ptr],
    "hs_flat_rows_to_img": [c_ptr, c_int, c_ptr, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_i64, c_ptr],
    "hs_flat_resize": [c_ptr, c_int, c_i64, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_int,
                       c_int, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_ptr],
    "hs_rel_bias_gather": [c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_ptr],
    "hs_rel_bias_scatter_grad_sorted_add": [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_ptr],
    "hs_cos_head_scale_fwd": [c_ptr, c_ptr, c_int, c_ptr],
    "hs_cos_head_scale_bwd": [c_ptr, c_ptr, c_ptr, c_int, c_int, c_ptr],
    "hs_rel_bias_gather_many": [c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_int, c_ptr],
    "hs_rel_bias_scatter_grad_sorted_many": [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_int, c_int, c_ptr],
    "hs_cos_head_scale_many": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr],
    "hs_rel_bias_scatter_grad": [c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_ptr],
    "hs_rel_bias_scatter_grad_sorted": [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_ptr],
    "hs_window_attn_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr,
                           c_int, c_i64, c_int, c_int, c_int, c_uint, ctypes.c_float, ctypes.c_uint64, c_int, c_ptr],
    "hs_window_attn_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr,
                           c_int, c_i64, c_int, c_int, c_int, c_uint, ctypes.c_float, ctypes.c_uint64, c_int, c_ptr],
    "hs_gather_rows": [c_ptr, c_ptr, c_ptr, c_i64, c_int, c_i64, c_i64, c_ptr],
    "hs_pix2ang_nest": [c_int, c_i64, c_i64, c_ptr, c_ptr],
    "hs_ln_head_supported": [c_int, c_int, c_int],
    "hs_expand_ln_head_supported": [c_int, c_int, c_int, c_int],
    "hs_expand_ln_head_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_ptr],
    "hs_expand_ln_head_ce_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int,
                                 c_int, c_ptr],
    "hs_expand_ln_head_ce_step_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                      c_ptr, c_i64, c_int, c_int, c_int, c_ptr],
    "hs_ln_head_ce_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_ptr],
    "hs_expand_ln_head_depth_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_float, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64,
                                    c_int, c_int, c_int, c_ptr],
    "hs_expand_ln_head_depth_step_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_float, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                         c_int, c_int, c_float, c_float, c_int, ctypes.c_double, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr,
                                         c_i64, c_int, c_int, c_int, c_ptr],
    "hs_ln_head_depth_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_float, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int,
                             c_int, c_ptr],
    "hs_ln_head_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_ptr],
    "hs_ln_head_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_ptr],
    "hs_sample_bilinear_u8": [c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_i64, c_ptr, c_ptr],
    "hs_sample_mask_u8": [c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_ptr],
    "hs_hp_rotated_coords": [c_int, c_i64, c_i64, ctypes.POINTER(FisheyeCamera), c_ptr, c_int, c_ptr, c_ptr, c_ptr],
    "hs_sample_bilinear_u8_per_sample": [c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_i64, c_ptr, c_ptr],
    "hs_sample_mask_u8_per_sample": [c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_ptr],
    "hs_hp_rotated_interp": [c_int, c_i64, c_i64, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr],
    "hs_hp_rotated_interp_host": [c_int, c_i64, c_i64, c_ptr, c_int, c_ptr, c_ptr, c_ptr],
    "hs_hp_rotate": [c_int, c_i64, c_ptr, c_int, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_float, c_ptr],
    "hs_erp_to_hp": [c_int, c_i64, c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_int, c_int, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_float,
                     c_ptr],
    "hs_erp_to_hp_host": [c_int, c_i64, c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_int, c_int, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr,
                          c_float],
    "hs_surround_to_hp": [c_int, c_i64, ctypes.POINTER(SurroundRig), c_ptr, c_ptr, c_int, c_int, c_int, c_ptr, c_int, c_int, c_ptr, c_ptr,
                          c_ptr, c_int, c_ptr, c_ptr, c_float, c_ptr, c_ptr],
    "hs_surround_to_hp_host": [c_int, c_i64, ctypes.POINTER(SurroundRig), c_ptr, c_ptr, c_int, c_int, c_int, c_ptr, c_int, c_int, c_ptr, c_ptr,
                               c_ptr, c_int, c_ptr, c_ptr, c_float, c_ptr],
    "hs_hp_ensemble_add_seg": [c_int, c_i64, c_ptr, c_int, c_ptr, c_int, c_int, c_i64, c_i64, c_i64, c_ptr, c_int, c_int, c_ptr, c_ptr, c_ptr],
    "hs_hp_ensemble_add_seg_host": [c_int, c_i64, c_ptr, c_int, c_ptr, c_int, c_int, c_i64, c_i64, c_i64, c_ptr, c_int, c_int, c_ptr, c_ptr],
    "hs_hp_ensemble_add_depth": [c_int, c_i64, c_ptr, c_int, c_ptr, c_int, c_i64, c_i64, c_ptr, c_int, c_ptr, c_ptr, c_ptr],
    "hs_hp_ensemble_add_depth_host": [c_int, c_i64, c_ptr, c_int, c_ptr, c_int, c_i64, c_i64, c_ptr, c_int, c_ptr, c_ptr],
    "hs_hp_ensemble_finish_seg": [c_i64, c_int, c_int, c_ptr, c_ptr, c_float, c_int, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr],
    "hs_hp_ensemble_finish_depth": [c_i64, c_int, c_ptr, c_ptr, c_float, c_ptr, c_ptr],
    "hs_hp_interp_weights_nest": [c_int, c_ptr, c_ptr, c_i64, c_ptr, c_ptr],
    "hs_backproject_labels": [c_ptr, c_int, c_i64, c_i64, c_int, c_i64, c_i64, c_i64, c_ptr, c_i64, c_int, c_ptr, c_ptr],
    "hs_backproject_image": [c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_i64, c_ptr, c_ptr],
    "hs_seg_confusion": [c_ptr, c_int, c_i64, c_i64, c_int, c_i64, c_i64, c_i64, c_ptr, c_i64, c_ptr, c_int, c_ptr, c_ptr, c_ptr],
    "hs_depth_points": [c_ptr, c_int, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_ptr, c_i64, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_ptr,
                        c_ptr],
    "hs_chamfer_nn": [c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                      c_ptr],
    "hs_depth_metrics": [c_ptr, c_int, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_ptr, c_int, c_i64, c_i64, c_i64, c_int,
                         ctypes.c_double, c_ptr, c_int, c_ptr, c_ptr, c_ptr],
    "hs_backproject_depth": [c_ptr, c_int, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_i64, c_ptr, c_ptr],
    "hs_flat_depth_to_hp": [c_ptr, c_int, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr],
    "hs_depth_metrics_gather": [c_ptr, c_int, c_i64, c_i64, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_int, c_i64, c_i64,
                                c_int, ctypes.c_double, c_ptr, c_int, c_ptr, c_ptr, c_ptr],
    "hs_sample_bilinear_u8_f32": [c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_i64, c_ptr, c_ptr],
    "hs_sample_nearest_f32": [c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_i64, c_float, c_ptr, c_ptr],
    "hs_sample_bilinear_u8_f32_per_sample": [c_ptr, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_i64, c_ptr, c_ptr],
    "hs_sample_nearest_f32_per_sample": [c_ptr, c_int, c_int, c_int, c_ptr, c_ptr, c_i64, c_float, c_ptr, c_ptr],
    "hs_depth_target": [c_ptr, c_i64, c_i64, c_ptr, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_float, c_float, c_ptr],
    "hs_depth_stats_update": [c_ptr, c_i64, c_int, c_int, c_ptr, c_ptr, c_ptr],
    "hs_depth_stats_merge": [c_ptr, c_int, c_ptr, c_ptr],
    "hs_histogram_update": [c_ptr, c_i64, c_int, c_int, c_ptr, c_int, c_ptr, c_ptr],
    "hs_select_rows": [c_ptr, c_int, c_i64, c_i64, c_i64, c_int, c_int, c_ptr, c_ptr, c_ptr],
    "hs_gelu_fwd": [c_ptr, c_ptr, c_i64, ctypes.c_float, ctypes.c_uint64, c_int, c_ptr],
    "hs_gelu_bwd": [c_ptr, c_ptr, c_ptr, c_i64, ctypes.c_float, ctypes.c_uint64, c_int, c_ptr],
    "hs_residual_drop": [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, ctypes.c_float, ctypes.c_uint64, c_int, c_ptr],
    "hs_linear_wgrad": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_ptr],
    "hs_reduce_flush": [c_ptr],
    "hs_set_seed_epoch": [c_ptr],
    "hs_linear_wgrad_gelu": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_ptr],
    "hs_linear_wgrad_gelu_supported": [c_i64, c_int, c_int, c_int],
    "hs_linear_wgrad_group_variant": [c_i64, c_int, c_int, c_int],
    "hs_linear_wgrad_group": [c_ptr, c_int, c_ptr, c_i64, c_int, c_ptr],
    "hs_mlp_fused_supported": [c_int, c_int, c_int],
    "hs_mlp_fused_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_uint,
                         c_int, c_ptr],
    "hs_mlp_fused_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_ptr],
    "hs_mlp_fused_drop_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_float,
                              ctypes.c_uint64, ctypes.c_uint64, c_i64, c_int, c_int, c_uint, c_int, c_ptr],
    "hs_mlp_fused_drop_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_float, ctypes.c_uint64, c_i64, c_int, c_int, c_int, c_ptr],
    "hs_adam_step": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_float, c_ptr, c_float, c_float, c_float, c_float, c_int, c_ptr, c_ptr],
    "hs_adam_advance": [c_ptr, c_ptr],
    "hs_grad_stats": [c_ptr, c_i64, c_ptr, c_int, c_ptr, c_ptr],
    "hs_grad_guard_finalize": [c_ptr, c_i64, c_ptr, c_int, c_int, c_float, c_ptr, c_ptr, c_ptr, c_ptr],
    "hs_adam_step_guarded": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_float, c_ptr, c_float, c_float, c_float, c_float, c_int, c_ptr, c_float,
                             c_ptr, c_int, c_ptr],
    "hs_adam_advance_guarded": [c_ptr, c_ptr, c_int, c_ptr, c_ptr],
    "hs_adam_step_groups": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_int, c_ptr, c_int, c_ptr, c_int, c_i64, c_ptr, c_ptr],
    "hs_adam_step_groups_guarded": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_int, c_ptr, c_int, c_ptr, c_int, c_i64, c_ptr, c_float,
                                    c_ptr, c_int, c_ptr],
    "hs_grad_scale": [c_ptr, c_i64, c_float, c_ptr, c_ptr],
    "hs_weight_avg_update": [c_ptr, c_ptr, c_i64, c_int, c_float, c_ptr, c_ptr, c_int, c_ptr],
    "hs_weight_avg_advance": [c_ptr, c_ptr, c_int, c_ptr],
    "hs_weight_avg_swap": [c_ptr, c_ptr, c_ptr, c_i64, c_ptr],
    "hs_split_bf16x3": [c_ptr, c_ptr, c_i64, c_int, c_int, c_ptr],
    "hs_gelu_split3": [c_ptr, c_ptr, c_ptr, c_i64, c_int, ctypes.c_float, ctypes.c_uint64, c_ptr],
    "hs_linear_wgrad_ld": [c_ptr, c_i64, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_ptr],
    "hs_layernorm_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_ptr],
    "hs_add_layernorm_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_ptr],
    "hs_add_layernorm_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_i64, c_int, c_int, c_ptr],
    "hs_layernorm_drop_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, ctypes.c_float, ctypes.c_uint64,
                              c_i64, c_int, c_int, c_ptr],
    "hs_layernorm_drop_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_i64, ctypes.c_float,
                              ctypes.c_uint64, c_i64, c_int, c_int, c_ptr],
    "hs_add_layernorm_drop_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, ctypes.c_float,
                                  ctypes.c_uint64, c_i64, c_int, c_int, c_ptr],
    "hs_layernorm_fwd_ex": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, ctypes.c_float,
                            ctypes.c_uint64, c_i64, c_int, c_int, c_ptr],
    "hs_add_layernorm_drop_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_i64,
                                  ctypes.c_float, ctypes.c_uint64, c_i64, c_int, c_int, c_ptr],
    "hs_seg_ce_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_i64, c_i64, c_i64, c_int, c_i64, c_int, c_ptr],
    "hs_seg_ce_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_i64,
                      c_int, c_ptr],
    "hs_depth_loss_fwd": [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_i64, c_i64, c_i64, c_int, c_float, c_int, c_ptr],
    "hs_depth_loss_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_float, c_int, c_ptr],
    "hs_gemm_nt": [c_ptr, c_i64, c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int,
                   ctypes.c_float, ctypes.c_uint64, c_int, c_ptr],
    "hs_lib_gemm_supported": [],
    "hs_lib_gemm_set_supported": [c_int],
    "hs_lib_gemm_nt": [c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_i64, c_int, c_int, c_ptr],
    "hs_lib_gemm_pick": [c_i64, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.c_char_p, c_int],
    "hs_lib_gemm_set_pick": [c_i64, c_int, c_int, c_int, c_int],
    "hs_gemm_nt_set_tile": [c_int],
    "hs_gemm_nt_tile_variant": [c_i64, c_int, c_int, c_int, c_int],
    "hs_set_reserved_cus": [c_int],
    "hs_transpose_many_16": [c_ptr, c_int, c_int, c_ptr],
    "hs_debug_occupy_cus": [c_int, c_int, c_int, ctypes.c_double, c_ptr],
    "hs_debug_buffer_soffset_probe": [c_ptr, c_int, c_int, c_ptr, c_ptr],
    "hs_window_attn_module_supported": [c_int, c_int, c_int, c_int],
    "hs_window_attn_module_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_int, c_i64,
                                  c_int, c_int, c_int, c_uint, c_int, c_ptr],
    "hs_window_attn_module_fwd_train": [c_ptr] * 17 + [c_i64] + [c_ptr] * 6 + [c_int, c_i64, c_int, c_int, c_int, c_uint, c_int, c_ptr],
    "hs_window_attn_module_bwd_chain": [c_ptr] * 14 + [c_i64] + [c_ptr] * 11 + [c_int, c_int, c_i64, c_int, c_int, c_int, c_uint, c_int, c_ptr],
    "hs_layernorm_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_i64, c_int, c_int, c_ptr],
    "hs_patch_merge_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_ptr],
    "hs_patch_merge_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_i64,
                           c_int, c_int, c_int, c_ptr],
    "hs_patch_expand_fwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_ptr],
    "hs_patch_expand_bwd": [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_i64,
                            c_int, c_int, c_int, c_int, c_ptr],
}
_OTHER = {
    "hs_version": ([], ctypes.c_char_p),
    "hs_last_error": ([], ctypes.c_char_p),
    "hs_status_string": ([c_int], ctypes.c_char_p),
    "hs_device_count": ([], c_int),
    "hs_get_reserved_cus": ([], c_int),
    "hs_grad_guard_piece": ([], c_int),
    "hs_adam_max_groups": ([], c_int),
    "hs_get_seed_epoch": ([], c_ptr),
    "hs_reduce_pending": ([c_ptr], c_int),
    "hs_layernorm_bwd_workspace": ([c_i64, c_int], c_i64),
    "hs_seg_ce_partials": ([c_i64, c_i64], c_i64),
    "hs_depth_loss_partials": ([c_i64, c_i64], c_i64),
    "hs_depth_points_workspace": ([c_i64, c_i64], c_i64),
    "hs_depth_metrics_partials": ([c_i64], c_i64),
    "hs_depth_stats_partials": ([c_i64], c_i64),
    "hs_select_rows_workspace": ([c_int], c_i64),
    "hs_flat_resize_lds_bytes": ([c_int, c_int, c_int, c_int, c_int, c_int], c_i64),
    "hs_ln_head_partials": ([c_i64], c_i64),
    "hs_expand_ln_head_blocks": ([c_i64], c_i64),
    "hs_linear_wgrad_workspace": ([c_i64, c_int, c_int], c_i64),
    "hs_linear_wgrad_group_workspace": ([c_ptr, c_int, c_i64, c_int], c_i64),
    "hs_window_attn_bwd_workspace": ([c_int, c_i64, c_int, c_int, c_int, c_int], c_i64),
    "hs_patch_merge_bwd_workspace": ([c_i64, c_int, c_int], c_i64),
    "hs_window_attn_module_bwd_chain_workspace": ([c_int, c_i64, c_int, c_int, c_int], c_i64),
    "hs_patch_expand_bwd_workspace": ([c_i64, c_int, c_int, c_int], c_i64),
}
EXPORTED_SYMBOLS = sorted(list(_SIGNATURES) + list(_OTHER))


def _load():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libhealswin.so not found at {LIB_PATH}: build it first (python heal_swin_amd/build.py, or "
            "__graft_entry__.build()).  heal_swin_amd has no CPU or PyTorch fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = c_int
    for name, (argtypes, restype) in _OTHER.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    return lib


lib = _load()


def check(status, what):
    if status != 0:
        msg = lib.hs_last_error().decode()
        kind = lib.hs_status_string(status).decode()
        if status == 1:  # HS_ERR_INVALID_ARG mirrors the reference's bare asserts
            raise AssertionError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed ({kind}): {msg}")


def version():
    return lib.hs_version().decode()


def device_count():
    return int(lib.hs_device_count())


def np_ptr(a):
    return None if a is None else a.ctypes.data_as(c_ptr)


def ptr(t):
    """Raw device/host pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr(device):
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dtype_code(dtype):
    import torch

    if dtype == torch.float32:
        return HS_F32
    if dtype == torch.bfloat16:
        return HS_BF16
    raise TypeError(f"heal_swin_amd kernels support float32 and bfloat16 activations, got {dtype}")


# ------------------------------------------------------------------ host tables (numpy in / out)
def nest2ring(nside, ipix):
    a = np.ascontiguousarray(ipix, dtype=np.int64)
    out = np.empty_like(a)
    check(lib.hs_nest2ring(int(nside), np_ptr(a), np_ptr(out), a.size), "hs_nest2ring")
    return out


def ring2nest(nside, ipix):
    a = np.ascontiguousarray(ipix, dtype=np.int64)
    out = np.empty_like(a)
    check(lib.hs_ring2nest(int(nside), np_ptr(a), np_ptr(out), a.size), "hs_ring2nest")
    return out


def nest_win_idcs(window_size):
    side = int(round(window_size ** 0.5))
    out = np.empty((max(side, 1), max(side, 1)), dtype=np.int64)
    check(lib.hs_nest_win_idcs(int(window_size), np_ptr(out)), "hs_nest_win_idcs")
    return out


def rel_pos_index(window_size):
    out = np.empty((window_size, window_size), dtype=np.int64)
    check(lib.hs_rel_pos_index(int(window_size), np_ptr(out)), "hs_rel_pos_index")
    return out


def _shift_out(n):
    return np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint8)


def build_nest_roll_shift(n_pix, window_size, shift_size):
    idx, inv, lab = _shift_out(n_pix)
    check(lib.hs_build_nest_roll_shift(int(n_pix), int(window_size), int(shift_size), np_ptr(idx), np_ptr(inv), np_ptr(lab)),
          "hs_build_nest_roll_shift")
    return idx, inv, lab


def build_nest_grid_shift(nside, base_pix, window_size):
    idx, inv, lab = _shift_out(max(base_pix, 0) * nside * nside)
    check(lib.hs_build_nest_grid_shift(int(nside), int(base_pix), int(window_size), np_ptr(idx), np_ptr(inv), np_ptr(lab)),
          "hs_build_nest_grid_shift")
    return idx, inv, lab


def build_ring_shift(nside, base_pix, window_size, shift_size):
    idx, inv, lab = _shift_out(max(base_pix, 0) * nside * nside)
    check(lib.hs_build_ring_shift(int(nside), int(base_pix), int(window_size), int(shift_size), np_ptr(idx), np_ptr(inv),
                                  np_ptr(lab)), "hs_build_ring_shift")
    return idx, inv, lab


def attn_mask_from_labels(labels, window_size):
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    out = np.empty((lab.size // window_size, window_size, window_size), dtype=np.float32)
    check(lib.hs_attn_mask_from_labels(np_ptr(lab), lab.size, int(window_size), np_ptr(out)), "hs_attn_mask_from_labels")
    return out


# ------------------------------------------------------------------ flat Swin-UNet tables (tiled Z order, include/healswin.h)
def flat_zorder(Ht, Wt, T):
    """(z_of_rm, rm_of_z) int32[Ht*Wt]: the tiled-Z index of each row-major token and its inverse."""
    z = np.empty(Ht * Wt, np.int32)
    rm = np.empty(Ht * Wt, np.int32)
    check(lib.hs_flat_zorder(int(Ht), int(Wt), int(T), np_ptr(z), np_ptr(rm)), "hs_flat_zorder")
    return z, rm


def build_flat_shift(Ht, Wt, T, window, shift):
    idx, inv, lab = _shift_out(max(Ht * Wt, 0))
    check(lib.hs_build_flat_shift(int(Ht), int(Wt), int(T), int(window), int(shift), np_ptr(idx), np_ptr(inv), np_ptr(lab)),
          "hs_build_flat_shift")
    return idx, inv, lab


def flat_rel_pos_index(window):
    """(row-major, Z-order) int64[w*w, w*w] relative-position indices of a w x w window."""
    n = window * window
    rm = np.empty((n, n), np.int64)
    z = np.empty((n, n), np.int64)
    check(lib.hs_flat_rel_pos_index(int(window), np_ptr(rm), np_ptr(z)), "hs_flat_rel_pos_index")
    return rm, z


def flat_attn_mask(Ht, Wt, window, shift):
    out = np.empty(((Ht // window) * (Wt // window), window * window, window * window), np.float32)
    check(lib.hs_flat_attn_mask(int(Ht), int(Wt), int(window), int(shift), np_ptr(out)), "hs_flat_attn_mask")
    return out
