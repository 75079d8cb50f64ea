"""Decoder tail: final LayerNorm + class head (+ expand, + cross-entropy) in one launch per direction
(swin_hp_transformer.py:433-452, :756-761, :781-788)."""

import torch

from .. import _lib
from .._lib import check, lib, ptr, stream_ptr
from .runtime import RT, _cast_param, _require_gpu, _timed  # noqa: F401
from .gemm import LinearFn, _input_grad, _param_grads  # noqa: F401


FUSED_LN_HEAD = True  # (tests flip the attribute to compare with the unfused tail)


def ln_head_ok(x, width, n_classes):
    """Whether `ln_head` (hs_ln_head_*) runs this decoder tail: bf16 rows on the GPU, C in 64..256 (multiple of 32), <= 16 classes."""
    return bool(FUSED_LN_HEAD and x.is_cuda and x.dtype == torch.bfloat16 and
                lib.hs_ln_head_supported(int(width), int(n_classes), _lib.HS_BF16))


class LnHeadFn(torch.autograd.Function):
    """LayerNorm(C) + bias-free 1x1 head as one pass over the rows, forward and backward (reference: the `norm` of
    FinalPatchExpand_X4, swin_hp_transformer.py:448-452, followed by `self.output`, :785-788): the normalised [rows, C] tensor is
    neither written nor saved.  Returns the padded logits [rows, 16] in FP32 (columns >= f_out are zero); backward takes their gradient.
    Parameter gradients come from ONE weight-gradient product over the raw rows (see csrc/ln_head.hip):
        X[k, c] = sum_rows dlogits[row, k] xhat[row, c] = hs_linear_wgrad(dlogits * rstd, y)[k, c] - sum_rows dlogits rstd mean
        dW = gamma X + beta u,   dgamma_c = sum_k W X,   dbeta_c = sum_k W u,   u[k] = sum_rows dlogits[row, k]."""

    KP = 16

    @staticmethod
    def forward(ctx, y2, gamma, beta, weight):
        _require_gpu(y2, gamma, beta, weight)
        rows, C = y2.shape
        wfold, bvec = _fold_head(gamma, beta, weight, C, y2.device)
        # fp32 logits: the tail's roundings (norm_up -> expand -> xhat -> logits) dominate the bf16 logit error of the whole
        # model (csrc/ln_head.hip); the logits therefore keep their accumulator value and xhat enters the head as hi + lo
        logits = torch.empty((rows, LnHeadFn.KP), dtype=torch.float32, device=y2.device)
        mean = torch.empty(rows, dtype=torch.float32, device=y2.device)
        rstd = torch.empty_like(mean)
        with _timed("ln_head_fwd", y2.device, rows * (2 * C + 4 * LnHeadFn.KP) + 8 * rows, 2 * rows * C * 32):
            check(lib.hs_ln_head_fwd(ptr(y2), ptr(wfold), ptr(bvec), ptr(logits), ptr(mean), ptr(rstd), rows, C, _lib.HS_BF16,
                                     _lib.HS_F32, stream_ptr(y2.device)), "hs_ln_head_fwd")
        ctx.save_for_backward(y2, mean, rstd, gamma, beta, weight)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        y2, mean, rstd, gamma, beta, weight = ctx.saved_tensors
        dy, dgamma, dbeta, dw = _ln_head_backward(y2, mean, rstd, gamma, beta, weight, dlogits, any(ctx.needs_input_grad[1:]))
        return (dy if ctx.needs_input_grad[0] else None), dgamma, dbeta, dw


def _ln_head_backward(y2, mean, rstd, gamma, beta, weight, dlogits, want_params, ce=None, depth=None):
    """(dy, dgamma, dbeta, dWhead) of logits = head(LayerNorm(y2)) by `hs_ln_head_bwd` + one weight-gradient product (LnHeadFn).
    ce = (labels u8 [rows], class weights or None, scale f32[1]): the logits' gradient is that of the weighted cross-entropy and is
    formed inside the kernel (`hs_ln_head_ce_bwd`) instead of being read; depth = (target f32 [rows], HS_DEPTH_* kind, huber
    delta, scale f32[1]): likewise for the depth-regression loss (`hs_ln_head_depth_bwd`)."""
    rows, C = y2.shape
    f_out, KP = weight.shape[0], LnHeadFn.KP
    dev = y2.device
    w = weight.detach().reshape(f_out, C).float()
    g32, b32 = gamma.detach().float(), beta.detach().float()
    afold = torch.zeros((C, KP), dtype=torch.bfloat16, device=dev)
    afold[:, :f_out] = (w * g32).t().to(torch.bfloat16)
    dy = torch.empty_like(y2)
    dprime = torch.empty((rows, KP), dtype=torch.bfloat16, device=dev)
    part = torch.empty((int(lib.hs_ln_head_partials(rows)), 32), dtype=torch.float32, device=dev)
    if ce is not None:
        labels, class_w, scale = ce
        wfold, bvec = _fold_head_ce(gamma, beta, weight, C, dev)
        with _timed("ln_head_ce_bwd", dev, rows * (4 * C + 2 * KP + 1) + 8 * rows, 2 * rows * C * (KP + 96)):
            check(lib.hs_ln_head_ce_bwd(ptr(y2), ptr(mean), ptr(rstd), ptr(labels), ptr(class_w), ptr(scale), f_out, ptr(wfold), ptr(bvec),
                                        ptr(afold), ptr(dy), ptr(dprime), ptr(part), rows, C, _lib.HS_BF16, stream_ptr(dev)),
                  "hs_ln_head_ce_bwd")
    elif depth is not None:
        target, kind, delta, scale = depth
        # (plain folded weight: the exchange of _fold_head_ce moves classes 4..11 only, a one- or two-channel head is unaffected)
        wfold, bvec = _fold_head(gamma, beta, weight, C, dev)
        with _timed("ln_head_depth_bwd", dev, rows * (4 * C + 2 * KP + 4) + 8 * rows, 2 * rows * C * (KP + 96)):
            check(lib.hs_ln_head_depth_bwd(ptr(y2), ptr(mean), ptr(rstd), ptr(target), kind, delta, ptr(scale), f_out, ptr(wfold),
                                           ptr(bvec), ptr(afold), ptr(dy), ptr(dprime), ptr(part), rows, C, _lib.HS_BF16, stream_ptr(dev)),
                  "hs_ln_head_depth_bwd")
    else:
        dlogits = dlogits.to(torch.float32).contiguous()
        with _timed("ln_head_bwd", dev, rows * (4 * C + 6 * KP) + 8 * rows, 2 * rows * C * KP):
            check(lib.hs_ln_head_bwd(ptr(y2), ptr(mean), ptr(rstd), ptr(dlogits), ptr(afold), ptr(dy), ptr(dprime), ptr(part), rows, C,
                                     _lib.HS_BF16, _lib.HS_F32, stream_ptr(dev)), "hs_ln_head_bwd")
    dgamma = dbeta = dw = None
    if want_params:
        ut = part.sum(0)
        u, t = ut[:f_out], ut[KP:KP + f_out]
        G = LinearFn._wgrad_hip(dprime, y2, KP, C, False)[0][:f_out]
        X = G - t[:, None]
        dw = (g32 * X + b32 * u[:, None]).to(weight.dtype).view(weight.shape)
        dgamma = (w * X).sum(0).to(gamma.dtype)
        dbeta = (w * u[:, None]).sum(0).to(beta.dtype)
    return dy, dgamma, dbeta, dw


def _fold_head(gamma, beta, weight, C, device):
    """(wfold [64, C] bf16: rows 0..31 = gamma * W rounded to bf16, rows 32..63 the rounding remainder (read by
    hs_expand_ln_head_fwd only); bvec [32] f32 = W beta) of the fused LayerNorm + head kernels."""
    f_out = weight.shape[0]
    w = weight.detach().reshape(f_out, C).float()
    wfold = torch.zeros((64, C), dtype=torch.bfloat16, device=device)
    prod = w * gamma.detach().float()
    wfold[:f_out] = prod.to(torch.bfloat16)
    wfold[32:32 + f_out] = (prod - wfold[:f_out].float()).to(torch.bfloat16)
    bvec = torch.zeros(32, dtype=torch.float32, device=device)
    bvec[:f_out] = w @ beta.detach().float()
    return wfold, bvec


FUSED_EXPAND_HEAD = True


def expand_ln_head_ok(x, width, children, n_classes):
    """Whether `expand_ln_head` (hs_expand_ln_head_fwd) runs the decoder tail: bf16 rows on the GPU, 4 children, C in {64, 96, 128}."""
    return bool(FUSED_EXPAND_HEAD and FUSED_LN_HEAD and x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] == width and
                lib.hs_expand_ln_head_supported(int(width), int(children), int(n_classes), _lib.HS_BF16))


def _tail_prelude(ctx, xn2, wexp, gamma, beta, weight, xn_lo):
    """The common start of the one-launch tail forwards (ExpandLnHeadFn, _tail_ce_forward, _tail_depth_forward): the operands as
    the kernels take them and the buffers a backward needs.  Returns (xn2, xn_lo [tokens, C] or None, wq: wexp in bf16, wfold, bvec,
    need: whether one of the five differentiable inputs wants a gradient, y [rows, C] bf16, mean, rstd f32 [rows]: None without
    `need`) and records on ctx what _tail_backward's input gradient reads (w_cast, cast_cache)."""
    tokens, C = xn2.shape
    xn2 = xn2.contiguous()
    xn_lo = None if xn_lo is None else xn_lo.reshape(tokens, C).contiguous()
    wq = _cast_param(wexp, torch.bfloat16).contiguous()
    wfold, bvec = _fold_head(gamma, beta, weight, C, xn2.device)
    need = any(ctx.needs_input_grad[:5])
    rows = tokens * (wexp.shape[0] // C)
    y = torch.empty((rows, C), dtype=torch.bfloat16, device=xn2.device) if need else None
    mean = torch.empty(rows, dtype=torch.float32, device=xn2.device) if need else None
    rstd = torch.empty_like(mean) if need else None
    ctx.w_cast = wq if wq.dtype != wexp.dtype else None
    ctx.cast_cache = RT.cast_cache
    return xn2, xn_lo, wq, wfold, bvec, need, y, mean, rstd


def _tail_backward(ctx, dy, dgamma, dbeta, dw):
    """The common end of the tail backwards: from `_ln_head_backward`'s results on the expanded rows, the gradients (dxn, dWexpand,
    dgamma, dbeta, dWhead) of the five differentiable inputs.  ctx: saved by a forward that began with _tail_prelude (xn2 first,
    wexp eighth)."""
    xn2, wexp = ctx.saved_tensors[0], ctx.saved_tensors[7]
    dy2 = dy.view(xn2.shape[0], wexp.shape[0])  # 'b (n p) c -> b n (p c)': the children of a token are consecutive rows
    dxn = _input_grad(dy2, wexp, ctx.w_cast, None, ctx.cast_cache) if ctx.needs_input_grad[0] else None
    ctx.w_cast = ctx.cast_cache = None
    dwexp, _ = _param_grads(dy2, xn2, wexp, None, ctx.needs_input_grad[1], False)
    return dxn, dwexp, dgamma, dbeta, dw


class ExpandLnHeadFn(torch.autograd.Function):
    """FinalPatchExpand_X4 (Linear C -> 4 C, view, LayerNorm(C)) + the 1x1 head as ONE forward kernel (reference
    swin_hp_transformer.py:442-452, :785-788; csrc/expand_ln_head.hip).  xn2 [tokens, C] bf16 -> padded fp32 logits [4 tokens, 16].
    With a gradient wanted the kernel also writes the expanded rows once (the backward's LayerNorm input); the backward is
    `hs_ln_head_bwd` on them followed by the Linear's input / weight gradients.  Without, the [4 tokens, C] tensor never exists."""

    @staticmethod
    def forward(ctx, xn2, wexp, gamma, beta, weight, xn_lo=None):
        _require_gpu(xn2, wexp, gamma, beta, weight, xn_lo)
        xn2, xn_lo, wq, wfold, bvec, need, y, mean, rstd = _tail_prelude(ctx, xn2, wexp, gamma, beta, weight, xn_lo)
        (tokens, C), P = xn2.shape, wexp.shape[0] // xn2.shape[1]
        rows = tokens * P
        logits = torch.empty((rows, LnHeadFn.KP), dtype=torch.float32, device=xn2.device)
        # algorithmic traffic: xn in, logits out (+ the expanded rows once in training); flops: expand + head (hi + lo)
        with _timed("expand_ln_head_fwd", xn2.device, 2 * tokens * C + rows * (4 * LnHeadFn.KP + (2 * C + 8 if need else 0)),
                    2 * rows * C * C + 4 * rows * C * 32):
            check(lib.hs_expand_ln_head_fwd(ptr(xn2), ptr(xn_lo), ptr(wq), ptr(wfold), ptr(bvec), ptr(y), ptr(logits), ptr(mean), ptr(rstd),
                                            tokens, C, P, _lib.HS_BF16, stream_ptr(xn2.device)), "hs_expand_ln_head_fwd")
        ctx.save_for_backward(xn2, y, mean, rstd, gamma, beta, weight, wexp)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        _, y, mean, rstd, gamma, beta, weight, _ = ctx.saved_tensors
        grads = _ln_head_backward(y, mean, rstd, gamma, beta, weight, dlogits, any(ctx.needs_input_grad[2:5]))
        return _tail_backward(ctx, *grads) + (None,)


_CE_PERM = {}


def _fold_head_ce(gamma, beta, weight, C, device):
    """The folded head weight for `hs_ln_head_ce_bwd`: as _fold_head, but with row blocks 4..7 and 8..11 exchanged, so that the
    kernel's accumulator register r < 8 of lane half h is class 8 h + r (csrc/ln_head_device.h:class_exchanged)."""
    wfold, bvec = _fold_head(gamma, beta, weight, C, device)
    key = str(device)
    if key not in _CE_PERM:  # (built once per device: six tiny launches per step otherwise)
        perm = list(range(4)) + list(range(8, 12)) + list(range(4, 8)) + list(range(12, 32))
        _CE_PERM[key] = (torch.tensor(perm + [i + 32 for i in perm], device=device), torch.tensor(perm, device=device))
    perm64, perm = _CE_PERM[key]
    return wfold[perm64], bvec[perm]  # (advanced indexing: fresh contiguous tensors)


def _tail_ce_forward(ctx, xn2, wexp, gamma, beta, weight, labels, class_w, xn_lo, step=False, preds=None, confmat=None, bad=None):
    """The forward of ExpandLnHeadCeFn, and with `step` (preds u8 [rows] or None, confmat i64 [K, K] or None, bad i64 [2] or None)
    that of ExpandLnHeadCeStepFn: the same launch arguments and saved tensors, `hs_expand_ln_head_ce_step_fwd` instead of
    `hs_expand_ln_head_ce_fwd`."""
    _require_gpu(xn2, wexp, gamma, beta, weight, labels, class_w, xn_lo)
    xn2, xn_lo, wq, wfold, bvec, need, y, mean, rstd = _tail_prelude(ctx, xn2, wexp, gamma, beta, weight, xn_lo)
    (tokens, C), P, f_out = xn2.shape, wexp.shape[0] // xn2.shape[1], weight.shape[0]
    rows = tokens * P
    labels = labels.reshape(-1)
    assert labels.dtype == torch.uint8 and labels.numel() == rows and labels.is_contiguous(), "labels: contiguous uint8, one per pixel row"
    parts = torch.empty((4 * int(lib.hs_expand_ln_head_blocks(tokens)), 2), dtype=torch.float32, device=xn2.device)
    # algorithmic traffic: xn in, labels in (+ the expanded rows once in training, + one byte per row of predictions); no logits
    if not step:
        with _timed("expand_ln_head_ce_fwd", xn2.device, 2 * tokens * C + rows * (1 + (2 * C + 8 if need else 0)),
                    2 * rows * C * C + 4 * rows * C * 32):
            check(lib.hs_expand_ln_head_ce_fwd(ptr(xn2), ptr(xn_lo), ptr(wq), ptr(wfold), ptr(bvec), ptr(labels), ptr(class_w), f_out,
                                               ptr(y), None, ptr(mean), ptr(rstd), ptr(parts), tokens, C, P, _lib.HS_BF16,
                                               stream_ptr(xn2.device)), "hs_expand_ln_head_ce_fwd")
    else:
        with _timed("expand_ln_head_ce_step_fwd", xn2.device,
                    2 * tokens * C + rows * (1 + (preds is not None) + (2 * C + 8 if need else 0)), 2 * rows * C * C + 4 * rows * C * 32):
            check(lib.hs_expand_ln_head_ce_step_fwd(ptr(xn2), ptr(xn_lo), ptr(wq), ptr(wfold), ptr(bvec), ptr(labels), ptr(class_w), f_out,
                                                    ptr(y), None, ptr(mean), ptr(rstd), ptr(parts), ptr(preds), ptr(confmat), ptr(bad),
                                                    tokens, C, P, _lib.HS_BF16, stream_ptr(xn2.device)), "hs_expand_ln_head_ce_step_fwd")
    tot = parts.sum(0)
    ctx.save_for_backward(xn2, y, mean, rstd, gamma, beta, weight, wexp, labels, class_w, tot)
    return tot[0] / tot[1]


class ExpandLnHeadCeFn(torch.autograd.Function):
    """The decoder tail AND the segmentation caller's weighted cross-entropy (reference swin_hp_transformer.py:442-452, :785-788 and
    models_lightning/segmentation/model_lightning_swin_hp.py:39-45, :104-111) as one forward and one backward kernel
    (`hs_expand_ln_head_ce_fwd`, `hs_ln_head_ce_bwd`): the [B, Npix, 16] fp32 logits and their gradient never exist in
    HBM.  xn2 [tokens, C] bf16, labels u8 [4 tokens] in pixel order -> scalar loss (fp32)."""

    @staticmethod
    def forward(ctx, xn2, wexp, gamma, beta, weight, labels, class_w, xn_lo):
        return _tail_ce_forward(ctx, xn2, wexp, gamma, beta, weight, labels, class_w, xn_lo)

    @staticmethod
    def backward(ctx, dloss):
        _, y, mean, rstd, gamma, beta, weight, _, labels, class_w, tot = ctx.saved_tensors
        scale = (dloss.to(torch.float32) / tot[1]).reshape(1)
        grads = _ln_head_backward(y, mean, rstd, gamma, beta, weight, None, any(ctx.needs_input_grad[2:5]), ce=(labels, class_w, scale))
        return _tail_backward(ctx, *grads) + (None, None, None)


class ExpandLnHeadCeStepFn(torch.autograd.Function):
    """The segmentation caller's whole `shared_step` on the decoder tail (models_lightning/segmentation/model_lightning_swin_hp.py:
    104-111: `preds = torch.max(outputs, 1)`, the weighted cross-entropy, IoU / Accuracy on (preds, masks)) as ONE forward kernel
    (`hs_expand_ln_head_ce_step_fwd`): ExpandLnHeadCeFn's loss bit for bit, plus the class id of every pixel row (uint8) and
    their confusion matrix with the labels, added to `confmat` (int64 [K, K]; labels >= K are counted in bad[0] instead) in place;
    still no logits.  The backward is ExpandLnHeadCeFn's.  Runs without a gradient too (nothing saved: validation)."""

    @staticmethod
    def forward(ctx, xn2, wexp, gamma, beta, weight, labels, class_w, xn_lo, confmat, bad, want_preds):
        f_out = weight.shape[0]
        if confmat is not None:
            _require_gpu(confmat, bad)
            assert bad is not None and bad.dtype == torch.int64 and bad.numel() == 2 and bad.is_contiguous(), "bad: int64 [2]"
            assert confmat.dtype == torch.int64 and confmat.shape == (f_out, f_out) and confmat.is_contiguous(), \
                f"confmat: contiguous int64 [{f_out}, {f_out}]"
        preds = torch.empty(labels.numel(), dtype=torch.uint8, device=xn2.device) if want_preds else None
        loss = _tail_ce_forward(ctx, xn2, wexp, gamma, beta, weight, labels, class_w, xn_lo, True, preds, confmat, bad)
        if preds is None:
            return loss, None
        ctx.mark_non_differentiable(preds)
        return loss, preds

    @staticmethod
    def backward(ctx, dloss, _dpreds):
        return ExpandLnHeadCeFn.backward(ctx, dloss) + (None, None, None)


def expand_ln_head_ce_step(xn2, wexp, gamma, beta, weight, labels, class_weights=None, xn_lo=None, confmat=None, bad=None, want_preds=True):
    """(loss, preds): expand_ln_head_ce's loss (bit for bit) and gradients, with the argmax of every pixel row (uint8 [4 tokens], as
    torch.max(logits, 1); None unless want_preds) and, with confmat int64 [K, K] + bad int64 [2], their confusion matrix with
    the labels added in place (evaluation.SegConfusion's `confmat` and `_bad`) -- one launch, no logits (ExpandLnHeadCeStepFn)."""
    return ExpandLnHeadCeStepFn.apply(xn2, wexp, gamma, beta, weight, labels, class_weights, xn_lo, confmat, bad, bool(want_preds))


def expand_ln_head_depth_ok(x, width, children, f_out, kind, delta):
    """Whether `expand_ln_head_depth` runs the decoder tail with the depth loss: as expand_ln_head_ok, and a head of one or two
    channels that the kind accepts (Huber: one; log variance: two)."""
    from ..losses import DEPTH_KINDS
    if kind in (DEPTH_KINDS["l1"], DEPTH_KINDS["l2"]):
        heads = (1, 2)
    else:
        heads = (1,) if kind == DEPTH_KINDS["huber"] else (2,)
    return f_out in heads and delta > 0 and expand_ln_head_ok(x, width, children, f_out)


def _tail_depth_forward(ctx, xn2, wexp, gamma, beta, weight, target, kind, delta, xn_lo, step=False, transform=None, metrics=None,
                        want_preds=False, batch=1):
    """The forward of ExpandLnHeadDepthFn, and with `step` (transform or None, DepthMetrics or None, want_preds, batch) that of
    ExpandLnHeadDepthStepFn: the same launch arguments and saved tensors, `hs_expand_ln_head_depth_step_fwd` instead of
    `hs_expand_ln_head_depth_fwd`; then returns (loss, preds f32 [f_out, rows] or None)."""
    _require_gpu(xn2, wexp, gamma, beta, weight, target, xn_lo)
    xn2, xn_lo, wq, wfold, bvec, need, y, mean, rstd = _tail_prelude(ctx, xn2, wexp, gamma, beta, weight, xn_lo)
    (tokens, C), P, f_out, dev = xn2.shape, wexp.shape[0] // xn2.shape[1], weight.shape[0], xn2.device
    rows = tokens * P
    target = target.reshape(-1)
    assert target.dtype == torch.float32 and target.numel() == rows and target.is_contiguous(), "target: contiguous fp32, one per pixel row"
    blocks = int(lib.hs_expand_ln_head_blocks(tokens))
    parts = torch.empty((4 * blocks, 2), dtype=torch.float32, device=dev)
    preds = None
    # algorithmic traffic: xn in, target in (+ the expanded rows once in training, + the predictions); no head rows
    if not step:
        with _timed("expand_ln_head_depth_fwd", dev, 2 * tokens * C + rows * (4 + (2 * C + 8 if need else 0)),
                    2 * rows * C * C + 4 * rows * C * 32):
            check(lib.hs_expand_ln_head_depth_fwd(ptr(xn2), ptr(xn_lo), ptr(wq), ptr(wfold), ptr(bvec), ptr(target), kind, delta, f_out,
                                                  ptr(y), None, ptr(mean), ptr(rstd), ptr(parts), tokens, C, P, _lib.HS_BF16,
                                                  stream_ptr(dev)), "hs_expand_ln_head_depth_fwd")
    else:
        flags, tcode, shift, scale = (0, _lib.HS_DT_NONE, 0.0, 1.0) if transform is None else transform.inverse_op()
        use_logvar = metrics is not None and metrics.use_logvar
        preds = torch.empty((f_out, rows), dtype=torch.float32, device=dev) if want_preds else None
        # MeanSTDMedian reads the log variance itself: channel 1 of the predictions, or 4 bytes per row of scratch
        logvar = torch.empty(rows, dtype=torch.float32, device=dev) if use_logvar and preds is None else None
        state = mparts = rng = None
        n_ranges, total_mean = 0, 0.0
        if metrics is not None:
            state, rng, n_ranges = metrics.state, metrics._ranges, len(metrics.distance_ranges)
            total_mean = 0.0 if metrics.total_mean is None else metrics.total_mean
            mparts = torch.empty((blocks, state.numel()), dtype=torch.float64, device=dev)
        written = (0 if preds is None else 4 * f_out) + (0 if logvar is None else 4)
        with _timed("expand_ln_head_depth_step_fwd", dev, 2 * tokens * C + rows * (4 + written + (2 * C + 8 if need else 0)),
                    2 * rows * C * C + 4 * rows * C * 32):
            check(lib.hs_expand_ln_head_depth_step_fwd(ptr(xn2), ptr(xn_lo), ptr(wq), ptr(wfold), ptr(bvec), ptr(target), kind, delta, f_out,
                                                       ptr(y), None, ptr(mean), ptr(rstd), ptr(parts), flags, tcode, shift, scale,
                                                       int(use_logvar), total_mean, _lib.np_ptr(rng) if n_ranges else None, n_ranges,
                                                       ptr(mparts), ptr(state), ptr(preds), ptr(logvar), tokens, C, P, _lib.HS_BF16,
                                                       stream_ptr(dev)), "hs_expand_ln_head_depth_step_fwd")
        if use_logvar:
            metrics.add_median((preds[1] if preds is not None else logvar).view(batch, -1))
    tot = parts.sum(0)
    ctx.save_for_backward(xn2, y, mean, rstd, gamma, beta, weight, wexp, target, tot)
    ctx.kind, ctx.delta = kind, delta
    loss = tot[0] / tot[1]
    return (loss, preds) if step else loss


class ExpandLnHeadDepthFn(torch.autograd.Function):
    """The decoder tail AND the depth caller's regression loss (losses.depth_loss's kinds; reference
    training/loss_depth_regression.py) as one forward and one backward kernel (`hs_expand_ln_head_depth_fwd`,
    `hs_ln_head_depth_bwd`): the [B, Npix, 16] fp32 head rows and their gradient never exist in HBM.  xn2 [tokens, C] bf16,
    target f32 [4 tokens] in pixel order -> scalar loss (fp32)."""

    @staticmethod
    def forward(ctx, xn2, wexp, gamma, beta, weight, target, kind, delta, xn_lo):
        return _tail_depth_forward(ctx, xn2, wexp, gamma, beta, weight, target, kind, delta, xn_lo)

    @staticmethod
    def backward(ctx, dloss):
        _, y, mean, rstd, gamma, beta, weight, _, target, tot = ctx.saved_tensors
        scale = (dloss.to(torch.float32) / tot[1]).reshape(1)
        grads = _ln_head_backward(y, mean, rstd, gamma, beta, weight, None, any(ctx.needs_input_grad[2:5]),
                                  depth=(target, ctx.kind, ctx.delta, scale))
        return _tail_backward(ctx, *grads) + (None, None, None, None)


def expand_ln_head_depth(xn2, wexp, gamma, beta, weight, target, kind, delta=1.0, xn_lo=None):
    """Depth-regression loss (HS_DEPTH_* kind, losses.DEPTH_KINDS) of head(LayerNorm(expand(xn2 [+ xn_lo]) viewed per child))
    against an fp32 per-pixel-row target, without the head rows (ExpandLnHeadDepthFn)."""
    return ExpandLnHeadDepthFn.apply(xn2, wexp, gamma, beta, weight, target, int(kind), float(delta), xn_lo)


class ExpandLnHeadDepthStepFn(torch.autograd.Function):
    """The depth caller's whole `shared_step` on the decoder tail (models_lightning/depth_estimation/model_lightning_depth_swin_hp.py:
    132-159: the loss in the normalised space, `unnormalize_and_retransform` of prediction and target, the metrics' update) as ONE
    forward kernel plus the one-workgroup merge of the metric records (`hs_expand_ln_head_depth_step_fwd`): ExpandLnHeadDepthFn's
    loss bit for bit, the sums of `hs_depth_metrics` on (metres, target in metres) added to a DepthMetrics' state, and the
    prediction fp32 [f_out, rows] (channel 0 in metres, channel 1 the log variance); still no head rows.  The backward is
    ExpandLnHeadDepthFn's.  Runs without a gradient too (nothing saved: validation).  No host synchronisation."""

    @staticmethod
    def forward(ctx, xn2, wexp, gamma, beta, weight, target, kind, delta, xn_lo, transform, metrics, want_preds, batch):
        loss, preds = _tail_depth_forward(ctx, xn2, wexp, gamma, beta, weight, target, kind, delta, xn_lo, True, transform, metrics,
                                          want_preds, batch)
        if preds is None:
            return loss, None
        ctx.mark_non_differentiable(preds)
        return loss, preds

    @staticmethod
    def backward(ctx, dloss, _dpreds):
        return ExpandLnHeadDepthFn.backward(ctx, dloss) + (None, None, None, None)


def expand_ln_head_depth_step(xn2, wexp, gamma, beta, weight, target, kind, delta=1.0, xn_lo=None, transform=None, metrics=None,
                              want_preds=True, batch=1):
    """(loss, preds): expand_ln_head_depth's loss (bit for bit) and gradients against the NORMALISED fp32 target, with the
    prediction fp32 [f_out, 4 tokens] (channel 0 = transform.unnormalize_and_retransform of the head's channel 0: metres; channel 1
    the raw log variance; None unless want_preds) and, with metrics (a depth_evaluation.DepthMetrics on the same device), its update
    on (preds, transform.unnormalize_and_retransform(target)) -- rows split into `batch` samples for median_std -- in one launch
    without the head rows (ExpandLnHeadDepthStepFn).  transform: a depth_data.DepthTargetTransform or None (the identity)."""
    if metrics is not None and metrics.use_logvar and weight.shape[0] < 2:
        raise ValueError("metrics.use_logvar needs a two-channel head (mean, log variance)")
    if metrics is not None and metrics.state.device != xn2.device:
        raise ValueError(f"metrics live on {metrics.state.device}, the rows on {xn2.device}")
    return ExpandLnHeadDepthStepFn.apply(xn2, wexp, gamma, beta, weight, target, int(kind), float(delta), xn_lo, transform, metrics,
                                         bool(want_preds), int(batch))


def expand_ln_head_ce(xn2, wexp, gamma, beta, weight, labels, class_weights=None, xn_lo=None):
    """Weighted cross-entropy of head(LayerNorm(expand(xn2 [+ xn_lo]) viewed per child)) against uint8 pixel labels, without the
    logits (ExpandLnHeadCeFn)."""
    return ExpandLnHeadCeFn.apply(xn2, wexp, gamma, beta, weight, labels, class_weights, xn_lo)


def expand_ln_head(xn2, wexp, gamma, beta, weight, xn_lo=None):
    """Padded fp32 logits [4 tokens, 16] of head(LayerNorm(expand(xn2 [+ xn_lo]) viewed per child)); the caller slices [..., :f_out].
    xn_lo: the rounding remainder of xn2 (`layer_norm_hilo`), used by the forward product only (the gradients take xn2)."""
    return ExpandLnHeadFn.apply(xn2, wexp, gamma, beta, weight, xn_lo)


def ln_head(y2, gamma, beta, weight):
    """Padded logits [rows, 16] of head(LayerNorm(y2)); the caller slices [..., :f_out]."""
    return LnHeadFn.apply(y2, gamma, beta, weight)
