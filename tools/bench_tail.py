#!/usr/bin/env python3
"""Decoder tail + segmentation loss at the headline shape (HEAL-SWIN-B, nside 256, 12 base pixels, batch 8: 1 572 864 tokens x 128
channels -> 6 291 456 pixel rows x 12 classes), forward + backward, event-timed:
   fused    ops.expand_ln_head_ce      (hs_expand_ln_head_ce_fwd, hs_ln_head_ce_bwd: no logits tensor)
   unfused  ops.expand_ln_head + losses.seg_loss   (fp32 logits written, CE forward / backward kernels, dlogits read back)
usage: bench_tail.py [--mode fused|unfused|both] [--iters 5]
Under `rocprofv3 --pmc WRITE_SIZE --kernel-trace` with one --mode, tools/pmc_db.py sums the bytes the tail's kernels write.

--forward times the FORWARD of the segmentation caller's shared_step (loss, class ids, confusion matrix), with a gradient wanted
(training: the expanded rows are written for the backward) and without (validation), alternating the forms in every round:
   step      ops.expand_ln_head_ce_step  (hs_expand_ln_head_ce_step_fwd: one launch, labels in, one byte per pixel out)
   loss      ops.expand_ln_head_ce       (hs_expand_ln_head_ce_fwd: the loss alone)
   composed  ops.expand_ln_head + losses.seg_loss + losses.seg_predictions + SegConfusion.update (the logits written, read thrice)
`step` is skipped on a build that lacks it (the parent commit's, for the baseline of the same session); --forms picks a subset
and --grad train|valid one of the two (one form and one mode per process under rocprofv3 --pmc: tools/collect_tail_step_pmc.sh).

--depth times the FORWARD of the depth caller's shared_step at the depth T model's tail (nside 256, 8 base pixels, batch 8:
1 048 576 tokens x 96 -> 4 194 304 pixel rows), f_out 1 and 2 (--f-out), with and without a gradient, the forms alternating:
   loss        ops.expand_ln_head_depth       (hs_expand_ln_head_depth_fwd: the loss alone; exists on the parent commit)
   composed    ops.expand_ln_head + losses.depth_step_from_rows' parts: the rows written, hs_depth_loss_fwd, hs_depth_target twice,
               hs_depth_metrics (+ the hs_select_rows median with the log variance): the validation route without the fused step
   step        ops.expand_ln_head_depth_step  (hs_expand_ln_head_depth_step_fwd + the merge of the records), predictions returned
   step_nop    the same without the predictions
Each line gives min / median / max over the rounds and the HBM bytes the form writes."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heal_swin_amd import ops  # noqa: E402
from heal_swin_amd.losses import seg_loss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="both")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=8 * 196608)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--forms", default="step,loss,composed")
    ap.add_argument("--grad", default="both", choices=("train", "valid", "both"))
    ap.add_argument("--depth", action="store_true")
    ap.add_argument("--f-out", default="1,2")
    a = ap.parse_args()
    if a.depth:
        return depth_forms(a)
    dev, C, f_out, B = "cuda", a.width, 12, 8
    g = torch.Generator(device=dev).manual_seed(0)
    xn = torch.randn(a.tokens, C, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    wexp = (torch.randn(4 * C, C, device=dev, generator=g) * C ** -0.5).requires_grad_(True)
    gamma = torch.ones(C, device=dev, requires_grad=True)
    beta = torch.zeros(C, device=dev, requires_grad=True)
    w = (torch.randn(f_out, C, 1, device=dev, generator=g) * C ** -0.5).requires_grad_(True)
    labels = torch.randint(0, f_out, (B, 4 * a.tokens // B), device=dev, dtype=torch.uint8, generator=g)

    def fused():
        ops.expand_ln_head_ce(xn, wexp, gamma, beta, w, labels, None).backward()

    def unfused():
        lg = ops.expand_ln_head(xn, wexp, gamma, beta, w)
        logits = ops.pad_slice(lg.view(B, -1, 16), f_out).transpose(1, 2)
        seg_loss(logits, labels).backward()

    if a.forward:
        return forward_forms(a, xn, wexp, gamma, beta, w, labels, f_out, B)

    for name, fn in (("fused", fused), ("unfused", unfused)):
        if a.mode not in ("both", name):
            continue
        ts = []
        for it in range(a.iters + 2):
            for t in (xn, wexp, gamma, beta, w):
                t.grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:
                ts.append(e0.elapsed_time(e1))
        print(f"{name:8s} tail fwd + loss + bwd: min {min(ts):.3f} ms  median {sorted(ts)[len(ts) // 2]:.3f} ms  ({a.tokens} tokens x {C})", flush=True)


def forward_forms(a, xn, wexp, gamma, beta, w, labels, f_out, B):
    from heal_swin_amd.evaluation import SegConfusion
    from heal_swin_amd.losses import seg_predictions
    conf = SegConfusion(f_out)
    rows, C = 4 * a.tokens, a.width

    def step():
        return ops.expand_ln_head_ce_step(xn, wexp, gamma, beta, w, labels, None, confmat=conf.confmat, bad=conf._bad)

    def loss():
        return ops.expand_ln_head_ce(xn, wexp, gamma, beta, w, labels, None)

    def composed():
        lg = ops.expand_ln_head(xn, wexp, gamma, beta, w)
        logits = ops.pad_slice(lg.view(B, -1, 16), f_out).transpose(1, 2)
        out = seg_loss(logits, labels)
        conf.update(logits.detach(), labels, check=False)
        return out, seg_predictions(logits.detach()).to(torch.uint8)

    forms = [(n, f) for n, f in (("step", step), ("loss", loss), ("composed", composed)) if n in a.forms.split(",")]
    if not hasattr(ops, "expand_ln_head_ce_step"):
        forms = [(n, f) for n, f in forms if n != "step"]
    # the bytes the algorithm needs: xn and the labels in (+ the expanded rows, mean, rstd out in training)
    base = {True: 2 * a.tokens * C + rows * (1 + 2 * C + 8), False: 2 * a.tokens * C + rows}
    # composed: the padded fp32 logits written once, read by the loss, the argmax and the confusion kernel (which reads the labels
    # again); the argmax's int64 indices written, read and narrowed to bytes
    extra = {"step": rows, "loss": 0, "composed": rows * (64 + 3 * 64 + 1 + 8 + 8 + 1)}
    for grad in [g for g, n in ((True, "train"), (False, "valid")) if a.grad in ("both", n)]:
        ts = {n: [] for n, _ in forms}
        with torch.set_grad_enabled(grad):
            for it in range(a.iters + 2):
                for n, fn in forms:  # alternating: every round times each form once
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= 2:
                        ts[n].append(e0.elapsed_time(e1))
        for n, _ in forms:
            t = sorted(ts[n])
            print(f"{'train' if grad else 'valid'} forward {n:9s} min {t[0]:.3f} ms  median {t[len(t) // 2]:.3f} ms  max {t[-1]:.3f} ms  "
                  f"algorithmic {(base[grad] + extra[n]) / 1e6:.1f} MB  ({a.tokens} tokens x {C}, {len(t)} rounds)", flush=True)


def depth_forms(a):
    from heal_swin_amd.depth_data import DepthTargetTransform
    from heal_swin_amd.depth_evaluation import DepthMetrics
    from heal_swin_amd.losses import DEPTH_KINDS, _DepthLossFn
    dev, B = "cuda", 8
    tokens = a.tokens if a.tokens != 8 * 196608 else 8 * 131072
    C = a.width if a.width != 128 else 96
    rows = 4 * tokens
    tr = DepthTargetTransform("log", "standardize")
    for f_out in [int(v) for v in a.f_out.split(",")]:
        g = torch.Generator(device=dev).manual_seed(0)
        xn = torch.randn(tokens, C, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
        wexp = (torch.randn(4 * C, C, device=dev, generator=g) * C ** -0.5).requires_grad_(True)
        gamma = torch.ones(C, device=dev, requires_grad=True)
        beta = torch.zeros(C, device=dev, requires_grad=True)
        w = (torch.randn(f_out, C, 1, device=dev, generator=g) * 0.3 * C ** -0.5).requires_grad_(True)
        depth = 0.3 + 40.0 * torch.rand(B, rows // B, device=dev, generator=g) ** 2
        depth[torch.rand(B, rows // B, device=dev, generator=g) < 0.04] = 0.0
        target = tr.prepare(depth)
        use_logvar = f_out == 2
        kind = DEPTH_KINDS["logvar" if use_logvar else "l1"]
        met = DepthMetrics(total_mean=11.5, distance_ranges=[(0.0, 5.0), (5.0, 20.0), (20.0, 100.0)], use_logvar=use_logvar)

        def loss():
            return ops.expand_ln_head_depth(xn, wexp, gamma, beta, w, target, kind, 1.0)

        def composed():  # (the calls of losses.depth_step_from_rows, every one of which the parent commit has)
            lg = ops.expand_ln_head(xn, wexp, gamma, beta, w)
            pred = ops.pad_slice(lg.view(B, -1, 16), f_out).transpose(1, 2)
            out = _DepthLossFn.apply(pred, target, kind, 1.0)
            with torch.no_grad():
                preds = pred.detach().clone()
                tr.unnormalize_and_retransform(preds[:, 0], out=preds[:, 0])
                met.update(preds, tr.unnormalize_and_retransform(target))
            return out, preds

        def step():
            return ops.expand_ln_head_depth_step(xn, wexp, gamma, beta, w, target, kind, 1.0, None, tr, met, True, B)

        def step_nop():
            return ops.expand_ln_head_depth_step(xn, wexp, gamma, beta, w, target, kind, 1.0, None, tr, met, False, B)

        forms = [("loss", loss), ("composed", composed), ("step", step), ("step_nop", step_nop)]
        if not hasattr(ops, "expand_ln_head_depth_step"):
            forms = forms[:2]
        # HBM bytes WRITTEN: the expanded rows, mean and rstd in training; composed: the padded fp32 rows, the clone of the f_out
        # channels, channel 0 rewritten in place, the target in metres; step: the predictions (or the log variance alone)
        train = rows * (2 * C + 8)
        written = {"loss": 0, "composed": rows * (64 + 4 * f_out + 4 + 4), "step": rows * 4 * f_out, "step_nop": rows * 4 * (f_out - 1)}
        for grad in [gr for gr, n in ((True, "train"), (False, "valid")) if a.grad in ("both", n)]:
            ts = {n: [] for n, _ in forms}
            with torch.set_grad_enabled(grad):
                for it in range(a.iters + 3):
                    for n, fn in forms:  # alternating: every round times each form once
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        torch.cuda.synchronize()
                        if it >= 3:
                            ts[n].append(e0.elapsed_time(e1))
            for n, _ in forms:
                t = sorted(ts[n])
                print(f"depth f_out={f_out} {'train' if grad else 'valid'} forward {n:9s} min {t[0]:.3f} ms  median {t[len(t) // 2]:.3f} ms  "
                      f"max {t[-1]:.3f} ms  written {((train if grad else 0) + written[n]) / 1e6:.1f} MB  ({tokens} tokens x {C}, "
                      f"{len(t)} rounds)", flush=True)


if __name__ == "__main__":
    main()
