"""Depth training step with the loss fused into the decoder tail (model.forward_depth_loss) against the composition
(losses.depth_l1_loss(model(x), target)) on the same box, same weights, same data:

  D256 (HEAL-SWIN-T, nside 256, 8 base pixels, f_out 1): bf16 at batch 8 and fp32 at batch 2;
  the flat depth model (the paper's flat Swin-UNet at 640 x 768, f_out 1): bf16 at batch 2.

One JSON line per case: median step time (forward + loss + backward, parameter gradients zeroed in place) of both paths.
    python tools/bench_depth_loss.py [--steps 10] [--warmup 3] [--cases D256_bf16,D256_fp32,flat_bf16]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAT_CFG = dict(patch_size=2, window_size=8, shift_size=2, embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24],
                use_cos_attn=True, use_v2_norm_placement=True, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0)


def build(case):
    if case.startswith("D256"):
        import bench
        model, _, spec = bench.build_model(bench.WORKLOADS["D256"])
        batch, dtype = (8, torch.bfloat16) if case.endswith("bf16") else (2, torch.float32)
        shape_x, shape_t = (batch, 3, spec["dim_in"]), (batch, spec["dim_in"])
    else:
        from heal_swin_amd.data_spec import DataSpec
        from heal_swin_amd.models_torch.swin_transformer import SwinTransformerConfig, SwinTransformerSys
        torch.manual_seed(0)
        model = SwinTransformerSys(SwinTransformerConfig(**FLAT_CFG), DataSpec(dim_in=(640, 768), f_in=3, f_out=1, base_pix=None,
                                                                               class_names=[]))
        batch, dtype = 2, torch.bfloat16
        shape_x, shape_t = (batch, 3, 640, 768), (batch, 640, 768)
    model = model.cuda().train()
    model.compute_dtype = dtype
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randint(0, 256, shape_x, generator=g, device="cuda", dtype=torch.uint8).float()
    t = torch.rand(shape_t, generator=g, device="cuda") * 4 - 2
    t.view(-1)[::17] = float("inf")  # background pixels
    return model, x, t, batch, dtype


def time_steps(fn, model, steps, warmup):
    params = [p for p in model.parameters() if p.requires_grad]
    times = []
    for i in range(warmup + steps):
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn().backward()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="D256_bf16,D256_fp32,flat_bf16")
    args = ap.parse_args()
    from heal_swin_amd.losses import depth_l1_loss
    for case in args.cases.split(","):
        model, x, t, batch, dtype = build(case)
        fused = time_steps(lambda: model.forward_depth_loss(x, t, "l1"), model, args.steps, args.warmup)
        composed = time_steps(lambda: depth_l1_loss(model(x), t), model, args.steps, args.warmup)
        with torch.no_grad():
            lf, lc = float(model.forward_depth_loss(x, t, "l1")), float(depth_l1_loss(model(x), t))
        print(json.dumps(dict(case=case, batch=batch, dtype=str(dtype).replace("torch.", ""), fused_ms=round(fused[0], 3),
                              fused_min_ms=round(fused[1], 3), composed_ms=round(composed[0], 3), composed_min_ms=round(composed[1], 3),
                              gain=round(1 - fused[0] / composed[0], 4), loss_fused_nograd=lf, loss_composed=lc)), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
