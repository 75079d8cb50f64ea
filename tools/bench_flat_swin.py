#!/usr/bin/env python3
"""bf16 training step of the paper's flat Swin-UNet (640 x 768, patch 2, window 8, shift 2, embed 96, depths [2, 2, 6, 2], cosine
attention, v2 placement, 12 classes) next to HEAL-SWIN-T at nside 256 (bench.WORKLOADS["T256"]), same process, same warm-up and
timing: forward + forward_seg_loss, backward, FlatAdam.  Prints images/s and time per token of both, then the time and achieved
bandwidth of each image-boundary layout kernel (csrc/flat_layout.hip; bytes from the shapes: one read + one write).

    python tools/bench_flat_swin.py [--batch 8] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAT_CFG = dict(patch_size=2, window_size=8, shift_size=2, embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24],
                use_cos_attn=True, use_v2_norm_placement=True)
FLAT_SIZE = (640, 768)


def build_flat():
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_transformer import SwinTransformerConfig, SwinTransformerSys
    torch.manual_seed(0)
    spec = DataSpec(dim_in=FLAT_SIZE, f_in=3, f_out=12, base_pix=None)
    return SwinTransformerSys(SwinTransformerConfig(**FLAT_CFG), spec), spec


def time_train_step(model, imgs, labels, steps, warmup):
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    model = model.cuda().train()
    model.compute_dtype = torch.bfloat16
    dp = GradBucketAllReduce(model.parameters())
    opt = FlatAdam(model.parameters(), dp, lr=1e-4, model=model)

    def step():
        dp.zero_grad()
        loss = model.forward_seg_loss(imgs, labels)
        loss.backward()
        dp.finish()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    assert torch.isfinite(loss)
    return dt


def time_op(fn, reps=50):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import bench
    from heal_swin_amd import ops

    B = args.batch
    g = torch.Generator(device="cuda").manual_seed(1234)
    H, W = FLAT_SIZE
    results = {}

    flat, _ = build_flat()
    imgs = torch.randint(0, 256, (B, 3, H, W), generator=g, device="cuda", dtype=torch.uint8)
    labels = torch.randint(0, 12, (B, H, W), generator=g, device="cuda", dtype=torch.uint8)
    dt = time_train_step(flat, imgs.float(), labels, args.steps, args.warmup)
    tokens = (H // 2) * (W // 2)
    results["flat_swin"] = dict(step_ms=dt * 1e3, images_per_s=B / dt, ns_per_token=dt / (B * tokens) * 1e9, tokens_per_image=tokens)
    T = flat.tile
    del flat
    torch.cuda.empty_cache()

    wl = bench.WORKLOADS["T256"]
    hp_model, _, spec = bench.build_model(wl)
    n = spec["dim_in"]
    imgs_hp = torch.randint(0, 256, (B, 3, n), generator=g, device="cuda", dtype=torch.uint8).float()
    labels_hp = torch.randint(0, 12, (B, n), generator=g, device="cuda", dtype=torch.uint8)
    dt = time_train_step(hp_model, imgs_hp, labels_hp, args.steps, args.warmup)
    tokens = n // 4
    results["T256"] = dict(step_ms=dt * 1e3, images_per_s=B / dt, ns_per_token=dt / (B * tokens) * 1e9, tokens_per_image=tokens)
    del hp_model
    torch.cuda.empty_cache()
    results["flat_over_T256_per_token"] = results["flat_swin"]["ns_per_token"] / results["T256"]["ns_per_token"]

    # layout kernels at the step's shapes
    x8 = imgs
    x32 = imgs.float()
    rows16 = torch.randn((B, H * W, 16), device="cuda")[:, :, :12]
    dimg = torch.randn((B, 12, H, W), device="cuda")
    patch_rows = ops.flat_patch_rows(x32, 2, T, torch.bfloat16)
    K = patch_rows.shape[-1]
    npatch = B * (H // 2) * (W // 2)
    kernels = {
        "patch_rows u8->bf16": (lambda: ops.patch._img_to_rows(x8, patch_rows, 2, T, 0, K), x8.numel() + npatch * K * 2),
        "patch_rows f32->bf16": (lambda: ops.patch._img_to_rows(x32, patch_rows, 2, T, 0, K), x32.numel() * 4 + npatch * K * 2),
        "patch_rows bwd bf16->f32": (lambda: ops.patch._rows_to_img(patch_rows, x32, 2, T, 0, K), x32.numel() * 4 + npatch * K * 2),
        "logits rows(16)->NCHW": (lambda: ops.flat_pixel_image(rows16, H, W, 2, T), B * H * W * 16 * 4 + dimg.numel() * 4),
        "NCHW->logits rows(16) (bwd)": (lambda: ops.patch._img_to_rows(dimg, rows16._base if rows16._base is not None else rows16, 2, T, 1, 16),
                                        B * H * W * 16 * 4 + dimg.numel() * 4),
        "labels u8->pixel rows": (lambda: ops.flat_labels(labels, 2, T), 2 * labels.numel()),
    }
    lay = {}
    for name, (fn, nbytes) in kernels.items():
        t = time_op(fn)
        lay[name] = dict(us=t * 1e6, GBps=nbytes / t / 1e9, bytes=nbytes)
    results["layout_kernels"] = lay
    step_s = results["flat_swin"]["step_ms"] * 1e-3
    in_step = lay["patch_rows f32->bf16"]["us"] + lay["labels u8->pixel rows"]["us"]
    results["layout_share_of_step"] = in_step * 1e-6 / step_s
    for k in ("flat_swin", "T256"):
        r = results[k]
        print(f"{k:10s} batch {B}: {r['step_ms']:.1f} ms/step  {r['images_per_s']:.1f} images/s  {r['ns_per_token']:.3f} ns/token "
              f"({r['tokens_per_image']} tokens/image)")
    print(f"flat / T256 time per token: {results['flat_over_T256_per_token']:.3f}")
    for k, v in lay.items():
        print(f"  {k:30s} {v['us']:8.1f} us  {v['GBps']:7.1f} GB/s")
    print(f"layout kernels of the training step (patch rows, labels): {100 * results['layout_share_of_step']:.2f} % of the step")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
