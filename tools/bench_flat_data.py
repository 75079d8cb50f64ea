#!/usr/bin/env python3
"""The flat data path at WoodScape size (batch 8 of 966 x 1280 frames), two workloads, each timed two ways:
  seg     frames + class masks -> 640 x 768                                       (p = 2, tile 64: the paper's flat model)
  depth   frames + depth maps  -> 512 x 678 -> 512 x 640, bilinear depth, log + standardize + mask_background
  (a) composed   what was available before flat_data: F.interpolate, torch.round, F.pad, DepthTargetTransform.prepare, then
                 ops.flat_patch_rows / flat_labels / flat_depth_target
  (b) fused      FlatFrameTransform.frames / .masks / .depth with layout="rows": one hs_flat_resize launch per tensor
The two are timed alternately, `--repeats` times each; the spread is (max - min) / median over the repeats.  The bytes/s of (b)
are its minimal traffic (the raw input read once, the rows written once) over its time.
python tools/bench_flat_data.py [--batch 8] [--dtype bf16] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heal_swin_amd import depth_data as DD  # noqa: E402
from heal_swin_amd import flat_data as FD  # noqa: E402
from heal_swin_amd import ops  # noqa: E402

P, T = 2, 64


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def resize_pad(x, t, mode):
    x = F.interpolate(x, size=list(t.resized), mode=mode, **(dict(align_corners=False) if mode == "bilinear" else {}))
    left, top, right, bottom = t.padding
    x = x[..., max(-top, 0):x.shape[-2] - max(-bottom, 0), max(-left, 0):x.shape[-1] - max(-right, 0)]
    return F.pad(x, [max(left, 0), max(right, 0), max(top, 0), max(bottom, 0)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="bf16")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (a.batch, 3, 966, 1280), dtype=np.uint8)).cuda()
    masks = torch.from_numpy(rng.integers(0, 12, (a.batch, 966, 1280), dtype=np.uint8)).cuda()
    depth_np = rng.uniform(0.2, 400, (a.batch, 966, 1280)).astype(np.float32)
    depth_np[rng.random(depth_np.shape) < 0.05] = 1000.0
    depth = torch.from_numpy(depth_np).cuda()
    target = DD.DepthTargetTransform("log", "standardize", mask_background=True, zero_is_background=False)
    seg = FD.FlatFrameTransform((966, 1280), size=(640, 768), device="cuda", patch_size=P, tile=T)
    dep = FD.FlatFrameTransform((966, 1280), size=512, padding=(-19, 0, -19, 0), device="cuda", patch_size=P, tile=T)

    def composed_frames(t):
        return ops.flat_patch_rows(torch.round(resize_pad(frames.float(), t, "bilinear")).to(torch.uint8), P, T, dtype)

    def composed_seg():
        m = resize_pad(masks[:, None].float(), seg, "nearest")[:, 0].to(torch.uint8)
        return composed_frames(seg), ops.flat_labels(m, P, T)

    def composed_depth():
        d = resize_pad(depth[:, None], dep, "bilinear")[:, 0]
        return composed_frames(dep), ops.flat_depth_target(target.prepare(d.flatten(1)).view_as(d), P, T)

    def fused_seg():
        return seg.frames(frames, dtype=dtype, layout="rows"), seg.masks(masks, layout="rows")

    def fused_depth():
        return dep.frames(frames, dtype=dtype, layout="rows"), dep.depth(depth, "bilinear", target, layout="rows")

    # (the same values both ways: rows bit-equal for masks; frames and depth differ only as the bilinear rules allow)
    assert torch.equal(composed_seg()[1], fused_seg()[1].rows)
    esz = 2 if a.dtype == "bf16" else 4
    work = {"seg": (composed_seg, fused_seg, seg, frames.numel() + masks.numel(), 1),
            "depth": (composed_depth, fused_depth, dep, frames.numel() + depth.numel() * 4, 4)}
    res = dict(batch=a.batch, frame="3x966x1280 uint8", rows_dtype=a.dtype, patch=P, tile=T, iters=a.iters, repeats=a.repeats)
    for name, (composed, fused, t, in_bytes, pix_bytes) in work.items():
        h, w = t.out_size
        out_bytes = a.batch * ((h // P) * (w // P) * 16 * esz + h * w * pix_bytes)  # K = 3 p^2 = 12 padded to 16 columns
        ca, fb = [], []
        for _ in range(a.repeats):
            ca.append(timed(composed, a.iters))
            fb.append(timed(fused, a.iters))
        mc, mf = statistics.median(ca), statistics.median(fb)
        res[name] = dict(out_size=[h, w], composed_ms=mc, composed_spread=(max(ca) - min(ca)) / mc, fused_ms=mf,
                         fused_spread=(max(fb) - min(fb)) / mf, speedup=mc / mf, fused_min_bytes=in_bytes + out_bytes,
                         fused_GBps=(in_bytes + out_bytes) / mf / 1e6, composed_ms_all=ca, fused_ms_all=fb)
    print(json.dumps(res, indent=1))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
