#!/usr/bin/env python3
"""The depth data kernels at WoodScape size (16 frames of 966 x 1280, nside 256, 8 base pixels): time per launch and the
algorithmic bandwidth of
  projection  hs_sample_bilinear_u8_f32 + hs_sample_nearest_f32 (per output pixel: 16 B of coordinates once per launch; per
              image plane 4 neighbour bytes in, 4 out; per depth map 4 B in, 4 out)
  prepare     hs_depth_target on [8, 524288] float32 (log + standardize + mask_background: 4 B in, 4 B out per element)
  stats       hs_depth_stats_update over the 16 raw 966 x 1280 maps in one call (4 B in per element)
python tools/bench_depth_data.py [--batch 16] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heal_swin_amd import depth_data as DD  # noqa: E402

CAL = dict(name="FV", intrinsic=dict(aspect_ratio=1.0, cx_offset=3.942, cy_offset=-0.472, width=1280.0, height=966.0, poly_order=4,
                                     k1=339.749, k2=-31.988, k3=48.275, k4=-7.201),
           extrinsic=dict(quaternion=[0.5946970238045494, -0.5837953694518585, 0.39063952590941586, -0.39195666481783994]))


def timed(fn, iters=50, warmup=5):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--nside", type=int, default=256)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.integers(0, 256, (a.batch, 3, 966, 1280), dtype=np.uint8)).cuda()
    depth_np = rng.uniform(0.2, 999, (a.batch, 966, 1280)).astype(np.float32)
    depth_np[rng.random(depth_np.shape) < 0.05] = 1000.0
    depths = torch.from_numpy(depth_np).cuda()
    proj = DD.HPDepthProjector(CAL, a.nside, 8, rotate_pole=True)
    n = proj.npix
    ms_img = timed(lambda: DD.sample_bilinear_f32(imgs, proj.v, proj.u))
    ms_dep = timed(lambda: DD.sample_depth(depths, proj.v, proj.u))
    img_bytes = 16 * n + a.batch * n * 3 * (4 + 4)
    dep_bytes = 16 * n + a.batch * n * (4 + 4)
    tr = DD.DepthTargetTransform("log", "standardize", mask_background=True)
    x = torch.from_numpy(rng.uniform(0.2, 1000, (8, 524288)).astype(np.float32)).cuda()
    y = torch.empty_like(x)
    ms_prep = timed(lambda: tr.prepare(x, out=y), iters=200)
    acc = DD.DepthStatsAccumulator("log")
    ms_stats = timed(lambda: acc.update(depths), iters=50)
    res = dict(nside=a.nside, base_pix=8, npix=n, batch=a.batch, frame="3x966x1280 uint8 + 966x1280 float32",
               projection_image_ms=ms_img, projection_image_GBps=img_bytes / ms_img / 1e6,
               projection_depth_ms=ms_dep, projection_depth_GBps=dep_bytes / ms_dep / 1e6,
               projection_frames_per_s=a.batch / (ms_img + ms_dep) * 1e3,
               prepare_shape=[8, 524288], prepare_ms=ms_prep, prepare_GBps=x.numel() * 8 / ms_prep / 1e6,
               stats_elements=depths.numel(), stats_update_ms=ms_stats, stats_GBps=depths.numel() * 4 / ms_stats / 1e6)
    print(json.dumps(res, indent=1))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
