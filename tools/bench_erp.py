#!/usr/bin/env python3
"""Equirectangular panoramas onto the sphere at the flagship size (nside 256, 12 base pixels, batch 8, from 1024 x 2048 uint8
panoramas with three channels): `hs_erp_to_hp` for frame + labels at supersample 0 / 1 / 2, the frame alone, and, in the same
process, `hs_hp_rotate` for frame + labels at the same pixel count -- the kernel of the same shape (one thread per sample and
pixel, float64 transcendentals) whose time on the same machine in the same run is the yardstick.  Every figure is the median of
--repeats windows of --iters launches between device events; the routes alternate inside each repeat.  A record, not an
acceptance threshold.
python tools/bench_erp.py [--batch 8] [--nside 256] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heal_swin_amd import erp as E  # noqa: E402
from heal_swin_amd import hp_rotate as R  # noqa: E402
from heal_swin_amd import projection as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nside", type=int, default=256)
    ap.add_argument("--base-pix", type=int, default=12)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_erp needs a GPU: there is no CPU path to time")
    npix = a.base_pix * a.nside * a.nside
    rng = np.random.default_rng(0)
    pano = torch.from_numpy(rng.integers(0, 256, (a.batch, 3, a.height, a.width), dtype=np.uint8)).cuda()
    pano_lab = torch.from_numpy(rng.integers(0, 10, (a.batch, a.height, a.width), dtype=np.uint8)).cuda()
    hp_img = torch.from_numpy(rng.integers(0, 256, (a.batch, 3, npix), dtype=np.uint8)).cuda()
    hp_lab = torch.from_numpy(rng.integers(0, 10, (a.batch, npix), dtype=np.uint8)).cuda()
    rot = P.random_rotations(a.batch, 7.0, flip=0.5, generator=torch.Generator().manual_seed(0), device="cuda")
    proj = {s: E.ERPProjector(a.nside, a.base_pix, supersample=s) for s in (0, 1, 2)}
    rotator = R.HPRotator(a.nside, a.base_pix)

    routes = {f"erp_to_hp_frame_labels_s{s}_ms": (lambda s=s: proj[s](pano, pano_lab, rotations=rot)) for s in (0, 1, 2)}
    routes["erp_to_hp_frame_s0_ms"] = lambda: proj[0](pano, rotations=rot)
    routes["hp_rotate_frame_labels_ms"] = lambda: rotator(hp_img, hp_lab, rotations=rot)
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, fn in routes.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(a.iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]) / a.iters)
    res = dict(nside=a.nside, base_pix=a.base_pix, npix=npix, batch=a.batch, height=a.height, width=a.width, iters=a.iters, repeats=a.repeats)
    for k, t in times.items():
        res[k] = statistics.median(t)
        res[k.replace("_ms", "_min_max_ms")] = [min(t), max(t)]
    rotate = res["hp_rotate_frame_labels_ms"]
    for s in (0, 1, 2):
        res[f"s{s}_over_hp_rotate"] = res[f"erp_to_hp_frame_labels_s{s}_ms"] / rotate
    res["Gpix_per_s_frame_labels_s0"] = a.batch * npix / res["erp_to_hp_frame_labels_s0_ms"] / 1e6
    print(json.dumps(res, indent=1))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
