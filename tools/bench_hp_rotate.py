#!/usr/bin/env python3
"""Rotation of HEALPix-resident maps at the size a training run uses (nside 256, 8 base pixels, batch 8): the fused launch
`hs_hp_rotate` for frame + labels and for frame + depth, the unfused route (`hs_hp_rotated_interp` writing its tables, then torch
gathers for the same three planes), and `hs_hp_rotated_coords` alone -- the kernel of the same shape (one thread per sample and
pixel, float64 transcendentals) whose time on the same machine in the same run is the yardstick.  Every figure is the median of
--repeats windows of --iters launches between device events; the four routes alternate inside each repeat.
python tools/bench_hp_rotate.py [--batch 8] [--nside 256] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heal_swin_amd import hp_rotate as R  # noqa: E402
from heal_swin_amd import projection as P  # noqa: E402
from tools.bench_projection import CAL  # noqa: E402


def gather_planes(pix, wgt, nearest, img, lab, background=0):
    """frame and labels of hs_hp_rotate from the tables of hs_hp_rotated_interp, in torch operators: what a user without the fused
    kernel would write (the tables are 52 B per sample and pixel, written and read back)"""
    npix = img.shape[-1]
    ok = (pix >= 0) & (pix < npix)
    v = torch.take_along_dim(img[:, :, None, :], pix.clamp(0, npix - 1).long()[:, None], 3).double()  # [B, C, 4, npix]
    frame = (v * (wgt * ok)[:, None]).sum(2).round_().clamp_(0, 255).to(torch.uint8)
    okn = (nearest >= 0) & (nearest < npix)
    labels = torch.take_along_dim(lab, nearest.clamp(0, npix - 1).long(), 1)
    return frame, torch.where(okn, labels, torch.full_like(labels, background))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nside", type=int, default=256)
    ap.add_argument("--base-pix", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_hp_rotate needs a GPU: there is no CPU path to time")
    npix = a.base_pix * a.nside * a.nside
    rng = np.random.default_rng(0)
    img = torch.from_numpy(rng.integers(0, 256, (a.batch, 3, npix), dtype=np.uint8)).cuda()
    lab = torch.from_numpy(rng.integers(0, 10, (a.batch, npix), dtype=np.uint8)).cuda()
    dep = torch.from_numpy(rng.uniform(0.2, 400, (a.batch, npix)).astype(np.float32)).cuda()
    rot = P.random_rotations(a.batch, 7.0, flip=0.5, generator=torch.Generator().manual_seed(0), device="cuda")
    rotator = R.HPRotator(a.nside, a.base_pix, cal_info=CAL, rotate_pole=True)
    mats = rotator.matrices(rot)
    plain = R.HPRotator(a.nside, a.base_pix)  # the matrices as they are: the launch alone, as for the coordinate kernel below
    cam = P.camera_record(CAL)

    def unfused():
        return gather_planes(*R.rotated_interp(a.nside, mats, count=npix), img, lab)

    routes = {
        "hp_rotate_frame_labels_ms": lambda: plain(img, lab, rotations=mats),
        "hp_rotate_frame_depth_ms": lambda: plain(img, hp_depth=dep, rotations=mats),
        "rotated_interp_plus_torch_gathers_ms": unfused,
        "rotated_interp_alone_ms": lambda: R.rotated_interp(a.nside, mats, count=npix),
        "hp_rotated_coords_ms": lambda: P._rotated_coords(a.nside, a.base_pix, cam, mats, None, "cuda"),
    }
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
    res = dict(nside=a.nside, base_pix=a.base_pix, npix=npix, batch=a.batch, iters=a.iters, repeats=a.repeats)
    for k, t in times.items():
        res[k] = statistics.median(t)
        res[k.replace("_ms", "_min_max_ms")] = [min(t), max(t)]
    coords = res["hp_rotated_coords_ms"]
    res["frame_labels_over_coords"] = res["hp_rotate_frame_labels_ms"] / coords
    res["frame_depth_over_coords"] = res["hp_rotate_frame_depth_ms"] / coords
    res["unfused_over_fused"] = res["rotated_interp_plus_torch_gathers_ms"] / res["hp_rotate_frame_labels_ms"]
    res["Gpix_per_s_frame_labels"] = a.batch * npix / res["hp_rotate_frame_labels_ms"] / 1e6
    print(json.dumps(res, indent=1))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
