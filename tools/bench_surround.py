#!/usr/bin/env python3
"""A rig of fisheye cameras onto the sphere at the flagship size (nside 256, 12 base pixels, batch 8, four cameras of
three-channel uint8 966 x 1280 frames plus labels): `hs_surround_to_hp` under both blends, and, in the same process as
yardsticks, `hs_erp_to_hp` (frame + labels, supersample 0, from 1024 x 2048 panoramas) at the same pixel count, and the
composition the existing entry points offer for a winner rule: per camera one `hs_hp_rotated_coords` launch (a 16 B / pixel table
per sample) and the two `_per_sample` samplers, then the choice in torch.  The table carries no angle from the optical axis, so
the composition's rule is the distance to the nearest image border alone; it is timed for its cost, not for its output.  Every
figure is the median of --repeats windows of --iters calls between device events after warm-up; the routes alternate inside each
repeat.  A record, not an acceptance threshold.
python tools/bench_surround.py [--batch 8] [--nside 256] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heal_swin_amd import erp as E  # noqa: E402
from heal_swin_amd import projection as P  # noqa: E402
from heal_swin_amd import surround as S  # noqa: E402

# WoodScape-like optics (the polynomial of a 190-degree lens at 966 x 1280), one camera per side of the vehicle
INTRINSIC = dict(aspect_ratio=1.0, cx_offset=3.942, cy_offset=-0.472, width=1280.0, height=966.0, poly_order=4, k1=339.749, k2=-31.988,
                 k3=48.275, k4=-7.201)
QUATERNIONS = {"FV": (0.5946970238045494, -0.5837953694518585, 0.39063952590941586, -0.39195666481783994), "RV": (-0.4057, -0.4038, 0.5817, 0.5789),
               "MVL": (0.1215, -0.8817, 0.4417, 0.1153), "MVR": (0.8817, 0.1215, -0.1153, 0.4417)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nside", type=int, default=256)
    ap.add_argument("--base-pix", type=int, default=12)
    ap.add_argument("--height", type=int, default=966)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_surround needs a GPU: there is no CPU path to time")
    npix = a.base_pix * a.nside * a.nside
    cals = [dict(name=n, intrinsic=dict(INTRINSIC, height=float(a.height), width=float(a.width)), extrinsic=dict(quaternion=list(q)))
            for n, q in QUATERNIONS.items()]
    n_cam = len(cals)
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.integers(0, 256, (a.batch, n_cam, 3, a.height, a.width), dtype=np.uint8)).cuda()
    labs = torch.from_numpy(rng.integers(0, 10, (a.batch, n_cam, a.height, a.width), dtype=np.uint8)).cuda()
    per_cam = [(imgs[:, c].contiguous(), labs[:, c].contiguous()) for c in range(n_cam)]  # the composition's layout, made outside the clock
    pano = torch.from_numpy(rng.integers(0, 256, (a.batch, 3, 1024, 2048), dtype=np.uint8)).cuda()
    pano_lab = torch.from_numpy(rng.integers(0, 10, (a.batch, 1024, 2048), dtype=np.uint8)).cuda()
    rot = P.random_rotations(a.batch, 7.0, generator=torch.Generator().manual_seed(0), device="cuda")
    proj = {b: S.SurroundProjector(cals, a.nside, a.base_pix, blend=b) for b in ("winner", "feather")}
    erp = E.ERPProjector(a.nside, a.base_pix)
    cams = [P.camera_record(c) for c in cals]

    def composition():
        m = proj["winner"].matrices(rot)
        weight, frame, label = [], [], []
        for c in range(n_cam):
            u, v = P._rotated_coords(a.nside, a.base_pix, cams[c], m[:, c], None, "cuda")
            weight.append(torch.minimum(torch.minimum(u + 0.5, a.width - 0.5 - u), torch.minimum(v + 0.5, a.height - 0.5 - v)))
            frame.append(P.sample_bilinear_u8(per_cam[c][0], v, u, per_sample=True))
            label.append(P.sample_mask(per_cam[c][1], v, u, 0, per_sample=True))
        best = torch.stack(weight).argmax(0)  # [B, Npix]
        hp_img = torch.stack(frame).gather(0, best[None, :, None].expand(1, a.batch, 3, npix))[0]
        return hp_img, torch.stack(label).gather(0, best[None])[0]

    routes = {f"surround_{b}_frame_labels_ms": (lambda b=b: proj[b](imgs, labs, rotations=rot)) for b in proj}
    routes["erp_to_hp_frame_labels_s0_ms"] = lambda: erp(pano, pano_lab, rotations=rot)
    routes["composition_winner_ms"] = composition
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
    res = dict(nside=a.nside, base_pix=a.base_pix, npix=npix, batch=a.batch, cameras=n_cam, height=a.height, width=a.width, iters=a.iters,
               repeats=a.repeats, table_MB_composition=a.batch * n_cam * npix * 16 / 1e6)
    for k, t in times.items():
        res[k] = statistics.median(t)
        res[k.replace("_ms", "_min_max_ms")] = [min(t), max(t)]
    for b in proj:
        res[f"{b}_over_erp"] = res[f"surround_{b}_frame_labels_ms"] / res["erp_to_hp_frame_labels_s0_ms"]
        res[f"composition_over_{b}"] = res["composition_winner_ms"] / res[f"surround_{b}_frame_labels_ms"]
        res[f"Gpix_per_s_{b}"] = a.batch * npix / res[f"surround_{b}_frame_labels_ms"] / 1e6
    covered = (proj["winner"](masks=labs, rotations=rot, return_camera=True)[1] != 255).float().mean()
    res["covered_share"] = float(covered)
    print(json.dumps(res, indent=1))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
