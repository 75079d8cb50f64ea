#!/usr/bin/env python3
"""Rotation ensembles at the size an evaluation run uses (nside 256, 8 base pixels, batch 8, 12 classes, the model's padded bf16
head rows): one `HPRotationEnsemble.add` of a rotated member (`hs_hp_ensemble_add_seg`, with and without a valid plane), the
unrotated member, `finish`, a depth member; `hs_hp_rotate` for frame + labels at the same shape -- the kernel with the same float64
geometry per (sample, pixel), the yardstick -- and the route in torch operators that the fused kernel replaces: the tables of
`hs_hp_rotated_interp` written out (52 bytes per pixel and member), a softmax, four gathers of [B, K, Npix], a weighted sum and the
add into the accumulators.  Every figure is the median of --repeats windows of --iters launches between device events; the routes
alternate inside each repeat.
python tools/bench_hp_ensemble.py [--batch 8] [--nside 256] [--classes 12] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heal_swin_amd import hp_ensemble as E  # noqa: E402
from heal_swin_amd import hp_rotate as R  # noqa: E402
from heal_swin_amd import projection as P  # noqa: E402


def torch_add(nside, pred, mt, valid, acc, wsum):
    """one member added in torch operators: acc [B, K, Npix], wsum [B, Npix] fp32"""
    b, k, npix = pred.shape
    pix, wgt, _ = R.rotated_interp(nside, mt, count=npix)
    ok = (pix >= 0) & (pix < npix)
    safe = pix.clamp(0, npix - 1).long()
    ok &= torch.gather(valid, 1, safe.view(b, -1)).view(b, 4, npix) != 0
    w = (wgt * ok).float()
    prob = torch.softmax(pred.float(), 1)
    for j in range(4):
        acc += w[:, j, None, :] * torch.gather(prob, 2, safe[:, j, None, :].expand(-1, k, -1))
    wsum += w.sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nside", type=int, default=256)
    ap.add_argument("--base-pix", type=int, default=8)
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_hp_ensemble needs a GPU: there is no CPU path to time")
    npix, k = a.base_pix * a.nside * a.nside, a.classes
    rng = np.random.default_rng(0)
    rows = torch.randn((a.batch, npix, 16), device="cuda").mul_(2).bfloat16()
    pred = rows.transpose(1, 2)[:, :k]  # the head's padded rows, viewed as [B, K, Npix]: read by 16-byte loads
    dense = pred.float().contiguous()
    depth = torch.rand((a.batch, npix), device="cuda") * 100
    img = torch.from_numpy(rng.integers(0, 256, (a.batch, 3, npix), dtype=np.uint8)).cuda()
    lab = torch.from_numpy(rng.integers(0, 10, (a.batch, npix), dtype=np.uint8)).cuda()
    rot = P.random_rotations(a.batch, 7.0, flip=0.5, generator=torch.Generator().manual_seed(0), device="cuda")
    ens, dens, rotator = E.HPRotationEnsemble(a.nside, a.base_pix), E.HPRotationEnsemble(a.nside, a.base_pix), R.HPRotator(a.nside, a.base_pix)
    valid = ens.valid_plane(rot)
    mt = rotator.matrices(rot).transpose(1, 2).contiguous()
    t_acc = torch.zeros((a.batch, k, npix), device="cuda")
    t_wsum = torch.zeros((a.batch, npix), device="cuda")
    lens = E.HPRotationEnsemble(a.nside, a.base_pix, mode="logit")  # the same traffic and geometry without the softmax
    ens.add(pred)  # the accumulators exist and hold a first member: every timed add accumulates
    dens.add(depth)
    lens.add(pred)

    routes = {
        "ensemble_add_ms": lambda: ens.add(pred, rot, valid),
        "ensemble_add_no_valid_ms": lambda: ens.add(pred, rot),
        "ensemble_add_logit_mode_ms": lambda: lens.add(pred, rot, valid),
        "ensemble_add_dense_fp32_ms": lambda: ens.add(dense, rot, valid),
        "ensemble_add_identity_ms": lambda: ens.add(pred),
        "ensemble_finish_ms": lambda: ens.finish(),
        "ensemble_add_depth_ms": lambda: dens.add(depth, rot, valid),
        "valid_plane_ms": lambda: ens.valid_plane(rot),
        "hp_rotate_frame_labels_ms": lambda: rotator(img, lab, rotations=rot),
        "torch_operators_add_ms": lambda: torch_add(a.nside, pred, mt, valid, t_acc, t_wsum),
    }
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(a.repeats):
        for name, fn in routes.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(a.iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            times[name].append(ev[0].elapsed_time(ev[1]) / a.iters)
    res = dict(nside=a.nside, base_pix=a.base_pix, npix=npix, batch=a.batch, classes=k, iters=a.iters, repeats=a.repeats)
    for name, t in times.items():
        res[name] = statistics.median(t)
        res[name.replace("_ms", "_min_max_ms")] = [min(t), max(t)]
    res["add_over_hp_rotate"] = res["ensemble_add_ms"] / res["hp_rotate_frame_labels_ms"]
    res["torch_operators_over_add"] = res["torch_operators_add_ms"] / res["ensemble_add_ms"]
    res["Gpix_per_s_add"] = a.batch * npix / res["ensemble_add_ms"] / 1e6
    print(json.dumps(res, indent=1))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
