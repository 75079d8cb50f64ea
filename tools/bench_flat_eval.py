#!/usr/bin/env python3
"""Scoring the flat Swin-UNet baseline on the sphere (heal_swin_amd/flat_evaluation.py) at the paper's size against the torch
composition a user would write otherwise: batch 8, 640 x 768 predictions, WoodScape 966 x 1280 frames, nside 256, 8 base pixels,
12 classes in the model's padded fp32 head rows (16 floats).  Segmentation, from the head rows to the confusion matrix:
  torch      rows -> NCHW (ops.flat_pixel_image, what forward() ends in) + argmax + interpolate(nearest) + index + bincount
  nchw       rows -> NCHW + SegConfusion through FlatToHPProjector(layout="image")
  rows       SegConfusion through FlatToHPProjector(layout="rows") on the head rows themselves
Depth (one channel), nearest and bilinear, from an NCHW prediction to the metric sums:
  torch      interpolate + index + the five masked sums in torch
  two_pass   projector.depth() + DepthMetrics.update(map, target)
  gather     DepthMetrics.update(pred, target, projector)   (`hs_depth_metrics_gather`: the map is never written)
Every output is compared with the torch composition before timing.  Means of CUDA-event timings after warm-up.
python tools/bench_flat_eval.py [--batch 8] [--iters 20] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heal_swin_amd import flat_evaluation as FE  # noqa: E402
from heal_swin_amd import ops  # noqa: E402
from heal_swin_amd.depth_evaluation import DepthMetrics  # noqa: E402
from heal_swin_amd.evaluation import SegConfusion  # noqa: E402

CAL = dict(name="FV", intrinsic=dict(aspect_ratio=1.0, cx_offset=3.942, cy_offset=-0.472, width=1280.0, height=966.0, poly_order=4,
                                     k1=339.749, k2=-31.988, k3=48.275, k4=-7.201),
           extrinsic=dict(quaternion=[0.5946970238045494, -0.5837953694518585, 0.39063952590941586, -0.39195666481783994]))


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nside", type=int, default=256)
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flat_eval.py measures the HIP kernels: no GPU visible")
    dev = torch.device("cuda", 0)
    b, k, (h, w), orig, ps, tile = a.batch, a.classes, (640, 768), (966, 1280), 2, 64
    kpad = k + (-k) % 8

    t0 = time.perf_counter()
    kw = dict(model_size=(h, w), orig_size=orig, device=dev)
    p_img = FE.FlatToHPProjector(CAL, a.nside, **kw)
    torch.cuda.synchronize()
    table_s = time.perf_counter() - t0
    p_rows = FE.FlatToHPProjector(CAL, a.nside, layout="rows", patch_size=ps, tile=tile, **kw)
    p_bil = FE.FlatToHPProjector(CAL, a.nside, interpolation="bilinear", **kw)
    n = p_img.n_out
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.randn((b, h * w, kpad), generator=g, device=dev)[:, :, :k]
    target = torch.randint(0, k, (b, n), generator=g, device=dev).to(torch.uint8)
    r, c = torch.from_numpy(np.around(p_img.v)).to(dev), torch.from_numpy(np.around(p_img.u)).to(dev)
    ok = (r >= 0) & (r < orig[0]) & (c >= 0) & (c < orig[1])
    at = torch.where(ok, r * orig[1] + c, 0).long()

    def nchw():
        return ops.flat_pixel_image(rows, h, w, ps, tile)

    def sample(plane, mode, fill):
        x = F.interpolate(plane[:, None], size=list(orig), mode=mode, **({} if mode == "nearest" else {"align_corners": False}))
        flat = x.flatten(1)[:, at]
        return torch.where(ok, flat, torch.full_like(flat, fill))

    def seg_torch():
        labels = sample(nchw().argmax(1).float(), "nearest", float(p_img.s2_bkgd_class)).long()
        return torch.bincount(target.long().reshape(-1) * k + labels.reshape(-1), minlength=k * k).reshape(k, k)

    conf = SegConfusion(k, device=dev)

    def seg_nchw():
        conf.update(p_img.logits(nchw()), target, p_img, check=False)

    def seg_rows():
        conf.update(p_rows.logits(rows), target, p_rows, check=False)

    want = seg_torch()
    for fn in (seg_nchw, seg_rows):
        conf.reset()
        fn()
        assert torch.equal(conf.confmat, want), f"{fn.__name__}: the confusion matrix differs from the torch composition"
    res = dict(batch=b, nside=a.nside, base_pix=8, hp_pixels=n, covered=round(float(p_img.covered_host.mean()), 4), classes=k,
               row_floats=kpad, model_size=[h, w], orig_size=list(orig), host_table_build_s=round(table_s, 2))
    seg = {name: round(timed(fn, a.iters), 1) for name, fn in (("torch_us", seg_torch), ("nchw_us", seg_nchw), ("rows_us", seg_rows),
                                                               ("rows_to_nchw_alone_us", nchw))}
    res["segmentation"] = seg

    depth = nchw()[:, :1].contiguous()
    dtarget = torch.rand((b, n), generator=g, device=dev) * 50 + 0.5
    dtarget[:, ~p_img.covered] = float("inf")

    def depth_torch(mode):
        p = sample(depth[:, 0], mode, float("nan"))
        sel = torch.isfinite(p) & torch.isfinite(dtarget)
        d = (p - dtarget)[sel].double()
        pos = sel & (p > 0) & (dtarget > 0)
        dl = (torch.log(dtarget[pos]) - torch.log(p[pos])).double()
        ip, it = 1 / (0.001 * p), 1 / (0.001 * dtarget)
        si = torch.isfinite(ip) & torch.isfinite(it)
        return torch.stack([sel.sum().double(), (d * d).sum(), d.abs().sum(), (dl * dl).sum(),
                            ((ip - it)[si].double() ** 2).sum()])

    res["depth"] = {}
    for mode, proj in (("nearest", p_img), ("bilinear", p_bil)):
        ms = [DepthMetrics(total_mean=20.0, device=dev) for _ in range(2)]

        def two_pass():
            ms[0].update(proj.depth(depth), dtarget)

        def gather():
            ms[1].update(depth, dtarget, proj)

        two_pass()
        gather()
        assert torch.equal(ms[0].state, ms[1].state), f"{mode}: the gather kernel's sums differ from the two-pass sums"
        ref = depth_torch(mode)
        got = ms[1].state[[0, 1, 2, 8, 10]]  # N, SE, AE, SILog d^2, iRMSE SE
        if mode == "bilinear":  # torch's GPU bilinear forms its own weights: 1 / p near p = 0 magnifies that without bound
            got, ref = got[:3], ref[:3]
        rel = ((got - ref).abs() / ref.abs().clamp_min(1e-30)).max().item()
        assert got[0] == ref[0] and rel <= (1e-6 if mode == "nearest" else 1e-4), (mode, rel)
        res["depth"][mode] = dict(torch_us=round(timed(lambda: depth_torch(mode), a.iters), 1), two_pass_us=round(timed(two_pass, a.iters), 1),
                                  gather_us=round(timed(gather, a.iters), 1),
                                  map_alone_us=round(timed(lambda: proj.depth(depth), a.iters), 1), sums_rel_err_vs_torch=rel)
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
