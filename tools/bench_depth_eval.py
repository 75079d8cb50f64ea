#!/usr/bin/env python3
"""Depth evaluation kernels (csrc/depth_eval.hip) at the sizes the reference's writers use, against the torch compositions a
user would write otherwise:
  * hs_chamfer_nn, HEALPix <-> HEALPix (nside 256, 8 base pixels: 524,288 points a side) and HEALPix <-> full-res image
    (966 x 1280), with and without indices, against a chunked direct-difference min in fp32 (the same distances) and
    torch.cdist (the expanded |a|^2 - 2 a.b + |b|^2 form: its distances DIFFER, timed for reference only).  Each is also given
    as a fraction of the fp32 vector roofline: 6.5 lane-ops per pair at 157.3 TFLOPS (7.9e13 lane-FMA/s) -> 1.2e13 pairs/s.
  * hs_depth_metrics (one update of DepthMetrics with logvar and 4 ranges), batch 8, nside 256, against the reference's update
    code composed in torch on the device (one composition per metric, as the reference's metric classes run them).
  * MeanSTDMedian by hs_select_rows against torch.median inside the same update, the two routes taking turns (min /
    median / max per route, a random and an all-equal log variance, the select's share of its four-pass floor): --select runs
    this part alone.
python tools/bench_depth_eval.py [--iters 5] [--select] [--reps 15] [--json out.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heal_swin_amd import depth_evaluation as DE  # noqa: E402

CAL = dict(name="FV", intrinsic=dict(aspect_ratio=1.0, cx_offset=3.942, cy_offset=-0.472, width=1280.0, height=966.0, poly_order=4,
                                     k1=339.749, k2=-31.988, k3=48.275, k4=-7.201),
           extrinsic=dict(quaternion=[0.5946970238045494, -0.5837953694518585, 0.39063952590941586, -0.39195666481783994]))
PAIRS_PER_S = 157.3e12 / 2 / 6.5  # lane-FMA/s over lane-ops per pair


def timed(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters  # ms


def torch_direct(a, b, chunk=256):
    """Chunked direct-difference nearest neighbours in fp32 (both directions)."""
    da = torch.empty(a.shape[0], device=a.device)
    db = torch.full((b.shape[0],), float("inf"), device=a.device)
    for i in range(0, a.shape[0], chunk):
        d = ((a[i:i + chunk, None, :] - b[None, :, :]) ** 2).sum(-1)
        da[i:i + chunk] = d.min(1).values
        db = torch.minimum(db, d.min(0).values)
    return da, db


def torch_cdist(a, b, chunk=1024):
    da = torch.empty(a.shape[0], device=a.device)
    db = torch.full((b.shape[0],), float("inf"), device=a.device)
    for i in range(0, a.shape[0], chunk):
        d = torch.cdist(a[i:i + chunk], b).square()
        da[i:i + chunk] = d.min(1).values
        db = torch.minimum(db, d.min(0).values)
    return da, db


def ref_metrics(pred, target, tm, ranges):
    """The reference's update() bodies (custom_metrics.py), composed on the device."""
    means, lv = pred[:, 0], pred[:, 1]
    ok = ~(means.isinf() | target.isinf()) & ~(means.isnan() | target.isnan())
    out = [torch.square(means[ok] - target[ok]).sum(), torch.count_nonzero(ok)]
    out += [torch.square(tm - target[ok]).sum(), torch.abs(means[ok] - target[ok]).sum(), torch.abs(tm - target[ok]).sum()]
    im, it = 1 / (0.001 * means.clone()), 1 / (0.001 * target.clone())
    ok2 = ~(im.isinf() | it.isinf()) & ~(im.isnan() | it.isnan())
    out += [torch.square(im[ok2] - it[ok2]).sum(), torch.count_nonzero(ok2)]
    s = ok & (means > 0) & (target > 0)
    dl = torch.log(target[s]) - torch.log(means[s])
    out += [torch.square(dl).sum(), dl.sum(), dl.numel()]
    for lo, hi in ranges:
        r = (lo <= target) & (target < hi) & ok
        out += [torch.square(means - target)[r].sum(), torch.count_nonzero(r)]
    t2 = target.clone()
    t2[t2 == float("inf")] = float("nan")
    keep = ~t2.isnan()
    out += [torch.sqrt(torch.exp(lv[keep])).sum(), torch.count_nonzero(keep)]
    out += [torch.sqrt(torch.exp(lv)).view(lv.shape[0], -1).median(1).values.sum(), means[ok].sum()]
    return out


class TorchMedianMetrics(DE.DepthMetrics):
    """DepthMetrics as it was before hs_select_rows: MeanSTDMedian through torch.median (the comparison composition)."""

    def _add_stds(self, stds):
        self.median[0] += stds.median(1).values.double().sum()
        self.median[1] += stds.shape[0]


def timed_alternately(fns, reps, inner=10, warmup=2):
    """One sample = `inner` calls of one function between two events; the functions take turns, `reps` samples each.
    -> per function {min, median, max} of a call in us."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    samples = [[] for _ in fns]
    for _ in range(reps):
        for fn, s in zip(fns, samples):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(inner):
                fn()
            ev[1].record()
            ev[1].synchronize()
            s.append(ev[0].elapsed_time(ev[1]) / inner * 1e3)
    return [{"min": min(s), "median": sorted(s)[len(s) // 2], "max": max(s)} for s in samples]


def faster(new, old):
    """new's median below old's minimum by more than the two spreads (max - min) added"""
    return new["median"] < old["min"] - ((new["max"] - new["min"]) + (old["max"] - old["min"]))


def bench_select(a, dev, npix):
    """DepthMetrics.update with the radix select (hs_select_rows) against the same update with torch.median, taking turns in
    one process, on a random and on an all-equal log variance (every key in one LDS counter), and the two medians alone.  The
    floor of the select is its four passes over the fp32 rows at a cached-read rate: the rows were just written by the sqrt and
    fit the Infinity Cache (8.6 TB/s random rows) and, an eighth per XCD, the L2s (34.5 TB/s)."""
    from heal_swin_amd.order_stats import row_median
    b = a.batch
    g = torch.Generator(device=dev).manual_seed(1)
    target = torch.rand(b, npix, generator=g, device=dev) * 80 + 0.5
    ranges = [(0, 10), (10, 20), (20, 40), (40, 80)]
    res = {"batch": b, "npix": npix, "reps": a.reps}
    floor_bytes = 4 * 4 * b * npix
    res["select_floor_us"] = {"infinity_cache_8.6TBps": floor_bytes / 8.6e12 * 1e6, "l2_34.5TBps": floor_bytes / 34.5e12 * 1e6}
    for name in ("random", "all_equal"):
        pred = torch.rand(b, 2, npix, generator=g, device=dev) * 80 + 0.5
        pred[:, 1] = torch.randn(b, npix, generator=g, device=dev) if name == "random" else -1.25
        new, old = (cls(total_mean=30.0, distance_ranges=ranges, use_logvar=True, device=dev) for cls in (DE.DepthMetrics, TorchMedianMetrics))
        new.update(pred, target)
        old.update(pred, target)
        assert torch.equal(new.median, old.median) and torch.equal(new.state, old.state)  # the same bits by either route
        t_new, t_old = timed_alternately([lambda: new.update(pred, target), lambda: old.update(pred, target)], a.reps)
        stds = torch.sqrt(torch.exp(pred[:, 1])).reshape(b, -1)
        s_new, s_old = timed_alternately([lambda: row_median(stds), lambda: stds.median(1)], a.reps)
        r = {"update_select_us": t_new, "update_torch_median_us": t_old, "update_select_is_faster": faster(t_new, t_old),
             "row_median_us": s_new, "torch_median_us": s_old, "row_median_is_faster": faster(s_new, s_old)}
        r["row_median_share_of_floor"] = {k: v / s_new["median"] for k, v in res["select_floor_us"].items()}
        res[name] = r
        print("select", name, json.dumps(r), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nside", type=int, default=256)
    ap.add_argument("--skip-torch", action="store_true", help="time only the kernels")
    ap.add_argument("--select", action="store_true", help="only the median comparison: hs_select_rows against torch.median")
    ap.add_argument("--reps", type=int, default=15, help="samples per route of the median comparison")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_eval.py measures the HIP kernels: no GPU visible")
    dev = torch.device("cuda", 0)
    res = {}
    if a.select:
        res["select"] = bench_select(a, dev, 8 * a.nside * a.nside)
        if a.json:
            with open(a.json, "w") as fh:
                json.dump(res, fh, indent=1)
        return
    hp = DE.HPDepthGeometry(CAL, a.nside, 8, device=dev)
    img = DE.ImageDepthGeometry(CAL, 966, 1280, False, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    pa, oa = hp.points(torch.rand(1, hp.n, generator=g, device=dev) * 80 + 1)
    pb, ob = hp.points(torch.rand(1, hp.n, generator=g, device=dev) * 80 + 1)
    pi, oi = img.points(torch.rand(1, 966, 1280, generator=g, device=dev) * 80 + 1)
    for name, (x, ox, y, oy) in (("hp_hp", (pa, oa, pb, ob)), ("hp_fullres", (pa, oa, pi, oi))):
        pairs = x.shape[0] * y.shape[0]
        r = {"points": [x.shape[0], y.shape[0]], "pairs_per_direction": pairs,
             "roofline_ms_per_direction": pairs / PAIRS_PER_S * 1e3}
        for idx in (False, True):
            ms = timed(lambda: DE.chamfer_nn(x, y, ox, oy, return_idx=idx), a.iters)
            key = "hs_chamfer_nn_idx_ms" if idx else "hs_chamfer_nn_ms"
            r[key] = ms
            r[key.replace("_ms", "_roofline_fraction")] = 2 * r["roofline_ms_per_direction"] / ms
        if not a.skip_torch:
            da, db = DE.chamfer_nn(x, y, ox, oy)
            ta, tb = torch_direct(x, y)
            r["torch_direct_max_rel_diff"] = max(((da - ta).abs() / ta.clamp_min(1e-30)).max().item(),
                                                 ((db - tb).abs() / tb.clamp_min(1e-30)).max().item())
            r["torch_direct_ms"] = timed(lambda: torch_direct(x, y), 1, warmup=0)
            ca, cb = torch_cdist(x, y)
            r["torch_cdist_max_abs_diff"] = max((da - ca).abs().max().item(), (db - cb).abs().max().item())
            r["torch_cdist_ms"] = timed(lambda: torch_cdist(x, y), 1, warmup=0)
        res[name] = r
        print(name, json.dumps(r), flush=True)

    b = a.batch
    pred = torch.rand(b, 2, hp.n, generator=g, device=dev) * 80 + 0.5
    target = torch.rand(b, hp.n, generator=g, device=dev) * 80 + 0.5
    target[:, ::97] = float("nan")
    target[:, ::89] = float("inf")
    ranges = [(0, 10), (10, 20), (20, 40), (40, 80)]
    m = DE.DepthMetrics(total_mean=30.0, distance_ranges=ranges, use_logvar=True, device=dev)
    r = {"batch": b, "npix": hp.n, "hs_depth_metrics_us": timed(lambda: m.update(pred, target), 20, warmup=3) * 1e3}
    r["hs_depth_metrics_no_median_us"] = timed(lambda: DE.DepthMetrics(30.0, ranges, False, device=dev).update(pred, target), 20,
                                               warmup=3) * 1e3
    r["torch_reference_update_us"] = timed(lambda: ref_metrics(pred, target, 30.0, ranges), 20, warmup=3) * 1e3
    res["depth_metrics"] = r
    print("depth_metrics", json.dumps(r), flush=True)
    res["select"] = bench_select(a, dev, hp.n)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
