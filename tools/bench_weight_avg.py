#!/usr/bin/env python3
"""What weight averaging costs next to the optimizer step: flat buffers of HEAL-SWIN-B's parameter tensors (the shapes of bench.py's
B256 model; random values, no model is run), three things timed alternately in one process:

  step     FlatAdam.step()                               -- hs_adam_step, 30 B per bucket element (16 read, 14 written): the yardstick
  update   FlatWeightAverage.update()                    -- hs_weight_avg_update + advance, 12 B per element (8 read, 4 written)
  swaps    one pass into FlatWeightAverage.applied() and out again -- 2 x hs_weight_avg_swap, 2 x 18 B per element (8 read, 10 written)

`--rounds` windows each, every window at least `--window` seconds of device time between two events after a warm-up; the spread of a
variant over its windows is the margin its median is read with.  The average is an EMA that has already taken updates, so `update`
runs the lerp, not the first update's copy.  Prints one line per variant (microseconds: median, min, max; achieved bytes per second;
the share of `step`) and one JSON line.

    python tools/bench_weight_avg.py [--workload B256] [--kind ema] [--rounds 5] [--window 1.0]
"""
import argparse
import json
import math
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES = {"step": 30, "update": 12, "swaps": 36}  # per bucket element and call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="B256")
    ap.add_argument("--kind", default="ema", choices=["swa", "ema"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="least seconds of device time per timed window")
    args = ap.parse_args()
    import bench
    from heal_swin_amd.optim import FlatAdam, FlatWeightAverage

    model, _, _ = bench.build_model(bench.WORKLOADS[args.workload])
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    print(f"{args.workload}: {len(shapes)} tensors, {sum(math.prod(s) for s in shapes) / 1e6:.1f} M parameters")
    if not torch.cuda.is_available():
        raise SystemExit("bench_weight_avg.py measures on an MI355X; no GPU found")
    from heal_swin_amd.parallel import GradBucketAllReduce

    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.02) for s in shapes]
    dp = GradBucketAllReduce(params, direct_wgrad=False)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for p in params:  # (the views only: the alignment gaps keep their zeros, as in a training step)
        p.grad.copy_(torch.randn(p.shape, generator=gen, device="cuda") * 1e-3)
    # (FlatAdam writes the bf16 copies only for a model: the headline step has them, and so has the swap)
    opt = FlatAdam(params, dp, lr=1e-4, model=types.SimpleNamespace())
    avg = FlatWeightAverage(opt, args.kind, decay=0.999, every_step=False)
    elements = sum(f.numel() for f in dp.buckets)

    def swaps():
        with avg.applied():
            pass
    calls = {"step": opt.step, "update": avg.update, "swaps": swaps}

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n  # us per call
    count = {}
    for k, fn in calls.items():  # warm-up (the first update is the copy), and how many calls make a window
        window(fn, 20)
        count[k] = max(100, math.ceil(1.1 * args.window * 1e6 / window(fn, 100)))
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():
            times[k].append(window(fn, count[k]))
    n_averaged = int(avg.n_averaged)
    dp.remove()
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"{len(dp.buckets)} buckets, {elements / 1e6:.1f} M bucket elements ({4 * elements / 1e6:.0f} MB per fp32 buffer); {args.kind}, "
          f"{n_averaged} updates taken; {args.rounds} windows of >= {args.window} s each, alternating")
    for k, v in times.items():
        print(f"{k:7s} {med[k]:8.1f} us (min {min(v):.1f}, max {max(v):.1f}; {count[k]} calls per window)  {BYTES[k] * elements / 1e6:7.0f} MB moved  "
              f"{BYTES[k] * elements / med[k] / 1e6:.2f} TB/s  {med[k] / med['step']:.3f} x step")
    print(json.dumps(dict(tool="bench_weight_avg", workload=args.workload, kind=args.kind, tensors=len(shapes), bucket_elements=elements,
                          buckets=len(dp.buckets), rounds=args.rounds, calls_per_window=count, bytes_per_element=BYTES,
                          us={k: [round(t, 2) for t in v] for k, v in times.items()}, median_us={k: round(v, 2) for k, v in med.items()},
                          tb_per_s={k: round(BYTES[k] * elements / med[k] / 1e6, 3) for k in med},
                          share_of_step={k: round(med[k] / med["step"], 4) for k in med})))


if __name__ == "__main__":
    main()
