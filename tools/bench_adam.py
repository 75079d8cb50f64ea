#!/usr/bin/env python3
"""What parameter groups cost FlatAdam: one optimizer step over flat buffers of HEAL-SWIN-B's parameter tensors (the shapes and names of
bench.py's B256 model: nside 256, 12 base pixels; random values, no forward is run), three ways, in one process:

  one      FlatAdam(params)                                   -- hs_adam_step, the yardstick (what bench.py runs)
  decay    FlatAdam(weight_decay_groups(model, wd))           -- 2 groups, hs_adam_step_groups
  blocks   one group per transformer block x (decay | no decay), neighbouring blocks folded together until the count fits
           adam_max_groups(); each group with a learning rate of its own (layer-wise decay)

The three are timed alternately, `--rounds` windows each, every window at least `--window` seconds of device time between two events
after a warm-up; the spread of `one` over its windows is the margin the other two are read against.  As a control each grouped
variant's buffers are also stepped by the single-group kernel (its tables set aside), window by window.  Prints one line per variant
(microseconds per step: median, min, max; bytes per second from 30 B -- 16 read, 14 written -- per bucket element) and one JSON line.

    python tools/bench_adam.py [--workload B256] [--rounds 5] [--window 1.0]
"""
import argparse
import json
import math
import os
import re
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def block_of(name):
    """the transformer block a parameter belongs to ("layers.2.blocks.7"), or the stage / module around the blocks"""
    m = re.match(r"(.*\.blocks\.\d+)\.", name) or re.match(r"(.*?\.\d+)\.", name)
    return m.group(1) if m else name.split(".")[0]


def variants(model, weight_decay, max_groups):
    """{variant: [(parameter indices, options), ...]} over the model's trainable parameters in model.parameters() order"""
    from heal_swin_amd.optim import weight_decay_groups
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    index = {id(p): i for i, (_, p) in enumerate(named)}
    decay, no_decay = weight_decay_groups(model, weight_decay)
    in_decay = {index[id(p)] for p in decay["params"]}
    keys = []  # (block, decays) in order of first appearance
    for i, (n, _) in enumerate(named):
        key = (block_of(n), i in in_decay)
        if key not in keys:
            keys.append(key)
    blocks = list(dict.fromkeys(k[0] for k in keys))
    fold = 1
    while len({(blocks.index(b) // fold, d) for b, d in keys}) > max_groups:
        fold += 1
    members = {}
    for i, (n, _) in enumerate(named):
        members.setdefault((blocks.index(block_of(n)) // fold, i in in_decay), []).append(i)
    n_fold = -(-len(blocks) // fold)
    by_block = [(idx, dict(lr=1e-4 * 0.9 ** (n_fold - 1 - k), weight_decay=weight_decay if d else 0.0)) for (k, d), idx in sorted(members.items())]
    out = {"one": [(list(range(len(named))), {})],
           "decay": [(sorted(in_decay), dict(weight_decay=weight_decay)), (sorted(set(range(len(named))) - in_decay), dict(weight_decay=0.0))],
           "blocks": by_block}
    return named, out, dict(blocks=len(blocks), keys=len(keys), fold=fold)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="B256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="least seconds of device time per timed window")
    ap.add_argument("--weight-decay", type=float, default=0.05)
    ap.add_argument("--layout-only", action="store_true", help="print the groups of every variant and stop (needs no GPU)")
    args = ap.parse_args()
    import bench
    from heal_swin_amd.optim import FlatAdam, adam_max_groups

    model, _, _ = bench.build_model(bench.WORKLOADS[args.workload])
    named, groups_of, census = variants(model, args.weight_decay, adam_max_groups())
    shapes = [tuple(p.shape) for _, p in named]
    del model
    print(f"{args.workload}: {len(shapes)} tensors, {sum(math.prod(s) for s in shapes) / 1e6:.1f} M parameters; {census['blocks']} blocks and "
          f"modules around them, {census['keys']} (block, decay) classes, folded by {census['fold']}: "
          + ", ".join(f"{k} = {len(v)} group{'s' * (len(v) > 1)}" for k, v in groups_of.items()))
    if args.layout_only:
        for k, v in groups_of.items():
            print(k, [(len(idx), opts) for idx, opts in v])
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam.py measures on an MI355X; no GPU found")
    from heal_swin_amd.parallel import GradBucketAllReduce

    def setup(groups):
        torch.manual_seed(0)
        params = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.02) for s in shapes]
        dp = GradBucketAllReduce(params, direct_wgrad=False)
        gen = torch.Generator(device="cuda").manual_seed(1)
        for p in params:  # (the views only: the alignment gaps keep their zeros, as in a training step)
            p.grad.copy_(torch.randn(p.shape, generator=gen, device="cuda") * 1e-3)
        given = params if len(groups) == 1 else [dict(opts, params=[params[i] for i in idx]) for idx, opts in groups]
        # (FlatAdam writes the bf16 copies only for a model: the headline step has them)
        return params, dp, FlatAdam(given, dp, lr=1e-4, weight_decay=args.weight_decay, decoupled_weight_decay=True, model=types.SimpleNamespace())
    built = {k: setup(v) for k, v in groups_of.items()}
    elements = sum(f.numel() for f in built["one"][1].buckets)
    runs = {k: (sum(t[0].shape[0] for t in opt._group_tables) if opt._group_tables else 0) for k, (_, _, opt) in built.items()}

    def window(opt, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            opt.step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps  # us per step
    steps = {}
    for k, (_, _, opt) in built.items():  # warm-up, and how many steps make a window
        window(opt, 20)
        steps[k] = max(100, math.ceil(1.1 * args.window * 1e6 / window(opt, 100)))
    def single_on(opt, n):
        """the single-group kernel over a grouped optimizer's own buffers (group 0's options for every element): separates what the
        grouped kernel costs from where the allocator happened to put this variant's 2.7 GB"""
        tables, opt._group_tables = opt._group_tables, None
        try:
            return window(opt, n)
        finally:
            opt._group_tables = tables
    times = {k: [] for k in built}
    control = {k: [] for k in built if k != "one"}
    for _ in range(args.rounds):
        for k, (_, _, opt) in built.items():
            times[k].append(window(opt, steps[k]))
            if k in control:
                control[k].append(single_on(opt, steps[k]))
    for _, dp, _ in built.values():
        dp.remove()
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(times["one"]) - min(times["one"])
    print(f"{len(built['one'][1].buckets)} buckets, {elements / 1e6:.1f} M bucket elements, {30 * elements / 1e6:.0f} MB moved per step; "
          f"{args.rounds} windows of >= {args.window} s each, alternating")
    for k, v in times.items():
        print(f"{k:7s} {len(groups_of[k]):2d} groups {runs[k]:4d} runs  {med[k]:8.1f} us/step (min {min(v):.1f}, max {max(v):.1f}; {steps[k]} steps per window)  "
              f"{30 * elements / med[k] / 1e6:.2f} TB/s  {med[k] / med['one']:.4f} x one")
    for k, v in control.items():
        c = statistics.median(v)
        print(f"  hs_adam_step over the buffers of `{k}`: {c:8.1f} us/step (min {min(v):.1f}, max {max(v):.1f}); the grouped kernel there: {med[k] / c:.4f} x")
    print(f"spread of `one` over its windows: {spread:.1f} us ({100 * spread / med['one']:.2f} %)")
    print(json.dumps(dict(tool="bench_adam", workload=args.workload, tensors=len(shapes), bucket_elements=elements, rounds=args.rounds,
                          groups={k: len(v) for k, v in groups_of.items()}, runs=runs, steps_per_window=steps,
                          us_per_step={k: [round(t, 2) for t in v] for k, v in times.items()}, median_us=med, spread_one_us=round(spread, 2),
                          single_kernel_on_same_buffers_us={k: [round(t, 2) for t in v] for k, v in control.items()},
                          tb_per_s={k: round(30 * elements / med[k] / 1e6, 3) for k in med})))


if __name__ == "__main__":
    main()
