#!/usr/bin/env python3
"""What the gradient guard costs: one optimizer step over flat buffers of HEAL-SWIN-B's parameter tensors (the shapes of
bench.py's B256 model; random values, no model is run), four ways:

  plain     FlatAdam.step()                                             -- the yardstick
  guarded   FlatAdam(max_grad_norm=...).step()                          -- hs_grad_stats + finalize + hs_adam_step_guarded
  eager     torch.nn.utils.clip_grad_norm_(views) + FlatAdam.step()     -- what a caller could do before, outside a graph
  drop-in   parallel.clip_grad_norm_(sink) + torch.optim.Adam(fused=True).step()

max_norm is half the measured norm, so every variant really scales the gradients.  Prints one line per variant and the guard's own
kernels (hs_grad_stats over all buckets + finalize) with the rate at which they read the gradient bytes.

    python tools/bench_grad_guard.py [--workload B256] [--iters 20]
"""
import argparse
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def t_of(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="B256")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_guard.py measures on an MI355X; no GPU found")
    import bench
    from heal_swin_amd.optim import FlatAdam, GradGuard
    from heal_swin_amd.parallel import GradBucketAllReduce, clip_grad_norm_

    model, _, _ = bench.build_model(bench.WORKLOADS[args.workload])
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model

    def setup(flat_adam, **kw):
        torch.manual_seed(0)
        params = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.02) for s in shapes]
        dp = GradBucketAllReduce(params, direct_wgrad=False)
        gen = torch.Generator(device="cuda").manual_seed(1)
        for f in dp.buckets:  # (the alignment gaps get values too: harmless here, nothing below depends on them)
            f.copy_(torch.randn(f.shape, generator=gen, device="cuda") * 1e-3)
        # (FlatAdam writes the bf16 copies only for a model: the headline step has them)
        opt = FlatAdam(params, dp, lr=1e-4, model=types.SimpleNamespace(), **kw) if flat_adam else torch.optim.Adam(params, lr=1e-4, fused=True)
        return params, dp, opt

    params, dp, opt = setup(True)
    n = sum(p.numel() for p in params)
    grad_bytes = 4 * sum(f.numel() for f in dp.buckets)
    guard = GradGuard(dp)
    norm = float(guard.measure())
    max_norm = 0.5 * norm
    print(f"{args.workload}: {len(params)} tensors, {n / 1e6:.1f} M parameters, {len(dp.buckets)} buckets, {grad_bytes / 1e6:.0f} MB of gradients, "
          f"{guard.n_items} items; norm {norm:.4f}, max_norm {max_norm:.4f}")
    res = {}
    res["plain"] = t_of(opt.step, args.iters)
    t_guard = t_of(lambda: guard.measure(max_norm), args.iters)

    def eager():
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
    keep = [f.clone() for f in dp.buckets]

    def restore():  # the in-place variants shrink the gradients at every call: put them back (timed with the variant, and alone)
        for f, k in zip(dp.buckets, keep):
            f.copy_(k)
    t_restore = t_of(restore, args.iters)
    res["eager clip_grad_norm_ + FlatAdam"] = t_of(lambda: (restore(), eager()), args.iters) - t_restore
    dp.remove()
    del params, dp, opt, guard, keep

    params, dp, opt = setup(True, max_grad_norm=max_norm)
    res["guarded"] = t_of(opt.step, args.iters)
    dp.remove()
    del params, dp, opt

    params, dp, opt = setup(False)
    keep = [f.clone() for f in dp.buckets]

    def restore2():
        for f, k in zip(dp.buckets, keep):
            f.copy_(k)

    def drop_in():
        clip_grad_norm_(dp, max_norm)
        opt.step()
    t_restore = t_of(restore2, args.iters)
    res["sink clip_grad_norm_ + torch Adam(fused)"] = t_of(lambda: (restore2(), drop_in()), args.iters) - t_restore
    dp.remove()

    print(f"guard kernels alone (stats over every bucket + finalize): {t_guard:.3f} ms = {grad_bytes / t_guard / 1e9:.2f} TB/s of gradient bytes read")
    for k in ("plain", "guarded", "eager clip_grad_norm_ + FlatAdam", "sink clip_grad_norm_ + torch Adam(fused)"):
        print(f"{k:42s} {res[k]:8.3f} ms   ({res[k] / res['plain']:.2f} x plain)")


if __name__ == "__main__":
    main()
