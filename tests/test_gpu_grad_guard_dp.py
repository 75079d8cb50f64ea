"""The gradient guard under data parallelism: two processes share cuda:0 and exchange gradients over gloo, as in
tests/test_gpu_parallel.py::test_two_rank_dp_equals_single_process (same model, same data).  The guard reads the already averaged
buckets, so both ranks measure the same bits and take the same clipped step without a collective of their own."""
import os
import sys

import pytest
import torch

from test_gpu_parallel import ROOT, _build, _data, _free_port

pytestmark = pytest.mark.gpu
# Adam moves every element by about lr whatever its gradient's size: small enough that elements whose gradient is rounding noise
# (half-batch against full-batch sums) stay inside that test's 2e-2 tolerance, which is relative to max(1e-3, largest element)
LR = 1e-6


def _train(model, dp, xs, ys, max_norm, steps=2):
    from heal_swin_amd.losses import seg_loss
    from heal_swin_amd.optim import FlatAdam
    opt = FlatAdam(model.parameters(), dp, lr=LR, model=model, max_grad_norm=max_norm)
    norms = []
    for _ in range(steps):
        dp.zero_grad()
        seg_loss(model(xs), ys).backward()
        dp.finish()
        opt.step()
        norms.append(opt.grad_norm.clone())
    torch.cuda.synchronize()
    return [float(n) for n in norms], [p.detach().float().cpu().numpy().copy() for p in model.parameters()]


def _worker(rank, world, port, max_norm, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from heal_swin_amd.parallel import GradBucketAllReduce
    model = _build()
    x, y = _data()
    dp = GradBucketAllReduce(model.parameters(), bucket_bytes=256 << 10)  # several buckets
    assert dp.world == 2 and len(dp.buckets) > 1
    q.put((rank,) + _train(model, dp, x.chunk(world)[rank], y.chunk(world)[rank], max_norm))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_alike_and_as_a_single_process():
    import numpy as np
    import torch.multiprocessing as mp
    sys.path.insert(0, ROOT)
    from heal_swin_amd.losses import seg_loss
    from heal_swin_amd.optim import GradGuard
    from heal_swin_amd.parallel import GradBucketAllReduce
    # the gradient norm of this model on the whole batch; half of it as the threshold makes both steps clip
    model = _build()
    x, y = _data()
    dp = GradBucketAllReduce(model.parameters(), direct_wgrad=False)
    dp.zero_grad()
    seg_loss(model(x), y).backward()
    dp.finish()
    max_norm = 0.5 * float(GradGuard(dp).measure())
    dp.remove()
    assert max_norm > 0 and np.isfinite(max_norm)

    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, max_norm, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: (norms, params) for r, norms, params in (q.get(timeout=300) for _ in range(world))}
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    model = _build()
    dp = GradBucketAllReduce(model.parameters(), direct_wgrad=False)
    ref_norms, ref = _train(model, dp, x, y, max_norm)
    dp.remove()
    assert res[0][0] == res[1][0], "both ranks measure the same bits"
    assert all(n > max_norm for n in res[0][0] + ref_norms), "every step clips"
    for a, b in zip(res[0][1], res[1][1]):
        assert np.array_equal(a, b)  # replicas identical
    for a, b in zip(res[0][0], ref_norms):
        assert abs(a - b) <= 2e-2 * b, (res[0][0], ref_norms)
    worst = 0.0
    for a, b in zip(res[0][1], ref):
        worst = max(worst, float(np.abs(a - b).max()) / max(1e-3, float(np.abs(b).max())))
    assert worst < 2e-2, worst  # bf16 activations: half-batch vs full-batch reduction order differs
