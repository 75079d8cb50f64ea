"""Weight averaging over FlatAdam's buffers (csrc/weight_avg.hip, optim.FlatWeightAverage) against a float64 recomputation of the same
recurrence and against torch.optim.swa_utils.AveragedModel.

Lengths.  parallel.GradBucketAllReduce gives every parameter a slot of a multiple of 8 elements on a GPU, so a bucket of FlatAdam is
always a multiple of 8 long: the lengths that leave an element tail (1, 2, 3, 1027, 2 x 1024 + 5) are run through the C ABI on plain
tensors, the others (24, 1024 = one workgroup, 1032, 2 x 1024 + 8, and ~3e5 elements in three buckets) through the class on stacks of
nn.Linear layers.

Tolerance.  K = 6 updates; an update is at most three fp32 roundings (the difference, the product, the sum; w and 1 - w are exact
inputs of the recurrence), each at most half an ulp of a quantity <= 2 M, i.e. <= 2^-23 M with M the largest |value| among the inputs,
and 1 - w <= 1 never amplifies what is already there: |error| <= 3 K 2^-23 M against float64.  AveragedModel rounds as often and forms
its EMA weight as float(1 - decay) instead of 1.f - (float)decay (2e-8 apart): twice that bound."""
import copy
import ctypes
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 6
KINDS = [("swa", 0.0), ("ema", 0.9), ("ema", 0.999)]
KIND_IDS = ["swa", "ema0.9", "ema0.999"]
SMALL = 24  # elements of the two slots of nn.Linear(5, 3): 15 + 1 gap, 3 + 5 gap


def _layers(length=None, big=()):
    """nn.Linear(5, 3) -- two slots with alignment gaps -- and bias-free single-row layers that fill the bucket up to `length`"""
    layers = [torch.nn.Linear(5, 3)]
    if length is not None and length > SMALL:
        layers.append(torch.nn.Linear(length - SMALL, 1, bias=False))
    layers += [torch.nn.Linear(n, 1, bias=False) for n in big]
    return torch.nn.Sequential(*layers).to(DEV)


STACKS = {"24": dict(length=24), "1024": dict(length=1024), "1032": dict(length=1032), "2056": dict(length=2 * 1024 + 8),
          "buckets": dict(big=(100_003, 100_003, 100_003))}


class _Run:
    """A stack, its sink, its FlatAdam (bf16 copies as for a model) -- and, built before the sink re-homes anything, a plain twin module"""

    def __init__(self, name, seed=0, **adam):
        from heal_swin_amd.optim import FlatAdam
        from heal_swin_amd.parallel import GradBucketAllReduce
        torch.manual_seed(seed)
        self.model = _layers(**STACKS[name])
        self.twin = copy.deepcopy(self.model)
        self.params = list(self.model.parameters())
        self.dp = GradBucketAllReduce(self.params, bucket_bytes=(450_000 if name == "buckets" else 64 << 20), direct_wgrad=False)
        try:
            lengths = [f.numel() for f in self.dp.buckets]
            if name == "buckets":
                assert len(lengths) >= 3 and sum(lengths) > 300_000, lengths
            else:
                assert lengths == [int(name)], lengths
            self.opt = FlatAdam(self.params, self.dp, lr=1e-2, model=types.SimpleNamespace(), **adam)
        except BaseException:
            self.dp.remove()
            raise

    def close(self):
        self.dp.remove()

    def randomise(self, gen, scale=1.0):
        """fresh values into every parameter (through the views: the gaps keep their zeros) and the same into the twin's"""
        with torch.no_grad():
            for p, q in zip(self.params, self.twin.parameters()):
                v = torch.randn(p.shape, generator=gen, device=DEV) * scale
                p.copy_(v)
                q.copy_(v)
        return [p.detach().clone() for p in self.params]

    def fill_grads(self, gen):
        for p in self.params:
            p.grad.copy_(torch.randn(p.shape, generator=gen, device=DEV))

    def gap_masks(self):
        masks = []
        for b, f in enumerate(self.dp.buckets):
            owned = torch.zeros(f.numel(), dtype=torch.bool, device=DEV)
            for p in self.dp.params:
                if self.dp._where[p] == b:
                    off = self.dp._views[p].storage_offset() - f.storage_offset()
                    owned[off:off + p.numel()] = True
            masks.append(~owned)
        assert sum(int(m.sum()) for m in masks) >= 6  # (nn.Linear(5, 3) alone leaves 1 + 5)
        return masks


def _weight(kind, decay, n_averaged):
    """w of the update that finds `n_averaged` updates behind it, formed in fp32 as the kernel forms it"""
    one = torch.tensor(1.0, dtype=torch.float32)
    w = one / torch.tensor(float(n_averaged + 1), dtype=torch.float32) if kind == "swa" else one - torch.tensor(decay, dtype=torch.float32)
    return float(w)


def _recurrence(kind, decay, seq):
    """float64: avg = seq[0]; avg += w (p - avg) for every later p"""
    avg = seq[0].double()
    for n, p in enumerate(seq[1:], start=1):
        avg = avg + _weight(kind, decay, n) * (p.double() - avg)
    return avg


def _bound(seq):
    return 3 * K * 2.0 ** -23 * max(float(p.abs().max()) for p in seq)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("kind,decay", KINDS, ids=KIND_IDS)
def test_c_abi_at_lengths_with_an_element_tail(kind, decay):
    """hs_weight_avg_update / _advance / _swap on plain tensors: what lies behind element n - 1 is never written."""
    from heal_swin_amd import _lib as L
    gen = torch.Generator(device=DEV).manual_seed(7)
    for n in (1, 2, 3, 1024, 1027, 2 * 1024 + 5):
        room = n + 64
        avg = torch.full((room,), 123.0, device=DEV)
        count = torch.zeros((), dtype=torch.int64, device=DEV)
        seq = []
        for k in range(K):
            p = torch.full((room,), -77.0, device=DEV)
            p[:n] = torch.randn(n, generator=gen, device=DEV)
            seq.append(p[:n].clone())
            L.check(L.lib.hs_weight_avg_update(L.ptr(avg), L.ptr(p), n, int(kind == "ema"), decay, L.ptr(count), None, 0, _stream()),
                    "hs_weight_avg_update")
            L.check(L.lib.hs_weight_avg_advance(L.ptr(count), None, 0, _stream()), "hs_weight_avg_advance")
            if k == 0:
                assert torch.equal(avg[:n], p[:n]), (n, "the first update is a copy")
        assert int(count) == K
        assert bool((avg[n:] == 123.0).all()), (n, "written behind the end")
        err = float((avg[:n].double() - _recurrence(kind, decay, seq)).abs().max())
        print(f"{kind} {decay} n {n}: |error| {err:.3g}, bound {_bound(seq):.3g}")
        assert err <= _bound(seq), (n, err, _bound(seq))
        # the swap at the same length, with and without the bf16 copy
        p = torch.full((room,), -77.0, device=DEV)
        p[:n] = torch.randn(n, generator=gen, device=DEV)
        low = torch.full((room,), 5.0, dtype=torch.bfloat16, device=DEV)
        p0, avg0 = p.clone(), avg.clone()
        L.check(L.lib.hs_weight_avg_swap(L.ptr(p), L.ptr(avg), L.ptr(low), n, _stream()), "hs_weight_avg_swap")
        assert torch.equal(p[:n], avg0[:n]) and torch.equal(avg[:n], p0[:n]) and torch.equal(low[:n], avg0[:n].bfloat16()), n
        assert bool((p[n:] == -77.0).all()) and bool((avg[n:] == 123.0).all()) and bool((low[n:] == 5.0).all()), n
        L.check(L.lib.hs_weight_avg_swap(L.ptr(p), L.ptr(avg), None, n, _stream()), "hs_weight_avg_swap")
        assert torch.equal(p, p0) and torch.equal(avg, avg0) and torch.equal(low[:n], avg0[:n].bfloat16()), n


@pytest.mark.parametrize("name", list(STACKS))
@pytest.mark.parametrize("kind,decay", KINDS, ids=KIND_IDS)
def test_updates_follow_the_recurrence_and_averaged_model(kind, decay, name):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from heal_swin_amd.optim import FlatWeightAverage
    run = _Run(name)
    try:
        avg = FlatWeightAverage(run.opt, kind, decay=decay, every_step=False)
        assert avg.n_averaged.dim() == 0 and avg.n_averaged.dtype == torch.int64 and avg.n_averaged.is_cuda and int(avg.n_averaged) == 0
        assert [a.shape for a in avg._flat_avg] == [f.shape for f in run.dp.buckets]
        ref_model = AveragedModel(run.twin, multi_avg_fn=get_ema_multi_avg_fn(decay)) if kind == "ema" else AveragedModel(run.twin)
        gen = torch.Generator(device=DEV).manual_seed(11)
        seq = []
        for k in range(K):
            seq.append(run.randomise(gen, scale=1.0 + k))
            avg.update()
            ref_model.update_parameters(run.twin)
            if k == 0:
                assert all(torch.equal(avg.of(p), p) for p in run.params), "the first update is a copy"
        assert int(avg.n_averaged) == K == int(ref_model.n_averaged)
        worst = worst_torch = bound = 0.0
        for i, (p, q) in enumerate(zip(run.params, ref_model.module.parameters())):
            mine, steps = avg.of(p), [s[i] for s in seq]
            assert mine.shape == p.shape and mine.dtype == torch.float32
            err = float((mine.double() - _recurrence(kind, decay, steps)).abs().max())
            err_torch = float((mine.double() - q.detach().double()).abs().max())
            assert err <= _bound(steps), (i, err, _bound(steps))
            assert err_torch <= 2 * _bound(steps), (i, err_torch, 2 * _bound(steps))
            worst, worst_torch, bound = max(worst, err), max(worst_torch, err_torch), max(bound, _bound(steps))
        print(f"{kind} {decay} {name}: |error| {worst:.3g} against float64, {worst_torch:.3g} against AveragedModel; largest bound {bound:.3g}")
        for A, m in zip(avg._flat_avg, run.gap_masks()):
            assert bool((A[m] == 0).all()), "the alignment gaps of the average stay zero"
    finally:
        run.close()


def _guarded_step(run, gen, plant_inf=False):
    run.dp.zero_grad()
    run.fill_grads(gen)
    if plant_inf:
        run.params[0].grad.view(-1)[3] = float("inf")
    run.opt.step()


@pytest.mark.parametrize("kind,decay", [("swa", 0.0), ("ema", 0.9)], ids=["swa", "ema0.9"])
def test_a_skipped_step_is_not_averaged(kind, decay):
    from heal_swin_amd.optim import FlatWeightAverage
    run = _Run("1032", skip_nonfinite=True)
    try:
        avg = FlatWeightAverage(run.opt, kind, decay=decay, every_step=True)
        gen = torch.Generator(device=DEV).manual_seed(3)
        for _ in range(2):  # (two, so that the average has left the parameters behind: an update would now move it)
            _guarded_step(run, gen)
        assert int(avg.n_averaged) == 2 and not torch.equal(avg._flat_avg[0], run.opt._flat_p[0])
        before, p_before = avg._flat_avg[0].clone(), run.opt._flat_p[0].clone()
        _guarded_step(run, gen, plant_inf=True)
        assert int(run.opt.skipped_steps) == 1 and torch.equal(run.opt._flat_p[0], p_before)
        assert torch.equal(avg._flat_avg[0], before) and int(avg.n_averaged) == 2, "a skipped step was averaged"
        _guarded_step(run, gen)
        assert int(avg.n_averaged) == 3 and int(run.opt.skipped_steps) == 1
        want = before.double() + _weight(kind, decay, 2) * (run.opt._flat_p[0].double() - before.double())
        scale = max(float(run.opt._flat_p[0].abs().max()), float(before.abs().max()))
        assert float((avg._flat_avg[0].double() - want).abs().max()) <= 3 * 2.0 ** -23 * scale  # (one update: three roundings)
    finally:
        run.close()
    # without skip_nonfinite (a guard that only measures): the same sequence is averaged every time
    run = _Run("1032", track_grad_norm=True)
    try:
        avg = FlatWeightAverage(run.opt, kind, decay=decay, every_step=True)
        gen = torch.Generator(device=DEV).manual_seed(3)
        for _ in range(2):
            _guarded_step(run, gen)
        before = avg._flat_avg[0].clone()
        _guarded_step(run, gen, plant_inf=True)
        assert int(avg.n_averaged) == 3 and not torch.equal(avg._flat_avg[0], before)
        _guarded_step(run, gen)
        assert int(avg.n_averaged) == 4
    finally:
        run.close()


@pytest.mark.parametrize("name", ["1032", "buckets"])
def test_applied_swaps_and_restores_every_bit(name):
    from heal_swin_amd import ops
    from heal_swin_amd.optim import FlatWeightAverage
    run = _Run(name)
    try:
        avg = FlatWeightAverage(run.opt, "ema", decay=0.9, every_step=False)
        gen = torch.Generator(device=DEV).manual_seed(5)
        for _ in range(3):
            run.randomise(gen)
            avg.update()
        run.randomise(gen)
        opt = run.opt
        for S, P in zip(opt._flat_lowp, opt._flat_p):
            S.copy_(P)  # (the copies a step would have left)
        was_p, was_avg = [P.clone() for P in opt._flat_p], [A.clone() for A in avg._flat_avg]
        was_low = [S.clone() for S in opt._flat_lowp]

        def restored():
            return (all(torch.equal(a, b) for a, b in zip(opt._flat_p, was_p)) and all(torch.equal(a, b) for a, b in zip(avg._flat_avg, was_avg))
                    and all(torch.equal(a, b) for a, b in zip(opt._flat_lowp, was_low)))
        epoch = ops.RT.weight_epoch
        with avg.applied() as inside:
            assert inside is avg and ops.RT.weight_epoch > epoch
            for P, A, S, p0, a0 in zip(opt._flat_p, avg._flat_avg, opt._flat_lowp, was_p, was_avg):
                assert torch.equal(P, a0) and torch.equal(A, p0) and torch.equal(S, a0.bfloat16())
            for p in run.params:
                assert torch.equal(opt.lowp_copy(p, torch.bfloat16), p.detach().bfloat16())
            with pytest.raises(RuntimeError, match="applied"):
                opt.step()
            with pytest.raises(RuntimeError, match="applied"):
                avg.update()
            with pytest.raises(RuntimeError, match="applied"):
                with avg.applied():
                    pass
            assert torch.equal(opt._flat_p[0], was_avg[0]), "a refused call changed the parameters"
        assert restored() and ops.RT.weight_epoch > epoch + 1
        with pytest.raises(KeyError, match="validation"):
            with avg.applied():
                raise KeyError("validation failed")
        assert restored(), "an exception inside applied() left the averaged weights in the model"
        run.dp.zero_grad()
        opt.step()  # and the optimizer steps again
        # copy_to_model: parameters and copies become the average, which is kept
        avg.copy_to_model()
        for P, A, S, a0 in zip(opt._flat_p, avg._flat_avg, opt._flat_lowp, was_avg):
            assert torch.equal(P, a0) and torch.equal(A, a0) and torch.equal(S, a0.bfloat16())
    finally:
        run.close()


def _plain_twin(model):
    """a deep copy of the module alone: not of the optimizer behind its bf16 copies, nor of its cast cache"""
    held = {k: model.__dict__.pop(k) for k in ("_shadow_provider", "_cast_cache") if k in model.__dict__}
    try:
        return copy.deepcopy(model)
    finally:
        model.__dict__.update(held)


def test_a_model_forward_inside_applied_is_the_averaged_models():
    """The tiny SwinHPTransformerSys of test_gpu_optim_groups, bf16, FlatAdam(model=) and EMA: the no-grad forward inside applied() is the
    forward of a deep copy that holds avg.of(p) in every parameter, and the forward after it the forward before it -- bit for bit.  A
    cast cache that missed the swap would answer with the other set of weights."""
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys
    from heal_swin_amd.optim import FlatAdam, FlatWeightAverage
    from heal_swin_amd.parallel import GradBucketAllReduce
    spec = DataSpec(dim_in=12 * 32 * 32, f_in=3, f_out=12, base_pix=12, class_names=[])
    cfg = SwinHPTransformerConfig(patch_size=4, window_size=64, shift_size=32, rel_pos_bias="flat", embed_dim=64, depths=[2, 2],
                                  num_heads=[2, 4], drop_path_rate=0.0, use_cos_attn=True)
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randint(0, 256, (2, 3, spec.dim_in), generator=g, device=DEV).float()
    y = torch.randint(0, 12, (2, spec.dim_in), generator=g, device=DEV, dtype=torch.uint8)
    torch.manual_seed(0)
    model = SwinHPTransformerSys(cfg, spec).to(DEV).train()
    model.compute_dtype = torch.bfloat16
    dp = GradBucketAllReduce(model.parameters())
    try:
        opt = FlatAdam(model.parameters(), dp, lr=1e-2, model=model)
        avg = FlatWeightAverage(opt, "ema", decay=0.9)
        assert avg._hook is not None, "EMA follows every step by default"
        for _ in range(3):
            dp.zero_grad()
            model.forward_seg_loss(x, y).backward()
            dp.finish()
            opt.step()
        assert int(avg.n_averaged) == 3
        model.eval()
        twin = _plain_twin(model)
        with torch.no_grad():
            for p, q in zip(model.parameters(), twin.parameters()):
                assert q.data_ptr() != p.data_ptr()
                q.copy_(avg.of(p))
            before = model(x).clone()
            want = twin(x).clone()
            with avg.applied():
                inside = model(x).clone()
            after = model(x).clone()
        assert model.__dict__["_cast_cache"].all_external
        assert not torch.equal(want, before), "three steps at lr 1e-2 did not separate the average from the parameters"
        assert torch.equal(inside, want), "the forward inside applied() did not run on the averaged weights"
        assert torch.equal(after, before), "the forward after applied() did not run on the trained weights"
    finally:
        dp.remove()


def test_ema_in_a_captured_training_step():
    """GraphedTrainStep captures the step post-hook with the step: warm-up, capture, 3 replays against an eager twin."""
    from heal_swin_amd.graphs import GraphedTrainStep
    from heal_swin_amd.optim import FlatAdam, FlatWeightAverage
    from heal_swin_amd.parallel import GradBucketAllReduce
    torch.manual_seed(0)
    net_a = torch.nn.Sequential(torch.nn.Linear(32, 16), torch.nn.Linear(16, 5)).to(DEV)
    net_b = copy.deepcopy(net_a)
    xs = torch.randn(4, 64, 32, device=DEV)
    dummy = torch.zeros(1, device=DEV)
    dpa, dpb = GradBucketAllReduce(net_a.parameters(), direct_wgrad=False), GradBucketAllReduce(net_b.parameters(), direct_wgrad=False)
    step = None
    try:
        oa, ob = FlatAdam(net_a.parameters(), dpa, lr=1e-2), FlatAdam(net_b.parameters(), dpb, lr=1e-2)
        ea, eb = FlatWeightAverage(oa, "ema", decay=0.9), FlatWeightAverage(ob, "ema", decay=0.9)

        def eager(x):
            dpa.zero_grad()
            net_a(x).square().mean().backward()
            dpa.finish()
            oa.step()
        step = GraphedTrainStep(net_b, lambda out, t: out.square().mean(), ob, xs[0], dummy, warmup=2, grad_sink=dpb)
        for _ in range(2):
            eager(xs[0])
        for i in (1, 2, 3):
            eager(xs[i])
            step(xs[i], dummy)
            for p, q in zip(net_a.parameters(), net_b.parameters()):
                assert torch.equal(p, q) and torch.equal(ea.of(p), eb.of(q)), i
            assert int(ea.n_averaged) == int(eb.n_averaged) == 2 + i
        for A, B in zip(ea._flat_avg, eb._flat_avg):
            assert torch.equal(A, B)
        assert not torch.equal(ea._flat_avg[0], oa._flat_p[0])
    finally:
        if step is not None:
            torch.cuda.synchronize()
            step.close()
        dpa.remove()
        dpb.remove()


@pytest.mark.parametrize("kind,decay", [("swa", 0.0), ("ema", 0.999)], ids=["swa", "ema0.999"])
def test_state_dict_round_trip(kind, decay):
    from heal_swin_amd.optim import FlatWeightAverage
    a, b = _Run("buckets", seed=0), None
    try:
        b = _Run("buckets", seed=1)
        avg_a = FlatWeightAverage(a.opt, kind, decay=decay, every_step=False)
        gen = torch.Generator(device=DEV).manual_seed(9)
        for _ in range(3):
            a.randomise(gen)
            avg_a.update()
        sd = avg_a.state_dict()
        assert sd["kind"] == kind and sd["decay"] == decay and sd["n_averaged"] == 3 and type(sd["n_averaged"]) is int
        assert len(sd["averages"]) == len(a.dp.params)
        for t, p in zip(sd["averages"], a.dp.params):
            assert torch.equal(t, avg_a.of(p)) and t.data_ptr() != avg_a.of(p).data_ptr()
        avg_b = FlatWeightAverage(b.opt, kind, decay=0.5, every_step=False)
        flat_before = [A.data_ptr() for A in avg_b._flat_avg]
        avg_b.load_state_dict(copy.deepcopy(sd))
        assert avg_b.decay == decay and int(avg_b.n_averaged) == 3
        assert [A.data_ptr() for A in avg_b._flat_avg] == flat_before
        for A, B in zip(avg_a._flat_avg, avg_b._flat_avg):
            assert torch.equal(A, B)
        new = a.randomise(gen)
        with torch.no_grad():
            for q, v in zip(b.params, new):
                q.copy_(v)
        avg_a.update()
        avg_b.update()
        assert int(avg_a.n_averaged) == int(avg_b.n_averaged) == 4
        for A, B in zip(avg_a._flat_avg, avg_b._flat_avg):
            assert torch.equal(A, B)
        for p in b.dp.params:  # the views still alias the flat buffers
            bkt = avg_b._flat_avg[b.dp._where[p]]
            off = b.dp._views[p].storage_offset() - b.dp.buckets[b.dp._where[p]].storage_offset()
            assert avg_b.of(p).data_ptr() == bkt.data_ptr() + 4 * off
            assert torch.equal(avg_b.of(p).reshape(-1), bkt[off:off + p.numel()])
        with pytest.raises(ValueError, match="average"):
            avg_b.load_state_dict(dict(sd, kind="ema" if kind == "swa" else "swa"))
    finally:
        a.close()
        if b is not None:
            b.close()
