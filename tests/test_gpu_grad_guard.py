"""The gradient guard of the flat optimizer step (csrc/grad_guard.hip, hs_adam_step_guarded in csrc/adam.hip, optim.GradGuard,
FlatAdam's max_grad_norm / clip_value / skip_nonfinite / track_grad_norm, parallel.clip_grad_norm_) against torch's
clip_grad_norm_ / clip_grad_value_ followed by torch.optim.Adam on the same parameters and gradients.

Tolerances.  Norms: every element is squared and summed in fp64, so only the final rounding to fp32 is left: 2 fp32 ulps = 2.4e-7
relative.  Clipped steps: the bounds of test_gpu_optim.test_flat_adam_follows_torch_adam (parameters 2e-6 of scale, moments 5e-6);
clipping adds one fp32 multiply per gradient element."""
import ctypes
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NORM_TOL = 2.4e-7


def _piece():
    from heal_swin_amd.optim import grad_piece
    return grad_piece()


def _toy(seed=0):
    """a parameter shorter than a slot, a scalar, odd tails, an exact-plus-one and an off-by-8 multiple of the piece"""
    P = _piece()
    torch.manual_seed(seed)
    shapes = [(64, 32), (64,), (7, 5, 3), (1,), (129, 33), (1000,), (3, 1, 1), (P + 1,), (2 * P + 8,)]
    return [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]


def _sink(params):
    from heal_swin_amd.parallel import GradBucketAllReduce
    dp = GradBucketAllReduce(params, bucket_bytes=16 << 10, direct_wgrad=False)
    assert len(dp.buckets) >= 4
    return dp


def _fill(gen, it, *param_lists):
    """the same randn * (0.1 + it) gradient into every list: `.grad` of plain parameters is replaced, a sink's view is written"""
    for group in zip(*param_lists):
        grad = torch.randn(group[0].shape, generator=gen, device=DEV) * (0.1 + it)
        for p in group:
            if getattr(p, "_in_sink", False):
                p.grad.copy_(grad)
            else:
                p.grad = grad.clone()


def _in_sink(params):
    for p in params:
        p._in_sink = True
    return params


def _gap_masks(dp):
    masks = []
    for i, f in enumerate(dp.buckets):
        owned = torch.zeros(f.numel(), dtype=torch.bool, device=DEV)
        for p in dp.params:
            if dp._where[p] == i:
                off = dp._views[p].storage_offset() - f.storage_offset()
                owned[off:off + p.numel()] = True
        masks.append(~owned)
    assert sum(int(m.sum()) for m in masks) > 0
    return masks


def _rel(a, ref):
    return abs(float(a) - float(ref)) / float(ref)


def _ulps(a, b):
    """largest distance of two fp32 tensors in units in the last place (same-signed finite values)"""
    return int((a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max())


@pytest.mark.parametrize("norm_type", [2.0, math.inf])
def test_norms_match_float64_vector_norm(norm_type):
    from heal_swin_amd.optim import GradGuard
    b = _in_sink(_toy())
    dp = _sink(b)
    try:
        guard = GradGuard(dp, norm_type)
        gen = torch.Generator(device=DEV).manual_seed(1)
        for it in (0, 3):
            _fill(gen, it, b)
            total = guard.measure()
            assert total.dim() == 0 and total.dtype == torch.float32 and total.is_cuda
            assert guard.param_norms.shape == (len(b),) and guard.param_norms.dtype == torch.float32
            refs = [torch.linalg.vector_norm(p.grad.double().flatten(), norm_type) for p in dp.params]
            ref_total = torch.linalg.vector_norm(torch.cat([p.grad.double().flatten() for p in dp.params]), norm_type)
            got = guard.param_norms.tolist()
            worst = max(_rel(g, r) for g, r in zip(got, refs))
            print(f"norm {norm_type} it {it}: worst parameter error {worst:.3g}, total error {_rel(total, ref_total):.3g}")
            if norm_type == math.inf:
                assert all(g == float(r) for g, r in zip(got, refs)) and float(total) == float(ref_total)
            else:
                assert worst <= NORM_TOL and _rel(total, ref_total) <= NORM_TOL
            assert float(guard.clip_coef) == 1.0 and int(guard.finite) == 1
        # the gaps between the slots belong to no item: whatever they hold, the norms are the same bits
        before = (guard.param_norms.clone(), guard.record.clone())
        masks = _gap_masks(dp)
        for f, m in zip(dp.buckets, masks):
            f[m] = 1e3
        guard.measure()
        for f, m in zip(dp.buckets, masks):
            f[m] = 0.0
        assert torch.equal(guard.param_norms, before[0]) and torch.equal(guard.record, before[1])
        # clip coefficient: torch's formula in fp32
        guard.measure(max_norm=1.5)
        t = guard.total_norm.clone()
        assert _rel(guard.clip_coef, torch.clamp(1.5 / (t + 1e-6), max=1.0)) <= NORM_TOL and float(guard.clip_coef) < 1.0
    finally:
        dp.remove()


def test_measuring_twice_gives_the_same_bits():
    from heal_swin_amd import _lib
    from heal_swin_amd.optim import GradGuard
    b = _in_sink(_toy())
    dp = _sink(b)
    try:
        guard = GradGuard(dp)
        _fill(torch.Generator(device=DEV).manual_seed(1), 2, b)
        guard.measure(3.0)
        first = (guard.partials.clone(), guard.param_norms.clone(), guard.record.clone())
        guard.partials.fill_(-1.0)
        guard.measure(3.0)
        assert all(torch.equal(x, y) for x, y in zip(first, (guard.partials, guard.param_norms, guard.record)))
        # no grid of the guard follows the reserved-CU policy; the result must not either
        prev = int(_lib.lib.hs_get_reserved_cus())
        try:
            _lib.check(_lib.lib.hs_set_reserved_cus(16), "hs_set_reserved_cus")
            guard.measure(3.0)
            assert all(torch.equal(x, y) for x, y in zip(first, (guard.partials, guard.param_norms, guard.record)))
        finally:
            _lib.check(_lib.lib.hs_set_reserved_cus(prev), "hs_set_reserved_cus")
    finally:
        dp.remove()


def _assert_follows(ref, opt, a, b, it):
    for x, y in zip(a, b):
        err = float((x - y).detach().abs().max()) / (float(x.detach().abs().max()) + 1e-12)
        assert err < 2e-6, (it, tuple(x.shape), err)


def _assert_moments(ref, opt, a, b):
    for x, y in zip(a, b):
        for k in ("exp_avg", "exp_avg_sq"):
            assert float((ref.state[x][k] - opt.state[y][k]).abs().max()) <= 5e-6 * float(ref.state[x][k].abs().max()), (k, tuple(x.shape))


@pytest.mark.parametrize("wd,decoupled", [(0.0, False), (0.05, False), (0.05, True)])
def test_norm_clipping_follows_torch(wd, decoupled):
    """12 steps of torch.nn.utils.clip_grad_norm_(params, 400) + torch Adam against FlatAdam(max_grad_norm=400).  The total norms
    of these gradients are about 14, 155, 297, then 432 and rising: steps 0-2 pass unclipped, steps 3-11 clip."""
    from heal_swin_amd.optim import FlatAdam
    a, b = _toy(), _in_sink(_toy())
    ref = (torch.optim.AdamW if decoupled else torch.optim.Adam)(a, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd)
    dp = _sink(b)
    try:
        opt = FlatAdam(b, dp, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, decoupled_weight_decay=decoupled, max_grad_norm=400.0)
        gen = torch.Generator(device=DEV).manual_seed(1)
        norms = []
        for it in range(12):
            _fill(gen, it, a, b)
            ref_norm = torch.nn.utils.clip_grad_norm_(a, 400.0)
            ref.step()
            opt.step()
            norms.append(float(opt.grad_norm))
            assert _rel(norms[-1], ref_norm) <= 1e-6  # (torch sums in fp32)
            _assert_follows(ref, opt, a, b, it)
        print("total norms:", [round(n, 1) for n in norms])
        assert all(n < 400.0 for n in norms[:3]) and all(n > 400.0 for n in norms[3:]), norms
        _assert_moments(ref, opt, a, b)
        assert int(opt.state[b[0]]["step"]) == 12 and int(opt.skipped_steps) == 0
        assert opt.param_grad_norms.shape == (len(b),)
    finally:
        dp.remove()


def test_value_clipping_follows_torch():
    from heal_swin_amd.optim import FlatAdam
    a, b = _toy(), _in_sink(_toy())
    ref = torch.optim.Adam(a, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
    dp = _sink(b)
    try:
        opt = FlatAdam(b, dp, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05, clip_value=0.5)
        gen = torch.Generator(device=DEV).manual_seed(1)
        for it in range(12):
            _fill(gen, it, a, b)
            torch.nn.utils.clip_grad_value_(a, 0.5)
            ref.step()
            opt.step()
            _assert_follows(ref, opt, a, b, it)
        _assert_moments(ref, opt, a, b)
        assert float(opt.guard.clip_coef) == 1.0 and float(opt.grad_norm) > 400.0, "the value algorithm measures, and scales by 1"
        assert float(b[0].grad.abs().max()) > 0.5, "the buckets themselves are not rewritten"
    finally:
        dp.remove()


def _state(opt):
    return [t.clone() for group in (opt._flat_p, opt._flat_m, opt._flat_v, [s for s in opt._flat_lowp if s is not None]) for t in group] + [opt._step.clone()]


def test_an_idle_guard_changes_nothing():
    """max_grad_norm far above every norm and a skip that never triggers: the same bits as the plain step, bf16 copies included."""
    from heal_swin_amd.optim import FlatAdam
    b, c = _in_sink(_toy()), _in_sink(_toy())
    dpb, dpc = _sink(b), _sink(c)
    try:
        kw = dict(lr=3e-3, betas=(0.9, 0.99), weight_decay=0.05)
        plain = FlatAdam(b, dpb, model=types.SimpleNamespace(), **kw)
        guarded = FlatAdam(c, dpc, model=types.SimpleNamespace(), max_grad_norm=1e30, skip_nonfinite=True, **kw)
        assert plain.guard is None and all(s is not None for s in guarded._flat_lowp)
        gen = torch.Generator(device=DEV).manual_seed(1)
        for it in range(5):
            _fill(gen, it, b, c)
            plain.step()
            guarded.step()
        assert all(torch.equal(x, y) for x, y in zip(_state(plain), _state(guarded)))
        assert int(guarded._step) == 5 and int(guarded.skipped_steps) == 0
        with pytest.raises(RuntimeError):
            plain.grad_norm
    finally:
        dpb.remove()
        dpc.remove()


@pytest.mark.parametrize("poison", ["nan in the scalar parameter", "inf in the last element of the last bucket"])
def test_a_nonfinite_step_is_skipped(poison):
    from heal_swin_amd.optim import FlatAdam
    a, b = _toy(), _in_sink(_toy())
    ref = torch.optim.Adam(a, lr=3e-3, betas=(0.9, 0.99), eps=1e-8)
    dp = _sink(b)
    try:
        opt = FlatAdam(b, dp, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, model=types.SimpleNamespace(), skip_nonfinite=True)
        masks = _gap_masks(dp)
        assert not bool(masks[-1][-1]), "the last element of the last bucket belongs to a parameter"
        gen = torch.Generator(device=DEV).manual_seed(1)
        for it in range(6):
            _fill(gen, it, a, b)
            if it == 2:
                if poison.startswith("nan"):
                    b[3].grad.fill_(float("nan"))
                else:
                    dp.buckets[-1][-1] = float("inf")
                before = _state(opt)
                opt.step()
                assert all(torch.equal(x, y) for x, y in zip(before, _state(opt))), "a skipped step writes nothing"
                assert int(opt.skipped_steps) == 1 and int(opt._step) == 2 and int(opt.guard.finite) == 0
                for m, bufs in zip(masks, zip(opt._flat_p, opt._flat_m, opt._flat_v, opt._flat_lowp, dp.buckets)):
                    assert not any(bool(t[m].any()) for t in bufs), "the gaps stay zero"
                continue
            ref.step()
            opt.step()
        for x, y in zip(a, b):  # torch saw the five good steps only
            assert float((x - y).detach().abs().max()) < 2e-6 * (float(x.detach().abs().max()) + 1e-12), tuple(x.shape)
        _assert_moments(ref, opt, a, b)
        assert int(opt._step) == 5 and int(opt.skipped_steps) == 1 and int(opt.guard.finite) == 1
    finally:
        dp.remove()


def test_clip_grad_norm_in_place():
    from heal_swin_amd.parallel import clip_grad_norm_
    a, b = _toy(), _in_sink(_toy())
    dp = _sink(b)
    try:
        masks = _gap_masks(dp)
        gen = torch.Generator(device=DEV).manual_seed(1)
        for it in (0, 3):  # total norm about 14 (left alone) and about 432 (scaled)
            _fill(gen, it, a, b)
            untouched = [f.clone() for f in dp.buckets]
            ref_norm = torch.nn.utils.clip_grad_norm_(a, 400.0)
            ref64 = torch.linalg.vector_norm(torch.cat([f.double() for f in untouched]))
            norm = clip_grad_norm_(dp, 400.0)
            assert norm.is_cuda and norm.dim() == 0 and _rel(norm, ref64) <= NORM_TOL and _rel(norm, ref_norm) <= 1e-6
            worst = max(_ulps(y.grad, x.grad) for x, y in zip(a, b))
            print(f"it {it}: norm {float(norm):.4f}, scaled gradients differ from torch's by at most {worst} ulp")
            assert worst <= 2
            if it == 0:
                assert all(torch.equal(f, u) for f, u in zip(dp.buckets, untouched))
            else:
                assert float(norm) > 400.0 and not torch.equal(dp.buckets[0], untouched[0])
            assert not any(bool(f[m].any()) for f, m in zip(dp.buckets, masks)), "the gaps stay zero"
    finally:
        dp.remove()


def test_launch_census(monkeypatch):
    from _lib_spy import launches, spy_on
    from heal_swin_amd import optim
    from heal_swin_amd.optim import FlatAdam
    b, c = _in_sink(_toy()), _in_sink(_toy())
    dpb, dpc = _sink(b), _sink(c)
    try:
        plain, guarded = FlatAdam(b, dpb), FlatAdam(c, dpc, max_grad_norm=1.0)
        _fill(torch.Generator(device=DEV).manual_seed(1), 1, b, c)
        n = len(dpb.buckets)
        called = spy_on(monkeypatch, ("hs_adam", "hs_grad"), [optim])
        plain.step()
        assert launches(called) == ["hs_adam_advance"] + ["hs_adam_step"] * n
        del called[:]
        guarded.step()
        assert launches(called) == sorted(["hs_grad_stats"] * n + ["hs_grad_guard_finalize"] + ["hs_adam_step_guarded"] * n + ["hs_adam_advance_guarded"])
        assert called.index("hs_grad_guard_finalize") == n and called[-1] == "hs_adam_advance_guarded", "measure first, then step"
    finally:
        dpb.remove()
        dpc.remove()


def test_guarded_step_in_a_captured_training_step():
    """The tiny model of test_gpu_optim.test_flat_adam_in_a_captured_training_step through graphs.GraphedTrainStep: the guarded step is
    captured whole (no host read), replays equal the eager run bit for bit while some steps clip and some do not, and a replay whose
    loss is infinite leaves the parameters alone and counts as skipped."""
    from heal_swin_amd.graphs import GraphedTrainStep
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    torch.manual_seed(0)
    lins = [torch.nn.Linear(32, 16).to(DEV) for _ in range(3)]
    for lin in lins[1:]:
        lin.load_state_dict(lins[0].state_dict())
    amp = torch.tensor([1.0, 1.0, 0.5, 2.0, 0.5, 2.0], device=DEV)  # gradient norms a factor 16 apart, whatever the trajectory
    xs = torch.randn(6, 64, 32, device=DEV) * amp[:, None, None]
    dummy = torch.zeros(1, device=DEV)
    scale = torch.ones((), device=DEV)
    sinks = [GradBucketAllReduce(lin.parameters(), direct_wgrad=False) for lin in lins]
    step = None
    try:
        def eager(lin, dp, opt, x):
            dp.zero_grad()
            loss = lin(x).square().mean() * scale
            loss.backward()
            dp.finish()
            opt.step()
        # the eager norms of this model, unclipped: warm-up steps 0, 0 and then steps 2 ... 5
        probe = FlatAdam(lins[0].parameters(), sinks[0], lr=1e-2, track_grad_norm=True)
        seen = []
        for i in (0, 0, 2, 3, 4, 5):
            eager(lins[0], sinks[0], probe, xs[i])
            seen.append(float(probe.grad_norm))
        max_norm = math.sqrt(min(seen[2:]) * max(seen[2:]))
        oa = FlatAdam(lins[1].parameters(), sinks[1], lr=1e-2, max_grad_norm=max_norm, skip_nonfinite=True)
        ob = FlatAdam(lins[2].parameters(), sinks[2], lr=1e-2, max_grad_norm=max_norm, skip_nonfinite=True)
        step = GraphedTrainStep(lins[2], lambda out, t: out.square().mean() * scale, ob, xs[0], dummy, warmup=2, grad_sink=sinks[2])
        for i in (0, 0):
            eager(lins[1], sinks[1], oa, xs[i])
        norms = []
        for i in (2, 3, 4, 5):
            eager(lins[1], sinks[1], oa, xs[i])
            step(xs[i], dummy)
            assert torch.equal(oa.grad_norm, ob.grad_norm)
            norms.append(float(ob.grad_norm))
            for p, q in zip(lins[1].parameters(), lins[2].parameters()):
                assert torch.equal(p, q), i
        print("max_norm", max_norm, "norms", norms)
        assert any(n > max_norm for n in norms) and any(n < max_norm for n in norms), (max_norm, norms)
        assert int(ob._step) == 6 and int(ob.skipped_steps) == 0
        before = [p.detach().clone() for p in lins[2].parameters()]
        scale.fill_(float("inf"))
        step(xs[1], dummy)
        assert all(torch.equal(p, q) for p, q in zip(before, lins[2].parameters())) and int(ob.skipped_steps) == 1 and int(ob._step) == 6
        scale.fill_(1.0)
        step(xs[1], dummy)
        assert not any(torch.equal(p, q) for p, q in zip(before, lins[2].parameters())) and int(ob.skipped_steps) == 1 and int(ob._step) == 7
        assert all(bool(torch.isfinite(p).all()) for p in lins[2].parameters())
    finally:
        if step is not None:
            torch.cuda.synchronize()
            step.close()
        for dp in sinks:
            dp.remove()


def test_named_norms_on_the_heads_3_model():
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    spec = DataSpec(dim_in=12 * 32 * 32, f_in=3, f_out=12, base_pix=12, class_names=[])
    cfg = SwinHPTransformerConfig(patch_size=4, window_size=64, shift_size=32, rel_pos_bias="flat", embed_dim=96, depths=[2, 2],
                                  num_heads=[3, 6], drop_path_rate=0.0, use_cos_attn=True)
    torch.manual_seed(0)
    model = SwinHPTransformerSys(cfg, spec).to(DEV).train()
    model.compute_dtype = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randint(0, 256, (2, 3, spec.dim_in), generator=g, device=DEV).float()
    y = torch.randint(0, 12, (2, spec.dim_in), generator=g, device=DEV, dtype=torch.uint8)
    dp = GradBucketAllReduce(model.parameters())
    try:
        opt = FlatAdam(model.parameters(), dp, lr=1e-3, model=model, track_grad_norm=True)
        dp.zero_grad()
        model.forward_seg_loss(x, y).backward()
        dp.finish()
        opt.step()
        named = opt.guard.named_norms(model)
        trainable = {n: p for n, p in model.named_parameters() if p.requires_grad}
        assert set(named) == {f"grad_2.0_norm_{n}" for n in trainable} | {"grad_2.0_norm_total"}
        assert any(p.numel() == 3 for p in trainable.values()), "a 3-element logit_scale is what this layout is about"
        for n, p in trainable.items():
            ref = float(torch.linalg.vector_norm(p.grad.double().flatten()))
            assert abs(named[f"grad_2.0_norm_{n}"] - ref) <= NORM_TOL * ref, (n, named[f"grad_2.0_norm_{n}"], ref)
        ref = float(torch.linalg.vector_norm(torch.cat([p.grad.double().flatten() for p in trainable.values()])))
        assert abs(named["grad_2.0_norm_total"] - ref) <= NORM_TOL * ref and ref > 0
    finally:
        dp.remove()


def test_bad_arguments_are_refused():
    """Null pointers and n <= 0: HS_ERR_INVALID_ARG (1).  A pointer off its 16-byte boundary: HS_ERR_MISALIGNED (5), the library's
    status for that argument error (include/healswin.h, "Pointer alignment").  Nothing is launched: the buffers keep their values."""
    from heal_swin_amd import _lib
    from heal_swin_amd.optim import FlatAdam
    lib, ptr = _lib.lib, _lib.ptr
    n = 64
    f = torch.ones(4, n + 4, device=DEV)
    p, g, m, v = f[0], f[1], f[2], f[3]
    items = torch.tensor([[0, n]], dtype=torch.int64, device=DEV)
    params = torch.tensor([[0, 1]], dtype=torch.int32, device=DEV)
    part = torch.zeros(2, 2, dtype=torch.float64, device=DEV)
    work = torch.zeros(2, 2, dtype=torch.float64, device=DEV)
    norm = torch.zeros(1, device=DEV)
    rec = torch.zeros(8, device=DEV)
    step = torch.zeros((), dtype=torch.int64, device=DEV)
    skipped = torch.zeros((), dtype=torch.int64, device=DEV)
    s = _lib.stream_ptr(f.device)
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    adam = lambda P, G, M, V, N, R: lib.hs_adam_step_guarded(P, G, M, V, None, N, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0, ptr(step), 0.0, R, 1, s)
    invalid = [
        lib.hs_grad_stats(None, n, ptr(items), 1, ptr(part), s), lib.hs_grad_stats(ptr(g), n, None, 1, ptr(part), s),
        lib.hs_grad_stats(ptr(g), n, ptr(items), 1, None, s), lib.hs_grad_stats(ptr(g), 0, ptr(items), 1, ptr(part), s),
        lib.hs_grad_stats(ptr(g), n, ptr(items), 0, ptr(part), s),
        lib.hs_grad_guard_finalize(None, 1, ptr(params), 1, 0, -1.0, ptr(norm), ptr(work), ptr(rec), s),
        lib.hs_grad_guard_finalize(ptr(part), 1, None, 1, 0, -1.0, ptr(norm), ptr(work), ptr(rec), s),
        lib.hs_grad_guard_finalize(ptr(part), 1, ptr(params), 1, 0, -1.0, None, ptr(work), ptr(rec), s),
        lib.hs_grad_guard_finalize(ptr(part), 1, ptr(params), 1, 0, -1.0, ptr(norm), None, ptr(rec), s),
        lib.hs_grad_guard_finalize(ptr(part), 1, ptr(params), 1, 0, -1.0, ptr(norm), ptr(work), None, s),
        lib.hs_grad_guard_finalize(ptr(part), 1, ptr(params), 0, 0, -1.0, ptr(norm), ptr(work), ptr(rec), s),
        lib.hs_grad_guard_finalize(ptr(part), 0, ptr(params), 1, 0, -1.0, ptr(norm), ptr(work), ptr(rec), s),
        adam(None, ptr(g), ptr(m), ptr(v), n, ptr(rec)), adam(ptr(p), None, ptr(m), ptr(v), n, ptr(rec)),
        adam(ptr(p), ptr(g), ptr(m), ptr(v), n, None), adam(ptr(p), ptr(g), ptr(m), ptr(v), 0, ptr(rec)),
        adam(ptr(p), ptr(g), ptr(m), ptr(v), -4, ptr(rec)),
        lib.hs_adam_advance_guarded(None, ptr(rec), 1, ptr(skipped), s), lib.hs_adam_advance_guarded(ptr(step), None, 1, ptr(skipped), s),
        lib.hs_adam_advance_guarded(ptr(step), ptr(rec), 1, None, s),
        lib.hs_grad_scale(None, n, 0.0, ptr(rec), s), lib.hs_grad_scale(ptr(g), n, 0.0, None, s), lib.hs_grad_scale(ptr(g), 0, 0.0, ptr(rec), s),
    ]
    assert invalid == [1] * len(invalid), invalid
    misaligned = [
        lib.hs_grad_stats(off(g), n, ptr(items), 1, ptr(part), s), lib.hs_grad_stats(ptr(g), n, ctypes.c_void_p(items.data_ptr() + 8), 1, ptr(part), s),
        lib.hs_grad_stats(ptr(g), n, ptr(items), 1, ctypes.c_void_p(part.data_ptr() + 8), s),
        lib.hs_grad_guard_finalize(ctypes.c_void_p(part.data_ptr() + 8), 1, ptr(params), 1, 0, -1.0, ptr(norm), ptr(work), ptr(rec), s),
        lib.hs_grad_guard_finalize(ptr(part), 1, ptr(params), 1, 0, -1.0, ptr(norm), ptr(work), off(rec), s),
        adam(off(p), ptr(g), ptr(m), ptr(v), n, ptr(rec)), adam(ptr(p), off(g), ptr(m), ptr(v), n, ptr(rec)),
        adam(ptr(p), ptr(g), off(m), ptr(v), n, ptr(rec)), adam(ptr(p), ptr(g), ptr(m), off(v), n, ptr(rec)),
        adam(ptr(p), ptr(g), ptr(m), ptr(v), n, off(rec)),
        lib.hs_adam_advance_guarded(ptr(step), off(rec), 1, ptr(skipped), s),
        lib.hs_grad_scale(off(g), n, 0.0, ptr(rec), s), lib.hs_grad_scale(ptr(g), n, 0.0, off(rec), s),
    ]
    assert misaligned == [5] * len(misaligned), misaligned
    torch.cuda.synchronize()
    assert bool((f == 1).all()) and int(step) == 0 and int(skipped) == 0 and not bool(part.any()) and not bool(rec.any())
    # and the Python layer
    b = _in_sink(_toy())
    dp = _sink(b)
    try:
        for kw in (dict(max_grad_norm=1.0, clip_value=1.0), dict(max_grad_norm=0.0), dict(max_grad_norm=float("nan")), dict(clip_value=-1.0),
                   dict(clip_value=float("inf")), dict(norm_type=3.0)):
            with pytest.raises(ValueError):
                FlatAdam(b, dp, **kw)
    finally:
        dp.remove()
