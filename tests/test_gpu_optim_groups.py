"""FlatAdam with parameter groups (hs_adam_step_groups / hs_adam_step_groups_guarded in csrc/adam.hip, optim.group_tables,
optim.weight_decay_groups) against torch.optim.Adam / AdamW built over the same groups, on the same parameters and gradients.

Layout: the shapes of test_gpu_optim plus (2050,) and (3, 1, 1) in buckets of 4096 elements.  Bucket 0 holds (3, 1, 1) | (2050,) |
(1000,), bucket 1 (129, 33) alone, bucket 2 (1,) | (7, 5, 3) | (64,) | (64, 32); group = parameter index modulo 3, so neighbours in a
bucket always differ: runs of one slot (8 elements, 1 or 3 of them real), runs that start and end inside a 1024-element block, runs
that span blocks, blocks with several runs, parameter tails that are no multiple of 4.

Tolerances: the bounds of test_gpu_optim.test_flat_adam_follows_torch_adam (parameters 2e-6 of the tensor's scale after every step,
moments 5e-6 after the last); the grouped kernel runs the same arithmetic per element, only its operands come from the group's record.
What a group does not set comes from that test's constructor arguments, DEFAULTS = betas (0.9, 0.99), eps 1e-8, for which its bounds
were made: `adam_one` forms 1 - beta2 in fp32 from the fp32 beta2 (torch: in double, then rounded), which is 9e-7 from torch's factor
at beta2 = 0.99 and 1.3e-5 at torch's default 0.999 -- there exp_avg_sq sits 1.3e-5 below torch's (measured on the first run of this
file with the torch defaults: 3.6e-5 absolute at a scale of 2.77, against the 5e-6 bound; the parameters stayed within 2e-6 for all
12 steps).  That is the single-group kernel's arithmetic, which the grouped kernel has to reproduce bit for bit (the second test)."""
import copy
import ctypes
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(64, 32), (64,), (7, 5, 3), (1,), (129, 33), (1000,), (2050,), (3, 1, 1)]
OPTIONS = [dict(lr=3e-3, weight_decay=0.05, decoupled_weight_decay=True),
           dict(lr=1e-3, weight_decay=0.0),
           dict(lr=3e-4, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.05, decoupled_weight_decay=False)]
DEFAULTS = dict(lr=1.0, betas=(0.9, 0.99), eps=1e-8)  # (every group sets its own lr; torch takes decoupled_weight_decay per group)


def _toy(seed=0):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in SHAPES]


def _sink(params):
    from heal_swin_amd.parallel import GradBucketAllReduce
    dp = GradBucketAllReduce(params, bucket_bytes=16 << 10, direct_wgrad=False)
    assert len(dp.buckets) == 3
    return dp


def _groups(params, options=OPTIONS):
    """group k = the parameters whose index is k modulo the group count, with options[k]"""
    return [dict(opts, params=params[k::len(options)]) for k, opts in enumerate(options)]


def _fill(gen, it, plain, *in_sinks, offset=0.0):
    """the same randn * (0.1 + it) gradient for the plain parameters (`.grad` replaced; may be None) and for every list of parameters
    that live in a sink (the bucket views are written)"""
    for i, shape in enumerate(SHAPES):
        grad = torch.randn(shape, generator=gen, device=DEV) * (0.1 + it) + offset
        if plain is not None:
            plain[i].grad = grad.clone()
        for params in in_sinks:
            params[i].grad.copy_(grad)


def _assert_follows(a, b, it, bound=2e-6):
    for x, y in zip(a, b):
        err = float((x - y).detach().abs().max()) / (float(x.detach().abs().max()) + 1e-12)
        assert err < bound, (it, tuple(x.shape), err)


def _assert_moments(ref, opt, a, b):
    for x, y in zip(a, b):
        for k in ("exp_avg", "exp_avg_sq"):
            assert float((ref.state[x][k] - opt.state[y][k]).abs().max()) <= 5e-6 * float(ref.state[x][k].abs().max()), (k, tuple(x.shape))


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


def _state(opt):
    return [t.clone() for group in (opt._flat_p, opt._flat_m, opt._flat_v, [s for s in opt._flat_lowp if s is not None]) for t in group] + [opt._step.clone()]


def test_grouped_step_follows_torch_adam():
    from heal_swin_amd.optim import FlatAdam
    a, b = _toy(), _toy()
    ref = torch.optim.Adam(_groups(a), **DEFAULTS)
    dp = _sink(b)
    try:
        opt = FlatAdam(_groups(b), dp, **DEFAULTS)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "moving the parameters into the flat buffers must not change them"
        assert len(opt.param_groups) == 3 and all(g["capturable"] and g["fused"] for g in opt.param_groups)
        assert opt.param_groups[1]["betas"] == (0.9, 0.99) and opt.param_groups[2]["betas"] == (0.8, 0.9), "unset keys come from the defaults"
        assert [g["eps"] for g in opt.param_groups] == [1e-8, 1e-8, 1e-6] and [g["decoupled_weight_decay"] for g in opt.param_groups] == [True, False, False]
        # the layout this file is about: neighbours in a bucket are in different groups, so every slot is a run of its own
        for (runs, first), f in zip(opt._group_tables, dp.buckets):
            assert runs.shape[0] == sum(1 for p in b if dp.buckets[dp._where[p]] is f) and first.numel() == -(-f.numel() // 1024)
        assert any(len(set(first.tolist())) < runs.shape[0] for runs, first in opt._group_tables), "a block with several runs"
        with pytest.raises(ValueError, match="at construction"):
            opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(4, device=DEV))]))
        gen = torch.Generator(device=DEV).manual_seed(1)
        for it in range(12):
            _fill(gen, it, a, b)
            ref.step()
            opt.step()
            _assert_follows(a, b, it)
        _assert_moments(ref, opt, a, b)
        assert all(int(opt.state[y]["step"]) == 12 for y in b)
    finally:
        dp.remove()


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("betas", [(0.9, 0.99), (0.9, 0.999)])
def test_equal_groups_give_the_bits_of_the_single_group_kernel(betas, guarded):
    from heal_swin_amd.optim import FlatAdam
    b, c = _toy(), _toy()
    dpb, dpc = _sink(b), _sink(c)
    try:
        kw = dict(lr=3e-3, betas=betas, weight_decay=0.05)
        if guarded:  # total norms of these gradients: about 10, 107, 205, 303, 400 -- steps 0-2 pass, 3 and 4 clip
            kw.update(max_grad_norm=250.0, skip_nonfinite=True)
        one = FlatAdam(b, dpb, model=types.SimpleNamespace(), **kw)
        three = FlatAdam(_groups(c, [{}, {}, {}]), dpc, model=types.SimpleNamespace(), **kw)
        assert one._group_tables is None and len(three._group_tables) == 3 and all(s is not None for s in three._flat_lowp)
        gen = torch.Generator(device=DEV).manual_seed(1)
        norms = []
        for it in range(5):
            _fill(gen, it, None, b, c)
            one.step()
            three.step()
            if guarded:
                assert torch.equal(one.grad_norm, three.grad_norm)
                norms.append(float(three.grad_norm))
        for k, (x, y) in enumerate(zip(_state(one), _state(three))):
            assert torch.equal(x, y), k
        for x, y in zip(b, c):
            assert torch.equal(x, y) and torch.equal(one.state[x]["exp_avg"], three.state[y]["exp_avg"])
            assert torch.equal(one.state[x]["exp_avg_sq"], three.state[y]["exp_avg_sq"])
            assert torch.equal(one.lowp_copy(x, torch.bfloat16), three.lowp_copy(y, torch.bfloat16))
            assert torch.equal(three.lowp_copy(y, torch.bfloat16), y.detach().to(torch.bfloat16))
        if guarded:
            assert any(n < 250.0 for n in norms) and any(n > 250.0 for n in norms), norms
    finally:
        dpb.remove()
        dpc.remove()


def test_tensor_and_float_learning_rates_mix():
    """Group 0's lr is a device tensor updated in place, group 1's a float changed through param_groups, group 2's stays: against
    torch.optim.Adam driven by the same schedule (test 1's bounds), and bit for bit against a FlatAdam whose lrs are all floats."""
    from heal_swin_amd.optim import FlatAdam
    a, b, c = _toy(), _toy(), _toy()
    ref = torch.optim.Adam(_groups(a), **DEFAULTS)
    dpb, dpc = _sink(b), _sink(c)
    try:
        lr0 = torch.tensor(OPTIONS[0]["lr"], device=DEV)
        mixed = FlatAdam(_groups(b, [dict(OPTIONS[0], lr=lr0), OPTIONS[1], OPTIONS[2]]), dpb, **DEFAULTS)
        floats = FlatAdam(_groups(c), dpc, **DEFAULTS)
        gen = torch.Generator(device=DEV).manual_seed(1)
        for it in range(6):
            s0, s1 = OPTIONS[0]["lr"] * 0.7 ** it, OPTIONS[1]["lr"] * (1 + it) / 3
            ref.param_groups[0]["lr"], ref.param_groups[1]["lr"] = s0, s1
            floats.param_groups[0]["lr"], floats.param_groups[1]["lr"] = s0, s1
            lr0.fill_(s0)
            mixed.param_groups[1]["lr"] = s1
            _fill(gen, it, a, b, c)
            ref.step()
            mixed.step()
            floats.step()
            _assert_follows(a, b, it)
        _assert_moments(ref, mixed, a, b)
        assert all(torch.equal(y, z) for y, z in zip(b, c)), "a tensor lr and the same float lr must give the same bits"
        # the schedule really acted: an optimizer that kept the initial rates ends elsewhere
        assert mixed.param_groups[0]["lr"] is lr0 and abs(float(lr0) - OPTIONS[0]["lr"] * 0.7 ** 5) < 1e-9
    finally:
        dpb.remove()
        dpc.remove()


def test_the_guard_acts_across_groups():
    """max_grad_norm clips by the norm over ALL groups (torch.nn.utils.clip_grad_norm_ over all parameters, then the grouped torch step);
    skip_nonfinite with one NaN in one group's gradient leaves every group untouched and counts one skip."""
    from heal_swin_amd.optim import FlatAdam
    a, b = _toy(), _toy()
    ref = torch.optim.Adam(_groups(a), **DEFAULTS)
    dp = _sink(b)
    try:
        opt = FlatAdam(_groups(b), dp, **DEFAULTS, model=types.SimpleNamespace(), max_grad_norm=250.0, skip_nonfinite=True)
        gen = torch.Generator(device=DEV).manual_seed(1)
        norms = []
        for it in range(8):
            _fill(gen, it, a, b)
            if it == 4:  # one NaN, in a parameter of group 2 (index 5)
                b[5].grad.view(-1)[17] = float("nan")
                before = _state(opt)
                opt.step()
                assert all(torch.equal(x, y) for x, y in zip(before, _state(opt))), "a skipped step writes nothing, in any group"
                assert int(opt.skipped_steps) == 1 and int(opt._step) == 4 and int(opt.guard.finite) == 0
                continue
            ref_norm = torch.nn.utils.clip_grad_norm_(a, 250.0)
            ref.step()
            opt.step()
            norms.append(float(opt.grad_norm))
            assert abs(norms[-1] - float(ref_norm)) <= 1e-6 * float(ref_norm)  # (torch sums in fp32)
            _assert_follows(a, b, it)
        assert any(n < 250.0 for n in norms) and any(n > 250.0 for n in norms), norms
        _assert_moments(ref, opt, a, b)
        assert int(opt._step) == 7 and int(opt.skipped_steps) == 1 and int(opt.guard.finite) == 1
        assert opt.param_grad_norms.shape == (len(b),)
    finally:
        dp.remove()


def test_padding_stays_zero_for_every_group_setting():
    """Gaps and bucket tails (p = g = m = v = 0) go through the grouped kernel with everything else and stay exactly zero with eps = 0
    and decoupled decay in every group (test_gpu_optim.test_flat_adam_gaps_stay_zero_also_without_eps, with groups)."""
    from heal_swin_amd.optim import FlatAdam
    options = [dict(lr=3e-3, eps=0.0, weight_decay=0.05, decoupled_weight_decay=True),
               dict(lr=1e-3, eps=0.0, weight_decay=0.5, decoupled_weight_decay=True),
               dict(lr=3e-4, eps=0.0, betas=(0.8, 0.9), weight_decay=0.1, decoupled_weight_decay=True)]
    a, b = _toy(5), _toy(5)
    ref = torch.optim.Adam(_groups(a, options), lr=1.0)
    dp = _sink(b)
    try:
        opt = FlatAdam(_groups(b, options), dp, lr=1.0, model=types.SimpleNamespace())
        gaps = _gap_masks(dp)
        gen = torch.Generator(device=DEV).manual_seed(1)
        for it in range(3):
            _fill(gen, 0.9, a, b, offset=0.5)  # (randn + 0.5: no exact zeros, so eps = 0 stays finite on real elements)
            ref.step()
            opt.step()
            for P, M, V, S, G, gap in zip(opt._flat_p, opt._flat_m, opt._flat_v, opt._flat_lowp, dp.buckets, gaps):
                assert all(bool(torch.isfinite(t).all()) for t in (P, M, V, S.float()))
                assert not any(bool(t[gap].any()) for t in (P, M, V, S, G))
            _assert_follows(a, b, it)
    finally:
        dp.remove()


def test_state_dict_round_trips_with_groups_and_with_torch():
    from heal_swin_amd.optim import FlatAdam
    options = [dict(o, decoupled_weight_decay=True) for o in OPTIONS]  # (AdamW: every group decoupled)
    a, b = _toy(3), _toy(3)
    ref = torch.optim.AdamW(_groups(a, [{k: v for k, v in o.items() if k != "decoupled_weight_decay"} for o in options]), lr=1.0)
    dpb = _sink(b)
    sinks = [dpb]
    try:
        ob = FlatAdam(_groups(b, options), dpb, lr=1.0)
        gen = torch.Generator(device=DEV).manual_seed(2)
        for it in range(3):
            _fill(gen, it, a, b)
            ref.step()
            ob.step()
        sd = copy.deepcopy(ob.state_dict())
        assert [len(g["params"]) for g in sd["param_groups"]] == [3, 3, 2] and sorted(sd["state"]) == list(range(8))
        assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2], [3, 4, 5], [6, 7]], "parameter ids are numbered through the groups"

        def fresh(source):
            d = [torch.nn.Parameter(x.detach().clone()) for x in source]
            sinks.append(_sink(d))
            # built with other options than the state dict carries: load_state_dict must restore them per group
            return d, FlatAdam(_groups(d, [dict(lr=0.5), dict(lr=0.25, eps=1e-3), dict(lr=0.125)]), sinks[-1], decoupled_weight_decay=True)
        # ---- FlatAdam -> FlatAdam, and torch.optim.AdamW -> FlatAdam
        d, od = fresh(b)
        od.load_state_dict(sd)
        e, oe = fresh(a)
        oe.load_state_dict(copy.deepcopy(ref.state_dict()))
        for o in (od, oe):
            assert int(o._step) == 3
            for g, want in zip(o.param_groups, options):
                assert g["lr"] == want["lr"] and g["weight_decay"] == want["weight_decay"] and g["capturable"] and g["fused"]
                assert tuple(g["betas"]) == tuple(want.get("betas", (0.9, 0.999))) and g["eps"] == want.get("eps", 1e-8)
                assert g["decoupled_weight_decay"] is True
        # ---- and FlatAdam -> torch.optim.AdamW
        f = [torch.nn.Parameter(x.detach().clone()) for x in b]
        of = torch.optim.AdamW(_groups(f, [dict(lr=0.5), dict(lr=0.25), dict(lr=0.125)]), fused=True)
        of.load_state_dict(copy.deepcopy(ob.state_dict()))
        _fill(gen, 3, a, b)
        for x, others in zip(a, zip(d, e, f)):
            for y, in_sink in zip(others, (True, True, False)):
                if in_sink:
                    y.grad.copy_(x.grad)
                else:
                    y.grad = x.grad.clone()
        for o in (ref, ob, od, oe, of):
            o.step()
        for x, y, *others in zip(a, b, d, e, f):
            for z, base in zip(others, (y, x, y)):  # d resumed b, e resumed a, f resumed b
                assert float((z - base).abs().max()) <= 1e-6 * float(base.abs().max()), tuple(x.shape)
        for o, ps, dp in ((od, d, sinks[1]), (oe, e, sinks[2])):
            for p in ps:
                for k, buf in (("exp_avg", o._flat_m), ("exp_avg_sq", o._flat_v)):
                    flat = buf[dp._where[p]]
                    off = dp._views[p].storage_offset() - dp.buckets[dp._where[p]].storage_offset()
                    assert o.state[p][k].data_ptr() == flat.data_ptr() + 4 * off, "state must stay in the flat buffer"
                assert o.state[p]["step"] is o._step
    finally:
        for dp in sinks:
            dp.remove()


def test_grouped_step_in_a_captured_training_step():
    """The toy linear model of test_gpu_optim.test_flat_adam_in_a_captured_training_step through graphs.GraphedTrainStep with two groups
    (weight | bias; the bias group's lr a device tensor that changes between replays): replays equal the eager steps bit for bit."""
    from heal_swin_amd.graphs import GraphedTrainStep
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    torch.manual_seed(0)
    lin_a, lin_b = torch.nn.Linear(32, 16).to(DEV), torch.nn.Linear(32, 16).to(DEV)
    lin_b.load_state_dict(lin_a.state_dict())
    xs = torch.randn(4, 64, 32, device=DEV)
    dummy = torch.zeros(1, device=DEV)
    dpa, dpb = GradBucketAllReduce(lin_a.parameters(), direct_wgrad=False), GradBucketAllReduce(lin_b.parameters(), direct_wgrad=False)
    step = None
    try:
        lr_a, lr_b = torch.tensor(1e-2, device=DEV), torch.tensor(1e-2, device=DEV)

        def groups(lin, lr):
            return [dict(params=[lin.weight], lr=1e-2, weight_decay=0.05, decoupled_weight_decay=True), dict(params=[lin.bias], lr=lr, betas=(0.8, 0.9))]
        oa, ob = FlatAdam(groups(lin_a, lr_a), dpa), FlatAdam(groups(lin_b, lr_b), dpb)

        def eager(x):
            dpa.zero_grad()
            lin_a(x).square().mean().backward()
            dpa.finish()
            oa.step()
        step = GraphedTrainStep(lin_b, lambda out, t: out.square().mean(), ob, xs[0], dummy, warmup=2, grad_sink=dpb)
        for _ in range(2):
            eager(xs[0])
        for i in (1, 2, 3):
            lr_a.fill_(1e-2 / i)
            lr_b.fill_(1e-2 / i)
            eager(xs[i])
            step(xs[i], dummy)
            for p, q in zip(lin_a.parameters(), lin_b.parameters()):
                assert torch.equal(p, q), i
        assert int(oa._step) == int(ob._step) == 5
        for p, q in zip(lin_a.parameters(), lin_b.parameters()):
            assert torch.equal(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])
    finally:
        if step is not None:
            torch.cuda.synchronize()
            step.close()
        dpa.remove()
        dpb.remove()


def test_bad_grouped_calls_are_refused():
    """Each bad call alone: a status and a message, nothing launched -- the buffers keep their values.  Argument errors are
    HS_ERR_INVALID_ARG (1); a table off its boundary is HS_ERR_MISALIGNED (5), the library's status for that argument error
    (include/healswin.h, "Pointer alignment"), as for every other entry point."""
    from heal_swin_amd import _lib
    from heal_swin_amd.optim import adam_max_groups
    lib, ptr = _lib.lib, _lib.ptr
    n = 2048
    f = torch.ones(4, n, device=DEV)
    runs = torch.tensor([[0, 0], [8, 1], [1032, 0], [0, 0]], dtype=torch.int32, device=DEV)
    first = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    step = torch.zeros((), dtype=torch.int64, device=DEV)
    rec = torch.zeros(4, device=DEV)
    rec[1] = 1.0
    rec.view(torch.int32)[2] = 1
    s = _lib.stream_ptr(f.device)
    most = adam_max_groups()
    good = [(1e-3, 0.9, 0.999, 1e-8, 0.0, False), (1e-2, 0.8, 0.9, 1e-6, 0.05, True)]

    def call(groups=good, n_groups=2, runs_ptr=None, n_runs=3, first_ptr=None, n_blocks=2, covered=n, guarded=False):
        records = _lib.adam_groups(groups)
        args = [ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(f[3]), None, n, records, n_groups, runs_ptr or ptr(runs), n_runs,
                first_ptr or ptr(first), n_blocks, covered, ptr(step)]
        if guarded:
            return lib.hs_adam_step_groups_guarded(*args, 0.0, ptr(rec), 1, s)
        return lib.hs_adam_step_groups(*args, s)
    off4 = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    bad = [("group count 0", dict(n_groups=0), 1, "group count"),
           ("group count above the maximum", dict(groups=good * (most // 2 + 1), n_groups=most + 1), 1, "group count"),
           ("a misaligned run table", dict(runs_ptr=off4(runs)), 5, "aligned"),
           ("a run table whose last run does not reach n", dict(covered=n - 8), 1, "covers"),
           ("a run table that reaches past n", dict(covered=n + 8), 1, "covers"),
           ("more runs than slots", dict(n_runs=n // 8 + 1), 1, "run count"),
           ("no runs", dict(n_runs=0), 1, "run count"),
           ("a block table of another length", dict(n_blocks=1), 1, "block table"),
           ("a beta of 1 in the second group", dict(groups=[good[0], (1e-2, 0.8, 1.0, 1e-6, 0.05, True)]), 1, "group 1"),
           ("a negative weight decay", dict(groups=[(1e-3, 0.9, 0.999, 1e-8, -0.1, False), good[1]]), 1, "group 0")]
    for guarded in (False, True):
        for what, kw, status, word in bad:
            st = call(guarded=guarded, **kw)
            msg = lib.hs_last_error().decode()
            assert st == status and word in msg and ("hs_adam_step_groups_guarded" if guarded else "hs_adam_step_groups:") in msg, (what, st, msg)
    torch.cuda.synchronize()
    assert bool((f == 1).all()) and int(step) == 0, "a refused call launches nothing"
    # and the same call without a fault steps group 1's slots only where the table says
    assert call() == 0 and call(guarded=True) == 0
    torch.cuda.synchronize()
    assert bool((f[1] == 1).all()) and not bool((f[0] == 1).any()) and float(f[0, 8]) < float(f[0, 0]) == float(f[0, 1032])


def test_a_model_trains_with_weight_decay_groups():
    """One tiny SwinHPTransformerSys (position-bias tables, cosine attention) trained with `weight_decay_groups` and `model=`: the next
    forward sees the updated bf16 weights without a copy pass (test_gpu_optim.test_flat_adam_keeps_the_models_bf16_copies_current),
    and the losses follow torch.optim.AdamW over the same two groups."""
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys
    from heal_swin_amd.optim import FlatAdam, weight_decay_groups
    from heal_swin_amd.parallel import GradBucketAllReduce
    spec = DataSpec(dim_in=12 * 32 * 32, f_in=3, f_out=12, base_pix=12, class_names=[])
    cfg = SwinHPTransformerConfig(patch_size=4, window_size=64, shift_size=32, rel_pos_bias="flat", embed_dim=64, depths=[2, 2],
                                  num_heads=[2, 4], drop_path_rate=0.0, use_cos_attn=True)
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randint(0, 256, (2, 3, spec.dim_in), generator=g, device=DEV).float()
    y = torch.randint(0, 12, (2, spec.dim_in), generator=g, device=DEV, dtype=torch.uint8)
    losses = {}
    for kind in ("torch", "flat"):
        torch.manual_seed(0)
        model = SwinHPTransformerSys(cfg, spec).to(DEV).train()
        model.compute_dtype = torch.bfloat16
        dp = GradBucketAllReduce(model.parameters())
        try:
            groups = weight_decay_groups(model, 0.05)
            assert groups[0]["params"] and groups[1]["params"] and groups[1]["weight_decay"] == 0.0
            opt = (FlatAdam(groups, dp, lr=1e-3, decoupled_weight_decay=True, model=model) if kind == "flat"
                   else torch.optim.AdamW(groups, lr=1e-3, fused=True))
            copies = []
            orig = torch._foreach_copy_
            torch._foreach_copy_ = lambda *a, **k: (copies.append(1), orig(*a, **k))[1]
            try:
                ls = []
                for _ in range(4):
                    dp.zero_grad()
                    loss = model.forward_seg_loss(x, y)
                    loss.backward()
                    dp.finish()
                    opt.step()
                    ls.append(float(loss))
            finally:
                torch._foreach_copy_ = orig
            losses[kind] = ls
            if kind == "flat":
                assert opt._group_tables is not None and len(opt.param_groups) == 2
                assert len(copies) <= 1, f"the cast cache ran {len(copies)} copy passes; FlatAdam should have made them unnecessary"
                cache = model.__dict__["_cast_cache"]
                assert cache.all_external
                for p, sh in zip(cache.params, cache.shadows):
                    assert torch.equal(sh, p.detach().to(torch.bfloat16))
                for P in opt._flat_p:
                    assert bool(torch.isfinite(P).all())
            else:
                assert len(copies) == 4
        finally:
            dp.remove()
    assert losses["flat"][0] == losses["torch"][0]
    for a, b in zip(losses["torch"], losses["flat"]):
        assert abs(a - b) <= 2e-3 * abs(a), (losses["torch"], losses["flat"])
    assert losses["flat"][-1] < losses["flat"][0]
