"""optim.FlatAdam (csrc/adam.hip) against torch.optim.Adam / AdamW -- the optimizer the reference's trainer builds
(heal_swin/training/optimizer.py:57-66) -- on the same parameters and gradients, and its hand-over of the bf16 parameter copies
to the model's forward (ops.ParamCastCache)."""
import copy

import pytest
import torch

from _util import GRAD_TOL, TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _toy(seed=0):
    torch.manual_seed(seed)
    shapes = [(64, 32), (64,), (7, 5, 3), (1,), (129, 33), (1000,)]  # odd sizes: bucket tails that are no multiple of 4
    return [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]


@pytest.mark.parametrize("wd,decoupled", [(0.0, False), (0.05, False), (0.05, True)])
def test_flat_adam_follows_torch_adam(wd, decoupled):
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    a, b = _toy(), _toy()
    ref_cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    ref = ref_cls(a, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd)
    dp = GradBucketAllReduce(b, bucket_bytes=16 << 10, direct_wgrad=False)  # several buckets
    try:
        opt = FlatAdam(b, dp, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, decoupled_weight_decay=decoupled)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "moving the parameters into the flat buffers must not change them"
        g = torch.Generator(device=DEV).manual_seed(1)
        for it in range(12):
            for x, y in zip(a, b):
                grad = torch.randn(x.shape, generator=g, device=DEV) * (0.1 + it)
                x.grad = grad.clone()
                y.grad.copy_(grad)      # the sink's bucket view
            ref.step()
            opt.step()
            for x, y in zip(a, b):
                err = float((x - y).abs().max()) / (float(x.abs().max()) + 1e-12)
                assert err < 2e-6, (it, tuple(x.shape), err, x.flatten()[:4].tolist(), y.flatten()[:4].tolist(),
                                    ref.state[x]["exp_avg"].flatten()[:4].tolist(), opt.state[y]["exp_avg"].flatten()[:4].tolist(),
                                    ref.state[x]["exp_avg_sq"].flatten()[:4].tolist(), opt.state[y]["exp_avg_sq"].flatten()[:4].tolist())
        for x, y in zip(a, b):  # moments in torch.optim.Adam's state layout
            # (a few ulp after 12 steps: hipcc contracts g + wd p and the moment updates into FMAs, torch's foreach kernels do not)
            assert float((ref.state[x]["exp_avg"] - opt.state[y]["exp_avg"]).abs().max()) <= 5e-6 * float(ref.state[x]["exp_avg"].abs().max())
            assert float((ref.state[x]["exp_avg_sq"] - opt.state[y]["exp_avg_sq"]).abs().max()) <= 5e-6 * float(ref.state[x]["exp_avg_sq"].abs().max())
        assert int(opt.state[b[0]]["step"]) == 12
    finally:
        dp.remove()


def test_flat_adam_state_dict_round_trip_and_tensor_lr():
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    b, c = _toy(3), _toy(3)
    dpb, dpc = GradBucketAllReduce(b, direct_wgrad=False), GradBucketAllReduce(c, direct_wgrad=False)
    try:
        lr = torch.tensor(1e-2, device=DEV)
        ob, oc = FlatAdam(b, dpb, lr=lr), FlatAdam(c, dpc, lr=1e-2)
        g = torch.Generator(device=DEV).manual_seed(2)

        def grads():
            for x, y in zip(b, c):
                gr = torch.randn(x.shape, generator=g, device=DEV)
                x.grad.copy_(gr)
                y.grad.copy_(gr)
        for _ in range(3):
            grads()
            ob.step()
            oc.step()
        assert all(torch.equal(x, y) for x, y in zip(b, c)), "tensor lr and float lr must agree"
        sd = copy.deepcopy(ob.state_dict())
        # a fresh optimizer over fresh (equal) parameters resumes from the state dict
        d = [torch.nn.Parameter(x.detach().clone()) for x in b]
        dpd = GradBucketAllReduce(d, direct_wgrad=False)
        try:
            od = FlatAdam(d, dpd, lr=1e-2)
            od.load_state_dict(sd)
            assert int(od._step) == 3
            grads()
            for x, y in zip(c, d):
                y.grad.copy_(x.grad)
            oc.step()
            od.step()
            for x, y in zip(c, d):
                assert float((x - y).abs().max()) <= 1e-6 * float(x.abs().max()), tuple(x.shape)
            assert od.state[d[0]]["exp_avg"].data_ptr() >= od._flat_m[dpd._where[d[0]]].data_ptr(), "state must stay in the flat buffer"
        finally:
            dpd.remove()
    finally:
        dpb.remove()
        dpc.remove()


def test_flat_adam_keeps_the_models_bf16_copies_current():
    """A training step with FlatAdam: the next forward must see the UPDATED weights without a copy pass (the step kernel wrote
    the bf16 shadows), equal to what torch.optim.Adam + the cast cache's own refresh give."""
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    spec = DataSpec(dim_in=12 * 32 * 32, f_in=3, f_out=12, base_pix=12, class_names=[])
    cfg = SwinHPTransformerConfig(patch_size=4, window_size=64, shift_size=32, rel_pos_bias="flat", embed_dim=64, depths=[2, 2],
                                  num_heads=[2, 4], drop_path_rate=0.0)
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
            opt = (FlatAdam(model.parameters(), dp, lr=1e-3, model=model) if kind == "flat"
                   else torch.optim.Adam(model.parameters(), lr=1e-3, fused=True))
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
                assert len(copies) <= 1, f"the cast cache ran {len(copies)} copy passes; FlatAdam should have made them unnecessary"
                cache = model.__dict__["_cast_cache"]
                assert cache.all_external
                for p, sh in zip(cache.params, cache.shadows):
                    assert torch.equal(sh, p.detach().to(torch.bfloat16))
            else:
                assert len(copies) == 4
        finally:
            dp.remove()
    assert losses["flat"][0] == losses["torch"][0]
    for a, b in zip(losses["torch"], losses["flat"]):
        assert abs(a - b) <= 2e-3 * abs(a), (losses["torch"], losses["flat"])
    assert losses["flat"][-1] < losses["flat"][0]


def test_flat_adam_in_a_captured_training_step():
    """The whole step (zero_grad, fwd, loss, bwd, finish, FlatAdam.step) in one HIP graph: replays advance the device-side step
    counter and follow the eager optimizer."""
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    torch.manual_seed(0)
    lin_a, lin_b = torch.nn.Linear(32, 16).to(DEV), torch.nn.Linear(32, 16).to(DEV)
    lin_b.load_state_dict(lin_a.state_dict())
    xs = torch.randn(8, 64, 32, device=DEV)
    dpa, dpb = GradBucketAllReduce(lin_a.parameters(), direct_wgrad=False), GradBucketAllReduce(lin_b.parameters(), direct_wgrad=False)
    try:
        oa, ob = FlatAdam(lin_a.parameters(), dpa, lr=1e-2), FlatAdam(lin_b.parameters(), dpb, lr=1e-2)
        static_x = xs[0].clone()

        def step(lin, dp, opt, inp):
            dp.zero_grad()
            loss = lin(inp).square().mean()
            loss.backward()
            dp.finish()
            opt.step()
            return loss.detach()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(lin_b, dpb, ob, static_x)
        torch.cuda.current_stream().wait_stream(side)
        step(lin_a, dpa, oa, xs[0])
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(lin_b, dpb, ob, static_x)
        step(lin_a, dpa, oa, xs[0])   # (the capture itself does not execute; this pairs with the first replay below)
        static_x.copy_(xs[0])
        graph.replay()
        for i in range(1, 6):
            step(lin_a, dpa, oa, xs[i])
            static_x.copy_(xs[i])
            graph.replay()
        torch.cuda.synchronize()
        assert int(oa._step) == int(ob._step) == 7
        for p, q in zip(lin_a.parameters(), lin_b.parameters()):
            assert float((p - q).abs().max()) <= 1e-6 * float(p.abs().max())
    finally:
        dpa.remove()
        dpb.remove()


def _heads3_run(cos, kind, x, y):
    """One model of the heads-3 shape family (embed 96, heads [3, 6], window 64: a 225 x 3 position-bias table, a 3-element logit_scale)
    trained for one step through model(x) + seg_loss (logits and gradients kept) and four more through forward_seg_loss (losses kept).
    kind: "flat" FlatAdam with its bf16 shadows handed to the model | "own" FlatAdam, the cast cache makes its own copies |
    "fp32" FlatAdam, fp32 activations | "torch" torch.optim.Adam(fused=True)."""
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.losses import seg_loss
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    spec = DataSpec(dim_in=12 * 32 * 32, f_in=3, f_out=12, base_pix=12, class_names=[])
    cfg = SwinHPTransformerConfig(patch_size=4, window_size=64, shift_size=32, rel_pos_bias="flat", embed_dim=96, depths=[2, 2],
                                  num_heads=[3, 6], drop_path_rate=0.0, use_cos_attn=cos)
    torch.manual_seed(0)
    model = SwinHPTransformerSys(cfg, spec).to(DEV).train()
    model.compute_dtype = torch.float32 if kind == "fp32" else torch.bfloat16
    dp = GradBucketAllReduce(model.parameters())
    out = {}
    try:
        if kind == "torch":
            opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
        else:
            opt = FlatAdam(model.parameters(), dp, lr=1e-3, model=model)
            if kind == "own":
                model.__dict__.pop("_shadow_provider")
            named = dict(model.named_parameters())
            out["offsets"] = {n: (dp._views[p].storage_offset(), opt._lowp_view[id(p)].data_ptr() % 16, p.data_ptr() % 16, p.dim())
                              for n, p in named.items()}
            out["gaps"] = sum(f.numel() for f in dp.buckets) - sum(p.numel() for p in dp.params)
        dp.zero_grad()
        logits = model(x)
        loss = seg_loss(logits, y)
        loss.backward()
        dp.finish()
        out["logits"] = logits.detach().float().clone()
        out["grads"] = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
        out["losses"] = [float(loss)]
        opt.step()
        for _ in range(4):
            dp.zero_grad()
            loss = model.forward_seg_loss(x, y)
            loss.backward()
            dp.finish()
            opt.step()
            out["losses"].append(float(loss))
        cache = model.__dict__.get("_cast_cache")
        out["external"] = bool(cache is not None and cache.all_external)
        if cache is not None and kind != "torch":
            for p, sh in zip(cache.params, cache.shadows):
                assert sh.data_ptr() % 16 == 0, "a bf16 weight copy the kernels read must be 16-byte aligned"
            if out["external"]:
                for p, sh in zip(cache.params, cache.shadows):
                    assert torch.equal(sh, p.detach().to(torch.bfloat16))
        for P in getattr(opt, "_flat_p", []):
            assert bool(torch.isfinite(P).all())
    finally:
        dp.remove()
    return out


@pytest.mark.parametrize("cos", [False, True])
def test_flat_adam_on_the_heads_3_layout(cos):
    """The reference's default head counts make odd-sized parameters (675-element position-bias tables, 3-element logit scales).
    Packed back to back in the gradient buckets they would put Linear weights, their bf16 copies, biases, gamma / beta and the
    direct-deposit gradient views at odd element offsets (asserted below from the parameter sizes, so that the case cannot pass
    vacuously); with the slot rule every view FlatAdam hands out is 32-byte (bf16 copies: 16-byte) aligned, the model reads
    FlatAdam's bf16 copies directly and computes what it computes on copies of its own and in fp32."""
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randint(0, 256, (2, 3, 12 * 32 * 32), generator=g, device=DEV).float()
    y = torch.randint(0, 12, (2, 12 * 32 * 32), generator=g, device=DEV, dtype=torch.uint8)
    runs = {k: _heads3_run(cos, k, x, y) for k in ("flat", "own", "fp32", "torch")}
    offs = runs["flat"]["offsets"]
    # ---- the precondition, from the layout itself: where the same parameters would sit without the slot rule (reversed order,
    # no padding: a slot offset minus the padding in front of it)
    packed, pad = {}, 0
    for n, v in sorted(offs.items(), key=lambda kv: kv[1][0]):
        packed[n] = v[0] - pad
        pad += -runs["flat"]["grads"][n].numel() % 8
    weights = [n for n, v in offs.items() if v[3] == 2 and n.endswith(".weight")]  # the Linear weights
    if not cos:
        assert any(packed[n] % 2 for n in weights), "a Linear weight at an odd element offset is what this case is about"
    else:
        assert any(packed[n] % 2 for n in offs if n.endswith("logit_scale")), "a logit_scale view at an odd element offset"
        assert any((2 * packed[n]) % 16 for n in weights), "a bf16 weight copy at a nonzero 16-byte residue"
    assert pad > 0 and runs["flat"]["gaps"] == pad, "this model has odd-sized parameters: the slot rule must have left gaps"
    assert all(v[0] % 8 == 0 and v[1] == 0 and v[2] == 0 for v in offs.values()), "every view starts on its slot"
    assert runs["flat"]["external"], "aligned shadows are taken: no copy pass"
    assert not runs["own"]["external"]
    # ---- one step: logits and every parameter gradient, shadows vs own copies vs fp32
    BF = torch.bfloat16
    tag = f"heads-3 cos={cos}"
    assert_close(runs["flat"]["logits"], runs["own"]["logits"], TOL[BF], tag + ": logits, FlatAdam's shadows vs own copies")
    assert_close(runs["flat"]["logits"], runs["fp32"]["logits"], TOL[BF], tag + ": logits, shadows vs fp32")
    assert_close(runs["own"]["logits"], runs["fp32"]["logits"], TOL[BF], tag + ": logits, own copies vs fp32")
    bad = []
    for n, ref in runs["fp32"]["grads"].items():
        for a, b, what in ((runs["flat"]["grads"][n], runs["own"]["grads"][n], "shadows vs own copies"),
                           (runs["flat"]["grads"][n], ref, "shadows vs fp32"), (runs["own"]["grads"][n], ref, "own copies vs fp32")):
            try:
                assert_close(a, b, GRAD_TOL[BF], f"{tag}: grad {n}, {what}")
            except AssertionError as e:
                bad.append(str(e))
    assert not bad, "\n".join(bad)
    # ---- five steps against torch.optim.Adam(fused=True)
    assert runs["flat"]["losses"][0] == runs["torch"]["losses"][0]
    for kind in ("flat", "own"):
        for a, b in zip(runs["torch"]["losses"], runs[kind]["losses"]):
            assert abs(a - b) <= 2e-3 * abs(a), (kind, runs["torch"]["losses"], runs[kind]["losses"])
    assert runs["flat"]["losses"][-1] < runs["flat"]["losses"][0]


def test_flat_adam_gaps_stay_zero_also_without_eps():
    """The alignment gaps of the buckets (p = g = m = v = 0) go through the Adam kernel with everything else: they stay exactly zero,
    for eps > 0 and for eps = 0 (no 0 / 0: the kernel moves nothing where the first moment is zero)."""
    from heal_swin_amd.optim import FlatAdam
    from heal_swin_amd.parallel import GradBucketAllReduce
    for eps in (1e-8, 0.0):
        a, b = _toy(5), _toy(5)
        ref = torch.optim.Adam(a, lr=3e-3, eps=eps)
        dp = GradBucketAllReduce(b, direct_wgrad=False)
        try:
            opt = FlatAdam(b, dp, lr=3e-3, eps=eps, lowp_dtype=torch.bfloat16)
            assert all(p.data_ptr() % 32 == 0 and p.grad.data_ptr() % 32 == 0 for p in b)
            gaps = []
            for i, f in enumerate(dp.buckets):
                owned = torch.zeros(f.numel(), dtype=torch.bool, device=DEV)
                for p in b:
                    if dp._where[p] == i:
                        off = dp._views[p].storage_offset()
                        owned[off:off + p.numel()] = True
                gaps.append(~owned)
            assert sum(int(g.sum()) for g in gaps) > 0
            gen = torch.Generator(device=DEV).manual_seed(1)
            for it in range(3):
                for x, y in zip(a, b):
                    grad = torch.randn(x.shape, generator=gen, device=DEV) + 0.5  # (no exact zeros: eps = 0 stays finite on real elements)
                    x.grad = grad.clone()
                    y.grad.copy_(grad)
                ref.step()
                opt.step()
                for P, M, V, G, gap in zip(opt._flat_p, opt._flat_m, opt._flat_v, dp.buckets, gaps):
                    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(M).all()) and bool(torch.isfinite(V).all())
                    assert not bool(P[gap].any()) and not bool(M[gap].any()) and not bool(V[gap].any()) and not bool(G[gap].any())
            for x, y in zip(a, b):
                assert float((x - y).abs().max()) <= 2e-6 * float(x.abs().max()), (eps, tuple(x.shape))
        finally:
            dp.remove()


def test_a_gpu_sink_cannot_be_packed():
    """On a GPU the slot is a multiple of 8 elements by construction: no caller can make a sink whose views the kernels would refuse."""
    from heal_swin_amd.parallel import GradBucketAllReduce
    with pytest.raises(ValueError, match="multiple of 8"):
        GradBucketAllReduce(_toy(), slot=1, direct_wgrad=False)
    dp = GradBucketAllReduce(_toy(), slot=16, direct_wgrad=False)
    try:
        assert all(v.data_ptr() % 64 == 0 for v in dp._views.values())
    finally:
        dp.remove()
