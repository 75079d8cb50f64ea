"""Depth-regression losses on the HIP path: the standalone kernels (`losses.depth_loss`, hs_depth_loss_*), the decoder tail with the
loss fused in (`ops.expand_ln_head_depth`, hs_expand_ln_head_depth_fwd / hs_ln_head_depth_bwd) and `forward_depth_loss` of both
models, against the torch compositions of heal_swin_amd/losses.py (the restatement of training/loss_depth_regression.py) and
the golden vectors captured from the reference."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _golden import load
from _lib_spy import launches, spy_on
from tests._util import GRAD_TOL, assert_close, assert_unbiased

pytestmark = pytest.mark.gpu

GOLDEN_CASES = [("l1", dict(loss="l1"), "depth/pred"), ("l2", dict(loss="l2"), "depth/pred"),
                ("huber_d1", dict(loss="huber", huber_delta=1.0), "depth/pred"),
                ("huber_d0p3", dict(loss="huber", huber_delta=0.3), "depth/pred"),
                ("logvar", dict(loss="l1", use_logvar=True), "depth/logvar/pred")]


def _composition(kw):
    from heal_swin_amd import losses as L
    return L.get_depth_loss(NS(use_logvar=kw.get("use_logvar", False), loss=kw["loss"], huber_delta=kw.get("huber_delta", 1.0)))


def _padded_view(pred, dtype):
    """pred [B, C, P] as the model's head rows: [B, P, 16] with C used columns, seen as [B, C, P]"""
    B, C, P = pred.shape
    rows = torch.zeros(B, P, 16, dtype=dtype, device=pred.device)
    rows[:, :, :C] = pred.transpose(1, 2).to(dtype)
    return rows, rows[:, :, :C].transpose(1, 2)


@pytest.mark.parametrize("layout", ["dense", "rows16"])
@pytest.mark.parametrize("tag,kw,pkey", GOLDEN_CASES)
def test_depth_loss_matches_the_golden_vectors(tag, kw, pkey, layout):
    from heal_swin_amd.losses import depth_loss
    z = load("losses")
    tgt = torch.from_numpy(z["depth/target"]).cuda()
    p = torch.from_numpy(z[pkey]).cuda()
    if layout == "dense":
        leaf = p.clone().requires_grad_(True)
        pred = leaf
    else:
        rows, _ = _padded_view(p, torch.float32)
        leaf = rows.requires_grad_(True)
        pred = leaf[:, :, :p.shape[1]].transpose(1, 2)
    loss = depth_loss(pred, tgt, **kw)
    assert abs(float(loss) - float(z[f"depth/{tag}/loss"])) < 1e-6, (tag, float(loss), float(z[f"depth/{tag}/loss"]))
    loss.backward()
    g = leaf.grad if layout == "dense" else leaf.grad[:, :, :p.shape[1]].transpose(1, 2)
    assert np.abs(g.cpu().numpy() - z[f"depth/{tag}/dpred"]).max() < 2.5e-7, tag
    if layout == "rows16":
        assert not leaf.grad[:, :, p.shape[1]:].any()  # the padding columns stay zero


@pytest.mark.parametrize("layout", ["dense", "rows16"])
@pytest.mark.parametrize("tag,kw,pkey", GOLDEN_CASES)
def test_depth_loss_bf16_prediction_equals_the_composition(tag, kw, pkey, layout):
    """bf16 predictions are read as they are (fp32 arithmetic); the loss equals the composition's on the same rounded values and
    the gradient is the composition's, rounded to bf16."""
    from heal_swin_amd.losses import depth_loss
    z = load("losses")
    tgt = torch.from_numpy(z["depth/target"]).cuda()
    p16 = torch.from_numpy(z[pkey]).cuda().to(torch.bfloat16)
    ref_leaf = p16.clone().requires_grad_(True)
    ref = _composition(kw)(ref_leaf, tgt)
    ref.backward()
    if layout == "dense":
        leaf = p16.clone().requires_grad_(True)
        pred = leaf
    else:
        rows, _ = _padded_view(p16, torch.bfloat16)
        leaf = rows.requires_grad_(True)
        pred = leaf[:, :, :p16.shape[1]].transpose(1, 2)
    loss = depth_loss(pred, tgt, **kw)
    assert abs(float(loss) - float(ref)) <= 1e-6 * max(1.0, abs(float(ref))), (float(loss), float(ref))
    loss.backward()
    g = leaf.grad if layout == "dense" else leaf.grad[:, :, :p16.shape[1]].transpose(1, 2)
    assert g.dtype == torch.bfloat16
    torch.testing.assert_close(g.float(), ref_leaf.grad.float(), rtol=8e-3, atol=1e-9)


def _edge_target(B, P, g):
    t = torch.randn(B, P, generator=g, device="cuda") * 2
    t[0, ::7] = float("inf")
    t[1, 3::11] = -float("inf")
    t[0, 5] = float("nan")
    t[1, 100] = float("nan")
    return t


@pytest.mark.parametrize("kind", ["l1", "l2", "huber", "logvar"])
def test_depth_loss_edge_cases_equal_the_composition(kind):
    """NaN and +-inf targets, P not a multiple of the 256-thread block, huge log variances at the masked pixels (finite gradients
    there: exactly 0), an all-infinite target (NaN loss, as losses.py's 0 / 0), and two calls bit-identical."""
    from heal_swin_amd.losses import depth_loss
    g = torch.Generator(device="cuda").manual_seed(3)
    B, P = 2, 1000 + 7
    C = 2 if kind == "logvar" else 1
    kw = dict(loss="l1" if kind == "logvar" else kind, use_logvar=kind == "logvar", huber_delta=0.7)
    t = _edge_target(B, P, g)
    p = torch.randn(B, C, P, generator=g, device="cuda")
    if kind == "logvar":
        p[:, 1][torch.isinf(t)] = -1e4  # exp(-log_var) overflows at the masked pixels
    res = []
    for _ in range(2):
        leaf = p.clone().requires_grad_(True)
        loss = depth_loss(leaf, t, **kw)
        loss.backward()
        res.append((loss.detach(), leaf.grad))
    assert torch.equal(res[0][0], res[1][0]) or (res[0][0].isnan() and res[1][0].isnan())
    assert torch.equal(res[0][1].nan_to_num(7.0), res[1][1].nan_to_num(7.0))  # bit-identical (NaN positions included)
    ref_leaf = p.clone().requires_grad_(True)
    ref = _composition(kw)(ref_leaf, t)
    ref.backward()
    assert float(ref) != float(ref) and float(res[0][0]) != float(res[0][0])  # NaN targets propagate into the loss
    torch.testing.assert_close(res[0][1], ref_leaf.grad, rtol=4e-6, atol=1e-9, equal_nan=True)
    masked = torch.isinf(t)
    assert (res[0][1][:, 0][masked] == 0).all() and (res[0][1][:, -1][masked] == 0).all()
    # without the NaN targets the loss is finite and equals the composition
    t2 = t.nan_to_num(nan=0.5, posinf=float("inf"), neginf=-float("inf"))
    a, b = depth_loss(p, t2, **kw), _composition(kw)(p, t2)
    assert abs(float(a) - float(b)) <= 2e-6 * max(1.0, abs(float(b))), (float(a), float(b))
    # all targets infinite: 0 / 0
    tinf = torch.full((B, P), float("inf"), device="cuda")
    leaf = p.clone().requires_grad_(True)
    l_inf = depth_loss(leaf, tinf, **kw)
    assert float(l_inf) != float(l_inf) and float(_composition(kw)(p, tinf)) != float(_composition(kw)(p, tinf))
    l_inf.backward()
    assert not leaf.grad.any()


def test_depth_loss_argument_errors_on_the_gpu():
    from heal_swin_amd.losses import depth_loss
    p2 = torch.randn(1, 2, 64, device="cuda")
    t = torch.randn(1, 64, device="cuda")
    with pytest.raises(AssertionError, match="one-channel"):
        depth_loss(p2, t, loss="huber")
    with pytest.raises(AssertionError, match="two channels"):
        depth_loss(p2[:, :1], t, use_logvar=True)
    # a two-channel prediction with l1 / l2 reads channel 0 only: channel 1's gradient is exactly 0
    leaf = p2.clone().requires_grad_(True)
    depth_loss(leaf, t, loss="l2", mask_background=True).backward()
    assert not leaf.grad[:, 1].any() and leaf.grad[:, 0].any()


# ------------------------------------------------------------------ the decoder tail with the loss fused in
def _reference_tail_depth(xn, wexp, gamma, beta, w, target, kw, P=4):
    """fp32 composition of FinalPatchExpand_X4 + head + the losses.py depth loss, on bf16-exact inputs."""
    xn = xn.float().detach().requires_grad_(True)
    wexp, gamma, beta, w = (t.detach().clone().requires_grad_(True) for t in (wexp, gamma, beta, w))
    C = xn.shape[-1]
    yv = F.linear(xn, wexp).reshape(-1, C)
    pred = F.linear(F.layer_norm(yv, (C,), gamma, beta, 1e-5), w)  # [rows, f_out]
    loss = _composition(kw)(pred.t().unsqueeze(0), target.reshape(1, -1))
    loss.backward()
    return loss.detach(), xn.grad, wexp.grad, gamma.grad, beta.grad, w.grad


TAIL_CASES = [(4096, 128, 1, "l1"), (1000, 96, 1, "l2"), (33, 64, 1, "huber"), (5000, 128, 2, "logvar"), (2000, 64, 2, "l1"),
              (3000, 96, 2, "logvar"), (7000, 64, 1, "l2"), (1500, 128, 2, "l2")]


@pytest.mark.parametrize("tokens,C,f_out,kind", TAIL_CASES)
def test_expand_ln_head_depth_matches_the_composition(tokens, C, f_out, kind):
    """`hs_expand_ln_head_depth_fwd` + `hs_ln_head_depth_bwd` against the fp32 composition of the reference modules + the depth
    loss: the loss to 1e-3 (the kernel keeps fp32 from the expand product to the loss), every gradient to the bf16 bound the CE
    tail is held to, plus the slope check."""
    from heal_swin_amd import ops
    from heal_swin_amd.losses import depth_loss_spec

    torch.manual_seed(tokens + C + f_out)
    dev = "cuda"
    kw = dict(loss="l1" if kind == "logvar" else kind, use_logvar=kind == "logvar", huber_delta=0.5)
    xn = (torch.randn(tokens, C, device=dev) * 1.3 + 0.2).to(torch.bfloat16)
    wexp = (torch.randn(4 * C, C, device=dev) * C ** -0.5).to(torch.bfloat16).float().requires_grad_(True)
    gamma = (1 + 0.3 * torch.randn(C, device=dev)).requires_grad_(True)
    beta = (0.2 * torch.randn(C, device=dev)).requires_grad_(True)
    w = (torch.randn(f_out, C, 1, device=dev) * 2.0 * C ** -0.5).requires_grad_(True)
    with torch.no_grad():  # residuals kept away from 0: at |d| ~ 1e-3 the L1 gradient's sign is decided by the bf16 roundings
        pred0 = F.linear(F.layer_norm(F.linear(xn.float(), wexp).reshape(-1, C), (C,), gamma, beta, 1e-5), w.reshape(f_out, C))[:, 0]
        u = torch.rand(4 * tokens, device=dev)
        target = pred0 + torch.where(u < 0.5, -1.0, 1.0) * (0.2 + 2 * u)
    target[::13] = float("inf")
    k, delta = depth_loss_spec(**kw)
    assert ops.expand_ln_head_depth_ok(xn, C, 4, f_out, k, delta)
    xq = xn.clone().requires_grad_(True)
    loss = ops.expand_ln_head_depth(xq, wexp, gamma, beta, w, target, k, delta)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * 3.0).backward()
    ref_loss, ref_dx, ref_dwe, ref_dg, ref_db, ref_dw = _reference_tail_depth(xn, wexp, gamma, beta, w.reshape(f_out, C), target, kw)
    tag = f"expand_ln_head_depth[{tokens}x{C}->{f_out} {kind}]"
    assert abs(float(loss) - float(ref_loss)) <= 1e-3 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    for got, ref, name in ((xq.grad, ref_dx, "dxn"), (wexp.grad, ref_dwe, "dWexpand"), (gamma.grad, ref_dg, "dgamma"),
                           (beta.grad, ref_db, "dbeta"), (w.grad.reshape(f_out, C), ref_dw, "dWhead")):
        assert_close(got, 3.0 * ref, GRAD_TOL[torch.bfloat16], f"{tag} {name}")
        assert_unbiased(got, 3.0 * ref, f"{tag} {name}")


def test_expand_ln_head_depth_equals_the_tail_plus_the_standalone_kernels():
    """The fused pair against expand_ln_head (the same forward kernel writing its fp32 rows) + losses.depth_loss on those rows:
    the same head outputs enter the same per-row term, so the loss agrees to fp32 summation order and the gradients to the bf16
    rounding of the row gradient the unfused backward reads."""
    from heal_swin_amd import ops
    from heal_swin_amd.losses import depth_loss
    torch.manual_seed(11)
    tokens, C, f_out = 3000, 96, 2
    xn = (torch.randn(tokens, C, device="cuda") * 1.3).to(torch.bfloat16)
    params = [(torch.randn(4 * C, C, device="cuda") * C ** -0.5).to(torch.bfloat16).float(), 1 + 0.3 * torch.randn(C, device="cuda"),
              0.2 * torch.randn(C, device="cuda"), torch.randn(f_out, C, 1, device="cuda") * C ** -0.5]
    target = torch.randn(4 * tokens, device="cuda")
    target[::5] = -float("inf")
    res = []
    for fused in (True, False):
        ps = [p.clone().requires_grad_(True) for p in params]
        xq = xn.clone().requires_grad_(True)
        if fused:
            loss = ops.expand_ln_head_depth(xq, *ps, target, 3)
        else:
            rows = ops.pad_slice(ops.expand_ln_head(xq, *ps).view(1, 4 * tokens, -1), f_out)
            loss = depth_loss(rows.transpose(1, 2), target.view(1, -1), use_logvar=True)
        loss.backward()
        res.append((float(loss), [xq.grad] + [p.grad for p in ps]))
    assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[1][0]), (res[0][0], res[1][0])
    for a, b, n in zip(res[0][1], res[1][1], ("dxn", "dWexpand", "dgamma", "dbeta", "dWhead")):
        assert_close(a, b, 1e-2, f"fused vs rows + depth_loss {n}")


# ------------------------------------------------------------------ whole models
MODEL_KINDS = [dict(loss="l1"), dict(loss="l2"), dict(loss="huber", huber_delta=0.5), dict(loss="l2", use_logvar=True)]


def _hp_model(f_out):
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys
    cfg = dict(patch_size=4, window_size=64, shift_size=32, shift_strategy="nest_roll", rel_pos_bias="flat", embed_dim=96,
               depths=[2, 2], num_heads=[3, 6], mlp_ratio=4.0, qkv_bias=True, qk_scale=None, use_cos_attn=False, drop_rate=0.0,
               attn_drop_rate=0.0, drop_path_rate=0.0, use_v2_norm_placement=False, ape=False)
    spec = dict(dim_in=8 * 32 * 32, f_in=3, f_out=f_out, base_pix=8, class_names=[])
    torch.manual_seed(0)
    m = SwinHPTransformerSys(SwinHPTransformerConfig(**cfg), DataSpec(**spec)).cuda().train()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("relative_position_bias_table"):
                p.normal_(0, 0.3)
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randint(0, 256, (2, 3, spec["dim_in"]), generator=g, device="cuda", dtype=torch.uint8).float()
    t = torch.randn(2, spec["dim_in"], generator=g, device="cuda")
    t[:, ::9] = float("inf")
    return m, x, t


def _flat_model(f_out):
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_transformer import SwinTransformerConfig, SwinTransformerSys
    cfg = dict(patch_size=2, window_size=8, shift_size=2, embed_dim=64, depths=[2, 2], num_heads=[2, 4], drop_rate=0.0,
               attn_drop_rate=0.0, drop_path_rate=0.0)
    spec = dict(dim_in=(64, 96), f_in=3, f_out=f_out, base_pix=None, class_names=[])
    torch.manual_seed(0)
    m = SwinTransformerSys(SwinTransformerConfig(**cfg), DataSpec(**spec)).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randint(0, 256, (2, 3, 64, 96), generator=g, device="cuda", dtype=torch.uint8).float()
    t = torch.randn(2, 64, 96, generator=g, device="cuda")
    t[:, ::5, ::3] = float("inf")
    return m, x, t


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("which", ["healpix", "flat"])
def test_forward_depth_loss_equals_model_plus_the_composition(which, dtype):
    """model.forward_depth_loss(x, target, ...) against get_depth_loss(cfg)(model(x), target) on the same weights, for every kind:
    the loss and every parameter gradient (element bound and slope)."""
    tol_loss, tol_grad = (2e-4, 5e-2) if dtype == torch.bfloat16 else (1e-5, 1e-3)
    for kw in MODEL_KINDS:
        f_out = 2 if kw.get("use_logvar") else 1
        m, x, t = (_hp_model if which == "healpix" else _flat_model)(f_out)
        m.compute_dtype = dtype
        cfg = NS(use_logvar=kw.get("use_logvar", False), loss=kw["loss"], huber_delta=kw.get("huber_delta", 1.0))
        res = {}
        for fused in (True, False):
            m.zero_grad(set_to_none=True)
            loss = m.forward_depth_loss(x, t, cfg) if fused else _composition(kw)(m(x), t)
            loss.backward()
            res[fused] = (float(loss), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
        tag = f"{which} {dtype} {kw}"
        assert abs(res[True][0] - res[False][0]) <= tol_loss * abs(res[False][0]), (tag, res[True][0], res[False][0])
        assert set(res[True][1]) == set(res[False][1])
        for n, gr in res[False][1].items():
            tol = 1.6 * tol_grad if n.endswith(("relative_position_bias_table", "logit_scale")) else tol_grad
            assert_close(res[True][1][n], gr, tol, f"forward_depth_loss {tag} grad {n}")
            assert_unbiased(res[True][1][n], gr, f"forward_depth_loss {tag} grad {n}")
        with torch.no_grad():  # the no-grad call takes the standalone kernels on the rows
            l2 = m.forward_depth_loss(x, t, cfg)
        assert abs(float(l2) - res[False][0]) <= tol_loss * abs(res[False][0]), (tag, float(l2), res[False][0])


def test_flat_depth_target_keeps_inf_and_nan():
    from heal_swin_amd import ops
    t = torch.randn(2, 64, 96, device="cuda")
    t[0, 3, 5], t[1, 63, 95], t[0, 0, 0], t[1, 10, 20] = float("inf"), -float("inf"), float("nan"), float("nan")
    rows = ops.flat_depth_target(t, 2, 16)
    assert rows.shape == (2, 64 * 96) and rows.dtype == torch.float32
    for b in range(2):
        a, r = torch.sort(rows[b].nan_to_num(nan=1e30))[0], torch.sort(t[b].flatten().nan_to_num(nan=1e30))[0]
        assert torch.equal(a, r)  # a permutation of the image, values unchanged
    assert int(torch.isposinf(rows).sum()) == 1 and int(torch.isneginf(rows).sum()) == 1 and int(rows.isnan().sum()) == 2


# ------------------------------------------------------------------ launch census and graph replay
@pytest.mark.parametrize("which", ["healpix", "flat"])
def test_bf16_depth_step_runs_the_fused_tail_only(which, monkeypatch):
    """In a bf16 training step with forward_depth_loss the fused depth tail kernels run; neither the head-rows forward
    (hs_expand_ln_head_fwd) nor the standalone loss kernels do."""
    from heal_swin_amd import _lib
    m, x, t = (_hp_model if which == "healpix" else _flat_model)(1)
    m.compute_dtype = torch.bfloat16
    import heal_swin_amd.ops.tail as T
    called = spy_on(monkeypatch, ("hs_expand_ln_head", "hs_ln_head", "hs_depth_loss"), (T, _lib))
    loss = m.forward_depth_loss(x, t, "l1")
    loss.backward()
    torch.cuda.synchronize()
    assert "hs_expand_ln_head_depth_fwd" in called and "hs_ln_head_depth_bwd" in called, called
    assert "hs_expand_ln_head_fwd" not in called and not any(c.startswith("hs_depth_loss") for c in called), called
    # without a gradient: the rows-writing tail once, then the standalone loss kernel on the rows
    del called[:]
    with torch.no_grad():
        m.forward_depth_loss(x, t, "l1")
    torch.cuda.synchronize()
    assert launches(called) == ["hs_depth_loss_fwd", "hs_expand_ln_head_fwd"], called


def test_bf16_depth_step_of_three_channels_takes_the_rows_route(monkeypatch):
    """A three-channel head is outside ops.expand_ln_head_depth_ok: a bf16 training step with forward_depth_loss writes the head
    rows (hs_expand_ln_head_fwd) and takes the standalone loss kernels on them, forward and backward; no fused depth tail."""
    from heal_swin_amd import _lib
    import heal_swin_amd.ops.tail as T
    m, x, t = _hp_model(3)
    m.compute_dtype = torch.bfloat16
    called = spy_on(monkeypatch, ("hs_expand_ln_head", "hs_ln_head", "hs_depth_loss"), (T, _lib))
    m.forward_depth_loss(x, t, "l2").backward()
    torch.cuda.synchronize()
    assert launches(called) == ["hs_depth_loss_bwd", "hs_depth_loss_fwd", "hs_expand_ln_head_fwd", "hs_ln_head_bwd"], called


def test_graph_replay_of_a_depth_step_equals_the_eager_step():
    """forward_depth_loss + backward captured in one graph (torch.cuda.graph): the replay gives the eager step's loss and
    gradients bit for bit."""
    m, x, t = _hp_model(2)
    m.compute_dtype = torch.bfloat16
    params = [p for p in m.parameters() if p.requires_grad]

    def step():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        loss = m.forward_depth_loss(x, t, "l2", use_logvar=True)
        loss.backward()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager_loss = step().clone()
    eager = [p.grad.clone() for p in params]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = step()
    for p in params:
        if p.grad is not None:
            p.grad.fill_(123.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_loss, eager_loss), (float(static_loss), float(eager_loss))
    for p, g in zip(params, eager):
        assert torch.equal(p.grad, g)
