"""The depth caller's `shared_step` on the decoder tail (`ops.expand_ln_head_depth_step`, hs_expand_ln_head_depth_step_fwd) and
`forward_depth_step` of both models: the loss and the gradients are those of the loss-only tail BIT FOR BIT, the predictions are
`unnormalize_and_retransform` of the written head rows bit for bit, and the metric state is DepthMetrics.update's on them: counts
exact, every other sum within the float64 reordering bound rows * 2^-52 * sum |terms| (two orders of the same float64 terms, each
within (rows - 1) 2^-53 sum |terms| of the exact sum)."""
import math
import os

import numpy as np
import pytest
import torch

from _lib_spy import spy_on

pytestmark = pytest.mark.gpu

DEV = "cuda"
KINDS = {"l1": 0, "l2": 1, "huber": 2, "logvar": 3}
S_N, S_SE, S_AE, S_MEAN_SE, S_MEAN_AE, S_PRED, S_SIL_N, S_SIL_D, S_SIL_D2, S_INV_N, S_INV_SE, S_STD_N, S_STD, S_RANGE = range(14)
RANGES = [(0.0, 2.0), (5,), (2.0, 30.0)]


_INT = {4: torch.int32, 2: torch.int16, 8: torch.int64}


def _same_bits(a, b):
    """Same dtype, shape and bits (a NaN equals the same NaN: the loss of a target with NaNs is NaN)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(_INT[a.element_size()]),
                                                                     b.contiguous().view(_INT[b.element_size()]))


def _same_bits_nan(a, b):
    return _same_bits(a, b)


def _inputs(tokens, C, f_out):
    torch.manual_seed(tokens + C + f_out)
    xn = (torch.randn(tokens, C, device=DEV) * 1.3 + 0.2).to(torch.bfloat16)
    wexp = (torch.randn(4 * C, C, device=DEV) * C ** -0.5).to(torch.bfloat16).float().requires_grad_(True)
    gamma = (1 + 0.3 * torch.randn(C, device=DEV)).requires_grad_(True)
    w = (torch.randn(f_out, C, 1, device=DEV) * 0.2 * C ** -0.5).requires_grad_(True)
    # channel 0 around 0.5 in the normalised space (beta along the head's row 0 adds 0.5 to it): inside every transform's domain
    # for most rows, outside ('inv': below 1e-3 after the affine step -> inf metres) for some
    w0 = w.detach()[0, :, 0]
    beta = (0.05 * torch.randn(C, device=DEV) + 0.5 * w0 / (w0 * w0).sum()).requires_grad_(True)
    return xn, [wexp, gamma, beta, w]


def _transform(name):
    from heal_swin_amd.depth_data import DepthTargetTransform
    return DepthTargetTransform(*name)


def _target(rows, tr, seed, nans=True):
    """transform.prepare of positive depths with about 4 % zeros (background) and a few NaNs, fp32 [rows]."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    depth = 0.3 + 40.0 * torch.rand(rows, generator=g, device=DEV) ** 2
    depth[torch.rand(rows, generator=g, device=DEV) < 0.04] = 0.0
    if nans:
        depth[torch.randint(0, rows, (5,), generator=g, device=DEV)] = float("nan")
    return tr.prepare(depth[None])[0].contiguous()


def _written(xn, params, f_out, tr):
    """(preds [f_out, rows] from the rows written by ops.expand_ln_head, channel 0 through unnormalize_and_retransform)."""
    from heal_swin_amd import ops
    with torch.no_grad():
        rows = ops.expand_ln_head(xn, *params)[:, :f_out].t().contiguous()
        rows[0] = tr.unnormalize_and_retransform(rows[0][None])[0]
    return rows


def _abs_sums(preds, metres, m):
    """sum |term| of every sum of the state, in float64 with torch, under accumulate's selections (csrc/hs_depth_metrics.h)."""
    p, t = preds[0], metres
    out = torch.zeros(29, dtype=torch.float64, device=p.device)
    fin = torch.isfinite(p) & torch.isfinite(t)
    pd, td = p.double(), t.double()
    d = torch.where(fin, pd - td, 0.0)
    dm = torch.where(fin, (m.total_mean or 0.0) - td, 0.0)
    out[S_N], out[S_SE], out[S_AE] = fin.sum(), (d * d).sum(), d.abs().sum()
    out[S_MEAN_SE], out[S_MEAN_AE], out[S_PRED] = (dm * dm).sum(), dm.abs().sum(), torch.where(fin, pd, 0.0).abs().sum()
    sil = fin & (p > 0) & (t > 0)
    dl = torch.where(sil, torch.log(t).double() - torch.log(p).double(), 0.0)
    out[S_SIL_N], out[S_SIL_D], out[S_SIL_D2] = sil.sum(), dl.abs().sum(), (dl * dl).sum()
    ip, it = 1.0 / (0.001 * p), 1.0 / (0.001 * t)
    inv = torch.isfinite(ip) & torch.isfinite(it)
    di = torch.where(inv, ip.double() - it.double(), 0.0)
    out[S_INV_N], out[S_INV_SE] = inv.sum(), (di * di).sum()
    if m.use_logvar:
        std = ~torch.isnan(t) & (t != float("inf"))
        out[S_STD_N], out[S_STD] = std.sum(), torch.where(std, torch.sqrt(torch.exp(preds[1])).double(), 0.0).abs().sum()
    for r in range(len(m.distance_ranges)):
        lo, hi = float(m._ranges[2 * r]), float(m._ranges[2 * r + 1])
        sel = fin & (t >= lo) & (t < hi)
        out[S_RANGE + 2 * r], out[S_RANGE + 2 * r + 1] = sel.sum(), torch.where(sel, d * d, 0.0).sum()
    return out


COUNTS = [S_N, S_SIL_N, S_INV_N, S_STD_N] + [S_RANGE + 2 * r for r in range(8)]


def _check_state(got, ref, preds, metres, m, tag):
    """Counts exact; every other sum within rows * 2^-52 * sum |terms| (NaN / inf sums: the same NaN / inf)."""
    got, ref = got.detach().clone(), ref.detach().clone()
    bound = _abs_sums(preds, metres, m) * (metres.numel() * 2.0 ** -52)
    print(tag, "state", got.tolist(), "reference", ref.tolist(), "bound", bound.tolist())
    assert torch.equal(got[COUNTS], ref[COUNTS]), (tag, got[COUNTS].tolist(), ref[COUNTS].tolist())
    assert torch.equal(got[COUNTS], _abs_sums(preds, metres, m)[COUNTS]), tag  # (the torch restatement selects the same pairs)
    same = (got == ref) | (got.isnan() & ref.isnan())
    ok = same | ((got - ref).abs() <= bound)
    assert bool(ok.all()), (tag, [(k, got[k].item(), ref[k].item(), bound[k].item()) for k in range(29) if not ok[k]])


def _metrics(use_logvar, ranges, total_mean=11.5):
    from heal_swin_amd.depth_evaluation import DepthMetrics
    return DepthMetrics(total_mean=total_mean, distance_ranges=RANGES if ranges else (), use_logvar=use_logvar)


# (tokens, C): a partial 32-token group, every width, and more groups than resident waves (70000 tokens = 2188 groups on <= 1024
# waves: the persistent loop and the lane sums run more than one step)
SHAPES = [(33, 64), (1000, 96), (4096, 128), (70000, 128)]
TRANSFORMS = [(None, None), ("log", "standardize"), ("inv", "min-max")]
# (loss, f_out, transform, use_logvar, ranges): every loss on the heads it accepts, every transform, the log variance on and off,
# 0 and 3 distance ranges; all at every shape
COMBOS = [("l1", 1, 0, False, True), ("l2", 1, 1, False, False), ("huber", 1, 2, False, True),
          ("l1", 2, 1, True, True), ("logvar", 2, 2, True, False), ("logvar", 2, 0, False, True)]


@pytest.mark.parametrize("tokens,C", SHAPES)
@pytest.mark.parametrize("loss,f_out,ti,use_logvar,ranges", COMBOS)
def test_step_equals_the_loss_only_tail_and_the_written_rows(tokens, C, loss, f_out, ti, use_logvar, ranges):
    from heal_swin_amd import ops
    xn, params = _inputs(tokens, C, f_out)
    tr = _transform(TRANSFORMS[ti])
    tr_arg = None if ti == 0 else tr  # None is the identity
    rows = 4 * tokens
    target = _target(rows, tr, tokens + ti)
    kind, delta = KINDS[loss], 0.7
    want = _written(xn, params, f_out, tr)
    metres = tr.unnormalize_and_retransform(target[None])[0]
    ref = _metrics(use_logvar, ranges)
    ref.update(want[None], metres[None])
    # the loss and the five gradients, on the target as it is (its NaNs make the loss NaN) and with the NaNs replaced
    for tgt in (torch.where(target.isnan(), 0.25, target), target):
        res = []
        for step in (False, True):
            xq = xn.clone().requires_grad_(True)
            for p in params:
                p.grad = None
            if step:
                m = _metrics(use_logvar, ranges)
                lss, preds = ops.expand_ln_head_depth_step(xq, *params, tgt, kind, delta, None, tr_arg, m)
                assert not preds.requires_grad and preds.dtype == torch.float32 and preds.shape == (f_out, rows)
            else:
                lss = ops.expand_ln_head_depth(xq, *params, tgt, kind, delta)
            (lss * 3.0).backward()
            res.append((lss.detach(), [xq.grad] + [p.grad for p in params]))
        assert _same_bits(res[0][0], res[1][0]), (float(res[0][0]), float(res[1][0]))
        for a, b, n in zip(res[0][1], res[1][1], ("dxn", "dWexpand", "dgamma", "dbeta", "dWhead")):
            assert _same_bits(a, b), n
        assert bool(torch.isfinite(res[1][0])) == (tgt is not target)
    assert _same_bits_nan(preds[0], want[0]), int((preds[0].view(torch.int32) != want[0].view(torch.int32)).sum())
    if f_out == 2:
        assert _same_bits_nan(preds[1], want[1])
    tag = f"{tokens}x{C} {loss} f_out={f_out} {TRANSFORMS[ti]}"
    _check_state(m.state, ref.state, want, metres, ref, tag)
    assert torch.equal(m.median, ref.median)
    # the no-grad (validation) form: the same loss bits, predictions and state; two identical calls give identical states
    with torch.no_grad():
        m2 = _metrics(use_logvar, ranges)
        loss2, preds2 = ops.expand_ln_head_depth_step(xn, *params, target, kind, delta, None, tr_arg, m2)
    assert _same_bits(loss2, res[0][0]) and _same_bits_nan(preds2, preds)
    assert torch.equal(m2.state.view(torch.int64), m.state.view(torch.int64))
    # a second call on the same DepthMetrics doubles the counts; each output is optional
    with torch.no_grad():
        loss3, none = ops.expand_ln_head_depth_step(xn, *params, target, kind, delta, None, tr_arg, m2, want_preds=False)
        loss4, preds4 = ops.expand_ln_head_depth_step(xn, *params, target, kind, delta, None, tr_arg, None)
        loss5, none5 = ops.expand_ln_head_depth_step(xn, *params, target, kind, delta, None, tr_arg, None, want_preds=False)
    assert none is None and none5 is None and _same_bits_nan(preds4, preds)
    assert _same_bits(loss3, loss2) and _same_bits(loss4, loss2) and _same_bits(loss5, loss2)
    assert torch.equal(m2.state[COUNTS], 2 * m.state[COUNTS]) and torch.equal(m2.median, 2 * m.median)
    assert torch.equal(m2.state, m.state + m.state)  # (x + x is exact)


def test_non_finite_rows_targets_and_predictions_outside_the_domain():
    """Ordinary non-finite values: NaN / inf input tokens, +inf and NaN targets, and 'inv' predictions below 1e-3 metres (a wide
    min-max table): the state is DepthMetrics.update's, which pins accumulate's selections (iRMSE counts a +inf target, ...)."""
    from heal_swin_amd import ops
    from heal_swin_amd.depth_data import DataStats, DepthTargetTransform
    tokens, C, f_out = 2048, 96, 2
    xn, params = _inputs(tokens, C, f_out)
    with torch.no_grad():
        xn[17] = float("nan")
        xn[100, 3] = float("nan")
        xn[1999, ::2] = float("inf")
    tr = DepthTargetTransform("inv", "min-max", data_stats=DataStats("wide", max=5000.001, min=0.001, mean=1.0, std=1.0))
    target = _target(4 * tokens, tr, 3)
    target[5:9] = float("inf")
    target[40:44] = float("nan")
    target[900] = -float("inf")
    want = _written(xn, params, f_out, tr)
    small = (want[0] < 1e-3) & (want[0] > 0)
    assert int(small.sum()) > 100 and int(want[0].isnan().sum()) >= 12 and int(torch.isinf(want[0]).sum()) > 0
    metres = tr.unnormalize_and_retransform(target[None])[0]
    ref, m = _metrics(True, True), _metrics(True, True)
    ref.update(want[None], metres[None])
    with torch.no_grad():
        loss, preds = ops.expand_ln_head_depth_step(xn, *params, target, KINDS["logvar"], 1.0, None, tr, m)
        ref_loss = ops.expand_ln_head_depth(xn, *params, target, KINDS["logvar"], 1.0)
    assert _same_bits_nan(loss.reshape(1), ref_loss.reshape(1)) and _same_bits_nan(preds, want)
    _check_state(m.state, ref.state, want, metres, ref, "edge values")
    assert int(m.state[S_INV_N]) > int(m.state[S_N])  # +inf targets (0 after 1 / (0.001 t)) count for iRMSE, not for the MSE


# ------------------------------------------------------------------ whole models
def _hp_model(f_out):
    import bench
    model, cfg, spec = bench.build_model(dict(bench.WORKLOADS["D256"], f_out=f_out), nside=64)
    model = model.cuda().eval()
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randint(0, 256, (2, 3, spec["dim_in"]), generator=g, device=DEV, dtype=torch.uint8).float()
    return model, x, (2, spec["dim_in"])


def _flat_model(f_out):
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_transformer import SwinTransformerConfig, SwinTransformerSys
    cfg = dict(patch_size=2, window_size=8, shift_size=2, embed_dim=64, depths=[2, 2], num_heads=[2, 4], drop_rate=0.0,
               attn_drop_rate=0.0, drop_path_rate=0.0)
    spec = dict(dim_in=(64, 96), f_in=3, f_out=f_out, base_pix=None, class_names=[])
    torch.manual_seed(0)
    m = SwinTransformerSys(SwinTransformerConfig(**cfg), DataSpec(**spec)).cuda().eval()
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randint(0, 256, (2, 3, 64, 96), generator=g, device=DEV, dtype=torch.uint8).float()
    return m, x, (2, 64, 96)


def _model_case(which, f_out):
    model, x, shape = (_hp_model if which == "healpix" else _flat_model)(f_out)
    tr = _transform(("log", "standardize"))
    n = int(np.prod(shape))
    target = _target(n, tr, 11, nans=False).view(shape)  # (a finite loss: the gradients are compared)
    kw = dict(loss="l2", use_logvar=True) if f_out == 2 else dict(loss="l1")
    return model, x, target, tr, kw


def _reference_route(model, x, target, tr, use_logvar):
    """model(x) -> unnormalize_and_retransform -> DepthMetrics.update: (preds with channel 0 in metres, target in metres, metrics)."""
    out = model(x).detach().clone()
    B = out.shape[0]
    tr.unnormalize_and_retransform(out[:, 0].reshape(B, -1), out=out[:, 0].reshape(B, -1))
    metres = tr.unnormalize_and_retransform(target.reshape(B, -1)).view(target.shape)
    ref = _metrics(use_logvar, True)
    ref.update(out, metres)
    return out, metres, ref


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("f_out", [1, 2])
@pytest.mark.parametrize("which", ["healpix", "flat"])
def test_forward_depth_step_equals_the_reference_route_bf16(which, f_out, monkeypatch):
    from heal_swin_amd import _lib
    model, x, target, tr, kw = _model_case(which, f_out)
    use_logvar = f_out == 2
    model.compute_dtype = torch.bfloat16
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            # one warm-up call of each route: the per-shape GEMM choice is settled
            model.forward_depth_step(x, target, transform=tr, metrics=_metrics(use_logvar, True), **kw)
            model(x)
            if grad:
                model.forward_depth_loss(x, target, **kw).backward()
            model.zero_grad(set_to_none=True)
            m = _metrics(use_logvar, True)
            loss, preds = model.forward_depth_step(x, target, transform=tr, metrics=m, **kw)
            assert preds.dtype == torch.float32 and preds.shape == (2, f_out) + tuple(target.shape[1:]) and not preds.requires_grad
            if grad:
                loss.backward()
                g_step = _grads(model)
                model.zero_grad(set_to_none=True)
                ref_loss = model.forward_depth_loss(x, target, **kw)
                ref_loss.backward()
                g_ref = _grads(model)
                model.zero_grad(set_to_none=True)
                assert _same_bits(loss.detach(), ref_loss.detach()), (float(loss), float(ref_loss))
                assert set(g_step) == set(g_ref)
                for n in g_ref:
                    assert torch.equal(g_step[n], g_ref[n]), n
            want, metres, ref = _reference_route(model, x, target, tr, use_logvar)
            if not grad:  # (the no-grad forward_depth_loss composes from the written rows: the same loss to rounding, not to the bit)
                want_loss = float(model.forward_depth_loss(x, target, **kw))
                assert abs(float(loss) - want_loss) <= 2e-4 * abs(want_loss), (float(loss), want_loss)
        assert _same_bits_nan(preds, want)
        B = x.shape[0]
        flat = want.reshape(B, f_out, -1).transpose(0, 1).reshape(f_out, -1)
        _check_state(m.state, ref.state, flat, metres.reshape(-1), ref, f"{which} f_out={f_out} grad={grad}")
        a, b = m.compute(), ref.compute()
        assert set(a) == set(b)
        # (each sum of non-negative terms is within rows * 2^-52 = 2e-11 relative of the reference's; the quotients double that, and
        # SILogE's difference of two such quotients loses at most another two digits here: 1e-9)
        for k in b:
            assert a[k] == b[k] or abs(a[k] - b[k]) <= 1e-9 * abs(b[k]), (k, a[k], b[k])
        if use_logvar:
            assert torch.equal(m.median, ref.median) and a["median_std"] == b["median_std"]
    # the bf16 step is the one-launch tail, with and without a gradient: no rows-writing forward, no standalone loss, transform or
    # metric kernel
    import heal_swin_amd.depth_data as D
    import heal_swin_amd.depth_evaluation as E
    import heal_swin_amd.ops.tail as T
    called = spy_on(monkeypatch, ("hs_expand_ln_head", "hs_ln_head", "hs_depth_loss", "hs_depth_target", "hs_depth_metrics"), (T, E, D, _lib))
    model.forward_depth_step(x, target, transform=tr, metrics=_metrics(use_logvar, True), **kw)[0].backward()
    with torch.no_grad():
        model.forward_depth_step(x, target, transform=tr, metrics=_metrics(use_logvar, True), return_preds=False, **kw)
    torch.cuda.synchronize()
    assert sorted(c for c in called if not c.endswith(("_supported", "_blocks", "_partials"))) == \
        ["hs_expand_ln_head_depth_step_fwd", "hs_expand_ln_head_depth_step_fwd", "hs_ln_head_depth_bwd"], called


def _by_hand(model, x, target, tr, kw, use_logvar):
    """The three calls by hand: depth_loss on model(x), unnormalize_and_retransform, DepthMetrics.update."""
    from heal_swin_amd.losses import depth_loss
    out = model(x)
    B = out.shape[0]
    loss = depth_loss(out.reshape(B, out.shape[1], -1), target.reshape(B, -1), **kw)
    want, metres, ref = _reference_route(model, x, target, tr, use_logvar)
    return loss, want, metres, ref


@pytest.mark.parametrize("which,dtype,embed", [("healpix", torch.float32, None), ("flat", torch.float32, None),
                                                ("flat", torch.bfloat16, 48)])  # 48: 3 / 6 heads of 16
def test_forward_depth_step_composes_the_same_results_elsewhere(which, dtype, embed):
    """fp32, and a width the one-launch tail does not take (C = 48, bf16): (loss, preds, metrics) of the three calls by hand."""
    for f_out in (1, 2):
        model, x, target, tr, kw = _model_case(which, f_out)
        if embed is not None:
            from heal_swin_amd.data_spec import DataSpec
            from heal_swin_amd.models_torch.swin_transformer import SwinTransformerConfig, SwinTransformerSys
            torch.manual_seed(0)
            model = SwinTransformerSys(SwinTransformerConfig(patch_size=2, window_size=8, shift_size=2, embed_dim=embed, depths=[2, 2],
                                                             num_heads=[3, 6], drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0),
                                       DataSpec(dim_in=(64, 96), f_in=3, f_out=f_out, base_pix=None, class_names=[])).cuda().eval()
        model.compute_dtype = dtype
        use_logvar = f_out == 2
        for grad in (True, False):
            with torch.set_grad_enabled(grad):
                m = _metrics(use_logvar, True)
                loss, preds = model.forward_depth_step(x, target, transform=tr, metrics=m, **kw)
                want_loss, want, metres, ref = _by_hand(model, x, target, tr, kw, use_logvar)
                assert loss.requires_grad == grad
            assert abs(float(loss.detach()) - float(want_loss.detach())) <= 2e-4 * abs(float(want_loss.detach())), (loss, want_loss)
            assert _same_bits_nan(preds, want)
            B = x.shape[0]  # (the flat model's rows are summed in another pixel order than the image: the rule of the kernel test)
            _check_state(m.state, ref.state, want.reshape(B, f_out, -1).transpose(0, 1).reshape(f_out, -1), metres.reshape(-1), ref,
                         f"{which} {dtype} f_out={f_out} grad={grad}")
            assert torch.equal(m.median, ref.median)
        with torch.no_grad():
            loss2, none = model.forward_depth_step(x, target, transform=tr, return_preds=False, **kw)
        assert none is None and float(loss2) == float(loss)


def test_flat_preds_are_the_image_and_pixel_rows_targets_give_the_same_bits():
    from heal_swin_amd import ops
    from heal_swin_amd.flat_data import PixelRows
    model, x, target, tr, kw = _model_case("flat", 2)
    model.compute_dtype = torch.bfloat16
    with torch.no_grad():
        model(x)
        model.forward_depth_step(x, target, transform=tr, **kw)
        a, b = _metrics(True, True), _metrics(True, True)
        loss_a, preds_a = model.forward_depth_step(x, target, transform=tr, metrics=a, **kw)
        p = model.config.patch_size[0]
        rows = PixelRows(ops.flat_depth_target(target, p, model.tile), 64, 96, p, model.tile)
        loss_b, preds_b = model.forward_depth_step(x, rows, transform=tr, metrics=b, **kw)
        want = model(x).clone()
        tr.unnormalize_and_retransform(want[:, 0].reshape(2, -1), out=want[:, 0].reshape(2, -1))
    assert preds_a.shape == (2, 2, 64, 96) and preds_a.dtype == torch.float32
    assert _same_bits_nan(preds_a, want) and _same_bits_nan(preds_a, preds_b)
    assert _same_bits(loss_a, loss_b) and torch.equal(a.state.view(torch.int64), b.state.view(torch.int64))
    assert torch.equal(a.median, b.median)


# ------------------------------------------------------------------ the reference's own shared_step (tests/golden/depth_step.npz)
def test_depth_step_from_rows_matches_the_reference_shared_step():
    """The reference's shared_step body run on stored head outputs (tests/golden/make_golden_depth_step.py): predictions and metrics
    to 1e-6 relative (the level of the depth-evaluation golden tests), the loss to 2e-4 relative (a loss recomputed along another
    route: here on the raw outputs, there on transform_and_normalize(unnormalize_and_retransform(.)))."""
    from heal_swin_amd.depth_evaluation import DepthMetrics
    from heal_swin_amd.losses import depth_loss_spec, depth_step_from_rows
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_step.npz")
    g = np.load(path, allow_pickle=False)
    cases = [str(c) for c in g["cases"]]
    assert len({c.rsplit("|", 1)[0] for c in cases}) == 9 and {c.rsplit("|", 1)[1] for c in cases} == {"l1", "l2", "huber", "logvar"}
    for c in cases:
        transform, norm, loss_name = c.split("|")
        use_logvar = loss_name == "logvar"
        tr = _transform((None if transform == "None" else transform, None if norm == "None" else norm))
        out = torch.from_numpy(g[c + "/outputs"]).to(DEV)
        target = torch.from_numpy(g[c + "/target"]).to(DEV)
        kind, delta = depth_loss_spec("l2" if use_logvar else loss_name, float(g[c + "/huber_delta"]), use_logvar)
        m = DepthMetrics(use_logvar=use_logvar)
        loss, preds = depth_step_from_rows(out, target, kind, delta, tr, m)
        want_loss, want = float(g[c + "/loss"]), torch.from_numpy(g[c + "/returned"]).to(DEV)
        print(c, "loss", float(loss), want_loss)
        assert abs(float(loss) - want_loss) <= 2e-4 * abs(want_loss), (c, float(loss), want_loss)
        err = ((preds - want).abs() / want.abs().clamp_min(1e-30)).max()
        assert float(err) <= 1e-6, (c, float(err))
        got = m.compute()
        for k in ("mse",) + (("mean_std", "median_std") if use_logvar else ()):
            w = float(g[c + "/" + k])
            print(c, k, got[k], w)
            assert math.isfinite(w) and abs(got[k] - w) <= 1e-6 * abs(w), (c, k, got[k], w)
