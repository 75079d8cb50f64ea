"""The segmentation caller's `shared_step` on the decoder tail (`ops.expand_ln_head_ce_step`, hs_expand_ln_head_ce_step_fwd) and
`forward_seg_step` of both models: the loss and the gradients are those of the loss-only tail BIT FOR BIT (same arithmetic, same
backward kernel), the class ids are torch.max's on the written logits and the confusion matrix is torch.bincount's -- all exact."""
import pytest
import torch

from _lib_spy import launches, spy_on

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _inputs(tokens, C, f_out, weighted):
    torch.manual_seed(tokens + C + f_out)
    xn = (torch.randn(tokens, C, device=DEV) * 1.3 + 0.2).to(torch.bfloat16)
    wexp = (torch.randn(4 * C, C, device=DEV) * C ** -0.5).to(torch.bfloat16).float().requires_grad_(True)
    gamma = (1 + 0.3 * torch.randn(C, device=DEV)).requires_grad_(True)
    beta = (0.2 * torch.randn(C, device=DEV)).requires_grad_(True)
    w = (torch.randn(f_out, C, 1, device=DEV) * 2.0 * C ** -0.5).requires_grad_(True)
    labels = torch.randint(0, f_out, (4 * tokens,), device=DEV, dtype=torch.uint8)
    cw = (0.2 + torch.rand(f_out, device=DEV)) if weighted else None
    return xn, [wexp, gamma, beta, w], labels, cw


def _bincount(labels, preds, K):
    keep = labels < K
    return torch.bincount(labels[keep].long() * K + preds[keep].long(), minlength=K * K).view(K, K)


def _written_argmax(xn, params, f_out):
    from heal_swin_amd import ops
    with torch.no_grad():
        return torch.max(ops.expand_ln_head(xn, *params)[:, :f_out], 1).indices


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


SHAPES = [(4096, 128, 12, True), (1000, 96, 12, False), (33, 64, 5, True), (70000, 128, 16, True), (5000, 128, 1, False),
          (4096, 128, 12, False), (1000, 96, 12, True), (33, 64, 5, False), (70000, 128, 16, False), (5000, 128, 1, True)]


@pytest.mark.parametrize("tokens,C,f_out,weighted", SHAPES)
def test_step_equals_the_loss_only_tail_and_the_written_logits(tokens, C, f_out, weighted):
    from heal_swin_amd import ops
    xn, params, labels, cw = _inputs(tokens, C, f_out, weighted)
    K = f_out
    want_preds = _written_argmax(xn, params, f_out)
    want_conf = _bincount(labels, want_preds, K)
    res = []
    for step in (False, True):
        xq = xn.clone().requires_grad_(True)
        for p in params:
            p.grad = None
        if step:
            conf, bad = torch.zeros(K, K, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
            loss, preds = ops.expand_ln_head_ce_step(xq, *params, labels, cw, confmat=conf, bad=bad)
            assert not preds.requires_grad and preds.dtype == torch.uint8 and preds.shape == labels.shape
        else:
            loss = ops.expand_ln_head_ce(xq, *params, labels, cw)
        (loss * 3.0).backward()
        res.append((loss.detach(), [xq.grad] + [p.grad for p in params]))
    assert _same_bits(res[0][0], res[1][0]), (float(res[0][0]), float(res[1][0]))
    for a, b, n in zip(res[0][1], res[1][1], ("dxn", "dWexpand", "dgamma", "dbeta", "dWhead")):
        assert _same_bits(a, b), n
    assert int((preds.long() != want_preds).sum()) == 0
    assert torch.equal(conf, want_conf) and int(conf.sum()) == 4 * tokens and bad.tolist() == [0, 0]
    # the no-grad (validation) form: nothing saved, the same three results
    with torch.no_grad():
        conf2, bad2 = torch.zeros_like(conf), torch.zeros_like(bad)
        loss2, preds2 = ops.expand_ln_head_ce_step(xn, *params, labels, cw, confmat=conf2, bad=bad2)
        ref2 = ops.expand_ln_head_ce(xn, *params, labels, cw)
    assert _same_bits(loss2, ref2) and _same_bits(loss2, res[0][0])
    assert torch.equal(preds2, preds) and torch.equal(conf2, want_conf) and bad2.tolist() == [0, 0]
    # each output is optional
    with torch.no_grad():
        loss3, none = ops.expand_ln_head_ce_step(xn, *params, labels, cw, want_preds=False)
        loss4, preds4 = ops.expand_ln_head_ce_step(xn, *params, labels, cw)
    assert none is None and _same_bits(loss3, ref2) and _same_bits(loss4, ref2) and torch.equal(preds4, preds)


def test_ignored_labels_are_counted_as_bad_and_calls_accumulate():
    from heal_swin_amd import ops
    tokens, C, K = 3000, 128, 12
    xn, params, labels, cw = _inputs(tokens, C, K, True)
    labels[::7] = 255
    labels[5] = K  # the first id outside the matrix
    n_bad = int((labels >= K).sum())
    want_preds = _written_argmax(xn, params, K)
    conf, bad = torch.zeros(K, K, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        loss, preds = ops.expand_ln_head_ce_step(xn, *params, labels, cw, confmat=conf, bad=bad)
        ref = ops.expand_ln_head_ce(xn, *params, labels, cw)
    assert _same_bits(loss, ref)
    assert torch.equal(preds.long(), want_preds)  # ignored rows are still predicted
    want = _bincount(labels, want_preds, K)
    assert torch.equal(conf, want) and int(conf.sum()) == 4 * tokens - n_bad and bad.tolist() == [n_bad, 0]
    with torch.no_grad():
        ops.expand_ln_head_ce_step(xn, *params, labels, cw, confmat=conf, bad=bad, want_preds=False)
    assert torch.equal(conf, 2 * want) and bad.tolist() == [2 * n_bad, 0]


def test_ties_take_the_lower_class_and_nan_rows_follow_torch_max():
    from heal_swin_amd import ops
    tokens, C, K = 2048, 96, 12
    xn, params, labels, cw = _inputs(tokens, C, K, False)
    with torch.no_grad():
        w = params[3]
        # identical class rows: exact ties between classes of the two lanes of a pair (2 | 5 and 9 | 7), of one lane (0 | 1) and
        # across the register halves (3 | 11); scaled up so that the tied classes are the maximum on many rows
        for lo, hi in ((2, 5), (7, 9), (0, 1), (3, 11)):
            w[hi] = w[lo] = 3.0 * w[lo]
        xn[17] = float("nan")
        xn[100, 3] = float("nan")
        xn[1999, ::2] = float("inf")  # inf - inf inside LayerNorm: NaN again
    want = _written_argmax(xn, params, K)
    with torch.no_grad():
        logits = ops.expand_ln_head(xn, *params)[:, :K]
        _, preds = ops.expand_ln_head_ce_step(xn, *params, labels, cw)
    assert int(logits.isnan().any(1).sum()) >= 12  # the three tokens' four children each
    tied = (logits[:, 5] == logits.max(1).values) | (logits[:, 9] == logits.max(1).values) | (logits[:, 1] == logits.max(1).values) | \
           (logits[:, 11] == logits.max(1).values)
    assert int(tied.sum()) > 100
    assert int((preds.long() != want).sum()) == 0
    assert not any(int((preds == hi).sum()) for hi in (5, 9, 1, 11))  # the lower index is predicted everywhere


# ------------------------------------------------------------------ whole models
def _hp_model():
    import bench
    wl = bench.WORKLOADS["T128"]
    model, cfg, spec = bench.build_model(wl, nside=64)
    model = model.cuda().eval()
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randint(0, 256, (2, 3, spec["dim_in"]), generator=g, device=DEV, dtype=torch.uint8).float()
    labels = torch.randint(0, 12, (2, spec["dim_in"]), generator=g, device=DEV, dtype=torch.uint8)
    cw = 0.3 + torch.rand(12, generator=g, device=DEV)
    return model, x, labels, cw, 12


def _flat_model():
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_transformer import SwinTransformerConfig, SwinTransformerSys
    cfg = dict(patch_size=2, window_size=8, shift_size=2, embed_dim=64, depths=[2, 2], num_heads=[2, 4], drop_rate=0.0,
               attn_drop_rate=0.0, drop_path_rate=0.0)
    spec = dict(dim_in=(64, 96), f_in=3, f_out=5, base_pix=None, class_names=[])
    torch.manual_seed(0)
    m = SwinTransformerSys(SwinTransformerConfig(**cfg), DataSpec(**spec)).cuda().eval()
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randint(0, 256, (2, 3, 64, 96), generator=g, device=DEV, dtype=torch.uint8).float()
    labels = torch.randint(0, 5, (2, 64, 96), generator=g, device=DEV, dtype=torch.uint8)
    cw = 0.3 + torch.rand(5, generator=g, device=DEV)
    return m, x, labels, cw, 5


def _reference_route(model, x, labels, K):
    """The reference's shared_step on the written logits: (preds of torch.max, the SegConfusion of update(logits, labels))."""
    from heal_swin_amd.evaluation import SegConfusion
    from heal_swin_amd.losses import seg_predictions
    logits = model(x)
    ref = SegConfusion(K)
    ref.update(logits.detach().flatten(2), labels.flatten(1))
    return logits, seg_predictions(logits.detach()), ref


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("which", ["healpix", "flat"])
def test_forward_seg_step_equals_the_reference_route_bf16(which, monkeypatch):
    from heal_swin_amd import _lib
    from heal_swin_amd.evaluation import SegConfusion
    model, x, labels, cw, K = (_hp_model if which == "healpix" else _flat_model)()
    model.compute_dtype = torch.bfloat16
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            # one warm-up call of each route: the per-shape GEMM choice is settled
            model.forward_seg_step(x, labels, cw, confusion=SegConfusion(K))
            model(x)
            if grad:
                model.forward_seg_loss(x, labels, cw).backward()
            model.zero_grad(set_to_none=True)
            c = SegConfusion(K)
            loss, preds = model.forward_seg_step(x, labels, cw, confusion=c)
            assert preds.dtype == torch.uint8 and preds.shape == labels.shape and not preds.requires_grad
            if grad:
                loss.backward()
                g_step = _grads(model)
                model.zero_grad(set_to_none=True)
                ref_loss = model.forward_seg_loss(x, labels, cw)
                ref_loss.backward()
                g_ref = _grads(model)
                model.zero_grad(set_to_none=True)
                assert _same_bits(loss.detach(), ref_loss.detach()), (float(loss), float(ref_loss))
                assert set(g_step) == set(g_ref)
                for n in g_ref:
                    assert torch.equal(g_step[n], g_ref[n]), n
            logits, ref_preds, ref = _reference_route(model, x, labels, K)
            if not grad:  # (the no-grad forward_seg_loss composes from the written logits: the same loss to rounding, not to the bit)
                from heal_swin_amd.losses import seg_loss
                want = float(seg_loss(logits.flatten(2), labels.flatten(1), cw))
                assert abs(float(loss) - want) <= 2e-4 * abs(want), (float(loss), want)
        assert int((preds.long() != ref_preds).sum()) == 0
        assert torch.equal(c.confmat, ref.confmat) and int(c.confmat.sum()) == labels.numel()
        assert torch.equal(c.iou(), ref.iou()) and torch.equal(c.accuracy(), ref.accuracy())
        assert torch.equal(c.accuracy(ignore_index=0), ref.accuracy(ignore_index=0))
    # the bf16 step is the one-launch tail, with and without a gradient: no logits-writing forward, no standalone loss / confusion kernel
    import heal_swin_amd.evaluation as E
    import heal_swin_amd.ops.tail as T
    called = spy_on(monkeypatch, ("hs_expand_ln_head", "hs_ln_head", "hs_seg_"), (T, E, _lib))
    model.forward_seg_step(x, labels, cw, confusion=SegConfusion(K))[0].backward()
    with torch.no_grad():
        model.forward_seg_step(x, labels, cw, confusion=SegConfusion(K))
    torch.cuda.synchronize()
    assert sorted(c for c in called if not c.endswith(("_supported", "_blocks", "_partials"))) == \
        ["hs_expand_ln_head_ce_step_fwd", "hs_expand_ln_head_ce_step_fwd", "hs_ln_head_ce_bwd"], called
    # forward_seg_loss without a gradient: the rows-writing tail once, then the standalone loss kernel on the rows
    del called[:]
    with torch.no_grad():
        model.forward_seg_loss(x, labels, cw)
    torch.cuda.synchronize()
    assert launches(called) == ["hs_expand_ln_head_fwd", "hs_seg_ce_fwd"], called


@pytest.mark.parametrize("which", ["healpix", "flat"])
def test_forward_seg_step_fp32_composes_the_same_results(which):
    from heal_swin_amd.evaluation import SegConfusion
    from heal_swin_amd.losses import seg_loss
    model, x, labels, cw, K = (_hp_model if which == "healpix" else _flat_model)()
    model.compute_dtype = torch.float32
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            c = SegConfusion(K)
            loss, preds = model.forward_seg_step(x, labels, cw, confusion=c)
            assert preds.dtype == torch.uint8 and preds.shape == labels.shape
            logits, ref_preds, ref = _reference_route(model, x, labels, K)
            want = seg_loss(logits.flatten(2), labels.flatten(1), cw)
            assert abs(float(loss) - float(want)) <= 2e-4 * abs(float(want)), (float(loss), float(want))
            assert loss.requires_grad == grad
        assert int((preds.long() != ref_preds).sum()) == 0
        assert torch.equal(c.confmat, ref.confmat)
    loss2, none = model.forward_seg_step(x, labels, cw, return_preds=False)
    assert none is None and float(loss2) == float(loss)


def test_flat_preds_are_the_image_argmax_and_pixel_rows_labels_count_the_same():
    from heal_swin_amd import ops
    from heal_swin_amd.evaluation import SegConfusion
    from heal_swin_amd.flat_data import PixelRows
    model, x, labels, cw, K = _flat_model()
    model.compute_dtype = torch.bfloat16
    labels[:, :2] = 255  # ignored pixels
    with torch.no_grad():
        model(x)
        model.forward_seg_step(x, labels, cw)
        a, b = SegConfusion(K), SegConfusion(K)
        loss_a, preds_a = model.forward_seg_step(x, labels, cw, confusion=a)
        p = model.config.patch_size[0]
        rows = PixelRows(ops.flat_labels(labels, p, model.tile), 64, 96, p, model.tile)
        loss_b, preds_b = model.forward_seg_step(x, rows, cw, confusion=b)
        want = model(x).argmax(1)
    assert preds_a.shape == (2, 64, 96) and preds_a.dtype == torch.uint8
    assert int((preds_a.long() != want).sum()) == 0 and torch.equal(preds_a, preds_b)
    assert _same_bits(loss_a, loss_b) and torch.equal(a.confmat, b.confmat) and torch.equal(a._bad, b._bad)
    assert a._bad.tolist() == [2 * 2 * 96, 0] and int(a.confmat.sum()) == labels.numel() - 2 * 2 * 96
    with pytest.raises(ValueError, match="target values >= num_classes"):  # the deferred check at the metric read
        a.iou()
    # the uint8 rows -> image kernel is the inverse of flat_labels
    ids = torch.randint(0, 255, (2, 64, 96), device=DEV, dtype=torch.uint8)
    assert torch.equal(ops.flat_label_image(ops.flat_labels(ids, p, model.tile), 64, 96, p, model.tile), ids)
