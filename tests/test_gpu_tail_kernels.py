"""Operator-level net under the decoder tail kernels (csrc/ln_head.hip, csrc/expand_ln_head.hip): every width of `ln_head`, the
bf16-logits instantiations through the C ABI, the second trip of both persistent loops with a ragged end, and the `live`
predicate of every masked store.  References and bounds are those of test_gpu_ln_head.py, test_gpu_depth_loss.py,
test_gpu_seg_step.py and test_gpu_depth_step.py (TOL / GRAD_TOL of tests/_util.py, 1e-3 on a loss); relations the project states
bit for bit are asserted bit for bit."""
import pytest
import torch

from tests._util import GRAD_TOL, TOL, assert_close, assert_unbiased
from tests.test_gpu_depth_loss import _reference_tail_depth
from tests.test_gpu_depth_step import KINDS, _check_state, _metrics, _target, _transform, _written
from tests.test_gpu_depth_step import _inputs as _depth_inputs
from tests.test_gpu_depth_step import _same_bits as _same_bits_any
from tests.test_gpu_ln_head import reference, reference_tail, reference_tail_ce
from tests.test_gpu_seg_step import _bincount, _same_bits, _written_argmax
from tests.test_gpu_seg_step import _inputs as _seg_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
SENTINEL = -512.0  # exact in bf16 and fp32; 171 in a uint8 buffer
GROUP = 32         # rows of one wavefront step


def _ln_head_inputs(rows, C, f_out):
    torch.manual_seed(rows + C)
    y = (torch.randn(rows, C, device=DEV) * 1.7 + 0.6 * torch.randn(rows, 1, device=DEV) + 0.3).to(BF16)
    gamma = (1 + 0.3 * torch.randn(C, device=DEV)).requires_grad_(True)
    beta = (0.2 * torch.randn(C, device=DEV)).requires_grad_(True)
    w = (torch.randn(f_out, C, 1, device=DEV) * C ** -0.5).requires_grad_(True)
    dlog = torch.randn(rows, f_out, device=DEV).to(BF16)
    return y, gamma, beta, w, dlog


def _ln_head_against_the_composition(rows, C, f_out):
    """`ops.ln_head` forward and backward: the assertions of test_ln_head_matches_the_composition."""
    from heal_swin_amd import ops

    y, gamma, beta, w, dlog = _ln_head_inputs(rows, C, f_out)
    assert ops.ln_head_ok(y, C, f_out)
    yq = y.clone().requires_grad_(True)
    out = ops.ln_head(yq, gamma, beta, w)
    assert out.shape == (rows, 16) and not out[:, f_out:].any()
    out[:, :f_out].backward(dlog.float())
    ref_out, ref_dy, ref_dg, ref_db, ref_dw = reference(y, gamma, beta, w.reshape(f_out, C), dlog)
    tag = f"tail net ln_head[{rows}x{C}->{f_out}]"
    assert_close(out[:, :f_out], ref_out, TOL[BF16], tag + " logits")
    assert_close(yq.grad, ref_dy, GRAD_TOL[BF16], tag + " dy")
    assert_close(gamma.grad, ref_dg, GRAD_TOL[BF16], tag + " dgamma")
    assert_close(beta.grad, ref_db, GRAD_TOL[BF16], tag + " dbeta")
    assert_close(w.grad.reshape(f_out, C), ref_dw, GRAD_TOL[BF16], tag + " dWhead")


@pytest.mark.parametrize("C", [64, 96, 128, 160, 192, 224, 256])
def test_ln_head_at_every_width(C):
    """rows = 97: three full 32-row groups and one lane of a fourth."""
    _ln_head_against_the_composition(97, C, 12)


def _filled(shape, dtype, extra_rows=GROUP):
    """A buffer `extra_rows` rows longer than `shape`, full of the sentinel: (whole, the part the kernel may write, the tail)."""
    whole = torch.full((shape[0] + extra_rows,) + tuple(shape[1:]), 171 if dtype == torch.uint8 else SENTINEL, dtype=dtype, device=DEV)
    return whole, whole[:shape[0]], whole[shape[0]:]


def _untouched(*tails):
    return all(bool((t == (171 if t.dtype == torch.uint8 else SENTINEL)).all()) for t in tails)


@pytest.mark.parametrize("C", [64, 160, 256])
def test_bf16_logits_through_the_c_abi(C):
    """`hs_ln_head_fwd` / `hs_ln_head_bwd` with HS_BF16 logits (no caller in ops/): the forward's logits against the composition,
    its statistics bit for bit those of the HS_F32 call; the backward bit for bit that of the HS_F32 call on the same (bf16-exact)
    values -- both form the same d[] and the same packed operand.  Every output sits in a buffer one row group longer than `rows`
    whose tail must keep its sentinel."""
    from heal_swin_amd import _lib
    from heal_swin_amd._lib import check, lib, ptr, stream_ptr
    from heal_swin_amd.ops import tail as T

    rows, f_out, KP = 97, 12, 16
    y, gamma, beta, w, dlog = _ln_head_inputs(rows, C, f_out)
    wfold, bvec = T._fold_head(gamma, beta, w, C, y.device)
    s = stream_ptr(y.device)
    fwd = {}
    for code, dtype in ((_lib.HS_F32, torch.float32), (_lib.HS_BF16, BF16)):
        (_, logits, t0), (_, mean, t1), (_, rstd, t2) = _filled((rows, KP), dtype), _filled((rows,), torch.float32), _filled((rows,), torch.float32)
        check(lib.hs_ln_head_fwd(ptr(y), ptr(wfold), ptr(bvec), ptr(logits), ptr(mean), ptr(rstd), rows, C, _lib.HS_BF16, code, s), "hs_ln_head_fwd")
        torch.cuda.synchronize()
        assert _untouched(t0, t1, t2), f"hs_ln_head_fwd wrote beyond row {rows} (logits dtype {dtype})"
        fwd[code] = (logits, mean, rstd)
    ref_out = reference(y, gamma, beta, w.reshape(f_out, C), dlog)[0]
    logits16, mean16, rstd16 = fwd[_lib.HS_BF16]
    logits32, mean32, rstd32 = fwd[_lib.HS_F32]
    assert_close(logits16[:, :f_out], ref_out, TOL[BF16], f"tail net ln_head bf16 logits C={C}")
    assert_close(logits32[:, :f_out], ref_out, TOL[BF16], f"tail net ln_head f32 logits C={C}")
    assert not logits16[:, f_out:].any() and not logits32[:, f_out:].any()
    assert _same_bits(mean16, mean32) and _same_bits(rstd16, rstd32)

    afold = torch.zeros((C, KP), dtype=BF16, device=DEV)
    afold[:, :f_out] = (w.detach().reshape(f_out, C).float() * gamma.detach().float()).t().to(BF16)
    d16 = torch.zeros((rows, KP), dtype=BF16, device=DEV)
    d16[:, :f_out] = dlog
    nparts = int(lib.hs_ln_head_partials(rows))
    bwd = {}
    for code, d in ((_lib.HS_F32, d16.float().contiguous()), (_lib.HS_BF16, d16)):
        (_, dy, t0), (_, dprime, t1) = _filled((rows, C), BF16), _filled((rows, KP), BF16)
        part = torch.full((nparts, 32), SENTINEL, dtype=torch.float32, device=DEV)
        check(lib.hs_ln_head_bwd(ptr(y), ptr(mean32), ptr(rstd32), ptr(d), ptr(afold), ptr(dy), ptr(dprime), ptr(part), rows, C,
                                 _lib.HS_BF16, code, s), "hs_ln_head_bwd")
        torch.cuda.synchronize()
        assert _untouched(t0, t1), f"hs_ln_head_bwd wrote beyond row {rows} (dlogits code {code})"
        bwd[code] = (dy, dprime, part)
    for a, b, n in zip(bwd[_lib.HS_BF16], bwd[_lib.HS_F32], ("dy", "dprime", "partials")):
        assert _same_bits_any(a, b), n
    ref_dy = reference(y, gamma, beta, w.reshape(f_out, C), dlog)[1]
    assert_close(bwd[_lib.HS_BF16][0], ref_dy, GRAD_TOL[BF16], f"tail net ln_head bf16 dlogits C={C} dy")
    u = bwd[_lib.HS_BF16][2].sum(0)[:KP]
    assert_close(u[:f_out], dlog.float().sum(0), GRAD_TOL[BF16], f"tail net ln_head bf16 dlogits C={C} u") and not u[f_out:].any()


# ------------------------------------------------------------------ the second trip of ln_head.hip's row loop, ragged end
LN_ROWS = 262144 + 33


def _second_trip_of_ln_head(rows):
    from heal_swin_amd._lib import lib
    assert rows > GROUP * int(lib.hs_ln_head_partials(rows)), "every wave must own a second 32-row group"


@pytest.mark.parametrize("C", [64, 256])
def test_ln_head_second_trip_of_the_row_loop(C):
    _second_trip_of_ln_head(LN_ROWS)
    _ln_head_against_the_composition(LN_ROWS, C, 12)


def _grads_of(xq, params):
    return [xq.grad] + [p.grad for p in params]


GRAD_NAMES = ("dxn", "dWexpand", "dgamma", "dbeta", "dWhead")


def _ce_forms(tokens, C, f_out, tag):
    """`ops.expand_ln_head_ce` against the composition (loss 1e-3, gradients GRAD_TOL) and `ops.expand_ln_head_ce_step` against it
    (loss and gradients bit for bit, preds = torch.max on the written logits, confmat = torch.bincount)."""
    from heal_swin_amd import ops
    xn, params, labels, cw = _seg_inputs(tokens, C, f_out, True)
    K, res = f_out, []
    for step in (False, True):
        xq = xn.clone().requires_grad_(True)
        for p in params:
            p.grad = None
        if step:
            conf, bad = torch.zeros(K, K, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
            loss, preds = ops.expand_ln_head_ce_step(xq, *params, labels, cw, confmat=conf, bad=bad)
        else:
            loss = ops.expand_ln_head_ce(xq, *params, labels, cw)
        (loss * 3.0).backward()
        res.append((loss.detach(), _grads_of(xq, params)))
    wexp, gamma, beta, w = params
    ref = reference_tail_ce(xn, wexp, gamma, beta, w.reshape(f_out, C), labels, cw)
    assert abs(float(res[0][0]) - float(ref[0])) <= 1e-3 * abs(float(ref[0])), (float(res[0][0]), float(ref[0]))
    for got, want, n in zip(res[0][1], ref[1:], GRAD_NAMES):
        assert_close(got.reshape(want.shape), 3.0 * want, GRAD_TOL[BF16], f"{tag} ce {n}")
    assert _same_bits(res[0][0], res[1][0]), (float(res[0][0]), float(res[1][0]))
    for a, b, n in zip(res[0][1], res[1][1], GRAD_NAMES):
        assert _same_bits(a, b), n
    want_preds = _written_argmax(xn, params, f_out)
    assert preds.dtype == torch.uint8 and int((preds.long() != want_preds).sum()) == 0
    assert torch.equal(conf, _bincount(labels, want_preds, K)) and int(conf.sum()) == 4 * tokens and bad.tolist() == [0, 0]


def _depth_forms(tokens, C, tag):
    """`ops.expand_ln_head_depth` (log-variance loss, two channels) against the composition (loss 1e-3, gradients GRAD_TOL and
    slope) and `ops.expand_ln_head_depth_step` against it (loss and gradients bit for bit, predictions the written rows through
    unnormalize_and_retransform bit for bit, metric state within test_gpu_depth_step's float64 bound)."""
    from heal_swin_amd import ops
    f_out, rows = 2, 4 * tokens
    xn, params = _depth_inputs(tokens, C, f_out)
    tr = _transform(("log", "standardize"))
    target = _target(rows, tr, tokens, nans=False)
    kind, delta = KINDS["logvar"], 0.7
    res = []
    for step in (False, True):
        xq = xn.clone().requires_grad_(True)
        for p in params:
            p.grad = None
        if step:
            m = _metrics(True, True)
            loss, preds = ops.expand_ln_head_depth_step(xq, *params, target, kind, delta, None, tr, m)
        else:
            loss = ops.expand_ln_head_depth(xq, *params, target, kind, delta)
        (loss * 3.0).backward()
        res.append((loss.detach(), _grads_of(xq, params)))
    wexp, gamma, beta, w = params
    ref = _reference_tail_depth(xn, wexp, gamma, beta, w.reshape(f_out, C), target, dict(loss="l1", use_logvar=True, huber_delta=delta))
    assert abs(float(res[0][0]) - float(ref[0])) <= 1e-3 * abs(float(ref[0])), (float(res[0][0]), float(ref[0]))
    for got, want, n in zip(res[0][1], ref[1:], GRAD_NAMES):
        assert_close(got.reshape(want.shape), 3.0 * want, GRAD_TOL[BF16], f"{tag} depth {n}")
        assert_unbiased(got.reshape(want.shape), 3.0 * want, f"{tag} depth {n}")
    assert _same_bits_any(res[0][0], res[1][0]), (float(res[0][0]), float(res[1][0]))
    for a, b, n in zip(res[0][1], res[1][1], GRAD_NAMES):
        assert _same_bits_any(a, b), n
    want = _written(xn, params, f_out, tr)
    assert preds.shape == (f_out, rows) and _same_bits_any(preds, want)
    metres = tr.unnormalize_and_retransform(target[None])[0]
    refm = _metrics(True, True)
    refm.update(want[None], metres[None])
    _check_state(m.state, refm.state, want, metres, refm, tag)
    assert torch.equal(m.median, refm.median)


LN_TOKENS = 65536 + 9  # 4 children each: 262 180 rows


@pytest.mark.parametrize("C", [64, 96])
@pytest.mark.parametrize("form", ["ce", "depth"])
def test_fused_backwards_second_trip_of_the_row_loop(form, C):
    """`hs_ln_head_ce_bwd` / `hs_ln_head_depth_bwd` behind ops.expand_ln_head_ce / _depth with more rows than one trip of the
    backward's waves covers."""
    _second_trip_of_ln_head(4 * LN_TOKENS)
    tag = f"tail net {form}_bwd second trip C={C}"
    if form == "ce":
        _ce_forms(LN_TOKENS, C, 12, tag)
    else:
        _depth_forms(LN_TOKENS, C, tag)


# ------------------------------------------------------------------ the second trip of expand_ln_head.hip's token loop, ragged end
def _expand_second_trip_tokens():
    from heal_swin_amd._lib import lib
    cap = int(lib.hs_expand_ln_head_blocks(1 << 30))
    tokens = 128 * cap + 33
    assert int(lib.hs_expand_ln_head_blocks(tokens)) == cap, "the grid must sit at its cap: some waves loop a second time"
    return tokens


@pytest.mark.parametrize("C", [64, 96])
@pytest.mark.parametrize("form", ["plain", "ce", "depth"])
def test_expand_ln_head_second_trip_of_the_token_loop(form, C):
    """More tokens than 128 per workgroup of the capped grid, plus 33: the plain forward (+ its backward), the CE and CE-step
    forms and the depth and depth-step forms, each held to what its own test file asserts."""
    from heal_swin_amd import ops
    tokens = _expand_second_trip_tokens()
    tag = f"tail net expand second trip {form} C={C}"
    if form == "ce":
        return _ce_forms(tokens, C, 12, tag)
    if form == "depth":
        return _depth_forms(tokens, C, tag)
    f_out = 12
    torch.manual_seed(tokens + C)
    xn = (torch.randn(tokens, C, device=DEV) * 1.3 + 0.2).to(BF16)
    wexp = (torch.randn(4 * C, C, device=DEV) * C ** -0.5).to(BF16).float().requires_grad_(True)
    gamma = (1 + 0.3 * torch.randn(C, device=DEV)).requires_grad_(True)
    beta = (0.2 * torch.randn(C, device=DEV)).requires_grad_(True)
    w = (torch.randn(f_out, C, 1, device=DEV) * C ** -0.5).requires_grad_(True)
    dlog = torch.randn(4 * tokens, f_out, device=DEV).to(BF16).float()
    xq = xn.clone().requires_grad_(True)
    out = ops.expand_ln_head(xq, wexp, gamma, beta, w)
    assert out.dtype == torch.float32 and out.shape == (4 * tokens, 16) and not out[:, f_out:].any()
    out[:, :f_out].backward(dlog)
    ref = reference_tail(xn, wexp, gamma, beta, w.reshape(f_out, C), dlog)
    assert_close(out[:, :f_out], ref[0], 2e-3, tag + " logits")
    for got, want, n in zip(_grads_of(xq, [wexp, gamma, beta, w]), ref[1:], GRAD_NAMES):
        assert_close(got.reshape(want.shape), want, GRAD_TOL[BF16], f"{tag} {n}")
    with torch.no_grad():
        out2 = ops.expand_ln_head(xn, wexp, gamma, beta, w)
    assert torch.equal(out2, out.detach())


# ------------------------------------------------------------------ outputs written only under the `live` mask
def test_masked_stores_of_the_fused_kernels_stay_inside_their_rows():
    """The expand forward in its CE-step and depth-step forms and the two fused backwards, through the C ABI, with every per-row
    output (y, logits, mean, rstd, preds; dy, dprime) one 32-token group longer than the call's rows and pre-filled: the tail
    keeps the sentinel and the written part is bit for bit what the ops-level call returns."""
    from heal_swin_amd import _lib, ops
    from heal_swin_amd._lib import check, lib, ptr, stream_ptr
    from heal_swin_amd.ops import tail as T

    tokens, C, K, KP = 33, 96, 12, 16
    rows = 4 * tokens
    xn, params, labels, cw = _seg_inputs(tokens, C, K, True)
    wexp, gamma, beta, w = (p.detach() for p in params)
    wq = wexp.to(BF16).contiguous()
    wfold, bvec = T._fold_head(gamma, beta, w, C, xn.device)
    s = stream_ptr(xn.device)
    blocks = int(lib.hs_expand_ln_head_blocks(tokens))
    extra = 4 * GROUP  # the rows of one more 32-token group

    def outputs():
        return (_filled((rows, C), BF16, extra), _filled((rows, KP), torch.float32, extra), _filled((rows,), torch.float32, extra),
                _filled((rows,), torch.float32, extra))

    # ---- CE step: y, logits, mean, rstd, preds
    (_, y, ty), (_, logits, tl), (_, mean, tm), (_, rstd, tr_) = outputs()
    _, preds, tp = _filled((rows,), torch.uint8, extra)
    parts = torch.empty((4 * blocks, 2), dtype=torch.float32, device=DEV)
    conf, bad = torch.zeros(K, K, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    check(lib.hs_expand_ln_head_ce_step_fwd(ptr(xn), None, ptr(wq), ptr(wfold), ptr(bvec), ptr(labels), ptr(cw), K, ptr(y), ptr(logits),
                                            ptr(mean), ptr(rstd), ptr(parts), ptr(preds), ptr(conf), ptr(bad), tokens, C, 4, _lib.HS_BF16, s),
          "hs_expand_ln_head_ce_step_fwd")
    torch.cuda.synchronize()
    assert _untouched(ty, tl, tm, tr_, tp), "hs_expand_ln_head_ce_step_fwd wrote beyond its rows"
    with torch.no_grad():
        want_logits = ops.expand_ln_head(xn, *params)
        want_loss, want_preds = ops.expand_ln_head_ce_step(xn, *params, labels, cw)
    assert _same_bits(logits, want_logits) and torch.equal(preds, want_preds)
    tot = parts.sum(0)
    assert _same_bits(tot[0] / tot[1], want_loss)
    assert torch.equal(conf, _bincount(labels, want_preds.long(), K))

    # ---- CE backward on those rows: dy, dprime
    scale = (3.0 / tot[1]).reshape(1)
    want_dy = T._ln_head_backward(y, mean, rstd, gamma, beta, w, None, False, ce=(labels, cw, scale))[0]
    wfold_ce, bvec_ce = T._fold_head_ce(gamma, beta, w, C, xn.device)
    afold = torch.zeros((C, KP), dtype=BF16, device=DEV)
    afold[:, :K] = (w.reshape(K, C).float() * gamma.float()).t().to(BF16)
    nparts = int(lib.hs_ln_head_partials(rows))
    (_, dy, t0), (_, dprime, t1) = _filled((rows, C), BF16), _filled((rows, KP), BF16)
    part = torch.empty((nparts, 32), dtype=torch.float32, device=DEV)
    check(lib.hs_ln_head_ce_bwd(ptr(y), ptr(mean), ptr(rstd), ptr(labels), ptr(cw), ptr(scale), K, ptr(wfold_ce), ptr(bvec_ce), ptr(afold),
                                ptr(dy), ptr(dprime), ptr(part), rows, C, _lib.HS_BF16, s), "hs_ln_head_ce_bwd")
    torch.cuda.synchronize()
    assert _untouched(t0, t1), "hs_ln_head_ce_bwd wrote beyond its rows"
    assert _same_bits_any(dy, want_dy)

    # ---- depth step (one channel, L1): y, logits, mean, rstd, preds in metres
    w1 = w[:1].contiguous()
    wfold1, bvec1 = T._fold_head(gamma, beta, w1, C, xn.device)
    target = torch.randn(rows, device=DEV)
    target[::13] = float("inf")
    (_, y, ty), (_, logits, tl), (_, mean, tm), (_, rstd, tr_) = outputs()
    _, predf, tp = _filled((rows,), torch.float32, extra)
    check(lib.hs_expand_ln_head_depth_step_fwd(ptr(xn), None, ptr(wq), ptr(wfold1), ptr(bvec1), ptr(target), KINDS["l1"], 1.0, 1, ptr(y),
                                               ptr(logits), ptr(mean), ptr(rstd), ptr(parts), 0, _lib.HS_DT_NONE, 0.0, 1.0, 0, 0.0, None, 0,
                                               None, None, ptr(predf), None, tokens, C, 4, _lib.HS_BF16, s), "hs_expand_ln_head_depth_step_fwd")
    torch.cuda.synchronize()
    assert _untouched(ty, tl, tm, tr_, tp), "hs_expand_ln_head_depth_step_fwd wrote beyond its rows"
    with torch.no_grad():
        want_loss, want_pred = ops.expand_ln_head_depth_step(xn, wexp, gamma, beta, w1, target, KINDS["l1"], 1.0)
    tot = parts.sum(0)
    assert _same_bits_any(tot[0] / tot[1], want_loss) and _same_bits_any(predf, want_pred[0]) and _same_bits_any(logits[:, 0], predf)

    # ---- depth backward on those rows: dy, dprime
    scale = (3.0 / tot[1]).reshape(1)
    want_dy = T._ln_head_backward(y, mean, rstd, gamma, beta, w1, None, False, depth=(target, KINDS["l1"], 1.0, scale))[0]
    afold1 = torch.zeros((C, KP), dtype=BF16, device=DEV)
    afold1[:, :1] = (w1.reshape(1, C).float() * gamma.float()).t().to(BF16)
    (_, dy, t0), (_, dprime, t1) = _filled((rows, C), BF16), _filled((rows, KP), BF16)
    check(lib.hs_ln_head_depth_bwd(ptr(y), ptr(mean), ptr(rstd), ptr(target), KINDS["l1"], 1.0, ptr(scale), 1, ptr(wfold1), ptr(bvec1),
                                   ptr(afold1), ptr(dy), ptr(dprime), ptr(part), rows, C, _lib.HS_BF16, s), "hs_ln_head_depth_bwd")
    torch.cuda.synchronize()
    assert _untouched(t0, t1), "hs_ln_head_depth_bwd wrote beyond its rows"
    assert _same_bits_any(dy, want_dy) and not dprime[:, 1:].any()
