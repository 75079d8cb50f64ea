"""hs_lib_gemm_nt: the library product with the residual as its C operand (D = A W^T + bias + C, C != D) against fp32 torch on the
same bf16 operands, its refusals, the algorithm pick and pin, the v1 block pair whose fc2 add rides on it (the next block's
norm1 is then a plain LayerNorm), and a graphed step that replays it."""
import ctypes

import pytest
import torch

from _util import GRAD_TOL, TOL, assert_close, assert_unbiased

pytestmark = pytest.mark.gpu
DEV = "cuda"
RESID_TOL = 6e-3  # the bound tests/test_gpu_gemm.py puts on hs_gemm_nt's HS_EPI_RESID against the same reference


def _L():
    from heal_swin_amd import _lib
    return _lib


def _operands(m, n, k, seed=0):
    g = torch.Generator().manual_seed(seed + m + n + k)
    a = torch.randn(m, k, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(torch.bfloat16).to(DEV)
    bias = torch.randn(n, generator=g).to(torch.bfloat16).to(DEV)
    c = torch.randn(m, n, generator=g).to(torch.bfloat16).to(DEV)
    return a, w, bias, c


def _reference(a, w, bias, c):
    ref = a.float() @ w.float().t() + bias.float()
    return (ref if c is None else ref + c.float()).to(torch.bfloat16)


def _call(a, w, bias, c, d=None):
    L = _L()
    m, k = a.shape
    n = w.shape[0]
    d = torch.empty((m, n), dtype=torch.bfloat16, device=a.device) if d is None else d
    st = L.lib.hs_lib_gemm_nt(L.ptr(a), L.ptr(w), L.ptr(bias), L.HS_BF16, L.ptr(c), L.ptr(d), m, n, k, L.stream_ptr(a.device))
    return st, d


@pytest.fixture(scope="module")
def supported():
    assert _L().lib.hs_lib_gemm_supported() == 1, "hipBLASLt must be reachable in a PyTorch process on the GPU"


@pytest.mark.parametrize("k", [384, 2048])
@pytest.mark.parametrize("n", [96, 512])
@pytest.mark.parametrize("m", [64, 320, 1000])
def test_product_with_c_operand_matches_fp32(supported, m, n, k):
    a, w, bias, c = _operands(m, n, k)
    a0, c0 = a.clone(), c.clone()
    st, d = _call(a, w, bias, c)
    assert st == 0, _L().lib.hs_last_error()
    print(f"m={m} n={n} k={k}: resid err {assert_close(d, _reference(a, w, bias, c), RESID_TOL, 'lib resid'):.3e}")
    assert not torch.equal(d, c) and torch.equal(c, c0) and torch.equal(a, a0)
    st, d0 = _call(a, w, bias, None)  # C = NULL: the plain product
    assert st == 0, _L().lib.hs_last_error()
    print(f"m={m} n={n} k={k}: plain err {assert_close(d0, _reference(a, w, bias, None), RESID_TOL, 'lib plain'):.3e}")
    st, d1 = _call(a, w, None, c)     # no bias
    assert st == 0, _L().lib.hs_last_error()
    assert_close(d1, (a.float() @ w.float().t() + c.float()).to(torch.bfloat16), RESID_TOL, "lib resid, no bias")


def test_refusals(supported):
    from heal_swin_amd import ops
    L = _L()
    a, w, bias, c = _operands(64, 96, 384)
    for d, what in ((c, "d is c"), (a.view(-1)[:64 * 96].view(64, 96), "d overlaps a"), (w.view(-1)[:64 * 96].view(64, 96), "d overlaps w")):
        st, _ = _call(a, w, bias, c, d=d)
        assert st == 1 and "alias" in L.lib.hs_last_error().decode(), what
    assert torch.equal(c, _operands(64, 96, 384)[3])  # nothing was launched
    d = torch.empty((64, 96), dtype=torch.bfloat16, device=DEV)
    P = L.ptr
    for args, what in (((None, P(w), P(bias), L.HS_BF16, P(c), P(d), 64, 96, 384), "a NULL"), ((P(a), None, P(bias), L.HS_BF16, P(c), P(d), 64, 96, 384), "w NULL"),
                       ((P(a), P(w), P(bias), L.HS_BF16, P(c), None, 64, 96, 384), "d NULL"), ((P(a), P(w), P(bias), L.HS_BF16, P(c), P(d), 64, 92, 384), "n % 8"),
                       ((P(a), P(w), P(bias), L.HS_BF16, P(c), P(d), 64, 96, 380), "k % 8"), ((P(a), P(w), P(bias), 7, P(c), P(d), 64, 96, 384), "bias dtype"),
                       ((P(a), P(w), P(bias), L.HS_BF16, P(c), P(d), 0, 96, 384), "m = 0")):
        assert L.lib.hs_lib_gemm_nt(*args, L.stream_ptr(a.device)) == 1, what
    off = ctypes.c_void_p(a.data_ptr() + 2)
    assert L.lib.hs_lib_gemm_nt(off, P(w), P(bias), L.HS_BF16, P(c), P(d), 32, 96, 384, L.stream_ptr(a.device)) == 5  # misaligned
    # non-contiguous operands never reach the entry point as they are: the op layer hands over contiguous copies
    wide = torch.randn(64, 2 * 384, device=DEV).to(torch.bfloat16)
    y = ops.lib_gemm_nt(wide[:, :384], w, bias, c.t().contiguous().t())
    assert_close(y, _reference(wide[:, :384], w, bias, c), RESID_TOL, "strided operands")
    # an unreachable library: supported() says 0, the entry point returns HS_ERR_UNSUPPORTED, the policy keeps the deferred add
    try:
        L.lib.hs_lib_gemm_set_supported(0)
        assert L.lib.hs_lib_gemm_supported() == 0 and _call(a, w, bias, c)[0] == 2
        assert not ops.lib_resid_ok(96, 384, torch.bfloat16) and ops.lib_gemm_nt(a, w, bias, c) is None
        y = ops.gemm._lib_linear_resid(a, w, bias, c)  # ... and hs_gemm_nt's residual epilogue answers a call already under way
        assert_close(y, _reference(a, w, bias, c), RESID_TOL, "fallback")
    finally:
        L.lib.hs_lib_gemm_set_supported(1)
    assert L.lib.hs_lib_gemm_supported() == 1 and ops.lib_resid_ok(96, 384, torch.bfloat16)
    assert not ops.lib_resid_ok(96, 384, torch.float32) and not ops.lib_resid_ok(92, 384, torch.bfloat16)
    # nothing stochastic on the branch, no compensated residual stream: the block asks ops.resid_site for neither
    from heal_swin_amd.models_torch import swin_hp_transformer as M
    x = torch.zeros(2, 512, 96, device=DEV, dtype=torch.bfloat16)
    plain = M.SwinTransformerBlock(96, 512, 8, 3, window_size=64).train()
    assert plain._resid_sites(x, None, False) is not None
    assert M.SwinTransformerBlock(96, 512, 8, 3, window_size=64, drop_path=0.1).train()._resid_sites(x, None, False) is None
    assert plain._resid_sites(x, None, True) is None and plain._resid_sites(x, x, False) is None


def test_pick_is_stable_and_every_candidate_can_be_pinned(supported):
    from heal_swin_amd import ops
    m, n, k = 1000, 512, 1032  # a class no other test uses
    a, w, bias, c = _operands(m, n, k)
    ref = _reference(a, w, bias, c)
    ops.lib_gemm_set_pick(m, n, k, True, -1)
    assert ops.lib_gemm_pick(m, n, k, True)[0] == -1
    st, d = _call(a, w, bias, c)
    assert st == 0
    first = ops.lib_gemm_pick(m, n, k, True)
    assert first[0] >= 0 and first[1] >= 0 and "solution" in first[2]
    for _ in range(3):
        st, d2 = _call(a, w, bias, c)
        assert st == 0 and ops.lib_gemm_pick(m, n, k, True) == first and torch.equal(d, d2)
    assert ops.lib_gemm_pick(m - 100, n, k, True) == first  # same power-of-two bucket of rows
    assert ops.lib_gemm_pick(m, n, k, False)[0] == -1       # the plain product is a class of its own
    try:
        for index in range(8):
            ops.lib_gemm_set_pick(m, n, k, True, index)
            st, d = _call(a, w, bias, c)
            assert st == 0, (index, _L().lib.hs_last_error())
            got = ops.lib_gemm_pick(m, n, k, True)
            print(f"pinned {index}: {got[2]}, err {assert_close(d, ref, RESID_TOL, f'pinned candidate {index}'):.3e}")
            assert "pinned" in got[2]
        assert _L().lib.hs_lib_gemm_set_pick(m, n, k, 1, 8) == 1 and _L().lib.hs_lib_gemm_set_pick(m, n, k, 1, -2) == 1
    finally:
        ops.lib_gemm_set_pick(m, n, k, True, -1)


def test_a_class_first_met_inside_a_capture_runs_untimed_and_is_not_remembered(supported):
    from heal_swin_amd import ops
    m, n, k = 320, 96, 776  # a class no other test uses
    a, w, bias, c = _operands(m, n, k)
    ops.lib_gemm_set_pick(m, n, k, True, -1)
    d = torch.zeros((m, n), dtype=torch.bfloat16, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st, _ = _call(a, w, bias, c, d=d)
    assert st == 0, _L().lib.hs_last_error()
    assert ops.lib_gemm_pick(m, n, k, True)[0] == -1  # no trial ran, nothing was cached as tuned
    graph.replay()
    torch.cuda.synchronize()
    assert_close(d, _reference(a, w, bias, c), RESID_TOL, "captured call")
    st, d2 = _call(a, w, bias, c)  # the first EAGER call still gets its trial
    assert st == 0 and ops.lib_gemm_pick(m, n, k, True)[0] >= 0
    assert_close(d2, _reference(a, w, bias, c), RESID_TOL, "eager call after the capture")


class _NormSpy:
    """Passes every call of ops.norm's `lib` on and counts the LayerNorm forwards by form: hs_layernorm_fwd_ex's third pointer is the
    tensor added in front of the norm (the fused add + LayerNorm) or NULL (the plain LayerNorm)."""

    def __init__(self, real):
        self.real, self.add, self.plain = real, 0, 0

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name != "hs_layernorm_fwd_ex":
            return fn

        def wrap(*args):
            if args[2] is None:
                self.plain += 1
            else:
                self.add += 1
            return fn(*args)
        return wrap


def _force_library(monkeypatch):
    """GEMM_TUNE off and own_gemm_ok false for the bias / residual products: fc2 (and proj) run in the library."""
    from heal_swin_amd import ops
    L = _L()
    real = ops.own_gemm_ok
    monkeypatch.setattr(ops, "GEMM_TUNE", False)
    monkeypatch.setattr(ops, "own_gemm_ok", lambda epi, *a, **kw: False if epi == L.HS_EPI_BIAS else real(epi, *a, **kw))


def test_block_pair_add_on_the_library_product(supported, monkeypatch):
    from heal_swin_amd import ops
    from heal_swin_amd.models_torch import swin_hp_transformer as M
    _force_library(monkeypatch)
    torch.manual_seed(5)
    blocks = [M.SwinTransformerBlock(256, 512, 8, 8, window_size=16, shift_size=shift, shift_strategy="nest_roll", rel_pos_bias="flat").to(DEV).train()
              for shift in (0, 8)]
    g = torch.Generator().manual_seed(6)
    x0 = torch.randn(2, 512, 256, generator=g).to(DEV)
    dy = torch.randn(2, 512, 256, generator=g).to(DEV).to(torch.bfloat16)
    results = {}
    for on in (False, True):
        monkeypatch.setattr(ops, "LIB_RESID", on)
        spy = _NormSpy(_L().lib)
        monkeypatch.setattr(ops.norm, "lib", spy)
        calls0 = ops.LIB_GEMM_CALLS[0]
        for b in blocks:
            b.zero_grad(set_to_none=True)
        x = x0.to(torch.bfloat16).requires_grad_(True)
        h, pending = x, None
        for b in blocks:
            assert b.can_defer()
            h, pending, _ = b.forward_deferred(h, pending)
        if on:
            assert pending is None  # both adds rode on fc2
        y = M.SwinTransformerBlock.resolve_pending(h, pending)
        y.backward(dy)
        grads = {f"{i}.{k}": p.grad.detach().clone() for i, b in enumerate(blocks) for k, p in b.named_parameters() if p.grad is not None}
        results[on] = (y.detach().clone(), x.grad.detach().clone(), grads, spy.add, spy.plain, ops.LIB_GEMM_CALLS[0] - calls0)
    (ya, dxa, ga, add_a, plain_a, lib_a), (yb, dxb, gb, add_b, plain_b, lib_b) = results[False], results[True]
    # off: norm1 of block 0 is plain, the other three norms carry an add; on: fc2's add left the second block's norm1, which is plain too
    assert (add_a, plain_a, lib_a) == (3, 1, 0) and (add_b, plain_b, lib_b) == (2, 2, 2), (results[False][3:], results[True][3:])
    print(f"y err {assert_close(yb, ya, TOL[torch.bfloat16], 'block pair y'):.3e}")
    print(f"dx err {assert_close(dxb, dxa, GRAD_TOL[torch.bfloat16], 'block pair dx'):.3e}")
    assert set(ga) == set(gb) and len(ga) >= 20
    for k in ga:
        print(f"grad {k}: {assert_close(gb[k], ga[k], GRAD_TOL[torch.bfloat16], 'block pair grad ' + k):.3e}")
        assert_unbiased(gb[k], ga[k], "block pair grad " + k)


def test_graphed_step_replays_the_library_product(supported, monkeypatch):
    """The `tiny` workload's model, every bias / residual product forced to the library, LIB_RESID on: three replays of the captured
    step give the losses and parameters of three eager steps, bit for bit (the bound of tests/test_gpu_graphs.py)."""
    from heal_swin_amd import ops
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.graphs import GraphedTrainStep
    from heal_swin_amd.losses import seg_loss
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys
    _force_library(monkeypatch)
    monkeypatch.setattr(ops, "LIB_RESID", True)
    cfg = dict(patch_size=4, window_size=16, shift_size=8, shift_strategy="nest_roll", rel_pos_bias="flat", embed_dim=48, depths=[2, 2, 2],
               num_heads=[3, 6, 12], mlp_ratio=4.0, qkv_bias=True, qk_scale=None, use_cos_attn=False, drop_rate=0.0, attn_drop_rate=0.0,
               drop_path_rate=0.0, use_v2_norm_placement=False, ape=False)
    spec = dict(dim_in=4 * 32 * 32, f_in=3, f_out=12, base_pix=4, class_names=[])
    g = torch.Generator(device=DEV).manual_seed(7)
    data = [(torch.randint(0, 256, (2, 3, spec["dim_in"]), generator=g, device=DEV, dtype=torch.uint8),
             torch.randint(0, spec["f_out"], (2, spec["dim_in"]), generator=g, device=DEV, dtype=torch.uint8)) for _ in range(4)]
    losses, finals, lib_calls = {}, {}, {}
    for mode in ("graph", "eager"):  # the graph first: its warm-up steps meet every shape class, the capture none
        torch.manual_seed(0)
        model = SwinHPTransformerSys(SwinHPTransformerConfig(**cfg), DataSpec(**spec)).cuda().train()
        model.compute_dtype = torch.bfloat16
        # window 16 with 16-wide heads runs the generic attention backward, which sums the bias gradient with float atomics (the one
        # order-dependent sum of the step, eager or replayed): the tables are not trained here, every other parameter is bit-exact
        for name, p in model.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.requires_grad_(False)
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3, fused=True, capturable=True)
        calls0, out = ops.LIB_GEMM_CALLS[0], []
        if mode == "graph":
            step = GraphedTrainStep(model, seg_loss, opt, data[0][0], data[0][1], warmup=2, pre_forward=lambda x: x.float())
            lib_calls[mode] = (ops.LIB_GEMM_CALLS[0] - calls0) // 3  # two warm-up steps and the capture
            rows = 2 * spec["dim_in"] // cfg["patch_size"]
            assert ops.lib_gemm_pick(rows, 48, 192, True)[0] >= 0  # stage 0's fc2: chosen during the warm-up, before the capture
            for x, y in data[1:]:
                out.append(float(step(x, y)))
        else:
            def eager(x, y):
                opt.zero_grad(set_to_none=False)
                loss = seg_loss(model(x.float()), y)
                loss.backward()
                opt.step()
                return float(loss.detach())
            for _ in range(2):
                eager(*data[0])
            lib_calls[mode] = (ops.LIB_GEMM_CALLS[0] - calls0) // 2
            for x, y in data[1:]:
                out.append(eager(x, y))
        losses[mode] = out
        finals[mode] = {k: v.detach().clone() for k, v in model.named_parameters()}
    assert lib_calls["graph"] == lib_calls["eager"] and lib_calls["eager"] >= 6, lib_calls
    assert losses["eager"] == losses["graph"], (losses["eager"], losses["graph"])
    for k, v in finals["eager"].items():
        assert torch.equal(v, finals["graph"][k]), k
