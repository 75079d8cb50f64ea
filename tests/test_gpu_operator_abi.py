"""The three operator-level backward entry points of INTEGRATION.md -- hs_patch_merge_bwd, hs_patch_expand_bwd and
hs_window_attn_module_bwd_chain -- through `lib.*`, in every way a caller may use them: overwrite and accumulate, micro-batches
through one workspace, the workspace extent, and the two kinds of refusal (a deferring `accumulate`, a shape one of the chained
kernels does not take), each of which must leave every buffer of the caller untouched.

References.  Patch operators: the operation written plainly in torch, fp64 on the CPU, from the bf16-rounded inputs, gradients
from autograd.  Attention chain: the Python mirror's recorded autograd nodes (tests/_attn_chain.py), as in
tests/test_gpu_attn_module.py.

The bound of the accumulate test (derived from the reducers, not from their output).  With accumulate = 1 the kernels that end a
gradient add the caller's value P to the same partial records, in the same order, as the accumulate = 0 run that gave g0:
  * reduce_many_kernel (csrc/reduce_many.hip: dw, dgamma / dbeta of widths % 4 == 0, the Linear biases): the records are summed
    into `acc` first -- bit for bit the g0 of the overwriting run -- and P is added LAST: `acc += o`.  result = fl(g0 + P).
  * layernorm_param_reduce_kernel (csrc/layernorm.hip: widths % 4 != 0): `*dst = accumulate ? *dst + tot : tot`, tot = g0.  Same.
  * reduce_scale_partials_kernel (csrc/window_attn_mfma.hip: dhead_scale): `dst[h] = overwrite ? acc : dst[h] + acc`.  Same.
  One rounding of the exact g0 + P:  |result - (P + g0)| <= 2^-24 |P + g0| <= 2^-24 (|P| + |g0|), and |g0| <= sum |partials|.
  * reduce_partials_kernel (dbias of the attention core) starts FROM P: `t = overwrite ? 0 : dst; t += part_s[0..15]`, part_s[w]
    being wave w's in-order sum of the slots w, w + 16, ...  Against the overwriting run P sits at the other end of the same
    sequence: each run rounds at most 16 + ceil(slots / 16) times, every rounding by at most 2^-24 of a partial sum that is at
    most |P| + S, S = sum over the slots of |partial|.  So |result - (P + g0)| <= 2 (16 + ceil(slots / 16)) 2^-24 (|P| + S) / (1 - 64 2^-24).
    A slot's partial is the sum over its windows of dS = P~ (dP - sum_j P~ dP), P~ the softmax row (0 <= P~ <= 1, sum 1) and
    dP_ij = dO_i . V_j over the head's 32 channels, so |dS_ij| <= 2 max_j |dP_ij| <= 2 |dO_i| |V_j| and
    S <= windows * 2 max_i |dO_i,h| max_j |V_j,h| (1.05: dO and P~ are bf16 inside the kernel, 2^-8 each), with dO = dout W_proj
    formed here in fp64 and V read from the saved qkv.
"""
import math

import pytest
import torch

from _util import GRAD_TOL, TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
U = 2.0 ** -24  # unit roundoff of fp32
GUARD = 4096
HS_ERR_INVALID_ARG, HS_ERR_UNSUPPORTED = 1, 2
WORST = {}  # operator -> worst observed |result - (P + g0)| / bound of the accumulate test (printed by it)


def _bits(t):
    return t.detach().clone().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, snapshot):
    return torch.equal(a.view(snapshot.dtype), snapshot)


# --------------------------------------------------------------------------------------------------------------- the three operators
class PatchCase:
    """One patch operator at one shape: inputs from a seed, the C-ABI forward, the fp64 reference, and the backward as a status."""

    def __init__(self, kind, shape, seed=0):
        self.kind, self.shape = kind, shape
        g = torch.Generator().manual_seed(1000 * seed + sum(shape))
        bf = lambda t: t.to(BF)  # noqa: E731
        if kind == "merge":
            rows, dim, dim_out = shape
            self.rows, self.k_x, self.n_w, self.k_w, self.width, self.ln_rows = rows, 4 * dim, dim_out, 4 * dim, 4 * dim, rows
            self.n_out = dim_out
        else:
            rows, dim, dim_exp, children = shape
            self.rows, self.k_x, self.n_w, self.k_w, self.width, self.ln_rows = rows, dim, dim_exp, dim, dim_exp // children, rows * children
            self.n_out = dim_exp
        self.x = bf(torch.randn(self.rows, self.k_x, generator=g) * 1.5 + 0.3)
        self.w = bf(torch.randn(self.n_w, self.k_w, generator=g) * self.k_w ** -0.5)
        self.gamma = torch.rand(self.width, generator=g) + 0.5
        self.beta = torch.randn(self.width, generator=g) * 0.2
        out_shape = (self.rows, self.n_out) if kind == "merge" else (self.ln_rows, self.width)
        self.dout = bf(torch.randn(*out_shape, generator=g))
        self._ref = None
        self._fwd = None

    keys = ("dw", "dgamma", "dbeta")

    def reference(self):
        """(y, dx, {dw, dgamma, dbeta}) in fp64 on the CPU."""
        if self._ref is None:
            x, w = self.x.double().requires_grad_(True), self.w.double().requires_grad_(True)
            ga, be = self.gamma.double().requires_grad_(True), self.beta.double().requires_grad_(True)
            ln = lambda t: torch.nn.functional.layer_norm(t, (self.width,), ga, be, 1e-5)  # noqa: E731
            y = ln(x) @ w.t() if self.kind == "merge" else ln((x @ w.t()).view(self.ln_rows, self.width))
            y.backward(self.dout.double())
            self._ref = (y.detach(), x.grad, dict(dw=w.grad, dgamma=ga.grad, dbeta=be.grad))
        return self._ref

    def forward(self):
        """The C-ABI forward; keeps what the backward reads.  Returns its output."""
        from heal_swin_amd import _lib
        from heal_swin_amd._lib import check, lib, ptr
        if self._fwd is None:
            d = lambda t: t.to(DEV).contiguous()  # noqa: E731
            s = self.s = dict(x=d(self.x), w=d(self.w), w_t=d(self.w.t()), gamma=d(self.gamma), beta=d(self.beta), dout=d(self.dout))
            s["mean"], s["rstd"] = torch.empty(self.ln_rows, device=DEV), torch.empty(self.ln_rows, device=DEV)
            out = torch.empty_like(s["dout"])
            if self.kind == "merge":
                rows, dim, dim_out = self.shape
                s["mid"] = torch.empty(rows, 4 * dim, dtype=BF, device=DEV)
                check(lib.hs_patch_merge_fwd(ptr(s["x"]), ptr(s["gamma"]), ptr(s["beta"]), ptr(s["w"]), ptr(s["mid"]), ptr(s["mean"]), ptr(s["rstd"]),
                                             ptr(out), rows, dim, dim_out, _lib.HS_BF16, None), "hs_patch_merge_fwd")
            else:
                rows, dim, dim_exp, children = self.shape
                s["mid"] = torch.empty(rows, dim_exp, dtype=BF, device=DEV)
                check(lib.hs_patch_expand_fwd(ptr(s["x"]), ptr(s["w"]), ptr(s["gamma"]), ptr(s["beta"]), ptr(s["mid"]), ptr(s["mean"]), ptr(s["rstd"]),
                                              ptr(out), rows, dim, dim_exp, children, _lib.HS_BF16, None), "hs_patch_expand_fwd")
            self._fwd = out
        return self._fwd

    def ws_floats(self):
        from heal_swin_amd._lib import lib
        if self.kind == "merge":
            return int(lib.hs_patch_merge_bwd_workspace(*self.shape))
        return int(lib.hs_patch_expand_bwd_workspace(*self.shape))

    def check_ws_size(self, n):
        """the size is the largest of the chained kernels' own (they take turns)"""
        from heal_swin_amd._lib import lib
        parts = (int(lib.hs_layernorm_bwd_workspace(self.ln_rows, self.width)), int(lib.hs_linear_wgrad_workspace(self.rows, self.n_w, self.k_w)))
        assert n > 0 and n == max(parts) and min(parts) > 0, (n, parts)

    def buffers(self):
        """(dx, {gradient buffers}, [scratch the call also writes]) as torch.empty"""
        self.forward()
        G = dict(dw=torch.empty(self.n_w, self.k_w, device=DEV), dgamma=torch.empty(self.width, device=DEV), dbeta=torch.empty(self.width, device=DEV))
        return torch.empty_like(self.s["x"]), G, [torch.empty_like(self.s["mid"])]

    def backward(self, dx, G, scratch, ws, accumulate):
        from heal_swin_amd import _lib
        from heal_swin_amd._lib import lib, ptr
        s = self.s
        fn = lib.hs_patch_merge_bwd if self.kind == "merge" else lib.hs_patch_expand_bwd
        return fn(ptr(s["dout"]), ptr(s["x"]), ptr(s["mid"]), ptr(s["gamma"]), ptr(s["mean"]), ptr(s["rstd"]), ptr(s["w_t"]), ptr(scratch[0]), ptr(dx),
                  ptr(G["dw"]), ptr(G["dgamma"]), ptr(G["dbeta"]), ptr(ws), accumulate, *self.shape, _lib.HS_BF16, None)

    def accumulate_bound(self, key, P, g0):
        return U * (P.abs() + g0.abs()) + 2.0 ** -149  # P enters last: one rounding (module docstring)


class ChainCase:
    """hs_window_attn_module_bwd_chain at one configuration, behind the same interface."""

    def __init__(self, cfg, seed=0):
        from _attn_chain import chain_inputs
        C, v1, use_bias, cosine, strategy = cfg
        self.c = chain_inputs(v1, cosine, strategy, B=1, nside=8, C=C, nH=C // 32, use_bias=use_bias, seed=40 + seed)
        self._ref = None
        self._fwd = None
        # head_scale is a parameter of cosine attention only (:144-147); without it dhead_scale is not produced (hs_window_attn_bwd)
        self.keys = tuple(k for k in self.c.P if not (k == "hs" and not cosine))

    def reference(self):
        from _attn_chain import chain_autograd
        if self._ref is None:
            y, dx, D = chain_autograd(self.c)
            self._ref = (y, dx, {k: D[k] for k in self.keys})
        return self._ref

    def forward(self):
        from _attn_chain import chain_forward
        if self._fwd is None:
            self._fwd = chain_forward(self.c)
        return self._fwd

    def ws_floats(self):
        from _attn_chain import chain_workspace_floats
        return chain_workspace_floats(self.c)

    def check_ws_size(self, n):
        """three bf16 activation buffers, rounded up to whole float4s, in front of the largest of the chained kernels' own"""
        from heal_swin_amd import _lib
        from heal_swin_amd._lib import lib
        c = self.c
        M = c.B * c.N
        parts = (int(lib.hs_window_attn_bwd_workspace(c.B, c.N, c.C, c.nH, 64, _lib.HS_BF16)), int(lib.hs_linear_wgrad_workspace(M, 3 * c.C, c.C)),
                 int(lib.hs_linear_wgrad_workspace(M, c.C, c.C)), int(lib.hs_layernorm_bwd_workspace(M, c.C)))
        front = n - max(parts)
        assert n > 0 and min(parts) > 0 and front % 4 == 0 and 2 * front >= 5 * M * c.C, (n, parts)

    def buffers(self):
        from _attn_chain import chain_grad_buffers
        self.forward()
        dx, G = chain_grad_buffers(self.c)
        return dx, G, []

    def backward(self, dx, G, scratch, ws, accumulate, **kw):
        from _attn_chain import chain_backward
        return chain_backward(self.c, dx, G, ws, accumulate, **kw)

    def accumulate_bound(self, key, P, g0):
        if key != "bias":
            return U * (P.abs() + g0.abs()) + 2.0 ** -149  # P enters last: one rounding
        c = self.c
        windows = c.B * c.N // 64  # one slot per window at these sizes (slots = min(resident, windows), resident >= 8)
        assert windows <= 8
        d_o = (c.dout.double().view(-1, c.C) @ c.P["wp"].to(BF).double()).view(-1, c.nH, 32)
        v = c.qkv.double().view(-1, 3, c.nH, 32)[:, 2]
        S = windows * 2 * 1.05 * d_o.norm(dim=-1).amax(0) * v.norm(dim=-1).amax(0)  # [nH]
        n_round = 2 * (16 + math.ceil(windows / 16))
        return n_round * U / (1 - 64 * U) * (P.abs() + S.view(-1, 1, 1))


MERGE_SHAPES = [(64, 32, 64), (257, 24, 48), (3, 8, 16)]
EXPAND_SHAPES = [(64, 64, 128, 4), (129, 32, 512, 16), (5, 8, 24, 4)]
CHAIN_CFGS = [  # C, v1 (LayerNorm in front + residual behind; False: v2 placement), relative bias, cosine, shift strategy
    (128, True, True, False, "nest_roll"), (96, True, True, True, "ring_shift"), (128, True, False, True, "nest_grid_shift"),
    (96, True, False, False, "none"), (96, False, True, False, "nest_roll"), (128, False, True, True, "ring_shift"),
    (96, False, False, True, "nest_grid_shift"), (128, False, False, False, "none")]
OPS = ([("merge", s) for s in MERGE_SHAPES] + [("expand", s) for s in EXPAND_SHAPES] + [("chain", c) for c in CHAIN_CFGS])
_CASES = {}


def case(op, seed=0):
    """Cases are built once (inputs, forward, reference) and shared by the tests; nothing below changes them."""
    if (op, seed) not in _CASES:
        _CASES[(op, seed)] = ChainCase(op[1], seed) if op[0] == "chain" else PatchCase(op[0], op[1], seed)
    return _CASES[(op, seed)]


def _id(op):
    return op[0] + "-" + "-".join(str(v) for v in op[1])


def _ok(status, what):
    from heal_swin_amd._lib import check
    check(status, what)


def _run0(cs):
    """The accumulate = 0 result on buffers pre-filled with NaN: (dx, G), computed once per case."""
    if not hasattr(cs, "_g0"):
        dx, G, scratch = cs.buffers()
        for t in [dx, *G.values(), *scratch]:
            t.fill_(float("nan"))
        ws = torch.full((cs.ws_floats(),), float("nan"), device=DEV)
        _ok(cs.backward(dx, G, scratch, ws, 0), "accumulate = 0")
        cs._g0 = (dx, G)
    return cs._g0


# ------------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("op", OPS, ids=_id)
def test_forward_and_overwrite_really_overwrites(op):
    """accumulate = 0 on NaN-filled outputs (and a NaN-filled workspace): no NaN survives, every gradient matches the reference."""
    cs = case(op)
    y_ref, dx_ref, G_ref = cs.reference()
    if op[0] == "chain":
        assert torch.equal(cs.forward(), y_ref)
    else:
        assert_close(cs.forward(), y_ref, TOL[BF], _id(op) + " y")
    dx, G = _run0(cs)
    assert not torch.isnan(dx.float()).any(), "dx keeps a NaN of its pre-fill"
    assert_close(dx, dx_ref, GRAD_TOL[BF], _id(op) + " dx")
    assert set(cs.keys) <= set(G)
    for k in cs.keys:
        assert not torch.isnan(G[k]).any(), f"{k} keeps a NaN of its pre-fill: not every element is overwritten"
        assert_close(G[k], G_ref[k], GRAD_TOL[BF], f"{_id(op)} {k}")
    for k in set(G) - set(cs.keys):  # dhead_scale without cosine attention: not a gradient of this call, left alone
        assert torch.isnan(G[k]).all()


@pytest.mark.parametrize("op", OPS, ids=_id)
def test_accumulate_adds_exactly_once(op):
    """accumulate = 1 on buffers holding a random P of the gradient's magnitude: P + g0 to the rounding of the reducers (module
    docstring), dx bit-equal to the overwriting run."""
    cs = case(op)
    dx0, G0 = _run0(cs)
    dx, G, scratch = cs.buffers()
    g = torch.Generator(device=DEV).manual_seed(77)
    Ps = {}
    for k in G:
        scale = float(G0[k].abs().max()) if k in cs.keys else 1.0
        Ps[k] = torch.randn(G[k].shape, generator=g, device=DEV) * max(scale, 1e-3)
        G[k].copy_(Ps[k])
    dx.fill_(float("nan"))
    ws = torch.empty(cs.ws_floats(), device=DEV)
    _ok(cs.backward(dx, G, scratch, ws, 1), "accumulate = 1")
    assert torch.equal(dx.view(torch.int16), dx0.view(torch.int16)), "dx depends on accumulate"
    worst = 0.0
    for k in cs.keys:
        want = Ps[k].double() + G0[k].double()
        bound = cs.accumulate_bound(k, Ps[k].double(), G0[k].double())
        ratio = float(((G[k].double() - want).abs() / bound).max())
        print(f"{_id(op)} {k}: worst |result - (P + g0)| / bound = {ratio:.3f} (largest bound {float(bound.max()):.3e}, scale {float(want.abs().max()):.3e})")
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{k}: accumulate = 1 is not P + g0: {ratio:.3g} times the rounding bound"
    for k in set(G) - set(cs.keys):
        assert torch.equal(G[k], Ps[k])
    WORST[op[0]] = max(WORST.get(op[0], 0.0), worst)
    print(f"worst ratio so far: {WORST}")


@pytest.mark.parametrize("op", OPS, ids=_id)
def test_micro_batches_through_one_workspace(op):
    """Two different inputs, accumulate = 0 then 1 into the same gradient buffers through the same workspace, back to back on one
    stream: the sum of the two references."""
    a, b = case(op), case(op, seed=1)
    dx, G, scratch = a.buffers()
    b.forward()
    for t in G.values():
        t.fill_(float("nan"))
    ws = torch.empty(a.ws_floats(), device=DEV)
    _ok(a.backward(dx, G, scratch, ws, 0), "first micro-batch")
    _ok(b.backward(dx, G, scratch, ws, 1), "second micro-batch")
    (_, _, Ga), (_, dxb, Gb) = a.reference(), b.reference()
    assert_close(dx, dxb, GRAD_TOL[BF], _id(op) + " dx of the second micro-batch")
    for k in a.keys:
        assert_close(G[k], Ga[k].double().cpu() + Gb[k].double().cpu(), GRAD_TOL[BF], f"{_id(op)} summed {k}")


@pytest.mark.parametrize("op", OPS, ids=_id)
def test_workspace_size_is_enough_and_not_exceeded(op):
    """The call gets exactly *_bwd_workspace floats at the front of a larger tensor; the 4096 floats behind them keep their bits and
    the result is that of a roomy call."""
    cs = case(op)
    dx0, G0 = _run0(cs)
    n = cs.ws_floats()
    cs.check_ws_size(n)
    ws = torch.empty(n + GUARD, device=DEV)
    ws.view(torch.int32)[n:] = 0x5A5AC3C3
    ws[:n] = float("nan")
    dx, G, scratch = cs.buffers()
    for accumulate in (0, 1):
        if accumulate:
            for k in G:
                G[k].zero_()
        _ok(cs.backward(dx, G, scratch, ws, accumulate), f"accumulate = {accumulate}")
        assert bool((ws.view(torch.int32)[n:] == 0x5A5AC3C3).all()), "the call wrote past the workspace size it asked for"
        assert torch.equal(dx.view(torch.int16), dx0.view(torch.int16))
        for k in cs.keys:  # (0 + g0 is exact)
            assert torch.equal(G[k], G0[k]), k


@pytest.mark.parametrize("accumulate", [2, 3])
@pytest.mark.parametrize("op", [OPS[1], OPS[5], OPS[6], OPS[12]], ids=_id)
def test_a_deferring_flag_is_refused_and_changes_nothing(op, accumulate):
    """HS_ACC_DEFER (2, 3): the chained kernels share one workspace, so the operators refuse it: HS_ERR_INVALID_ARG, nothing queued
    for hs_reduce_flush, every buffer bit-identical."""
    from heal_swin_amd._lib import lib
    cs = case(op)
    dx, G, scratch = cs.buffers()
    ws = torch.empty(cs.ws_floats(), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    everything = [dx, *G.values(), *scratch, ws]
    for t in everything:
        t.copy_(torch.randn(t.shape, generator=g, device=DEV))
    before = [_bits(t) for t in everything]
    pending = lib.hs_reduce_pending(None)
    status = cs.backward(dx, G, scratch, ws, accumulate)
    msg = lib.hs_last_error().decode()
    torch.cuda.synchronize()
    try:
        assert status == HS_ERR_INVALID_ARG, (status, msg)
        assert "HS_ACC_DEFER" in msg and "workspace" in msg, msg
        assert lib.hs_reduce_pending(None) == pending
        for t, b in zip(everything, before):
            assert _same_bits(t, b), "a refused call changed a buffer"
    finally:
        lib.hs_reduce_flush(None)  # (whatever a wrong library queued must not outlive the workspace it points into)
        torch.cuda.synchronize()


# shapes a chained kernel refuses although the first links take them: (kind, shape, what refuses)
REFUSED = [
    ("merge", (16, 6, 12), "hs_gemm_nt of the backward: k = dim_out = 12 is no multiple of 8"),
    ("merge", (4, 1026, 16), "the LayerNorm, last link of the backward: 4 dim = 4104 > 4096"),
    ("expand", (16, 8, 12, 4), "hs_gemm_nt of the backward: k = dim_exp = 12 is no multiple of 8"),
    ("expand", (4, 8, 8240, 8), "the LayerNorm, last link of the forward: width 1030 > 1024 and no multiple of 8"),
]


@pytest.mark.parametrize("kind,shape,why", REFUSED, ids=[r[0] + "-" + "-".join(map(str, r[1])) for r in REFUSED])
def test_a_refused_patch_shape_changes_nothing_in_either_direction(kind, shape, why):
    """Forward and backward refuse the same shapes, with the same status, before anything is launched: every output of either call
    keeps its bits (accumulate 0 and 1)."""
    from heal_swin_amd._lib import lib
    cs = PatchCase(kind, shape)
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    s = cs.s = dict(x=d(cs.x), w=d(cs.w), w_t=d(cs.w.t()), gamma=d(cs.gamma), beta=d(cs.beta), dout=d(cs.dout))
    g = torch.Generator(device=DEV).manual_seed(6)
    rnd = lambda *sh, dt=torch.float32: torch.randn(*sh, generator=g, device=DEV).to(dt)  # noqa: E731
    s["mean"], s["rstd"] = rnd(cs.ln_rows), rnd(cs.ln_rows)
    s["mid"] = rnd(cs.rows, cs.n_out if kind == "expand" else cs.k_x, dt=BF)
    out = rnd(*cs.dout.shape, dt=BF)
    from heal_swin_amd import _lib
    from heal_swin_amd._lib import ptr
    fwd_outs = [s["mid"], s["mean"], s["rstd"], out]
    before = [_bits(t) for t in fwd_outs]
    if kind == "merge":
        st_f = lib.hs_patch_merge_fwd(ptr(s["x"]), ptr(s["gamma"]), ptr(s["beta"]), ptr(s["w"]), ptr(s["mid"]), ptr(s["mean"]), ptr(s["rstd"]), ptr(out),
                                      *shape, _lib.HS_BF16, None)
    else:
        st_f = lib.hs_patch_expand_fwd(ptr(s["x"]), ptr(s["w"]), ptr(s["gamma"]), ptr(s["beta"]), ptr(s["mid"]), ptr(s["mean"]), ptr(s["rstd"]), ptr(out),
                                       *shape, _lib.HS_BF16, None)
    msg_f = lib.hs_last_error().decode()
    torch.cuda.synchronize()
    assert st_f == HS_ERR_UNSUPPORTED, (st_f, msg_f, why)
    for t, b in zip(fwd_outs, before):
        assert _same_bits(t, b), "the refused forward wrote an output"
    cs._fwd = out  # (nothing to run: buffers() only needs the operands on the device)
    dx, G, scratch = cs.buffers()
    ws = torch.empty(cs.ws_floats(), device=DEV)
    everything = [dx, *G.values(), *scratch, ws]
    for t in everything:
        t.copy_(torch.randn(t.shape, generator=g, device=DEV))
    before = [_bits(t) for t in everything]
    for accumulate in (0, 1):
        st_b = cs.backward(dx, G, scratch, ws, accumulate)
        msg_b = lib.hs_last_error().decode()
        torch.cuda.synchronize()
        assert st_b == st_f, (st_b, msg_b, why)  # forward and backward agree on what they accept
        for t, b in zip(everything, before):
            assert _same_bits(t, b), f"the refused backward (accumulate = {accumulate}) changed a buffer"


@pytest.mark.parametrize("kw,why", [(dict(n_tokens=480), "n_tokens is no multiple of the window"), (dict(roll=512), "roll = n_tokens")],
                         ids=["n_tokens-480", "roll-512"])
def test_a_refused_chain_call_changes_nothing(kw, why):
    """What hs_window_attn_bwd -- the third link, behind the proj gradients -- refuses: the forward refuses it too, and the backward
    returns before its first launch (accumulate 0 and 1).  (All buffers are those of the valid 512-token call.)"""
    from heal_swin_amd import _lib
    from heal_swin_amd._lib import lib, ptr
    cs = case(OPS[6])
    c = cs.c
    dx, G, scratch = cs.buffers()
    # the forward on the same arguments
    out = torch.zeros_like(c.x)
    v1, P = c.v1, c.P
    wq16, wp16 = P["wq"].to(BF), P["wp"].to(BF)
    saved = [torch.empty_like(t) for t in (c.xn, c.mean, c.rstd, c.qkv, c.o, c.lse)]
    st_f = lib.hs_window_attn_module_fwd_train(ptr(c.x), ptr(out), *(ptr(t) for t in saved), ptr(wq16), ptr(P["bq"]), ptr(wp16), ptr(P["bp"]), ptr(P["lg"]), ptr(P["lb"]),
                                               ptr(P.get("bias")), ptr(P["hs"]), ptr(c.idx), kw.get("roll", c.roll), ptr(c.labels), None, None, None,
                                               None, None, c.B, kw.get("n_tokens", c.N), c.C, c.nH, 64, c.flags, _lib.HS_BF16, None)
    assert v1 and st_f == HS_ERR_INVALID_ARG, (st_f, lib.hs_last_error().decode(), why)
    assert not out.any()
    ws = torch.empty(cs.ws_floats(), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(8)
    everything = [dx, *G.values(), ws]
    for t in everything:
        t.copy_(torch.randn(t.shape, generator=g, device=DEV))
    before = [_bits(t) for t in everything]
    for accumulate in (0, 1):
        st_b = cs.backward(dx, G, scratch, ws, accumulate, **kw)
        msg = lib.hs_last_error().decode()
        torch.cuda.synchronize()
        assert st_b == st_f, (st_b, msg, why)
        for t, b in zip(everything, before):
            assert _same_bits(t, b), f"the refused backward (accumulate = {accumulate}) changed a buffer"
