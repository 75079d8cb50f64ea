"""Operands that are views into flat buffers at element offsets that miss the kernels' 16-byte operand alignment (what
parallel.GradBucketAllReduce / optim.FlatAdam produced for a heads-3 model before their slots were rounded to 8 elements).

Contract (include/healswin.h, "Pointer alignment"), asserted per entry point, operand and residue, one operand misaligned at a time:
  * the C ABI either returns the correct result or returns HS_ERR_MISALIGNED (a RuntimeError in the binding) BEFORE it launches
    anything -- the outputs, pre-filled with a sentinel, are untouched;
  * the model-facing `ops` route never raises: it computes the correct result at every residue (through an aligned copy);
  * "correct" = the tolerance and the fp32 / fp64 torch reference of the entry point's own test (TOL / GRAD_TOL, or its bound), on
    the operands as rounded to the kernel's input dtype -- never the aligned call alone.  A one-element shift of a random operand is
    an O(1) error, far outside every bound used here.

Covered through the C ABI: hs_gemm_nt, hs_mlp_fused_fwd / _bwd, hs_window_attn_module_fwd, hs_layernorm_bwd (destinations),
hs_linear_wgrad / _ld / _gelu / _group and the deferred sums (hs_reduce_flush), hs_rel_bias_*, hs_cos_head_scale_*,
hs_transpose_many_16, hs_gelu_* (hs_gelu_split3 included), hs_split_bf16x3, hs_residual_drop, hs_adam_step.  hs_window_attn_module_fwd_train / _bwd_chain,
hs_expand_ln_head_ce / _ce_step / _depth_fwd, hs_ln_head_ce_bwd / _depth_bwd (refusal before launch).  Covered through ops (the route
the model takes), forward and backward: linear, layer_norm, add_layer_norm and their _stream forms, window_attn_module and its training
form, ln_head, expand_ln_head and its _ce / _ce_step / depth forms (class weights included), gelu_dropout, residual_drop, the bf16x3
splits of fp32 operands (ops.gemm.split3 / _weight_split), and the
direct deposit into gradient-sink views (Linear / LayerNorm: aligned or refused; position-bias table / logit_scale: any residue)."""
import ctypes

import pytest
import torch

from _util import GRAD_TOL, TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
E_BF16 = [0, 1, 2, 4]  # element offsets: bytes 0, 2, 4, 8
E_F32 = [0, 1, 2]      # bytes 0, 4, 8
SENTINEL = 7.0


def at_offset(t, e):
    """A tensor equal to t inside a larger allocation, e elements behind a 256-byte-aligned base, >= 64 elements of slack on both
    sides (an access rounded down or up to 16 bytes stays inside the allocation)."""
    per = 256 // t.element_size()
    buf = torch.zeros(2 * per + t.numel() + 64, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 256 == 0
    v = buf[per + e:per + e + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (e * t.element_size()) % 16 and per >= 64
    return v


def offsets(t):
    return E_BF16 if t.dtype == BF else E_F32


def _lib():
    from heal_swin_amd import _lib
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def c_call(status, what, outputs=()):
    """True if the entry point ran; False if it refused the pointers -- then nothing may have been written."""
    L = _lib()
    if status == 0:
        return True
    msg = L.lib.hs_last_error().decode()
    assert status == 5 and "aligned" in msg, (what, status, msg)  # HS_ERR_MISALIGNED
    with pytest.raises(RuntimeError, match="aligned"):
        L.check(status, what)
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o == SENTINEL).all()), f"{what}: refused the call but wrote an output"
    return False


def must_run(ran, e, t):
    """Residue 0 is never refused."""
    if (e * t.element_size()) % 16 == 0:
        assert ran, "an aligned call was refused"


# ----------------------------------------------------------------------------- hs_gemm_nt / ops.gemm_nt
GEMM_OPERANDS = ["b", "b2", "bias", "aux"]


def _gemm_case(m, n, k):
    g = torch.Generator().manual_seed(m + n + k)
    t = dict(a=torch.randn(m, k, generator=g).to(BF), b=(torch.randn(n, k, generator=g) * k ** -0.5).to(BF),
             a2=torch.randn(m, k, generator=g).to(BF), b2=(torch.randn(n, k, generator=g) * k ** -0.5).to(BF),
             bias=torch.randn(n, generator=g), aux=torch.randn(m, n, generator=g).to(BF))
    t = {k_: v.to(DEV) for k_, v in t.items()}
    t["ref1"] = t["a"].float() @ t["b"].float().t() + t["bias"]
    t["ref2"] = t["ref1"] + t["a2"].float() @ t["b2"].float().t()
    return t


_GEMM = {}


def _gemm_shared(m, n, k):
    if (m, n, k) not in _GEMM:
        _GEMM[(m, n, k)] = _gemm_case(m, n, k)
    return _GEMM[(m, n, k)]


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("m,n,k", [(256, 128, 64), (300, 132, 96)])
@pytest.mark.parametrize("operand", GEMM_OPERANDS)
def test_gemm_nt_operands_at_every_residue(m, n, k, tile, operand):
    L = _lib()
    lib, ptr = L.lib, L.ptr
    from heal_swin_amd import ops
    t = _gemm_shared(m, n, k)
    gelu = torch.nn.functional.gelu
    lib.hs_gemm_nt_set_tile(tile)
    try:
        for e in offsets(t[operand]):
            o = dict(t)
            o[operand] = at_offset(t[operand], e)
            two = operand == "b2"
            ref = t["ref2"] if two else t["ref1"]
            for epi, want in ((L.HS_EPI_BIAS, ref), (L.HS_EPI_GELU, gelu(ref)), (L.HS_EPI_RESID, ref + t["aux"].float())):
                if operand == "aux" and epi != L.HS_EPI_RESID:
                    continue  # (aux is an input of the residual epilogue only)
                c = torch.full((m, n), SENTINEL, dtype=BF, device=DEV)
                act = torch.full((m, n), SENTINEL, dtype=BF, device=DEV) if epi == L.HS_EPI_GELU else o["aux"]
                st = lib.hs_gemm_nt(ptr(o["a"]), k, ptr(o["b"]), k, k, ptr(o["a2"] if two else None), k if two else 0,
                                    ptr(o["b2"] if two else None), k if two else 0, k if two else 0, ptr(o["bias"]), ptr(c), ptr(act), m, n,
                                    epi, 0.0, 0, L.HS_BF16, _stream())
                tag = f"hs_gemm_nt tile {tile} epi {epi} {operand}+{e}"
                ran = c_call(st, tag, [c] + ([act] if epi == L.HS_EPI_GELU else []))
                must_run(ran, e, t[operand])
                if ran:
                    assert_close(act if epi == L.HS_EPI_GELU else c, want, 6e-3, tag)
                # the wrapper the model calls takes any residue
                c2, act2 = ops.gemm_nt(o["a"], o["b"], o["bias"], epi, aux=o["aux"] if epi == L.HS_EPI_RESID else None,
                                       a2=o["a2"] if two else None, w2=o["b2"] if two else None)
                assert_close(act2 if epi == L.HS_EPI_GELU else c2, want, 6e-3, "ops " + tag)
    finally:
        lib.hs_gemm_nt_set_tile(0)


@pytest.mark.parametrize("operand", ["weight", "bias"])
def test_ops_linear_with_parameters_at_every_residue(operand):
    """ops.linear forward and backward with an fp32 master weight / bias that is a view at an odd offset."""
    from heal_swin_amd import ops
    m, n, k = 300, 132, 96
    g = torch.Generator().manual_seed(9)
    x = torch.randn(m, k, generator=g).to(BF).to(DEV)
    w0 = (torch.randn(n, k, generator=g) * k ** -0.5).to(BF).float().to(DEV)
    b0 = torch.randn(n, generator=g).to(DEV)
    dy = torch.randn(m, n, generator=g).to(BF).to(DEV)
    xr = x.float().requires_grad_(True)
    wr, br = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    ref = torch.nn.functional.linear(xr, wr, br)
    ref.backward(dy.float())
    for e in E_F32:
        w = (at_offset(w0, e) if operand == "weight" else w0.clone()).requires_grad_(True)
        b = (at_offset(b0, e) if operand == "bias" else b0.clone()).requires_grad_(True)
        xq = x.clone().requires_grad_(True)
        y = ops.linear(xq, w, b)
        y.backward(dy)
        tag = f"ops.linear {operand}+{e}"
        assert_close(y, ref, TOL[BF], tag + " y")
        assert_close(xq.grad, xr.grad, GRAD_TOL[BF], tag + " dx")
        assert_close(w.grad, wr.grad, GRAD_TOL[BF], tag + " dW")
        assert_close(b.grad, br.grad, GRAD_TOL[BF], tag + " db")


# ----------------------------------------------------------------------------- hs_mlp_fused_fwd / _bwd
_MLP = {}


def _mlp_shared():
    if not _MLP:
        from test_gpu_mlp_fused import _case, _oracle_fwd
        t = _case(96, 96, 771)
        _MLP.update(t=t, ref=_oracle_fwd(t, True, True))
    return _MLP["t"], _MLP["ref"]


@pytest.mark.parametrize("operand", ["w1", "w2", "b1", "b2", "ln_w", "ln_b"])
def test_mlp_fused_fwd_operands_at_every_residue(operand):
    L = _lib()
    lib, ptr = L.lib, L.ptr
    t, ref = _mlp_shared()
    C, rows, H = 96, 96, 384
    for e in offsets(t[operand]):
        o = dict(t)
        o[operand] = at_offset(t[operand], e)
        out = torch.full((rows, C), SENTINEL, device=DEV, dtype=BF)
        h = torch.full((rows, H), SENTINEL, device=DEV, dtype=BF)
        act = torch.full((rows, H), SENTINEL, device=DEV, dtype=BF)
        st = lib.hs_mlp_fused_fwd(ptr(o["x"]), ptr(o["ln_w"]), ptr(o["ln_b"]), ptr(o["w1"]), ptr(o["b1"]), ptr(o["w2"]), ptr(o["b2"]), None, None,
                                  None, ptr(h), ptr(act), ptr(out), rows, C, H, L.HS_ATTN_RESIDUAL, L.HS_BF16, _stream())
        tag = f"hs_mlp_fused_fwd {operand}+{e}"
        ran = c_call(st, tag, [out, h, act])
        must_run(ran, e, t[operand])
        if ran:
            assert_close(out, ref["out"], TOL[BF], tag + " out")
            assert_close(h, ref["h"], TOL[BF], tag + " h")
            assert_close(act, ref["act"], TOL[BF], tag + " gelu(h)")


@pytest.mark.parametrize("operand", ["w2_t", "w1_t"])
def test_mlp_fused_bwd_operands_at_every_residue(operand):
    from oracle import model as OM
    L = _lib()
    lib, ptr = L.lib, L.ptr
    t, _ = _mlp_shared()
    C, rows, H = 96, 96, 384
    g = torch.Generator(device=DEV).manual_seed(5)
    dy = torch.randn((rows, C), generator=g, device=DEV).to(BF)
    h = (torch.randn((rows, H), generator=g, device=DEV) * 1.5).to(BF)
    w = dict(w2_t=t["w2"].t().contiguous(), w1_t=t["w1"].t().contiguous())
    hd = h.double().requires_grad_(True)
    (dh_ref,) = torch.autograd.grad(OM.gelu(hd), hd, dy.double() @ t["w2"].double())
    dn_ref = dh_ref.to(BF).double() @ t["w1"].double()
    for e in E_BF16:
        o = dict(w)
        o[operand] = at_offset(w[operand], e)
        dh = torch.full((rows, H), SENTINEL, device=DEV, dtype=BF)
        dn = torch.full((rows, C), SENTINEL, device=DEV, dtype=BF)
        st = lib.hs_mlp_fused_bwd(ptr(dy), ptr(h), ptr(o["w2_t"]), ptr(o["w1_t"]), None, ptr(dh), ptr(dn), rows, C, H, L.HS_BF16, _stream())
        tag = f"hs_mlp_fused_bwd {operand}+{e}"
        ran = c_call(st, tag, [dh, dn])
        must_run(ran, e, w[operand])
        if ran:
            assert_close(dh, dh_ref, TOL[BF], tag + " dh")
            assert_close(dn, dn_ref, TOL[BF], tag + " dn")


def test_fused_mlp_block_through_ops_takes_parameters_at_every_residue():
    """The MLP half on the route the model takes when the fused kernel is off: fc1 as an hs_gemm_nt GELU epilogue through
    ops.gemm_nt, with the bf16 weight / the fp32 bias as misaligned views."""
    from heal_swin_amd import ops
    L = _lib()
    t, ref = _mlp_shared()
    n = ref["n"].to(BF)
    for name in ("b1", "w1"):
        for e in offsets(t[name]):
            o = dict(t)
            o[name] = at_offset(t[name], e)
            h, act = ops.gemm_nt(n, o["w1"], o["b1"], L.HS_EPI_GELU)
            assert_close(h, ref["h"], TOL[BF], f"ops.gemm_nt gelu {name}+{e} h")
            assert_close(act, ref["act"], TOL[BF], f"ops.gemm_nt gelu {name}+{e} act")


# ----------------------------------------------------------------------------- ops.window_attn_module (hs_window_attn_module_fwd)
_ATTN = {}


def _attn_shared(masked):
    """C = 96, nH = 3, B = 1, nside = 8: the unmasked and a masked (nest_roll) case of test_gpu_attn_module.CASES' C = 96 rows."""
    if masked not in _ATTN:
        from oracle import tables as T
        from test_gpu_attn_module import _reference
        C, nH, N = 96, 3, 8 * 8 * 8
        g = torch.Generator().manual_seed(96 + 8 + (32 if masked else 0))
        bf = lambda v: v.to(BF).float()  # noqa: E731
        t = dict(x=bf(torch.randn(1, N, C, generator=g) * 3.0 + 0.5), qkv_w=bf(torch.randn(3 * C, C, generator=g) * C ** -0.5),
                 proj_w=bf(torch.randn(C, C, generator=g) * C ** -0.5), qkv_b=torch.randn(3 * C, generator=g) * 0.2,
                 proj_b=torch.randn(C, generator=g) * 0.2, bias=torch.randn(nH, 64, 64, generator=g),
                 head_scale=torch.rand(nH, generator=g) * 0.3 + 0.1, ln_w=torch.rand(C, generator=g) + 0.5,
                 ln_b=torch.randn(C, generator=g) * 0.2)
        idx = labels = None
        if masked:
            idx_np, _, lab_np = T.nest_roll_shift(N, 64, 32)
            idx, labels = torch.from_numpy(idx_np), torch.from_numpy(lab_np)
        ref = _reference(t["x"], t["qkv_w"], t["qkv_b"], t["proj_w"], t["proj_b"], t["bias"], t["head_scale"], idx, labels, nH, False,
                         (t["ln_w"], t["ln_b"]), True)
        _ATTN[masked] = ({k: v.to(DEV) for k, v in t.items()}, None if labels is None else labels.to(torch.uint8).to(DEV), ref)
    return _ATTN[masked]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("operand", ["qkv_w", "proj_w", "qkv_b", "proj_b", "ln_w", "ln_b", "bias", "head_scale"])
def test_window_attn_module_parameters_at_every_residue(operand, masked):
    """ops.window_attn_module with one parameter-like operand misaligned (fp32 masters: the bf16 copies are made by the op; a bf16
    copy at a bad residue is what ParamCastCache now refuses, tested in test_gpu_optim)."""
    from heal_swin_amd import ops
    t, labels, ref = _attn_shared(masked)
    xb = t["x"].to(BF)
    with torch.no_grad():
        assert ops.window_attn_module_ok(xb, 3, 64)
    for e in E_F32:
        o = dict(t)
        o[operand] = at_offset(t[operand], e)
        with torch.no_grad():
            y = ops.window_attn_module(xb, o["qkv_w"], o["qkv_b"], o["proj_w"], o["proj_b"], o["bias"], o["head_scale"], None,
                                       32 if masked else 0, labels, 3, 64, False, ln_weight=o["ln_w"], ln_bias=o["ln_b"], residual=True)
        assert_close(y, ref, 1.5e-2, f"window_attn_module masked={masked} {operand}+{e}")


@pytest.mark.parametrize("operand", ["qkv_w", "proj_w", "qkv_b", "ln_w", "bias", "head_scale"])
def test_window_attn_module_c_abi_refuses_or_computes(operand):
    L = _lib()
    lib, ptr = L.lib, L.ptr
    t, labels, ref = _attn_shared(False)
    base = dict(t, qkv_w=t["qkv_w"].to(BF), proj_w=t["proj_w"].to(BF))
    xb = t["x"].to(BF).contiguous()
    for e in offsets(base[operand]):
        o = dict(base)
        o[operand] = at_offset(base[operand], e)
        out = torch.full_like(xb, SENTINEL)
        st = lib.hs_window_attn_module_fwd(ptr(xb), ptr(out), ptr(o["qkv_w"]), ptr(o["qkv_b"]), ptr(o["proj_w"]), ptr(o["proj_b"]),
                                           ptr(o["ln_w"]), ptr(o["ln_b"]), ptr(o["bias"]), ptr(o["head_scale"]), None, 0, None, 1, 512, 96, 3, 64,
                                           L.HS_ATTN_RESIDUAL, L.HS_BF16, _stream())
        tag = f"hs_window_attn_module_fwd {operand}+{e}"
        ran = c_call(st, tag, [out])
        must_run(ran, e, base[operand])
        if ran:
            assert_close(out, ref, 1.5e-2, tag)


# ----------------------------------------------------------------------------- LayerNorm
def _ln_ref(x, res, gamma, beta, dy):
    xr = x.double().requires_grad_(True)
    rr = None if res is None else res.double().requires_grad_(True)
    g, b = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    s = xr if rr is None else xr + rr
    y = torch.nn.functional.layer_norm(s, (x.shape[-1],), g, b, 1e-5)
    y.backward(dy.double())
    return y, s, xr.grad, g.grad, b.grad


@pytest.mark.parametrize("rows,width", [(130, 96), (64, 1536)])
@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("form", ["layer_norm", "add_layer_norm", "layer_norm_stream", "add_layer_norm_stream"])
def test_layer_norm_parameters_at_every_residue(rows, width, dtype, form):
    """Forward and backward of the four forms with gamma / beta at every residue (the kernels read them as float4)."""
    from heal_swin_amd import ops
    g = torch.Generator(device=DEV).manual_seed(rows + width)
    x = (torch.randn(rows, width, generator=g, device=DEV) * 2 + 0.3).to(dtype)
    r = torch.randn(rows, width, generator=g, device=DEV).to(dtype)
    gamma0 = torch.rand(width, generator=g, device=DEV) + 0.5
    beta0 = torch.randn(width, generator=g, device=DEV) * 0.2
    dy = torch.randn(rows, width, generator=g, device=DEV).to(dtype)
    add = form.startswith("add")
    y_ref, s_ref, dx_ref, dg_ref, db_ref = _ln_ref(x, r if add else None, gamma0, beta0, dy)
    for operand in ("gamma", "beta"):
        for e in E_F32:
            gamma = (at_offset(gamma0, e) if operand == "gamma" else gamma0.clone()).requires_grad_(True)
            beta = (at_offset(beta0, e) if operand == "beta" else beta0.clone()).requires_grad_(True)
            xq, rq = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
            if form == "layer_norm":
                y = ops.layer_norm(xq, gamma, beta)
            elif form == "add_layer_norm":
                s, y = ops.add_layer_norm(xq, rq, gamma, beta)
            elif form == "layer_norm_stream":  # y + y_lo = residual + LN(x): compare the LayerNorm part
                zero = torch.zeros_like(x)
                y, _ = ops.layer_norm_stream(xq, gamma, beta, zero)
            else:
                s, y, _ = ops.add_layer_norm_stream(xq, None, rq, gamma, beta)
            y.backward(dy)
            tag = f"{form}[{rows}x{width} {dtype}] {operand}+{e}"
            assert_close(y, y_ref, TOL[dtype], tag + " y")
            if add:
                assert_close(s, s_ref, TOL[dtype], tag + " sum")
            assert_close(xq.grad, dx_ref, GRAD_TOL[dtype], tag + " dx")
            assert_close(gamma.grad, dg_ref, GRAD_TOL[dtype], tag + " dgamma")
            assert_close(beta.grad, db_ref, GRAD_TOL[dtype], tag + " dbeta")


@pytest.mark.parametrize("rows,width", [(130, 96), (64, 1536)])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("operand", ["gamma", "dgamma", "dbeta"])
def test_layernorm_bwd_c_abi_destinations_at_every_residue(rows, width, acc, operand):
    L = _lib()
    lib, ptr = L.lib, L.ptr
    g = torch.Generator(device=DEV).manual_seed(rows * 3 + width)
    x = (torch.randn(rows, width, generator=g, device=DEV) * 2 + 0.3).to(BF)
    gamma = torch.rand(width, generator=g, device=DEV) + 0.5
    dy = torch.randn(rows, width, generator=g, device=DEV).to(BF)
    _, _, dx_ref, dg_ref, db_ref = _ln_ref(x, None, gamma, torch.zeros_like(gamma), dy)
    mean = x.float().mean(1)
    rstd = (x.float().var(1, unbiased=False) + 1e-5).rsqrt()
    ws = torch.empty(int(lib.hs_layernorm_bwd_workspace(rows, width)), device=DEV)
    for e in E_F32:
        o = dict(gamma=gamma, dgamma=torch.full((width,), SENTINEL, device=DEV), dbeta=torch.full((width,), SENTINEL, device=DEV))
        o[operand] = at_offset(o[operand], e)
        dx = torch.full_like(x, SENTINEL)
        st = lib.hs_layernorm_bwd(ptr(dy), ptr(x), ptr(o["gamma"]), ptr(mean), ptr(rstd), ptr(dx), ptr(o["dgamma"]), ptr(o["dbeta"]), ptr(ws), acc,
                                  rows, width, L.HS_BF16, _stream())
        tag = f"hs_layernorm_bwd[{rows}x{width}] acc {acc} {operand}+{e}"
        ran = c_call(st, tag, [dx, o["dgamma"], o["dbeta"]])
        must_run(ran, e, gamma)
        if ran:
            assert_close(dx, dx_ref, GRAD_TOL[BF], tag + " dx")
            assert_close(o["dgamma"] - acc * SENTINEL, dg_ref, GRAD_TOL[BF], tag + " dgamma")
            assert_close(o["dbeta"] - acc * SENTINEL, db_ref, GRAD_TOL[BF], tag + " dbeta")


class _ViewSink:
    """A gradient sink that hands out the views it was given (what a flat-buffer optimizer other than FlatAdam might do)."""
    flushes_reductions = True

    def __init__(self, views):
        self.views, self.got = views, []

    def grad_buffer(self, p):
        return self.views.get(id(p))

    def deposited(self, p):
        self.got.append(id(p))


@pytest.mark.parametrize("e", E_F32)
def test_direct_deposit_into_a_sink_view_at_every_residue(e):
    """LayerNorm and Linear parameter gradients with a sink whose buffers sit at residue e: deposited (added) directly when aligned;
    a misaligned view is refused with a RuntimeError before any kernel of the backward runs on it -- never a silent wrong gradient."""
    from heal_swin_amd import ops
    rows, width, n = 130, 96, 132
    g = torch.Generator(device=DEV).manual_seed(17 + e)
    x = (torch.randn(rows, width, generator=g, device=DEV) * 2).to(BF)
    gamma = (torch.rand(width, generator=g, device=DEV) + 0.5).requires_grad_(True)
    beta = (torch.randn(width, generator=g, device=DEV) * 0.2).requires_grad_(True)
    w = (torch.randn(n, width, generator=g, device=DEV) * width ** -0.5).to(BF).float().requires_grad_(True)
    b = torch.randn(n, generator=g, device=DEV).requires_grad_(True)
    dy = torch.randn(rows, n, generator=g, device=DEV).to(BF)
    pr = [t.detach().double().requires_grad_(True) for t in (gamma, beta, w, b)]
    torch.nn.functional.linear(torch.nn.functional.layer_norm(x.double(), (width,), pr[0], pr[1], 1e-5).to(BF).double(), pr[2], pr[3]).backward(dy.double())
    views = {id(p): at_offset(torch.full_like(p, SENTINEL), e) for p in (gamma, beta, w, b)}
    sink = _ViewSink(views)
    with ops.RT.scoped(grad_sink=sink):
        y = ops.linear(ops.layer_norm(x.clone().requires_grad_(True), gamma, beta), w, b)
        if e % 4:
            with pytest.raises(RuntimeError, match="aligned"):
                y.backward(dy)
            ops.flush_reductions()
            torch.cuda.synchronize()
            assert not sink.got and all(bool((v == SENTINEL).all()) for v in views.values()), "refused, so nothing was deposited"
            return
        y.backward(dy)
        ops.flush_reductions()
    assert len(sink.got) == 4 and all(p.grad is None for p in (gamma, beta, w, b))
    for p, r, name in zip((gamma, beta, w, b), pr, ("dgamma", "dbeta", "dW", "db")):
        assert_close(views[id(p)] - SENTINEL, r.grad, GRAD_TOL[BF], f"sink at +{e}: {name}")


@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("e", E_F32)
def test_rel_bias_and_head_scale_backward_deposit_at_every_residue(e, many):
    """The position-bias table and logit_scale gradients are deposited by kernels that address single elements: a sink view at ANY
    residue is added into directly (these are the odd-sized parameters: their own views are the first to sit at odd offsets)."""
    from heal_swin_amd import ops
    L = _lib()
    ws, nh, rows = 64, 3, 225
    g = torch.Generator().manual_seed(40 + e)
    table = torch.randn(rows, nh, generator=g).to(DEV).requires_grad_(True)
    ls = (torch.randn(nh, 1, 1, generator=g) + 4.0).to(DEV).requires_grad_(True)
    rel = torch.from_numpy(L.rel_pos_index(ws)).to(torch.int32).to(DEV).reshape(-1)
    dbias = torch.randn(nh, ws, ws, generator=g).to(DEV)
    dscale = torch.randn(nh, generator=g).to(DEV)
    tr, lr = table.detach().double().requires_grad_(True), ls.detach().double().requires_grad_(True)
    (tr[rel.long()].t().reshape(nh, ws, ws) * dbias.double()).sum().backward()
    (torch.exp(torch.clamp(lr, max=4.605170185988092)).reshape(-1) * dscale.double()).sum().backward()
    views = {id(table): at_offset(torch.full_like(table, SENTINEL), e), id(ls): at_offset(torch.full_like(ls, SENTINEL), e)}
    sink = _ViewSink(views)
    with ops.RT.scoped(grad_sink=sink):
        if many:
            (bias,) = ops.rel_pos_bias_many(rel, ws, [table])
            (scale,) = ops.cos_head_scale_many([ls])
        else:
            bias = ops.RelPosBiasFn.apply(table, rel, ws)
            scale = ops.cos_head_scale(ls)
        assert torch.equal(bias, table.detach()[rel.long()].t().reshape(nh, ws, ws))
        ((bias * dbias).sum() + (scale.reshape(-1) * dscale).sum()).backward()
    assert sorted(sink.got) == sorted(views) and table.grad is None and ls.grad is None
    assert_close(views[id(table)] - SENTINEL, tr.grad, 1e-5, f"rel_bias backward many={many}: sink view +{e}")
    assert_close(views[id(ls)] - SENTINEL, lr.grad, 1e-5, f"cos_head_scale backward many={many}: sink view +{e}")


# ----------------------------------------------------------------------------- ops.ln_head / ops.expand_ln_head
@pytest.mark.parametrize("tokens,C,f_out", [(33, 64, 5), (1000, 96, 12)])
@pytest.mark.parametrize("operand", ["gamma", "beta", "w"])
def test_ln_head_parameters_at_every_residue(tokens, C, f_out, operand):
    from heal_swin_amd import ops
    from test_gpu_ln_head import reference
    torch.manual_seed(tokens + C)
    y = (torch.randn(tokens, C, device=DEV) * 1.7 + 0.6 * torch.randn(tokens, 1, device=DEV) + 0.3).to(BF)
    p0 = dict(gamma=1 + 0.3 * torch.randn(C, device=DEV), beta=0.2 * torch.randn(C, device=DEV), w=torch.randn(f_out, C, 1, device=DEV) * C ** -0.5)
    dlog = torch.randn(tokens, f_out, device=DEV).to(BF)
    ref_out, ref_dy, ref_dg, ref_db, ref_dw = reference(y, p0["gamma"], p0["beta"], p0["w"].reshape(f_out, C), dlog)
    for e in E_F32:
        p = {k: (at_offset(v, e) if k == operand else v.clone()).requires_grad_(True) for k, v in p0.items()}
        yq = y.clone().requires_grad_(True)
        out = ops.ln_head(yq, p["gamma"], p["beta"], p["w"])
        out[:, :f_out].backward(dlog.float())
        tag = f"ln_head[{tokens}x{C}->{f_out}] {operand}+{e}"
        assert_close(out[:, :f_out], ref_out, TOL[BF], tag + " logits")
        assert_close(yq.grad, ref_dy, GRAD_TOL[BF], tag + " dy")
        assert_close(p["gamma"].grad, ref_dg, GRAD_TOL[BF], tag + " dgamma")
        assert_close(p["beta"].grad, ref_db, GRAD_TOL[BF], tag + " dbeta")
        assert_close(p["w"].grad.reshape(f_out, C), ref_dw, GRAD_TOL[BF], tag + " dW")


@pytest.mark.parametrize("tokens,C,f_out", [(33, 64, 5), (1000, 96, 12)])
@pytest.mark.parametrize("operand", ["wexp", "gamma", "beta", "w"])
def test_expand_ln_head_parameters_at_every_residue(tokens, C, f_out, operand):
    from heal_swin_amd import ops
    from test_gpu_ln_head import reference_tail
    torch.manual_seed(tokens + C)
    xn = (torch.randn(tokens, C, device=DEV) * 1.3 + 0.2).to(BF)
    p0 = dict(wexp=(torch.randn(4 * C, C, device=DEV) * C ** -0.5).to(BF).float(), gamma=1 + 0.3 * torch.randn(C, device=DEV),
              beta=0.2 * torch.randn(C, device=DEV), w=torch.randn(f_out, C, 1, device=DEV) * C ** -0.5)
    dlog = torch.randn(4 * tokens, f_out, device=DEV).to(BF).float()
    ref_out, ref_dx, ref_dwe, ref_dg, ref_db, ref_dw = reference_tail(xn, p0["wexp"], p0["gamma"], p0["beta"], p0["w"].reshape(f_out, C), dlog)
    for e in E_F32:
        p = {k: (at_offset(v, e) if k == operand else v.clone()).requires_grad_(True) for k, v in p0.items()}
        xq = xn.clone().requires_grad_(True)
        out = ops.expand_ln_head(xq, p["wexp"], p["gamma"], p["beta"], p["w"])
        out[:, :f_out].backward(dlog)
        tag = f"expand_ln_head[{tokens}x{C}->{f_out}] {operand}+{e}"
        assert_close(out[:, :f_out], ref_out, 2e-3, tag + " logits")
        assert_close(xq.grad, ref_dx, GRAD_TOL[BF], tag + " dxn")
        assert_close(p["wexp"].grad, ref_dwe, GRAD_TOL[BF], tag + " dWexpand")
        assert_close(p["gamma"].grad, ref_dg, GRAD_TOL[BF], tag + " dgamma")
        assert_close(p["beta"].grad, ref_db, GRAD_TOL[BF], tag + " dbeta")
        assert_close(p["w"].grad.reshape(f_out, C), ref_dw, GRAD_TOL[BF], tag + " dWhead")


# ----------------------------------------------------------------------------- hs_linear_wgrad* and the deferred sums
_WG = {}


def _wgrad_shared(rows, n, k):
    if (rows, n, k) not in _WG:
        g = torch.Generator(device=DEV).manual_seed(rows + n + k)
        dy = torch.randn(rows, n, generator=g, device=DEV).to(BF)
        x = torch.randn(rows, k, generator=g, device=DEV).to(BF)
        dw = dy.double().t() @ x.double()
        dwg = dy.double().t() @ torch.nn.functional.gelu(x.double())
        _WG[(rows, n, k)] = (dy, x, dw, dwg, dy.double().sum(0))
    return _WG[(rows, n, k)]


@pytest.mark.parametrize("rows,n,k", [(777, 96, 288), (4096, 128, 128)])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("entry", ["plain", "ld", "gelu", "group", "deferred"])
@pytest.mark.parametrize("operand", ["dw", "dbias"])
def test_linear_wgrad_destinations_at_every_residue(rows, n, k, acc, entry, operand):
    """dW / dbias destinations at every residue, overwritten (acc 0) and added to (acc 1), through each entry point and through the
    queued sum that hs_reduce_flush launches.  Bound: test_gpu_wgrad_group._check (fp32 split-K sums of exact bf16 products against
    fp64: 2e-4 of the scale, growing with sqrt(rows / 4096) for dW)."""
    from test_gpu_wgrad_group import _check
    L = _lib()
    lib, ptr = L.lib, L.ptr
    dy, x, dw_ref, dwg_ref, db_ref = _wgrad_shared(rows, n, k)
    assert entry != "gelu" or lib.hs_linear_wgrad_gelu_supported(rows, n, k, L.HS_BF16), "both shapes are on the 128 x 128 LDS-DMA tile"
    L.check(lib.hs_reduce_flush(_stream()), "hs_reduce_flush")  # (nothing left queued by an earlier test)
    ws = torch.empty(2 * int(lib.hs_linear_wgrad_workspace(rows, n, k)) + 64, device=DEV)
    for e in E_F32:
        o = dict(dw=torch.full((n, k), SENTINEL, device=DEV), dbias=torch.full((n,), SENTINEL, device=DEV))
        o[operand] = at_offset(o[operand], e)
        flags = acc | (L.HS_ACC_DEFER if entry == "deferred" else 0)
        if entry in ("plain", "deferred"):
            st = lib.hs_linear_wgrad(ptr(dy), ptr(x), ptr(o["dw"]), ptr(o["dbias"]), ptr(ws), rows, n, k, flags, L.HS_BF16, _stream())
        elif entry == "ld":
            st = lib.hs_linear_wgrad_ld(ptr(dy), n, 0, ptr(x), k, 0, ptr(o["dw"]), ptr(o["dbias"]), ptr(ws), rows, n, k, flags, _stream())
        elif entry == "gelu":
            st = lib.hs_linear_wgrad_gelu(ptr(dy), ptr(x), ptr(o["dw"]), ptr(o["dbias"]), ptr(ws), rows, n, k, flags, L.HS_BF16, _stream())
        else:
            arr = L.wgrad_problems([(dy, x, o["dw"], o["dbias"], n, k, flags, False)])
            wsg = torch.empty(int(lib.hs_linear_wgrad_group_workspace(arr, 1, rows, L.HS_BF16)), device=DEV)
            st = lib.hs_linear_wgrad_group(arr, 1, ptr(wsg), rows, L.HS_BF16, _stream())
        tag = f"hs_linear_wgrad {entry}[{rows},{n},{k}] acc {acc} {operand}+{e}"
        ran = c_call(st, tag, [o["dw"], o["dbias"]])
        if entry == "deferred":
            assert int(lib.hs_reduce_pending(_stream())) == (1 if ran else 0), "a refused call must not queue a sum"
            L.check(lib.hs_reduce_flush(_stream()), "hs_reduce_flush")
        must_run(ran, e, o["dw"])
        if ran:
            if entry == "gelu":  # gelu(x) enters the MFMA rounded to bf16: the bounds of test_linear_wgrad_gelu_equals_wgrad_of_gelu
                assert_close(o["dw"].double() - acc * SENTINEL, dwg_ref, 3e-3, tag + " dW")
                assert_close(o["dbias"].double() - acc * SENTINEL, db_ref, 1e-3, tag + " db")
            else:
                _check(rows, o["dw"].double() - acc * SENTINEL, dw_ref, "dw")
                _check(rows, o["dbias"].double() - acc * SENTINEL, db_ref, "db")


# ----------------------------------------------------------------------------- relative-position bias, cosine head scale
@pytest.mark.parametrize("many", [False, True])
def test_rel_bias_and_head_scale_at_every_residue(many):
    """ws = 64, nh = 3: the 225 x 3 table and the 3-element logit_scale that put the heads-3 model at odd offsets.  These kernels
    address single elements: every residue must compute (exact gather; fp32 sums for the scatter)."""
    L = _lib()
    lib, ptr = L.lib, L.ptr
    ws, nh, rows = 64, 3, 225
    g = torch.Generator().manual_seed(4)
    table0 = torch.randn(rows, nh, generator=g).to(DEV)
    rel = torch.from_numpy(L.rel_pos_index(ws)).to(torch.int32).to(DEV)
    dbias = torch.randn(nh, ws, ws, generator=g).to(DEV)
    ls0 = (torch.randn(nh, generator=g) + 4.0).to(DEV)  # around ln 100: both sides of the clamp
    dscale = torch.randn(nh, generator=g).to(DEV)
    ref_bias = table0[rel.long().flatten()].t().reshape(nh, ws, ws)
    ref_dtable = torch.zeros(rows, nh, dtype=torch.float64, device=DEV).index_add_(0, rel.long().flatten(), dbias.double().reshape(nh, -1).t())
    ref_scale = torch.exp(torch.clamp(ls0.double(), max=4.605170185988092))
    ref_dls = torch.where(ls0.double() <= 4.605170185988092, dscale.double() * ref_scale, torch.zeros_like(ref_scale))
    order = torch.argsort(rel.flatten().long(), stable=True).to(torch.int32)
    counts = torch.bincount(rel.flatten().long(), minlength=rows)
    offs = torch.cat([torch.zeros(1, dtype=torch.long, device=DEV), counts.cumsum(0)]).to(torch.int32)

    def parr(ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def iarr(v):
        return (ctypes.c_int * len(v))(*v)
    for e in E_F32:
        table, ls = at_offset(table0, e), at_offset(ls0, e)
        bias = torch.full((nh, ws, ws), SENTINEL, device=DEV)
        if many:
            L.check(lib.hs_rel_bias_gather_many(parr([table]), iarr([nh]), 1, ptr(rel), ptr(bias), rows, ws, _stream()), "gather_many")
        else:
            L.check(lib.hs_rel_bias_gather(ptr(table), ptr(rel), ptr(bias), rows, nh, ws, _stream()), "gather")
        assert torch.equal(bias, ref_bias), f"rel_bias gather table+{e}"
        for acc in (0, 1):
            dtable = at_offset(torch.full((rows, nh), SENTINEL, device=DEV), e)
            if many:
                L.check(lib.hs_rel_bias_scatter_grad_sorted_many(parr([dbias]), parr([dtable]), iarr([nh]), iarr([acc]), 1, ptr(order), ptr(offs),
                                                                 rows, ws, _stream()), "scatter_many")
            elif acc:
                L.check(lib.hs_rel_bias_scatter_grad_sorted_add(ptr(dbias), ptr(order), ptr(offs), ptr(dtable), rows, nh, ws, _stream()), "scatter_add")
            else:
                L.check(lib.hs_rel_bias_scatter_grad_sorted(ptr(dbias), ptr(order), ptr(offs), ptr(dtable), rows, nh, ws, _stream()), "scatter")
            assert_close(dtable - acc * SENTINEL, ref_dtable, 1e-5, f"rel_bias scatter many={many} acc={acc} dtable+{e}")
            scale = at_offset(torch.full((nh,), SENTINEL, device=DEV), e)
            dls = at_offset(torch.full((nh,), SENTINEL, device=DEV), e)
            if many:
                L.check(lib.hs_cos_head_scale_many(parr([ls]), (ctypes.c_void_p * 1)(None), parr([scale]), iarr([nh]), iarr([0]), 1, _stream()), "scale_many")
                L.check(lib.hs_cos_head_scale_many(parr([ls]), parr([dscale]), parr([dls]), iarr([nh]), iarr([acc]), 1, _stream()), "scale_many bwd")
            else:
                L.check(lib.hs_cos_head_scale_fwd(ptr(ls), ptr(scale), nh, _stream()), "scale_fwd")
                L.check(lib.hs_cos_head_scale_bwd(ptr(ls), ptr(dscale), ptr(dls), nh, acc, _stream()), "scale_bwd")
            assert_close(scale, ref_scale, 1e-5, f"cos_head_scale many={many} logit_scale+{e}")
            assert_close(dls - acc * SENTINEL, ref_dls, 1e-5, f"cos_head_scale bwd many={many} acc={acc} +{e}")


# ----------------------------------------------------------------------------- hs_transpose_many_16
@pytest.mark.parametrize("rows,cols", [(33, 7), (96, 288)])
def test_transpose_many_16_at_every_residue(rows, cols):
    """2-byte element accesses: exact at every residue of the source shadow and of the destination."""
    L = _lib()
    src0 = torch.randn(rows, cols, device=DEV).to(BF)
    for which in ("src", "dst"):
        for e in E_BF16:
            src = at_offset(src0, e) if which == "src" else src0
            dst = at_offset(torch.full((cols, rows), SENTINEL, dtype=BF, device=DEV), e if which == "dst" else 0)
            jobs = torch.tensor([[src.data_ptr(), dst.data_ptr(), rows, cols]], dtype=torch.int64).to(DEV)
            L.check(L.lib.hs_transpose_many_16(L.ptr(jobs), 1, 4, _stream()), "hs_transpose_many_16")
            assert torch.equal(dst, src0.t()), f"transpose {which}+{e}"


# ----------------------------------------------------------------------------- entry points that already checked: loud, before any launch
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_gelu_and_residual_drop_refuse_before_launch_and_their_ops_fall_back(dtype):
    from heal_swin_amd import ops
    L = _lib()
    lib, ptr = L.lib, L.ptr
    dt = L.dtype_code(dtype)
    n = 4096 + 24
    x0 = torch.randn(n, device=DEV).to(dtype)
    t0 = torch.randn(n, device=DEV).to(dtype)
    for e in offsets(x0)[1:]:
        x = at_offset(x0, e)
        y = torch.full_like(x0, SENTINEL)
        assert not c_call(lib.hs_gelu_fwd(ptr(x), ptr(y), n, 0.0, 0, dt, _stream()), "hs_gelu_fwd", [y])
        assert not c_call(lib.hs_gelu_bwd(ptr(x0), ptr(x), ptr(y), n, 0.0, 0, dt, _stream()), "hs_gelu_bwd", [y])
        assert not c_call(lib.hs_gelu_bwd(ptr(x), ptr(x0), ptr(y), n, 0.0, 0, dt, _stream()), "hs_gelu_bwd", [y])
        assert not c_call(lib.hs_residual_drop(ptr(x), ptr(t0), ptr(y), None, n, n, 0.0, 0, dt, _stream()), "hs_residual_drop", [y])
        assert not c_call(lib.hs_residual_drop(ptr(x0), ptr(x), ptr(y), None, n, n, 0.0, 0, dt, _stream()), "hs_residual_drop", [y])
        yo = at_offset(y, e)
        assert not c_call(lib.hs_gelu_fwd(ptr(x0), ptr(yo), n, 0.0, 0, dt, _stream()), "hs_gelu_fwd", [yo])
        # the ops take the misaligned activation through an aligned copy
        xq = x.detach().requires_grad_(True)
        out = ops.gelu_dropout(xq)
        out.backward(at_offset(t0, e))
        xr = x0.double().requires_grad_(True)
        ref = torch.nn.functional.gelu(xr)
        ref.backward(t0.double())
        assert_close(out, ref, TOL[dtype], f"ops.gelu_dropout x+{e}")
        assert_close(xq.grad, xr.grad, TOL[dtype], f"ops.gelu_dropout dx+{e}")
        assert_close(ops.residual_drop(x.view(8, -1), at_offset(t0, e).view(8, -1)).flatten(), x0.double() + t0.double(), TOL[dtype],
                     f"ops.residual_drop +{e}")


def test_adam_step_refuses_misaligned_buffers_before_launch():
    L = _lib()
    lib, ptr = L.lib, L.ptr
    n = 1000
    step = torch.zeros((), dtype=torch.int64, device=DEV)

    def bufs():
        return dict(p=torch.full((n,), SENTINEL, device=DEV), g=torch.full((n,), SENTINEL, device=DEV), m=torch.full((n,), SENTINEL, device=DEV),
                    v=torch.full((n,), SENTINEL, device=DEV), s=torch.full((n,), SENTINEL, device=DEV, dtype=BF))
    for name in ("p", "g", "m", "v", "s"):
        for e in (1, 2):  # fp32 buffers: 4 and 8 bytes miss 16; the bf16 copy: 2 and 4 bytes miss its 8
            o = bufs()
            o[name] = at_offset(o[name], e)
            st = lib.hs_adam_step(ptr(o["p"]), ptr(o["g"]), ptr(o["m"]), ptr(o["v"]), ptr(o["s"]), n, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0, ptr(step),
                                  _stream())
            assert not c_call(st, f"hs_adam_step {name}+{e}", [o["p"], o["m"], o["v"], o["s"]])
    o = bufs()
    o["s"] = at_offset(o["s"], 4)  # 8 bytes: the bf16 copy's own requirement is met
    L.check(lib.hs_adam_step(ptr(o["p"]), ptr(o["g"]), ptr(o["m"]), ptr(o["v"]), ptr(o["s"]), n, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0, ptr(step),
                             _stream()), "hs_adam_step")
    assert torch.equal(o["s"], o["p"].to(BF)) and not bool((o["p"] == SENTINEL).any())


# ----------------------------------------------------------------------------- the loss-fused tails and the module's training form
@pytest.mark.parametrize("tokens,C,f_out", [(33, 64, 5), (1000, 96, 12)])
@pytest.mark.parametrize("form", ["ce", "ce_step"])
@pytest.mark.parametrize("operand", ["wexp", "gamma", "beta", "w", "class_w"])
def test_expand_ln_head_ce_forms_parameters_at_every_residue(tokens, C, f_out, form, operand):
    """expand_ln_head_ce and its _ce_step form (hs_expand_ln_head_ce(_step)_fwd + hs_ln_head_ce_bwd) with each parameter and the
    class weights at every residue: loss to 1e-3, gradients to the bf16 bound, as test_expand_ln_head_ce_matches_the_composition;
    the step form's predictions against the argmax of the fp32 composition's logits where its top-2 margin exceeds the bf16 bound."""
    from heal_swin_amd import ops
    from test_gpu_ln_head import reference_tail_ce
    torch.manual_seed(tokens + C + f_out)
    xn = (torch.randn(tokens, C, device=DEV) * 1.3 + 0.2).to(BF)
    p0 = dict(wexp=(torch.randn(4 * C, C, device=DEV) * C ** -0.5).to(BF).float(), gamma=1 + 0.3 * torch.randn(C, device=DEV),
              beta=0.2 * torch.randn(C, device=DEV), w=torch.randn(f_out, C, 1, device=DEV) * 2.0 * C ** -0.5)
    labels = torch.randint(0, f_out, (4 * tokens,), device=DEV, dtype=torch.uint8)
    cw0 = 0.2 + torch.rand(f_out, device=DEV)
    ref_loss, ref_dx, ref_dwe, ref_dg, ref_db, ref_dw = reference_tail_ce(xn, p0["wexp"], p0["gamma"], p0["beta"], p0["w"].reshape(f_out, C), labels, cw0)
    with torch.no_grad():
        F = torch.nn.functional
        logits = F.linear(F.layer_norm(F.linear(xn.float(), p0["wexp"]).reshape(-1, C), (C,), p0["gamma"], p0["beta"], 1e-5), p0["w"].reshape(f_out, C))
        top2 = logits.topk(2, dim=1).values
        sure = (top2[:, 0] - top2[:, 1]) > TOL[BF] * float(logits.abs().max())
    for e in E_F32:
        p = {k: (at_offset(v, e) if k == operand else v.clone()).requires_grad_(True) for k, v in p0.items()}
        cw = at_offset(cw0, e) if operand == "class_w" else cw0
        xq = xn.clone().requires_grad_(True)
        tag = f"expand_ln_head_{form}[{tokens}x{C}->{f_out}] {operand}+{e}"
        if form == "ce":
            loss = ops.expand_ln_head_ce(xq, p["wexp"], p["gamma"], p["beta"], p["w"], labels, cw)
        else:
            conf = torch.zeros(f_out, f_out, dtype=torch.int64, device=DEV)
            bad = torch.zeros(2, dtype=torch.int64, device=DEV)
            loss, preds = ops.expand_ln_head_ce_step(xq, p["wexp"], p["gamma"], p["beta"], p["w"], labels, cw, confmat=conf, bad=bad)
            assert torch.equal(preds[sure].long(), logits.argmax(1)[sure]), tag + " preds"
            assert int(conf.sum()) == 4 * tokens and int(bad.sum()) == 0
            assert int(conf.diagonal().sum()) == int((preds == labels).sum()), tag + " confusion matrix of its own predictions"
        (loss * 3.0).backward()
        assert abs(float(loss) - float(ref_loss)) <= 1e-3 * abs(float(ref_loss)), (tag, float(loss), float(ref_loss))
        for got, ref, name in ((xq.grad, ref_dx, "dxn"), (p["wexp"].grad, ref_dwe, "dWexpand"), (p["gamma"].grad, ref_dg, "dgamma"),
                               (p["beta"].grad, ref_db, "dbeta"), (p["w"].grad.reshape(f_out, C), ref_dw, "dWhead")):
            assert_close(got, 3.0 * ref, GRAD_TOL[BF], f"{tag} {name}")


@pytest.mark.parametrize("tokens,C,f_out,kind", [(33, 64, 1, "huber"), (1000, 96, 2, "logvar")])
@pytest.mark.parametrize("operand", ["wexp", "gamma", "beta", "w"])
def test_expand_ln_head_depth_parameters_at_every_residue(tokens, C, f_out, kind, operand):
    """The depth form (hs_expand_ln_head_depth_fwd + hs_ln_head_depth_bwd): loss to 1e-3 and gradients to the bf16 bound, as
    test_expand_ln_head_depth_matches_the_composition."""
    from heal_swin_amd import ops
    from heal_swin_amd.losses import depth_loss_spec
    from test_gpu_depth_loss import _reference_tail_depth
    F = torch.nn.functional
    torch.manual_seed(tokens + C + f_out)
    kw = dict(loss="l1" if kind == "logvar" else kind, use_logvar=kind == "logvar", huber_delta=0.5)
    xn = (torch.randn(tokens, C, device=DEV) * 1.3 + 0.2).to(BF)
    p0 = dict(wexp=(torch.randn(4 * C, C, device=DEV) * C ** -0.5).to(BF).float(), gamma=1 + 0.3 * torch.randn(C, device=DEV),
              beta=0.2 * torch.randn(C, device=DEV), w=torch.randn(f_out, C, 1, device=DEV) * 2.0 * C ** -0.5)
    with torch.no_grad():
        pred0 = F.linear(F.layer_norm(F.linear(xn.float(), p0["wexp"]).reshape(-1, C), (C,), p0["gamma"], p0["beta"], 1e-5), p0["w"].reshape(f_out, C))[:, 0]
        u = torch.rand(4 * tokens, device=DEV)
        target = pred0 + torch.where(u < 0.5, -1.0, 1.0) * (0.2 + 2 * u)
    target[::13] = float("inf")
    k, delta = depth_loss_spec(**kw)
    assert ops.expand_ln_head_depth_ok(xn, C, 4, f_out, k, delta)
    ref_loss, ref_dx, ref_dwe, ref_dg, ref_db, ref_dw = _reference_tail_depth(xn, p0["wexp"], p0["gamma"], p0["beta"], p0["w"].reshape(f_out, C), target, kw)
    for e in E_F32:
        p = {k_: (at_offset(v, e) if k_ == operand else v.clone()).requires_grad_(True) for k_, v in p0.items()}
        xq = xn.clone().requires_grad_(True)
        loss = ops.expand_ln_head_depth(xq, p["wexp"], p["gamma"], p["beta"], p["w"], target, k, delta)
        (loss * 3.0).backward()
        tag = f"expand_ln_head_depth[{tokens}x{C}->{f_out} {kind}] {operand}+{e}"
        assert abs(float(loss) - float(ref_loss)) <= 1e-3 * abs(float(ref_loss)), (tag, float(loss), float(ref_loss))
        for got, ref, name in ((xq.grad, ref_dx, "dxn"), (p["wexp"].grad, ref_dwe, "dWexpand"), (p["gamma"].grad, ref_dg, "dgamma"),
                               (p["beta"].grad, ref_db, "dbeta"), (p["w"].grad.reshape(f_out, C), ref_dw, "dWhead")):
            assert_close(got, 3.0 * ref, GRAD_TOL[BF], f"{tag} {name}")


_TRAIN = {}


def _train_shared(masked):
    if masked not in _TRAIN:
        from oracle import tables as T
        from test_gpu_attn_module import _reference
        C, nH, N = 96, 3, 8 * 8 * 8
        g = torch.Generator().manual_seed(96 + 8 + 17 + (32 if masked else 0))
        bf = lambda v: v.to(BF).float()  # noqa: E731
        x = bf(torch.randn(1, N, C, generator=g) * 3.0 + 0.5)
        P = dict(wqkv=bf(torch.randn(3 * C, C, generator=g) * C ** -0.5), wp=bf(torch.randn(C, C, generator=g) * C ** -0.5),
                 bp=torch.randn(C, generator=g) * 0.2, hscale=torch.rand(nH, generator=g) * 0.3 + 0.1, lng=torch.rand(C, generator=g) + 0.5,
                 lnb=torch.randn(C, generator=g) * 0.2, bqkv=torch.randn(3 * C, generator=g) * 0.2, bias=torch.randn(nH, 64, 64, generator=g))
        dout = bf(torch.randn(1, N, C, generator=g))
        idx = labels = None
        if masked:
            idx_np, _, lab_np = T.nest_roll_shift(N, 64, 32)
            idx, labels = torch.from_numpy(idx_np), torch.from_numpy(lab_np)
        xr = x.clone().requires_grad_(True)
        R = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        ref = _reference(xr, R["wqkv"], R["bqkv"], R["wp"], R["bp"], R["bias"], R["hscale"], idx, labels, nH, False, (R["lng"], R["lnb"]), True)
        ref.backward(dout)
        _TRAIN[masked] = (x, P, dout, None if labels is None else labels.to(torch.uint8).to(DEV), ref.detach(), xr.grad, {k: v.grad for k, v in R.items()})
    return _TRAIN[masked]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("operand", ["wqkv", "bqkv", "wp", "bp", "lng", "lnb", "bias"])
def test_window_attn_module_train_parameters_at_every_residue(operand, masked):
    """ops.window_attn_module_train (hs_window_attn_module_fwd_train, backward = the composed path's kernels) forward and backward with
    one parameter at each residue, against the oracle's autograd at the bounds of test_module_train_form_vs_oracle_and_composition
    (out 1.5e-2, dx and parameter gradients 4e-2, the gathered bias 8e-2; the constant head scale of the non-cosine form takes no
    gradient and is swept through the forward in test_window_attn_module_parameters_at_every_residue)."""
    from heal_swin_amd import ops
    x, P, dout, labels, ref, dx_ref, G_ref = _train_shared(masked)
    for e in E_F32:
        xd = x.to(DEV).to(BF).requires_grad_(True)
        D = {k: (at_offset(v.to(DEV), e) if k == operand else v.to(DEV).clone()).requires_grad_(True) for k, v in P.items()}
        assert ops.window_attn_module_train_ok(xd, 3, 64)
        out = ops.window_attn_module_train(xd, D["lng"], D["lnb"], D["wqkv"], D["bqkv"], D["wp"], D["bp"], D["bias"], D["hscale"], None,
                                           32 if masked else 0, labels, 3, 64, False)
        out.backward(dout.to(DEV).to(BF))
        tag = f"window_attn_module_train masked={masked} {operand}+{e}"
        assert_close(out, ref, 1.5e-2, tag + " out")
        assert_close(xd.grad, dx_ref, 4e-2, tag + " dx")
        for k in P:
            if k != "hscale":
                assert_close(D[k].grad, G_ref[k], 8e-2 if k == "bias" else 4e-2, f"{tag} d{k}")


def test_train_form_and_loss_tail_entry_points_refuse_before_launch():
    """C ABI of the entry points the model's training step calls: one pointer at a nonzero residue -> HS_ERR_MISALIGNED, outputs
    untouched (their computing side at residue 0 is what the ops cases above and the entry points' own tests run)."""
    L = _lib()
    lib, ptr = L.lib, L.ptr
    S = _stream()
    # ---- hs_window_attn_module_fwd_train / _bwd_chain: C = 96, nH = 3, one image of 512 tokens
    C, nH, N = 96, 3, 512
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    full = lambda *s, dt=BF: torch.full(s, SENTINEL, dtype=dt, device=DEV)  # noqa: E731
    f32 = torch.float32
    base = dict(x=z(N, C), qkv_w=z(3 * C, C), qkv_b=z(3 * C, dt=f32), proj_w=z(C, C), proj_b=z(C, dt=f32), ln_g=torch.ones(C, device=DEV),
                ln_b=z(C, dt=f32), bias=z(nH, 64, 64, dt=f32), hs=torch.ones(nH, device=DEV), n2_g=torch.ones(C, device=DEV), n2_b=z(C, dt=f32))
    for name, t in base.items():
        if name == "x":
            continue
        for e in offsets(t)[1:]:
            if (e * t.element_size()) % 16 == 0:
                continue
            o = dict(base)
            o[name] = at_offset(t, e)
            outs = dict(out=full(N, C), xn=full(N, C), qkv=full(N, 3 * C), att=full(N, C), n2=full(N, C))
            mean, rstd, mean2, rstd2, lse = (full(N, dt=f32), full(N, dt=f32), full(N, dt=f32), full(N, dt=f32), full(nH, N, dt=f32))
            st = lib.hs_window_attn_module_fwd_train(ptr(o["x"]), ptr(outs["out"]), ptr(outs["xn"]), ptr(mean), ptr(rstd), ptr(outs["qkv"]),
                                                     ptr(outs["att"]), ptr(lse), ptr(o["qkv_w"]), ptr(o["qkv_b"]), ptr(o["proj_w"]), ptr(o["proj_b"]),
                                                     ptr(o["ln_g"]), ptr(o["ln_b"]), ptr(o["bias"]), ptr(o["hs"]), None, 0, None, ptr(o["n2_g"]),
                                                     ptr(o["n2_b"]), ptr(outs["n2"]), ptr(mean2), ptr(rstd2), 1, N, C, nH, 64, L.HS_ATTN_RESIDUAL,
                                                     L.HS_BF16, S)
            assert not c_call(st, f"hs_window_attn_module_fwd_train {name}+{e}", list(outs.values()) + [mean, rstd, lse])
    nws = int(lib.hs_window_attn_module_bwd_chain_workspace(1, N, C, nH, 64))
    chain = dict(qkv_w_t=z(C, 3 * C), proj_w_t=z(C, C), ln_g=torch.ones(C, device=DEV), dqkv_w=full(3 * C, C, dt=f32), dqkv_b=full(3 * C, dt=f32),
                 dproj_w=full(C, C, dt=f32), dproj_b=full(C, dt=f32), dln_g=full(C, dt=f32), dln_b=full(C, dt=f32))
    for name, t in chain.items():
        for e in offsets(t)[1:]:
            if (e * t.element_size()) % 16 == 0:
                continue
            o = dict(chain)
            o[name] = at_offset(t, e)
            dx, dbias, dhs = full(N, C), full(nH, 64, 64, dt=f32), full(nH, dt=f32)
            ws = torch.empty(nws, device=DEV)
            st = lib.hs_window_attn_module_bwd_chain(ptr(z(N, C)), ptr(z(N, C)), ptr(z(N, C)), ptr(z(N, dt=f32)), ptr(torch.ones(N, device=DEV)),
                                                     ptr(z(N, 3 * C)), ptr(z(N, C)), ptr(z(nH, N, dt=f32)), ptr(o["qkv_w_t"]), ptr(o["proj_w_t"]),
                                                     ptr(o["ln_g"]), ptr(base["bias"]), ptr(base["hs"]), None, 0, None, ptr(dx), ptr(o["dqkv_w"]),
                                                     ptr(o["dqkv_b"]), ptr(o["dproj_w"]), ptr(o["dproj_b"]), ptr(o["dln_g"]), ptr(o["dln_b"]),
                                                     ptr(dbias), ptr(dhs), ptr(ws), 0, 1, N, C, nH, 64, L.HS_ATTN_RESIDUAL, L.HS_BF16, S)
            keep = [dx, dbias, dhs] + [v for k, v in o.items() if k.startswith("d")]
            assert not c_call(st, f"hs_window_attn_module_bwd_chain {name}+{e}", keep)
    # ---- the tails with the loss inside: tokens 64, C = 64, 5 classes / 1 depth channel
    T, Ct, K = 64, 64, 5
    rows = 4 * T
    tail = dict(wexp=z(4 * Ct, Ct), wfold=z(64, Ct), bvec=z(32, dt=f32), afold=z(Ct, 32))
    labels = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    target = z(rows, dt=f32)
    scale = torch.ones(1, device=DEV)
    nparts = 4 * int(lib.hs_expand_ln_head_blocks(T))
    for name, t in tail.items():
        for e in offsets(t)[1:]:
            if (e * t.element_size()) % 16 == 0:
                continue
            o = dict(tail)
            o[name] = at_offset(t, e)
            if name != "afold":  # the three forward entry points
                for entry in ("ce", "ce_step", "depth"):
                    y, mean, rstd, parts = full(rows, Ct), full(rows, dt=f32), full(rows, dt=f32), full(nparts, 2, dt=f32)
                    preds = torch.full((rows,), 7, dtype=torch.uint8, device=DEV)
                    if entry == "ce":
                        st = lib.hs_expand_ln_head_ce_fwd(ptr(z(T, Ct)), None, ptr(o["wexp"]), ptr(o["wfold"]), ptr(o["bvec"]), ptr(labels), None, K,
                                                          ptr(y), None, ptr(mean), ptr(rstd), ptr(parts), T, Ct, 4, L.HS_BF16, S)
                    elif entry == "ce_step":
                        st = lib.hs_expand_ln_head_ce_step_fwd(ptr(z(T, Ct)), None, ptr(o["wexp"]), ptr(o["wfold"]), ptr(o["bvec"]), ptr(labels), None,
                                                               K, ptr(y), None, ptr(mean), ptr(rstd), ptr(parts), ptr(preds), None, None, T, Ct, 4,
                                                               L.HS_BF16, S)
                    else:
                        st = lib.hs_expand_ln_head_depth_fwd(ptr(z(T, Ct)), None, ptr(o["wexp"]), ptr(o["wfold"]), ptr(o["bvec"]), ptr(target),
                                                             L.HS_DEPTH_L2, 1.0, 1, ptr(y), None, ptr(mean), ptr(rstd), ptr(parts), T, Ct, 4,
                                                             L.HS_BF16, S)
                    assert not c_call(st, f"hs_expand_ln_head_{entry}_fwd {name}+{e}", [y, mean, rstd, parts, preds])
            if name != "wexp":  # the two backward entry points
                for entry in ("ce", "depth"):
                    dy, dprime = full(rows, Ct), full(rows, 32)
                    part = full(int(lib.hs_ln_head_partials(rows)), 32, dt=f32)
                    if entry == "ce":
                        st = lib.hs_ln_head_ce_bwd(ptr(z(rows, Ct)), ptr(z(rows, dt=f32)), ptr(torch.ones(rows, device=DEV)), ptr(labels), None,
                                                   ptr(scale), K, ptr(o["wfold"]), ptr(o["bvec"]), ptr(o["afold"]), ptr(dy), ptr(dprime), ptr(part),
                                                   rows, Ct, L.HS_BF16, S)
                    else:
                        st = lib.hs_ln_head_depth_bwd(ptr(z(rows, Ct)), ptr(z(rows, dt=f32)), ptr(torch.ones(rows, device=DEV)), ptr(target),
                                                      L.HS_DEPTH_L2, 1.0, ptr(scale), 1, ptr(o["wfold"]), ptr(o["bvec"]), ptr(o["afold"]), ptr(dy),
                                                      ptr(dprime), ptr(part), rows, Ct, L.HS_BF16, S)
                    assert not c_call(st, f"hs_ln_head_{entry}_bwd {name}+{e}", [dy, dprime, part])


# ----------------------------------------------------------------------------- bf16 x 3 splits (float4 loads, uint2 stores)
def test_split3_entry_points_refuse_before_launch_and_their_ops_fall_back():
    """hs_split_bf16x3 / hs_gelu_split3: x and dy need 16 bytes, the bf16 output 8.  Residues 4 and 8 of a source and residue 4 of the
    output are refused before anything is launched; an output 8 bytes behind an aligned base is legal and gives the aligned call's
    bits.  ops.gemm.split3 / _weight_split take a view one element into a buffer through an aligned copy."""
    from heal_swin_amd.ops import gemm as G
    L = _lib()
    lib, ptr = L.lib, L.ptr
    rows, k = 36, 24  # (both multiples of 4: the transposed weight split has k = rows)
    x0 = torch.randn(rows, k, device=DEV)
    dy0 = torch.randn(rows, k, device=DEV)

    def out_buf():
        return torch.full((rows, 3 * k), SENTINEL, dtype=BF, device=DEV)
    want = {}
    for mode in (0, 1):
        want[mode] = out_buf()
        L.check(lib.hs_split_bf16x3(ptr(x0), ptr(want[mode]), rows, k, mode, _stream()), "hs_split_bf16x3")
    want_f, want_b = out_buf(), out_buf()
    L.check(lib.hs_gelu_split3(None, ptr(x0), ptr(want_f), rows, k, 0.3, 5, _stream()), "hs_gelu_split3")
    L.check(lib.hs_gelu_split3(ptr(dy0), ptr(x0), ptr(want_b), rows, k, 0.3, 5, _stream()), "hs_gelu_split3")
    hi = x0.bfloat16()
    assert torch.equal(want[1].view(torch.int16), torch.cat([hi, (x0 - hi.float()).bfloat16(), hi], 1).view(torch.int16))
    for e in E_F32[1:]:  # sources at 4 and 8 bytes
        x, dy = at_offset(x0, e), at_offset(dy0, e)
        for mode in (0, 1):
            y = out_buf()
            assert not c_call(lib.hs_split_bf16x3(ptr(x), ptr(y), rows, k, mode, _stream()), f"hs_split_bf16x3 x+{e}", [y])
        y = out_buf()
        assert not c_call(lib.hs_gelu_split3(None, ptr(x), ptr(y), rows, k, 0.3, 5, _stream()), f"hs_gelu_split3 x+{e}", [y])
        assert not c_call(lib.hs_gelu_split3(ptr(dy0), ptr(x), ptr(y), rows, k, 0.3, 5, _stream()), f"hs_gelu_split3 bwd x+{e}", [y])
        assert not c_call(lib.hs_gelu_split3(ptr(dy), ptr(x0), ptr(y), rows, k, 0.3, 5, _stream()), f"hs_gelu_split3 dy+{e}", [y])
    yo = at_offset(out_buf(), 2)  # output at 4 bytes
    assert not c_call(lib.hs_split_bf16x3(ptr(x0), ptr(yo), rows, k, 1, _stream()), "hs_split_bf16x3 out+2", [yo])
    assert not c_call(lib.hs_gelu_split3(None, ptr(x0), ptr(yo), rows, k, 0.3, 5, _stream()), "hs_gelu_split3 out+2", [yo])
    yo = at_offset(out_buf(), 4)  # output at 8 bytes: what its uint2 stores need
    assert c_call(lib.hs_split_bf16x3(ptr(x0), ptr(yo), rows, k, 1, _stream()), "hs_split_bf16x3 out+4")
    assert torch.equal(yo.view(torch.int16), want[1].view(torch.int16))
    assert c_call(lib.hs_gelu_split3(ptr(dy0), ptr(x0), ptr(yo), rows, k, 0.3, 5, _stream()), "hs_gelu_split3 out+4")
    assert torch.equal(yo.view(torch.int16), want_b.view(torch.int16))
    # the ops: a view one element into a buffer
    buf = torch.zeros(rows * k + 1, device=DEV)
    v = buf[1:].view(rows, k)
    v.copy_(x0)
    assert v.data_ptr() % 16 == 4
    for mode in (0, 1):
        assert torch.equal(G.split3(v, mode).view(torch.int16), want[mode].view(torch.int16)), f"ops.gemm.split3 mode {mode}"
    assert torch.equal(G._weight_split(v, False).view(torch.int16), want[1].view(torch.int16))
    assert torch.equal(G._weight_split(v, True).view(torch.int16), G.split3(x0.t().contiguous(), 1).view(torch.int16))
