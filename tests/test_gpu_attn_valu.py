"""Operator-level tests of the fp32-VALU attention kernels (csrc/window_attn_generic.hip) and of the attention dropout mask of all
four kernel families (`DropRng`, csrc/window_attn.h).

Reference: the composition of test_gpu_kernels._oracle_core written out in FLOAT64 with autograd (`reference`; it also returns the
log-sum-exp and takes the dropout multiplier), on the values the kernel sees (inputs rounded to the activation dtype first);
`test_reference_is_the_oracle_composition` ties it to `_oracle_core` on double tensors.  Dropout enters as P * keep / (1 - p) with
`keep` from the HOST reference of the mask (tests/_attn_mask_ref.py), so dropout runs are full forward / backward comparisons.

Inputs are hostile on purpose: `idx` a random permutation of N (not a HEALPix table), `labels` random in {0, 1, 2} per shifted
position, random bias and per-head scales, cosine and scaled form, table and roll form (rolls N - 1 and Ws / 2 + 1: the `s >= N`
wrap taken and not taken inside one window).

Shapes: one thread per (image, shifted position, head) row, a workgroup covers max(64, Ws) rows of one head.
  head-dim sweep  Ws 16, nH 3, B 2, N 48: 96 rows = 2 workgroups, the first spans images 0 and 1, the second is half empty; head_dim
                  1 ... 128 puts every template HD in {2, 4, 8, 16, 32, 64, 128} once at its top and once at a padded head dim; nH 3
                  makes the h * hd offset odd
  window sweep    every Ws in {4, 8, 16, 32, 64, 128, 256}; the backward's largest head dims at Ws 128 (64) and 256 (32)
Each test asserts its own precondition (B * N % 64 != 0 and an image boundary strictly inside a workgroup, for Ws < 64).

Exact probes (C ABI, fp32, torch.equal): q = 0 makes every probability exactly 1 / Ws, so `out` EQUALS the window mean of an integer
v and dv the window mean of an integer dout; out, lse and dqkv are views into guarded buffers, qkv and dout continue with NaN rows.
The decoded dropout masks and the "untouched" sentinels of the refused shapes are equalities too.

Bounds: TOL / GRAD_TOL of _util.py are the pass / fail line everywhere, with assert_unbiased on dqkv and dbias.  fp32 I/O against
float64 is far better than that; the second, tight bound `TIGHT` is 10 x the worst max|a-b|/max|b| measured over the fp32 VALU cases
of this file on an MI355X, rounded up to one significant digit (the factor covers the order of the dbias atomics and expf / logf
differences across seeds):
  fp32 I/O, shape classes and dropout    out 1.7e-6   dqkv 1.6e-6   dbias 1.3e-6   dhead_scale 4.5e-6
  TIGHT                                   out 2e-5     dqkv 2e-5     dbias 2e-5     dhead_scale 5e-5
The numeric edges are held to TOL / GRAD_TOL (their tensors cancel, so their own scale is not that of the shape classes); measured:
scores spread over +-150 out 5.2e-6, dqkv 1.3e-5 (dbias / dhead_scale cancel to ~1e-11 there and take an absolute floor); every key
masked: dbias 4.5e-4, dhead_scale 1.6e-5; the 1 / eps rows of the zero-norm case 2.5e-7 of their 1e12.
bf16 I/O: out 3.8e-3, dqkv 3.9e-3 (the output rounding), dbias 1.0e-6, dhead_scale 8.3e-6; against the rounded fp32 results
<= 0.95 bf16 ulp.  (Before the bf16 backward formed D = rowsum(P o dP) itself instead of dO . O from the ROUNDED saved output, the
same cases gave dqkv up to 50 bf16 ulp and dhead_scale 4.4e-2, over GRAD_TOL[bf16]: found by these tests.)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _attn_mask_ref as AR
from _util import GRAD_TOL, TOL, assert_close, assert_unbiased, errors

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
HS_ERR_UNSUPPORTED = 2
PAD, GUARD, TAIL = 64, 12345.0, 8  # guard elements around out / lse / dqkv and their value; NaN rows behind qkv / dout

# 10 x the worst scale_err of the fp32 VALU cases against float64 (module docstring); None: measure only
TIGHT = dict(out=2e-5, dqkv=2e-5, dbias=2e-5, dscale=5e-5)


def _L():
    from heal_swin_amd import _lib
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- float64 reference
def source_table(N, idx, roll):
    """Token read by every shifted position: the table, or (j + roll) mod N."""
    return idx.long() if idx is not None else (torch.arange(N) + roll) % N


def reference(qkv, bias, hscale, src, labels, nH, Ws, cosine, mult=None):
    """(out [B, N, C] natural order, lse [B, nH, N] shifted order) of the fused op, in the dtype of its arguments (float64 here).
    `mult` [B, N / Ws, nH, Ws, Ws]: the dropout multiplier of every probability (0 or 1 / (1 - p))."""
    B, N, C3 = qkv.shape
    C, hd, nW = C3 // 3, C3 // 3 // nH, N // Ws
    t = qkv[:, src].reshape(B, nW, Ws, 3, nH, hd)
    q, k, v = (t[:, :, :, i].permute(0, 1, 3, 2, 4) for i in range(3))  # [B, nW, nH, Ws, hd]
    if cosine:
        q, k = F.normalize(q, dim=-1, eps=1e-12), F.normalize(k, dim=-1, eps=1e-12)
    s = (q @ k.transpose(-1, -2)) * hscale.reshape(1, 1, nH, 1, 1)
    if bias is not None:
        s = s + bias[None, None]
    if labels is not None:
        lab = labels.reshape(nW, Ws).long()
        s = s + (lab[:, :, None] != lab[:, None, :]).to(s.dtype)[None, :, None] * -100.0  # additive, not -inf (as the reference)
    lse = torch.logsumexp(s, dim=-1)  # [B, nW, nH, Ws]
    p = torch.softmax(s, dim=-1)
    if mult is not None:
        p = p * mult
    o = (p @ v).permute(0, 1, 3, 2, 4).reshape(B, N, C)
    return o[:, torch.argsort(src)], lse.permute(0, 2, 1, 3).reshape(B, nH, N)


def mask_rows(B, N, nH):
    """DropRng's row number of every (image, head, shifted row): [B, nH, N]."""
    return (np.arange(B * nH, dtype=np.int64).reshape(B, nH, 1) * N + np.arange(N, dtype=np.int64)).astype(np.uint64)


def host_keep(B, N, nH, Ws, p, seed):
    """Keep decisions of the host reference, [B, nH, N, Ws] bool."""
    return AR.keep(mask_rows(B, N, nH)[..., None], np.arange(Ws, dtype=np.uint64), p, seed)


def host_mult(B, N, nH, Ws, p, seed):
    k = torch.from_numpy(host_keep(B, N, nH, Ws, p, seed)).double() * AR.keep_scale(p)
    return k.reshape(B, nH, N // Ws, Ws, Ws).permute(0, 2, 1, 3, 4)


# ----------------------------------------------------------------------------- inputs and runs
@functools.lru_cache(maxsize=None)
def make_inputs(B, N, nH, hd, Ws):
    """fp32 host tensors of one shape, made once and never changed."""
    g = torch.Generator().manual_seed(1000 * Ws + 10 * hd + nH + N)
    C = nH * hd
    return dict(B=B, N=N, nH=nH, hd=hd, C=C, Ws=Ws,
                qkv=torch.randn(B, N, 3 * C, generator=g), dout=torch.randn(B, N, C, generator=g),
                bias=torch.randn(nH, Ws, Ws, generator=g),
                hs_cos=torch.rand(nH, generator=g) * 8 + 0.1, hs_scaled=torch.rand(nH, generator=g) * 0.3 + 0.1,
                idx=torch.randperm(N, generator=g), labels=torch.randint(0, 3, (N,), generator=g).to(torch.uint8))


def shift_modes(inp):
    N, Ws = inp["N"], inp["Ws"]
    return [("idx", inp["idx"], 0), ("roll" + str(N - 1), None, N - 1), ("roll" + str(Ws // 2 + 1), None, Ws // 2 + 1)]


def run_reference(inp, dtype, cosine, idx, roll, qkv=None, dout=None, bias="default", labels="default", hscale=None, drop=0.0, seed=0):
    """float64 forward + backward on the inputs rounded to `dtype`."""
    B, N, nH, Ws = inp["B"], inp["N"], inp["nH"], inp["Ws"]
    qkv = (inp["qkv"] if qkv is None else qkv).to(dtype).double().requires_grad_(True)
    dout = (inp["dout"] if dout is None else dout).to(dtype).double()
    bias = inp["bias"] if isinstance(bias, str) else bias
    labels = inp["labels"] if isinstance(labels, str) else labels
    bias = None if bias is None else bias.double().requires_grad_(True)
    hs = (hscale if hscale is not None else inp["hs_cos" if cosine else "hs_scaled"]).double().requires_grad_(True)
    mult = host_mult(B, N, nH, Ws, drop, seed) if drop > 0 else None
    out, lse = reference(qkv, bias, hs, source_table(N, idx, roll), labels, nH, Ws, cosine, mult)
    out.backward(dout)
    return dict(out=out.detach(), lse=lse.detach(), dqkv=qkv.grad, dbias=None if bias is None else bias.grad,
                dscale=hs.grad if cosine else None)


def run_ops(inp, dtype, cosine, idx, roll, qkv=None, dout=None, bias="default", labels="default", hscale=None, drop=0.0, seed=0, valu=False):
    """Forward + backward of ops.window_attn_core (the production route of the shape, or the VALU kernels with `valu`)."""
    from heal_swin_amd import ops
    qkv = (inp["qkv"] if qkv is None else qkv).to(DEV).to(dtype).clone().requires_grad_(True)
    dout = (inp["dout"] if dout is None else dout).to(DEV).to(dtype)
    bias = inp["bias"] if isinstance(bias, str) else bias
    labels = inp["labels"] if isinstance(labels, str) else labels
    bias = None if bias is None else bias.to(DEV).clone().requires_grad_(True)
    hs = (hscale if hscale is not None else inp["hs_cos" if cosine else "hs_scaled"]).to(DEV).clone().requires_grad_(True)
    prev = ops.FORCE_VALU_ATTENTION
    ops.FORCE_VALU_ATTENTION = bool(valu)
    try:
        out = ops.window_attn_core(qkv, bias, hs, None if idx is None else idx.to(torch.int32).to(DEV), roll,
                                   None if labels is None else labels.to(DEV), inp["nH"], inp["Ws"], cosine, attn_drop=drop, seed=seed)
        out.backward(dout)
    finally:
        ops.FORCE_VALU_ATTENTION = prev
    assert out.dtype == dtype and qkv.grad.dtype == dtype
    return dict(out=out.detach(), dqkv=qkv.grad, dbias=None if bias is None else bias.grad, dscale=hs.grad if cosine else None)


def check(got, ref, dtype, tag, tight=True, floor=0.0):
    """The project's bounds, no systematic error, and (fp32 VALU cases) the tight bound; prints every figure.  `floor`: absolute error
    accepted on dbias / dhead_scale where they cancel to zero in exact arithmetic."""
    for name, tol in (("out", TOL[dtype]), ("dqkv", GRAD_TOL[dtype]), ("dbias", GRAD_TOL[dtype]), ("dscale", GRAD_TOL[dtype])):
        if ref[name] is None:
            continue
        assert bool(torch.isfinite(got[name].float()).all()), f"{tag} {name}: not finite"
        e = errors(got[name].double().cpu(), ref[name])["scale_err"]
        print(f"MEASURED {'tight' if tight and dtype == F32 else 'loose'} {name} {e:.3e} {tag} {str(dtype)[6:]}")
        assert_close(got[name].double().cpu(), ref[name], tol, f"{tag} {name}", floor=floor if name in ("dbias", "dscale") else 0.0)
        if name in ("dqkv", "dbias"):
            assert_unbiased(got[name].double().cpu(), ref[name], f"{tag} {name}")
        if tight and dtype == F32 and TIGHT is not None:
            assert e <= TIGHT[name], f"{tag} {name}: {e:.3e} of the tensor's scale against float64 > tight bound {TIGHT[name]}"


def assert_ragged_and_straddling(B, N, Ws):
    """For Ws < 64 a workgroup is 64 rows of the flat (image, shifted position) axis: the last one must be partly empty and one must
    hold rows of two images."""
    assert Ws < 64
    assert (B * N) % 64 != 0, "no ragged last workgroup"
    assert any((b * N) % 64 != 0 for b in range(1, B)), "no image boundary strictly inside a workgroup"


def sweep(B, N, nH, hd, Ws, dtype, valu=False):
    inp = make_inputs(B, N, nH, hd, Ws)
    for cosine in (True, False):
        for name, idx, roll in shift_modes(inp):
            ref = run_reference(inp, dtype, cosine, idx, roll)
            got = run_ops(inp, dtype, cosine, idx, roll, valu=valu)
            check(got, ref, dtype, f"Ws{Ws} hd{hd} {'cos' if cosine else 'scaled'} {name}")


def test_reference_is_the_oracle_composition():
    """`reference` equals test_gpu_kernels._oracle_core evaluated on double tensors (its primitives keep the dtype)."""
    from test_gpu_kernels import _oracle_core
    inp = make_inputs(2, 48, 3, 5, 16)
    for cosine in (True, False):
        hs = inp["hs_cos" if cosine else "hs_scaled"].double()
        a, _ = reference(inp["qkv"].double(), inp["bias"].double(), hs, inp["idx"], inp["labels"], 3, 16, cosine)
        b = _oracle_core(inp["qkv"].double(), inp["bias"].double(), hs, inp["idx"], inp["labels"], 3, 16, cosine)
        assert b.dtype == torch.float64 and float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())


# ----------------------------------------------------------------------------- shape classes
HEAD_DIMS = [1, 2, 3, 4, 5, 8, 12, 16, 24, 32, 40, 64, 96, 128]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_head_dim_sweep(hd, dtype):
    B, N, nH, Ws = 2, 48, 3, 16
    assert_ragged_and_straddling(B, N, Ws)
    sweep(B, N, nH, hd, Ws, dtype)


def test_head_dims_cover_every_template_at_its_top_and_padded():
    tmpl = lambda hd: next(t for t in (2, 4, 8, 16, 32, 64, 128) if hd <= t)  # noqa: E731
    tops = {hd for hd in HEAD_DIMS if tmpl(hd) == hd}
    padded = {tmpl(hd) for hd in HEAD_DIMS if tmpl(hd) != hd}
    assert tops == {2, 4, 8, 16, 32, 64, 128} and padded == {2, 4, 8, 16, 32, 64, 128}


WINDOW_CASES = [  # Ws, B, N, head_dim, forced VALU
    (4, 3, 40, 8, False), (8, 3, 40, 8, False), (16, 3, 48, 8, False), (32, 3, 96, 8, False), (64, 3, 128, 8, False),
    (64, 2, 128, 32, True), (128, 2, 256, 8, False), (128, 2, 256, 64, False), (256, 2, 512, 8, False), (256, 2, 512, 32, False),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("Ws,B,N,hd,valu", WINDOW_CASES, ids=[f"Ws{c[0]}-hd{c[3]}" for c in WINDOW_CASES])
def test_window_sweep(Ws, B, N, hd, valu, dtype):
    if Ws < 64:
        assert_ragged_and_straddling(B, N, Ws)
    assert valu == (Ws == 64 and hd == 32)  # every other shape is served by the VALU kernels anyway
    sweep(B, N, 2, hd, Ws, dtype, valu=valu)


# ----------------------------------------------------------------------------- C ABI
def abi_fwd(qkv, out, lse, bias, hs, idx, roll, labels, B, N, C, nH, Ws, flags=0, drop=0.0, seed=0):
    L = _L()
    return int(L.lib.hs_window_attn_fwd(L.ptr(qkv), L.ptr(out), L.ptr(lse), L.ptr(bias), L.ptr(hs), L.ptr(idx), int(roll), L.ptr(labels),
                                        B, N, C, nH, Ws, flags, float(drop), int(seed), L.dtype_code(qkv.dtype), _stream()))


def abi_bwd(qkv, out, dout, lse, dqkv, dbias, dscale, wsp, bias, hs, idx, roll, labels, B, N, C, nH, Ws, flags=0, drop=0.0, seed=0):
    L = _L()
    return int(L.lib.hs_window_attn_bwd(L.ptr(qkv), L.ptr(out), L.ptr(dout), L.ptr(lse), L.ptr(dqkv), L.ptr(dbias), L.ptr(dscale), L.ptr(wsp),
                                        L.ptr(bias), L.ptr(hs), L.ptr(idx), int(roll), L.ptr(labels), B, N, C, nH, Ws, flags, float(drop),
                                        int(seed), L.dtype_code(qkv.dtype), _stream()))


def ok(status, what):
    _L().check(status, what)


def guarded(shape, dtype=F32):
    """(buffer, view): a contiguous tensor of `shape` inside a buffer that continues with guard elements on both sides."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), GUARD, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def guards_intact(buf):
    return bool((buf[:PAD] == GUARD).all()) and bool((buf[-PAD:] == GUARD).all())


def with_nan_rows(t):
    """t [B, N, W] as the first B * N rows of an allocation that continues with NaN rows."""
    B, N, W = t.shape
    buf = torch.full((B * N + TAIL, W), float("nan"), dtype=t.dtype, device=DEV)
    buf[:B * N] = t.reshape(B * N, W)
    return buf, buf[:B * N].view(B, N, W)


def tables(N, Ws, mode, g):
    """(idx int32 on the device or None, roll, source table on the host) of a shift mode."""
    if mode == "idx":
        idx = torch.randperm(N, generator=g)
        return idx.to(torch.int32).to(DEV), 0, idx
    roll = N - 1 if mode == "wrap" else Ws // 2 + 1
    return None, roll, source_table(N, None, roll)


PROBE_WS = [4, 8, 16, 32, 64, 128, 256]


@pytest.mark.parametrize("mode", ["idx", "wrap", "inside"])
@pytest.mark.parametrize("Ws", PROBE_WS)
def test_uniform_probabilities_give_exact_window_means(Ws, mode):
    """q = 0, no bias, no labels: every probability is exactly 1 / Ws.  out == window mean of the integer v at the right natural token,
    lse == log Ws to 2 ulp, and for an integer dout dv == (1 / Ws) * sum of the window's dout rows -- all exact (integers of
    magnitude <= 3 Ws times a power of two).  Guards around out / lse / dqkv keep their value; NaN rows follow qkv and dout."""
    B, N, nH, hd = 3, 2 * Ws if Ws >= 64 else 40 if Ws <= 8 else 3 * Ws, 3, 5  # head_dim 5: padded to the template of 8
    C = nH * hd
    g = torch.Generator().manual_seed(Ws)
    idx, roll, src = tables(N, Ws, mode, g)
    qkv = torch.randn(B, N, 3 * C, generator=g)
    qkv[:, :, :C] = 0
    qkv[:, :, 2 * C:] = torch.randint(-3, 4, (B, N, C), generator=g).float()
    dout = torch.randint(-3, 4, (B, N, C), generator=g).float()
    hs = (torch.rand(nH, generator=g) + 0.5).to(DEV)
    qbuf, qkv_d = with_nan_rows(qkv.to(DEV))
    dbuf, dout_d = with_nan_rows(dout.to(DEV))
    obuf, out = guarded((B, N, C))
    lbuf, lse = guarded((B, nH, N))
    gbuf, dqkv = guarded((B, N, 3 * C))
    ok(abi_fwd(qkv_d, out, lse, None, hs, idx, roll, None, B, N, C, nH, Ws), "hs_window_attn_fwd")
    ok(abi_bwd(qkv_d, out, dout_d, lse, dqkv, None, None, None, None, hs, idx, roll, None, B, N, C, nH, Ws), "hs_window_attn_bwd")
    torch.cuda.synchronize()
    assert guards_intact(obuf) and guards_intact(lbuf) and guards_intact(gbuf), "wrote beside out / lse / dqkv"
    assert bool(torch.isnan(qbuf[B * N:]).all()) and bool(torch.isnan(dbuf[B * N:]).all())

    def window_mean(t):  # natural [B, N, C] -> the mean over the window of every token, back in natural order
        m = t[:, src].reshape(B, N // Ws, Ws, C).double().mean(dim=2, keepdim=True).expand(-1, -1, Ws, -1).reshape(B, N, C)
        return m[:, torch.argsort(src)].float()

    assert torch.equal(out.cpu(), window_mean(qkv[:, :, 2 * C:])), "out is not the window mean of v"
    want = torch.full((B, nH, N), float(np.log(np.float64(Ws))), dtype=torch.float64).float()
    ulp = float(np.spacing(np.float32(np.log(Ws))))
    assert float((lse.cpu() - want).abs().max()) <= 2 * ulp, "lse is not log Ws to 2 ulp"
    assert torch.equal(dqkv[:, :, 2 * C:].cpu(), window_mean(dout)), "dv is not the window mean of dout"
    assert bool(torch.isfinite(dqkv).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("hd", [3, 5, 12])
def test_one_hot_dout_leaves_the_other_heads_exactly_zero(hd, dtype):
    """The pad channels between head_dim and the template do not exist in memory: the channel behind a head's last one is the next
    head's first (or k's, or v's).  Random q, k, v whose heads differ in scale; dout is one-hot in head h: dqkv of
    every other head is exactly zero, that of head h is not, and equals the run on head h's columns alone."""
    B, N, nH, Ws = 2, 48, 3, 16
    C = nH * hd
    g = torch.Generator().manual_seed(hd)
    idx = torch.randperm(N, generator=g)
    head_of = torch.arange(C) // hd
    qkv = torch.randn(B, N, 3, C, generator=g) * (4.0 ** head_of.float())  # heads at scales 1, 4, 16: a neighbour is distinctive
    qkv = qkv.reshape(B, N, 3 * C).to(dtype)
    hs = torch.full((nH,), 0.01, device=DEV)
    for h in range(nH):
        dout = torch.zeros(B, N, C)
        dout[1, 7, h * hd + hd - 1] = 1.0
        qkv_d, dout_d = qkv.to(DEV), dout.to(DEV).to(dtype)
        out, lse, dqkv = torch.empty(B, N, C, device=DEV, dtype=dtype), torch.empty(B, nH, N, device=DEV), torch.empty(B, N, 3 * C, device=DEV, dtype=dtype)
        ok(abi_fwd(qkv_d, out, lse, None, hs, idx.to(torch.int32).to(DEV), 0, None, B, N, C, nH, Ws), "hs_window_attn_fwd")
        ok(abi_bwd(qkv_d, out, dout_d, lse, dqkv, None, None, None, None, hs, idx.to(torch.int32).to(DEV), 0, None, B, N, C, nH, Ws),
           "hs_window_attn_bwd")
        d = dqkv.float().cpu().reshape(B, N, 3, C)
        other = head_of != h
        assert bool((d[:, :, :, other] == 0).all()), f"one-hot dout in head {h} reached another head's dqkv"
        assert float(d[:, :, :, ~other].abs().max()) > 0 and bool(torch.isfinite(d).all())
        # head h alone (C = hd, one head): the same numbers
        q1 = qkv.reshape(B, N, 3, C)[:, :, :, ~other].reshape(B, N, 3 * hd).contiguous().to(DEV)
        o1, l1, g1 = torch.empty(B, N, hd, device=DEV, dtype=dtype), torch.empty(B, 1, N, device=DEV), torch.empty(B, N, 3 * hd, device=DEV, dtype=dtype)
        ok(abi_fwd(q1, o1, l1, None, hs[h:h + 1].clone(), idx.to(torch.int32).to(DEV), 0, None, B, N, hd, 1, Ws), "hs_window_attn_fwd")
        ok(abi_bwd(q1, o1, dout_d[:, :, h * hd:(h + 1) * hd].contiguous(), l1, g1, None, None, None, None, hs[h:h + 1].clone(),
                   idx.to(torch.int32).to(DEV), 0, None, B, N, hd, 1, Ws), "hs_window_attn_bwd")
        assert torch.equal(out[:, :, h * hd:(h + 1) * hd], o1) and torch.equal(lse[:, h], l1[:, 0])
        assert torch.equal(dqkv.reshape(B, N, 3, C)[:, :, :, ~other.to(DEV)].reshape(B, N, 3 * hd), g1)


# ----------------------------------------------------------------------------- numeric edges (fp32 I/O against float64)
EDGE_SHAPES = [(8, 3, 40), (64, 2, 128)]  # Ws, B, N; nH 2, head_dim 8: the VALU kernels


def _unshift(t_shifted, src):
    """A tensor laid out by shifted position -> natural token order."""
    return t_shifted[:, torch.argsort(src)]


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("cosine", [False, True], ids=["scaled", "cos"])
@pytest.mark.parametrize("Ws,B,N", EDGE_SHAPES)
def test_score_spread(Ws, B, N, cosine, where):
    """Scores spread over +-150 (scaled: q . k itself) or +-130 (cosine: head_scale 100 and a bias of +-30) inside every row, the row
    maximum in the first or in the last group of four keys: the online-softmax rescale expf(m - m_new) runs from -inf and either never
    again or across large steps."""
    nH, hd = 2, 8
    inp = make_inputs(B, N, nH, hd, Ws)
    C, g = nH * hd, torch.Generator().manual_seed(Ws + 7)
    src = inp["idx"]
    ramp = torch.linspace(1.0, -1.0, Ws)  # by key position inside the window
    if where == "last":
        ramp = ramp.flip(0)
    t = torch.randn(B, N // Ws, Ws, 3, nH, hd, generator=g) * 0.05  # [q|k|v][head][channel] by SHIFTED position
    t[..., 2, :, :] = torch.randn(B, N // Ws, Ws, nH, hd, generator=g)
    if cosine:
        t[..., 0, :, 0] += 1.0
        t[..., 1, :, 0] += ramp[None, None, :, None]
        t[..., 1, :, 1] += (1 - ramp * ramp).sqrt()[None, None, :, None]
        hscale = torch.full((nH,), 100.0)
        bias = (30.0 * ramp)[None, None, :].expand(nH, Ws, Ws) + 0.1 * torch.randn(nH, Ws, Ws, generator=g)
    else:
        t[..., 0, :, 0] += 1.0
        t[..., 1, :, 0] += 150.0 * ramp[None, None, :, None]
        hscale = torch.ones(nH)
        bias = None
    qkv = _unshift(t.reshape(B, N, 3 * C), src)
    ref = run_reference(inp, F32, cosine, src, 0, qkv=qkv, bias=bias, labels=None, hscale=hscale)
    got = run_ops(inp, F32, cosine, src, 0, qkv=qkv, bias=bias, labels=None, hscale=hscale)
    # one key takes the whole probability, so every addend P (dP - D) of dbias and dhead_scale cancels to ~0 in exact arithmetic
    # (reference scale 1e-11) and the fp32 value is the rounding of dP - D: 2^-20 |dO| |v| head_dim per addend, B N / Ws addends
    floor = (B * N // Ws) * hd * 2.0 ** -20 * float(inp["dout"].abs().max()) * float(qkv[:, :, 2 * C:].abs().max())
    check(got, ref, F32, f"spread Ws{Ws} {'cos' if cosine else 'scaled'} max-{where}", tight=False, floor=floor)
    e = {k: errors(got[k].double().cpu(), ref[k])["scale_err"] for k in ("out", "dqkv")}
    print(f"MEASURED edge out {e['out']:.3e} dqkv {e['dqkv']:.3e} spread Ws{Ws} cos{int(cosine)} {where}")


@pytest.mark.parametrize("cosine", [False, True], ids=["scaled", "cos"])
@pytest.mark.parametrize("Ws,B,N", EDGE_SHAPES + [(256, 2, 512)])
def test_every_key_masked_but_the_query(Ws, B, N, cosine):
    """labels 0 ... Ws - 1 inside a window: every key but the query's own takes -100, additively (not -inf), exactly as the
    reference; 256 labels fit uint8."""
    inp = make_inputs(B, N, 2, 8, Ws)
    labels = (torch.arange(N) % Ws).to(torch.uint8)
    assert int(labels.max()) == Ws - 1
    ref = run_reference(inp, F32, cosine, inp["idx"], 0, labels=labels)
    got = run_ops(inp, F32, cosine, inp["idx"], 0, labels=labels)
    check(got, ref, F32, f"all-masked Ws{Ws} {'cos' if cosine else 'scaled'}", tight=False)


@pytest.mark.parametrize("Ws,B,N", EDGE_SHAPES)
def test_zero_norm_rows_under_cosine_attention(Ws, B, N):
    """A q row and a k row of exact zeros: q / max(|q|, eps) is 0 and its gradient is dq_hat / eps (F.normalize).  The forward equals the
    reference; the gradients of the two rows are compared on their own scale (the 1 / eps factor would drown the rest), the rest
    without them."""
    nH, hd = 2, 8
    inp = make_inputs(B, N, nH, hd, Ws)
    C = nH * hd
    qkv = inp["qkv"].clone()
    tq, tk = 5, N + 9  # flat token rows (images 0 and 1)
    qkv.view(B * N, 3 * C)[tq, 0:hd] = 0           # q of head 0
    qkv.view(B * N, 3 * C)[tk, C + hd:C + 2 * hd] = 0  # k of head 1
    ref = run_reference(inp, F32, True, inp["idx"], 0, qkv=qkv)
    got = run_ops(inp, F32, True, inp["idx"], 0, qkv=qkv)
    assert bool(torch.isfinite(got["dqkv"]).all())
    gd, rd = got["dqkv"].double().cpu().reshape(B * N, 3 * C).clone(), ref["dqkv"].reshape(B * N, 3 * C).clone()
    for row, cols in ((tq, slice(0, hd)), (tk, slice(C + hd, C + 2 * hd))):
        assert float(rd[row, cols].abs().max()) > 1e9  # the clamp's 1 / eps
        e = assert_close(gd[row, cols], rd[row, cols], GRAD_TOL[F32], f"zero-norm row {row}")
        print(f"MEASURED edge zero-norm row {row}: {e:.3e} of its own scale {float(rd[row, cols].abs().max()):.3e}")
        gd[row, cols] = 0
        rd[row, cols] = 0
    got["dqkv"], ref["dqkv"] = gd.reshape(B, N, 3 * C), rd.reshape(B, N, 3 * C)
    check(got, ref, F32, f"zero-norm Ws{Ws}", tight=False)


# ----------------------------------------------------------------------------- bf16 I/O is one rounding of the fp32 results
@pytest.mark.parametrize("Ws,B,N,hd", [(16, 2, 48, 5), (8, 3, 40, 8), (64, 2, 128, 8), (256, 2, 512, 32)])
def test_bf16_io_is_one_rounding_of_the_fp32_results(Ws, B, N, hd):
    """On bf16-exact inputs both instantiations run the same fp32 arithmetic: the bf16 results are the fp32 results rounded once, to
    within one bf16 ulp per element, |a - b| <= 2^-7 max(|b|, 1e-2 scale).  A second rounding or a bf16 intermediate is ~100 x
    tighter to see here than at TOL[bf16]."""
    inp = make_inputs(B, N, 2, hd, Ws)
    qkv, dout = inp["qkv"].to(BF16).float(), inp["dout"].to(BF16).float()
    for cosine in (True, False):
        a = run_ops(inp, BF16, cosine, inp["idx"], 0, qkv=qkv, dout=dout)
        b = run_ops(inp, F32, cosine, inp["idx"], 0, qkv=qkv, dout=dout)
        for name in ("out", "dqkv"):
            x, y = a[name].double(), b[name].to(BF16).double()
            scale = float(y.abs().max())
            excess = ((x - y).abs() / torch.maximum(y.abs(), torch.full_like(y, 1e-2 * scale))).max()
            print(f"MEASURED one-rounding {name} {float(excess) * 128:.3f} bf16 ulp Ws{Ws} cos{int(cosine)}")
            assert float(excess) <= 2.0 ** -7, f"{name}: {float(excess) * 128:.2f} bf16 ulp from the rounded fp32 result"


# ----------------------------------------------------------------------------- entry-point contracts
def _abi_case(Ws, hd, dtype, nH=2, B=3, cosine=True):
    """Device operands of one C-ABI forward + its saved results."""
    N = 2 * Ws if Ws >= 16 else 40
    inp = make_inputs(B, N, nH, hd, Ws)
    C = nH * hd
    c = dict(B=B, N=N, C=C, nH=nH, Ws=Ws, qkv=inp["qkv"].to(DEV).to(dtype), dout=inp["dout"].to(DEV).to(dtype), bias=inp["bias"].to(DEV),
             hs=inp["hs_cos" if cosine else "hs_scaled"].to(DEV), idx=inp["idx"].to(torch.int32).to(DEV), labels=inp["labels"].to(DEV),
             flags=_L().HS_ATTN_COSINE if cosine else 0)
    c["out"] = torch.empty(B, N, C, device=DEV, dtype=dtype)
    c["lse"] = torch.empty(B, nH, N, device=DEV)
    return inp, c


def _bwd(c, dbias, dscale, flags, wsp=None):
    dqkv = torch.empty_like(c["qkv"])
    st = abi_bwd(c["qkv"], c["out"], c["dout"], c["lse"], dqkv, dbias, dscale, wsp, c["bias"], c["hs"], c["idx"], 0, c["labels"],
                 c["B"], c["N"], c["C"], c["nH"], c["Ws"], flags)
    return st, dqkv


@pytest.mark.parametrize("Ws,hd,dtype", [(16, 5, F32), (16, 5, BF16), (64, 32, F32)], ids=["valu-f32", "valu-bf16", "mfma-f32"])
def test_overwrite_grads_zeroes_the_accumulating_routes(Ws, hd, dtype):
    """HS_ATTN_OVERWRITE_GRADS is a contract of the entry point: the VALU and fp32-MFMA routes accumulate, so the entry point zeroes
    dbias / dhead_scale first.  With the flag and NaN pre-fills the results equal those of a plain call into zeroed buffers; without it,
    result - pre-fill is the gradient.  Tolerance 1e-5 of each tensor's scale: the VALU dbias is a sum of 6 windows' terms in the order
    of the float atomics (<= 6^2 x 2^-24 = 2e-6 even under full cancellation); the integer pre-fill (|x| <= 3) adds roundings at
    magnitude 4, 6 x 2^-22 absolute."""
    L = _L()
    inp, c = _abi_case(Ws, hd, dtype)
    nws = int(L.lib.hs_window_attn_bwd_workspace(c["B"], c["N"], c["C"], c["nH"], Ws, L.dtype_code(dtype)))
    assert (nws == 0) == (Ws != 64), "workspace query: 0 exactly for VALU-only shapes"
    wsp = torch.empty(nws, device=DEV) if nws else None  # (a VALU-route backward takes a null workspace)
    ok(abi_fwd(c["qkv"], c["out"], c["lse"], c["bias"], c["hs"], c["idx"], 0, c["labels"], c["B"], c["N"], c["C"], c["nH"], Ws, c["flags"]),
       "hs_window_attn_fwd")
    shape_b, shape_s = c["bias"].shape, c["hs"].shape
    zb, zs = torch.zeros(shape_b, device=DEV), torch.zeros(shape_s, device=DEV)
    st, dq0 = _bwd(c, zb, zs, c["flags"], wsp)
    ok(st, "hs_window_attn_bwd")
    ref = run_reference(inp, dtype, True, inp["idx"], 0)
    assert_close(zb.double().cpu(), ref["dbias"], GRAD_TOL[dtype], "plain dbias")
    assert_close(zs.double().cpu(), ref["dscale"], GRAD_TOL[dtype], "plain dscale")
    nb, ns = torch.full(shape_b, float("nan"), device=DEV), torch.full(shape_s, float("nan"), device=DEV)
    st, dq1 = _bwd(c, nb, ns, c["flags"] | L.HS_ATTN_OVERWRITE_GRADS, wsp)
    ok(st, "hs_window_attn_bwd")
    assert torch.equal(dq0, dq1)
    assert_close(nb, zb, 1e-5, "dbias with the flag, NaN pre-fill")
    assert_close(ns, zs, 1e-5, "dhead_scale with the flag, NaN pre-fill")
    g = torch.Generator().manual_seed(3)
    pb, ps = torch.randint(-3, 4, shape_b, generator=g).float().to(DEV), torch.randint(-3, 4, shape_s, generator=g).float().to(DEV)
    ab, as_ = pb.clone(), ps.clone()
    st, dq2 = _bwd(c, ab, as_, c["flags"], wsp)
    ok(st, "hs_window_attn_bwd")
    assert torch.equal(dq0, dq2)
    floor = 6 * 2.0 ** -22
    assert_close(ab - pb, zb, 1e-5, "dbias accumulated onto integers", floor=floor)
    assert_close(as_ - ps, zs, 1e-5, "dhead_scale accumulated onto integers", floor=floor)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("Ws,hd", [(128, 96), (256, 64)])
def test_backward_beyond_the_lds_is_refused_and_writes_nothing(Ws, hd, dtype):
    """The forward keeps K and V rows of a workgroup in LDS, the backward q, k, v and dout rows: at (Ws 128, head_dim 65 ... 128) and
    (Ws 256, head_dim 33 ... 64) the forward runs (and matches the reference) and the backward returns HS_ERR_UNSUPPORTED -- before
    the zero fill of HS_ATTN_OVERWRITE_GRADS: dqkv, dbias and dhead_scale keep every value."""
    L = _L()
    inp, c = _abi_case(Ws, hd, dtype, B=2)
    ok(abi_fwd(c["qkv"], c["out"], c["lse"], c["bias"], c["hs"], c["idx"], 0, c["labels"], c["B"], c["N"], c["C"], c["nH"], Ws, c["flags"]),
       "hs_window_attn_fwd")
    ref = run_reference(inp, dtype, True, inp["idx"], 0)
    e = assert_close(c["out"].double().cpu(), ref["out"], TOL[dtype], f"forward Ws{Ws} hd{hd}")
    print(f"MEASURED tight out {e:.3e} forward-only Ws{Ws} hd{hd} {str(dtype)[6:]}")
    assert dtype != F32 or TIGHT is None or e <= TIGHT["out"]
    assert_close(c["lse"].double().cpu(), ref["lse"], TOL[F32], f"lse Ws{Ws} hd{hd}")
    for flags in (c["flags"], c["flags"] | L.HS_ATTN_OVERWRITE_GRADS):
        db, ds = torch.full(c["bias"].shape, GUARD, device=DEV), torch.full(c["hs"].shape, GUARD, device=DEV)
        dqkv = torch.full(c["qkv"].shape, 77.0, device=DEV, dtype=dtype)
        st = abi_bwd(c["qkv"], c["out"], c["dout"], c["lse"], dqkv, db, ds, None, c["bias"], c["hs"], c["idx"], 0, c["labels"],
                     c["B"], c["N"], c["C"], c["nH"], Ws, flags)
        torch.cuda.synchronize()
        assert st == HS_ERR_UNSUPPORTED, st
        assert b"LDS" in L.lib.hs_last_error()
        assert bool((db == GUARD).all()) and bool((ds == GUARD).all()) and bool((dqkv == 77.0).all()), "a refused backward wrote"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("Ws,hd", [(256, 128), (16, 129), (4, 129)])
def test_unsupported_shapes_are_refused_in_both_directions(Ws, hd, dtype):
    """(Ws 256, head_dim 128) exceeds the LDS already in the forward; head_dim 129 has no template.  Nothing is written."""
    L = _L()
    inp, c = _abi_case(Ws, hd, dtype, nH=1, B=1)
    c["out"].fill_(77.0)
    c["lse"].fill_(GUARD)
    st = abi_fwd(c["qkv"], c["out"], c["lse"], c["bias"], c["hs"], c["idx"], 0, c["labels"], c["B"], c["N"], c["C"], c["nH"], Ws, c["flags"])
    torch.cuda.synchronize()
    assert st == HS_ERR_UNSUPPORTED, st
    assert bool((c["out"] == 77.0).all()) and bool((c["lse"] == GUARD).all()), "a refused forward wrote"
    for flags in (c["flags"], c["flags"] | L.HS_ATTN_OVERWRITE_GRADS):
        db, ds = torch.full(c["bias"].shape, GUARD, device=DEV), torch.full(c["hs"].shape, GUARD, device=DEV)
        dqkv = torch.full(c["qkv"].shape, 77.0, device=DEV, dtype=dtype)
        st = abi_bwd(c["qkv"], c["out"], c["dout"], c["lse"], dqkv, db, ds, None, c["bias"], c["hs"], c["idx"], 0, c["labels"],
                     c["B"], c["N"], c["C"], c["nH"], Ws, flags)
        torch.cuda.synchronize()
        assert st == HS_ERR_UNSUPPORTED, st
        assert bool((db == GUARD).all()) and bool((ds == GUARD).all()) and bool((dqkv == 77.0).all()), "a refused backward wrote"


def test_workspace_is_zero_for_valu_only_shapes():
    L = _L()
    for Ws, hd, nH in [(4, 8, 2), (8, 8, 2), (16, 5, 3), (32, 8, 2), (64, 8, 2), (64, 64, 2), (128, 64, 2), (256, 32, 2)]:
        for dt in (L.HS_F32, L.HS_BF16):
            assert int(L.lib.hs_window_attn_bwd_workspace(2, 4 * Ws, nH * hd, nH, Ws, dt)) == 0, (Ws, hd)
    for dt in (L.HS_F32, L.HS_BF16):
        assert int(L.lib.hs_window_attn_bwd_workspace(2, 256, 96, 3, 64, dt)) > 0  # the MFMA shapes need one


# ----------------------------------------------------------------------------- the dropout mask, read off every kernel family
def decode_mask(out_shifted, Ws, K, p):
    """out [B, N, nH, hd] by shifted position, of a run with uniform probabilities and v = binary code of the key position ->
    (keep [B, nH, N, Ws] bool, worst distance from an integer).  EVERY element must decode."""
    B, N, nH, hd = out_shifted.shape
    x = out_shifted.double() * (Ws / AR.keep_scale(p))
    r = x.round()
    dist = float((x - r).abs().max())
    code = r.long()
    assert int(code.min()) >= 0 and int(code.max()) < (1 << K)
    bits = ((code[..., None] >> torch.arange(K, device=code.device)) & 1).reshape(B, N, nH, hd * K)  # key = channel * K + bit
    assert int(bits[..., Ws:].sum()) == 0, "a channel that codes no key is not zero"
    return bits[..., :Ws].bool().permute(0, 2, 1, 3), dist


def code_values(B, N, nH, hd, Ws, K, dtype):
    """v[token at window position j, head, channel c] = 2^(j % K) if j // K == c else 0, by SHIFTED position."""
    assert hd * K >= Ws
    j = torch.arange(N) % Ws
    v = torch.zeros(N, hd)
    v[torch.arange(N), j // K] = 2.0 ** (j % K).float()
    return v[None, :, None, :].expand(B, N, nH, hd).reshape(B, N, nH * hd).to(dtype)


MASK_CASES = (
    [pytest.param(Ws, max(3, Ws // 16), 16, p, F32, False, id=f"valu-f32-Ws{Ws}-p{p}") for Ws in (4, 8, 32, 64, 256) for p in (0.25, 0.5)] +
    [pytest.param(Ws, max(3, Ws // 8), 8, 0.5, BF16, False, id=f"valu-bf16-Ws{Ws}") for Ws in (4, 8, 32, 64, 256)] +
    [pytest.param(64, 32, 16, p, F32, False, id=f"mfma-f32-p{p}") for p in (0.25, 0.5)] +
    [pytest.param(64, 32, 16, 0.25, F32, True, id="valu-f32-Ws64-hd32-forced"),
     pytest.param(64, 32, 8, 0.5, BF16, False, id="mfma-bf16"), pytest.param(64, 32, 8, 0.5, BF16, True, id="valu-bf16-Ws64-hd32-forced")])


@pytest.mark.parametrize("Ws,hd,K,p,dtype,valu", MASK_CASES)
def test_decoded_dropout_mask_equals_the_host_reference(Ws, hd, K, p, dtype, valu):
    """q = 0, no bias, no labels, v the binary code of the key position: out[i, c] * Ws / keep_scale is the integer whose bits are the
    keep decisions of K keys of query i.  The mask is keyed by SHIFTED row, so `out` is un-permuted with idx first.  Every element must
    decode (|x - round(x)| < 0.25; K = 8 and p = 0.5 keep the codes and keep_scale exact in bf16), and the mask must EQUAL the host
    reference."""
    L = _L()
    B, nH, seed = 2, 3, (0x1234 << 32) | 0x9ABCDEF0 + Ws
    N = 4 * Ws if Ws >= 64 else 40 if Ws <= 8 else 3 * Ws
    C = nH * hd
    g = torch.Generator().manual_seed(Ws + K)
    idx = torch.randperm(N, generator=g)
    qkv = torch.randn(B, N, 3 * C, generator=g).to(dtype)
    qkv[:, :, :C] = 0
    qkv[:, :, 2 * C:] = code_values(B, N, nH, hd, Ws, K, dtype)[:, torch.argsort(idx)]  # shifted position j reads token idx[j]
    qkv_d, idx_d = qkv.to(DEV), idx.to(torch.int32).to(DEV)
    out = torch.empty(B, N, C, device=DEV, dtype=dtype)
    hs = torch.full((nH,), 0.3, device=DEV)
    ok(abi_fwd(qkv_d, out, None, None, hs, idx_d, 0, None, B, N, C, nH, Ws, L.HS_ATTN_FORCE_VALU if valu else 0, p, seed), "hs_window_attn_fwd")
    got, dist = decode_mask(out[:, idx_d.long()].reshape(B, N, nH, hd), Ws, K, p)
    print(f"MEASURED decode distance {dist:.4f}")
    assert dist < 0.25, f"an element does not decode: {dist:.3f} from an integer"
    want = torch.from_numpy(host_keep(B, N, nH, Ws, p, seed))
    assert torch.equal(got.cpu(), want), f"{int((got.cpu() != want).sum())} of {want.numel()} keep decisions differ from the host reference"
    assert 0 < int(want.sum()) < want.numel()


DROP_CASES = ([pytest.param(Ws, max(3, Ws // 16), p, dt, id=f"valu-{'f32' if dt == F32 else 'bf16'}-Ws{Ws}-p{p}")
               for Ws, p in ((4, 0.25), (8, 0.5), (16, 0.25), (32, 0.5), (64, 0.25), (256, 0.5)) for dt in DTYPES] +
              [pytest.param(64, 32, p, F32, id=f"mfma-f32-p{p}") for p in (0.25, 0.5)])


@pytest.mark.parametrize("Ws,hd,p,dtype", DROP_CASES)
def test_dropout_forward_and_backward_against_float64_with_the_host_mask(Ws, hd, p, dtype):
    """Random q, k, v, bias, labels, dout: out, dqkv, dbias and dhead_scale under dropout against the float64 reference whose mask is
    the host reference's -- "equal to the definition", not "consistent with itself"."""
    B, nH, seed = 2, 3, 987654321 + (5 << 40)
    N = 2 * Ws if Ws >= 64 else 40 if Ws <= 8 else 3 * Ws
    inp = make_inputs(B, N, nH, hd, Ws)
    for cosine in (True, False):
        ref = run_reference(inp, dtype, cosine, inp["idx"], 0, drop=p, seed=seed)
        got = run_ops(inp, dtype, cosine, inp["idx"], 0, drop=p, seed=seed)
        check(got, ref, dtype, f"dropout {p} Ws{Ws} hd{hd} {'cos' if cosine else 'scaled'}", tight=not (Ws == 64 and hd == 32))


def test_dropout_mask_across_row_2_to_the_24():
    """`DropRng` takes another branch once row * 256 needs more than 32 bits (row >= 2^24; production: B 8 x 4 heads x 786432 tokens
    = 25 M rows).  The least memory that gets there: bf16, 3 heads of one channel, Ws 4, B 2, N 2^22 (150 MB of qkv).  K = 4: channel 0
    carries 2^j of key j.  Every element must decode; the mask is compared with the host reference on the 4096 rows on each side of
    row 2^24, the last 4096 rows and the first 4096."""
    L = _L()
    B, N, nH, Ws, p, seed, R = 2, 1 << 22, 3, 4, 0.5, (77 << 32) | 4242, 4096
    assert B * nH * N > 2 ** 24
    qkv = torch.zeros(B, N, 9, device=DEV, dtype=BF16)
    qkv[:, :, 6:] = (2.0 ** (torch.arange(N, device=DEV) % Ws).float())[None, :, None].to(BF16)
    out = torch.empty(B, N, 3, device=DEV, dtype=BF16)
    hs = torch.ones(nH, device=DEV)
    ok(abi_fwd(qkv, out, None, None, hs, None, 0, None, B, N, 3, nH, Ws, 0, p, seed), "hs_window_attn_fwd")
    del qkv
    x = out.float() * (Ws / AR.keep_scale(p))  # [B, N, nH]
    code = x.round()
    assert float((x - code).abs().max()) < 0.25 and float(code.min()) >= 0 and float(code.max()) <= 15
    by_row = code.permute(0, 2, 1).reshape(-1)  # row = (b * nH + h) * N + j
    total = B * nH * N
    for r0, r1 in ((2 ** 24 - R, 2 ** 24 + R), (total - R, total), (0, R)):
        got = by_row[r0:r1].long().cpu()
        got = ((got[:, None] >> torch.arange(Ws)) & 1).bool()
        want = torch.from_numpy(AR.keep(np.arange(r0, r1, dtype=np.uint64)[:, None], np.arange(Ws, dtype=np.uint64), p, seed))
        assert torch.equal(got, want), f"rows {r0} ... {r1}: {int((got != want).sum())} keep decisions differ from the host reference"
