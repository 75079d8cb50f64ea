"""Set-up shared by the tests of the C-ABI pair hs_window_attn_module_fwd_train / hs_window_attn_module_bwd_chain
(tests/test_gpu_attn_module.py, tests/test_gpu_operator_abi.py): the inputs of one call, the Python mirror's recorded autograd path
on them (ops.window_attn_module_train: the reference of the chain), the C-ABI forward with everything it saves, and the C-ABI
backward as a bare status so that a test can also look at a refusal."""
import types

import torch

DEV = "cuda"
GRAD_KEYS = ("wq", "bq", "wp", "bp", "lg", "lb", "bias", "hs")


def chain_inputs(v1, cosine, strategy, B=2, nside=16, C=128, nH=4, use_bias=True, seed=9, shift=32):
    """x, parameters, dout and the shift tables of one call, drawn on the GPU from `seed`."""
    from oracle import tables as T
    N = 8 * nside * nside
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s, k=1.0: torch.randn(*s, generator=g, device=DEV) * k  # noqa: E731
    x = (rnd(B, N, C) * 2 + 0.3).to(torch.bfloat16)
    P = dict(wq=rnd(3 * C, C, k=C ** -0.5), bq=rnd(3 * C, k=0.2), wp=rnd(C, C, k=C ** -0.5), bp=rnd(C, k=0.2))
    if use_bias:
        P["bias"] = rnd(nH, 64, 64)
    P["hs"] = torch.rand(nH, generator=g, device=DEV) * (8 if cosine else 0.3) + 0.1
    if v1:
        P.update(lg=torch.rand(C, generator=g, device=DEV) + 0.5, lb=rnd(C, k=0.2))
    dout = rnd(B, N, C).to(torch.bfloat16)
    if strategy == "none":
        idx, roll, labels = None, 0, None
    elif strategy == "nest_roll":
        idx, roll, lab_np = None, shift, T.nest_roll_shift(N, 64, shift)[2]
    else:
        idx_np, _, lab_np = T.nest_grid_shift(nside, 8, 64) if strategy == "nest_grid_shift" else T.ring_shift(nside, 8, 64, 4)
        idx, roll = torch.from_numpy(idx_np).to(torch.int32).to(DEV), 0
    if strategy != "none":
        labels = torch.from_numpy(lab_np).to(torch.uint8).to(DEV)
    from heal_swin_amd import _lib
    flags = (_lib.HS_ATTN_COSINE if cosine else 0) | (_lib.HS_ATTN_RESIDUAL if v1 else 0)
    return types.SimpleNamespace(v1=v1, cosine=cosine, B=B, N=N, C=C, nH=nH, x=x, P=P, dout=dout, idx=idx, roll=roll, labels=labels, flags=flags)


def chain_autograd(c):
    """The recorded autograd nodes of the Python mirror on the same inputs: (y, dx, {name: gradient})."""
    from heal_swin_amd import ops
    xd = c.x.clone().requires_grad_(True)
    D = {k: v.clone().requires_grad_(True) for k, v in c.P.items()}
    y = ops.window_attn_module_train(xd, D.get("lg"), D.get("lb"), D["wq"], D["bq"], D["wp"], D["bp"], D.get("bias"), D["hs"], c.idx, c.roll,
                                     c.labels, c.nH, 64, c.cosine)
    y.backward(c.dout)
    return y.detach(), xd.grad, {k: v.grad for k, v in D.items()}


def chain_forward(c):
    """hs_window_attn_module_fwd_train; keeps what the backward reads on `c` and returns `out`."""
    from heal_swin_amd import _lib
    from heal_swin_amd._lib import check, lib, ptr
    x, P, v1, B, N, C, nH = c.x, c.P, c.v1, c.B, c.N, c.C, c.nH
    wq16, wp16 = P["wq"].to(torch.bfloat16).contiguous(), P["wp"].to(torch.bfloat16).contiguous()
    out, c.xn, c.o = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    c.qkv = torch.empty(B, N, 3 * C, dtype=torch.bfloat16, device=DEV)
    c.mean, c.rstd, c.lse = torch.empty(B * N, device=DEV), torch.empty(B * N, device=DEV), torch.empty(B, nH, N, device=DEV)
    check(lib.hs_window_attn_module_fwd_train(ptr(x), ptr(out), ptr(c.xn) if v1 else None, ptr(c.mean) if v1 else None, ptr(c.rstd) if v1 else None,
                                              ptr(c.qkv), ptr(c.o), ptr(c.lse), ptr(wq16), ptr(P["bq"]), ptr(wp16), ptr(P["bp"]),
                                              ptr(P["lg"]) if v1 else None, ptr(P["lb"]) if v1 else None, ptr(P.get("bias")), ptr(P["hs"]),
                                              ptr(c.idx), c.roll, ptr(c.labels), None, None, None, None, None, B, N, C, nH, 64, c.flags, _lib.HS_BF16,
                                              None), "fwd_train")
    c.wq_t, c.wp_t = wq16.t().contiguous(), wp16.t().contiguous()
    return out


def chain_grad_buffers(c, fill=None):
    """(dx, {name: fp32 gradient buffer}) of the backward call: torch.empty, or filled with `fill`."""
    C, nH = c.C, c.nH
    shapes = dict(wq=(3 * C, C), bq=(3 * C,), wp=(C, C), bp=(C,), lg=(C,), lb=(C,), bias=(nH, 64, 64), hs=(nH,))
    G = {k: torch.empty(*s, device=DEV) for k, s in shapes.items() if k in c.P}
    dx = torch.empty_like(c.x)
    if fill is not None:
        dx.fill_(fill)
        for t in G.values():
            t.fill_(fill)
    return dx, G


def chain_workspace_floats(c):
    from heal_swin_amd._lib import lib
    return int(lib.hs_window_attn_module_bwd_chain_workspace(c.B, c.N, c.C, c.nH, 64))


def chain_backward(c, dx, G, ws, accumulate, n_tokens=None, roll=None):
    """hs_window_attn_module_bwd_chain on what chain_forward saved; returns the status (n_tokens / roll: what a refusal test passes
    in place of the call's own)."""
    from heal_swin_amd import _lib
    from heal_swin_amd._lib import lib, ptr
    v1, P = c.v1, c.P
    return lib.hs_window_attn_module_bwd_chain(ptr(c.dout), ptr(c.x), ptr(c.xn) if v1 else None, ptr(c.mean) if v1 else None,
                                               ptr(c.rstd) if v1 else None, ptr(c.qkv), ptr(c.o), ptr(c.lse), ptr(c.wq_t), ptr(c.wp_t),
                                               ptr(P["lg"]) if v1 else None, ptr(P.get("bias")), ptr(P["hs"]), ptr(c.idx),
                                               c.roll if roll is None else roll, ptr(c.labels), ptr(dx), ptr(G["wq"]), ptr(G["bq"]), ptr(G["wp"]),
                                               ptr(G["bp"]), ptr(G["lg"]) if v1 else None, ptr(G["lb"]) if v1 else None, ptr(G.get("bias")),
                                               ptr(G["hs"]), ptr(ws), accumulate, c.B, c.N if n_tokens is None else n_tokens, c.C, c.nH, 64,
                                               c.flags, _lib.HS_BF16, None)
