"""The persistent window loop of the attention kernels and every head group.

The bf16 MFMA kernels (csrc/window_attn_mfma.hip), the fp32 MFMA kernels (csrc/window_attn_mfma_f32.hip) and the module kernel
(csrc/window_attn_module.hip) launch a fixed number of workgroup SLOTS; slot s walks the windows s, s + slots, s + 2 slots, ...
across image boundaries and carries state from one window to the next: prefetched rows, the token rows of the window after
(table mode), the label prefetch, the per-slot dbias / dhead_scale partials, the dropout counter.  The other kernel-level tests
have at most 64 windows, i.e. ONE iteration per slot.  Here every slot walks at least two windows with an uneven tail
(`hs_set_reserved_cus` shrinks the slot count so that small tensors do), the grid is rounded up past the slot count, and the
head groups that only tensors >= 64 MB select (forward 8 heads, backward 4 heads per workgroup) are reached at the smallest
such shape.  Every multi-iteration test asserts its own precondition (windows > 2 slots, windows % slots != 0, or the 64 MB
line), so a change of the slot formulas cannot quietly turn it back into a one-iteration test."""
import pytest
import torch

import test_gpu_attn_module as TM
from _util import GRAD_TOL, TOL, assert_close, assert_unbiased, reserved_cus
from test_gpu_kernels import _oracle_core

pytestmark = pytest.mark.gpu
DEV = "cuda"
WS, HD = 64, 32
BF16, F32 = torch.bfloat16, torch.float32
LARGE_LINE = 64 << 20  # pick_head_group / pick_head_group_bwd: one [B, N, C] bf16 tensor of at least 64 MB


def _L():
    from heal_swin_amd import _lib
    return _lib


# ----------------------------------------------------------------------------- slot counts
def fwd_slots(nH, reserved, dtype, large=False):
    """Slots of the FORWARD launch before the cap at the window count (the library does not report it; the backward's is read
    back from its workspace size).  bf16: `persistent_slots` of csrc/window_attn_mfma.hip -- 8 XCDs x floor(usable CUs per XCD x
    floor(8 / waves per workgroup) / head groups), one wave per head, `pick_head_group` heads per workgroup.  fp32: `f32_slots` of
    csrc/window_attn_mfma_f32.hip -- floor(usable CUs x 4 / nH)."""
    per_xcd = 32 - reserved // 8
    if dtype == F32:
        return 8 * per_xcd * 4 // nH
    hg = 8 if (nH % 8 == 0 and large) else 4 if nH % 4 == 0 else 3 if nH % 3 == 0 else 2 if nH % 2 == 0 else 1
    return 8 * max(1, per_xcd * (8 // hg) // (nH // hg))


def bwd_slots(B, N, nH, dtype):
    """Slots of the BACKWARD launch under the current reservation, from hs_window_attn_bwd_workspace: slots x nH x (Ws^2 dbias
    words + the dhead_scale words: one per wave of a head, two in the bf16 kernel, one in the fp32 kernel)."""
    L = _L()
    words = int(L.lib.hs_window_attn_bwd_workspace(B, N, nH * HD, nH, WS, L.dtype_code(dtype)))
    per_slot = nH * (WS * WS + (2 if dtype == BF16 else 1))
    assert words > 0 and words % per_slot == 0, (words, per_slot)
    return words // per_slot


def module_slots(reserved):
    """hs_window_attn_module_fwd(_train): one persistent workgroup per usable CU (csrc/window_attn_module.hip)."""
    return 256 - reserved


def assert_multi_iteration(windows, slots, what):
    assert windows > 2 * slots and windows % slots != 0, f"{what}: {windows} windows on {slots} slots is not an uneven walk of > 2 windows"


# ----------------------------------------------------------------------------- cases
def _case(B, nH, strategy, shift, cosine, bias, nside=None, N=None):
    N = 8 * nside * nside if N is None else N
    return dict(B=B, N=N, nside=nside, nH=nH, C=nH * HD, strategy=strategy, shift=shift, cosine=cosine, bias=bias, windows=B * N // WS)


N67 = 64 * 67  # 67 windows per image: no HEALPix size (fine without a table), coprime with every slot count
SMALL = {
    # 603 windows, stride 256 / 128 over 67 windows per image
    "roll_nH4": _case(9, 4, "nest_roll", 32, False, True, N=N67),
    # 608 windows, 32 per image: the stride crosses image boundaries; table mode
    "ring_nH3": _case(19, 3, "ring_shift", 4, True, True, nside=16),
    # 1056 windows: more than twice the 512 slots of the forward with two heads (64-channel rows: half the bytes of "roll_nH4")
    "grid_nH2": _case(33, 2, "nest_grid_shift", 32, True, False, nside=16),
    # head group 1 (an odd head count other than 3): 469 windows on 200 / 96 / 102 slots
    "none_nH5": _case(7, 5, "none", 0, False, True, N=N67),
    # eight heads below the 64 MB line: forward in two groups of four heads, backward in four pairs; 335 windows on 128 / 64 slots
    "roll_nH8": _case(5, 8, "nest_roll", 32, True, True, N=N67),
}
# (case, reserved CUs).  At 128 the slot counts of the table cases are multiples of their 32 windows per image (256 / 128), so a slot
# meets the SAME window of a later image and the carried token rows never change; at 120 (17 CUs per XCD: 272 / 136 / 181 slots) the
# window changes from one iteration to the next.
SMALL_RUNS = [(name, 128) for name in SMALL] + [("ring_nH3", 120)]
LARGE = {
    # forward with EIGHT heads per workgroup (and backward with four, in two groups): 131072 tokens x 256 channels = 64 MB
    "fwd8_ring": _case(4, 8, "ring_shift", 4, True, True, nside=64),
    "fwd8_roll": _case(4, 8, "nest_roll", 32, False, True, N=32768),
    # backward with FOUR heads per workgroup in one group: 262144 tokens x 128 channels = 64 MB
    "bwd4_ring": _case(2, 4, "ring_shift", 4, True, True, nside=128),
    "bwd4_roll": _case(2, 4, "nest_roll", 32, True, True, N=131072),
}
_CACHE = {}


def _tables(c):
    """(idx or None, roll, labels or None) on the device as the op takes them, and (idx, labels) on the host for the oracle."""
    from oracle import tables as T
    if c["strategy"] == "none":
        return (None, 0, None), (None, None)
    N = c["N"]
    fn = {"nest_roll": lambda: T.nest_roll_shift(N, WS, c["shift"]), "nest_grid_shift": lambda: T.nest_grid_shift(c["nside"], 8, WS),
          "ring_shift": lambda: T.ring_shift(c["nside"], 8, WS, c["shift"])}[c["strategy"]]
    idx_np, _, lab_np = fn()
    idx, labels = torch.from_numpy(idx_np), torch.from_numpy(lab_np)
    use_roll = c["strategy"] == "nest_roll"
    dev = (None if use_roll else idx.to(torch.int32).to(DEV), c["shift"] if use_roll else 0, labels.to(torch.uint8).to(DEV))
    return dev, (idx, labels)


def small_inputs(name):
    """The input recipe of test_attn_core_vs_oracle (fixed seed), built once per case."""
    key = ("in", name)
    if key not in _CACHE:
        c = SMALL[name] if name in SMALL else GRID[name]
        g = torch.Generator().manual_seed(7)
        qkv = torch.randn(c["B"], c["N"], 3 * c["C"], generator=g)
        bias = torch.randn(c["nH"], WS, WS, generator=g) if c["bias"] else None
        hscale = torch.rand(c["nH"], generator=g) * (8 if c["cosine"] else 0.3) + 0.1
        dout = torch.randn(c["B"], c["N"], c["C"], generator=g)
        dev, host = _tables(c)
        _CACHE[key] = dict(c, qkv=qkv, bias_t=bias, hscale=hscale, dout=dout, dev=dev, host=host)
    return _CACHE[key]


def oracle_small(name, dtype):
    """CPU fp32 oracle with autograd on the values the kernel sees (inputs rounded to the activation dtype); once per (case, dtype)."""
    key = ("ref", name, dtype)
    if key not in _CACHE:
        inp = small_inputs(name)
        qkv_r = inp["qkv"].to(dtype).float().clone().requires_grad_(True)
        bias_r = None if inp["bias_t"] is None else inp["bias_t"].clone().requires_grad_(True)
        hs_r = inp["hscale"].clone().requires_grad_(True)
        o = _oracle_core(qkv_r, bias_r, hs_r, inp["host"][0], inp["host"][1], inp["nH"], WS, inp["cosine"])
        o.backward(inp["dout"].to(dtype).float())
        _CACHE[key] = dict(out=o.detach(), dqkv=qkv_r.grad, dbias=None if bias_r is None else bias_r.grad,
                           dscale=hs_r.grad if inp["cosine"] else None)
    return _CACHE[key]


def run_core(inp, dtype, images=None, drop=0.0, seed=0, valu=False):
    """Forward + backward of ops.window_attn_core under the CURRENT reservation.  `images`: a slice of the batch.  `valu`: the
    fp32-VALU kernels on the same values (inputs rounded to `dtype`, then handed over as fp32)."""
    from heal_swin_amd import ops
    sl = slice(None) if images is None else images
    to = lambda t: t[sl].to(DEV).to(dtype).float() if valu else t[sl].to(DEV).to(dtype)  # noqa: E731
    qkv = to(inp["qkv"]).clone().requires_grad_(True)  # (clones: the cached inputs may already live on the device)
    bias = None if inp["bias_t"] is None else inp["bias_t"].to(DEV).clone().requires_grad_(True)
    hs = inp["hscale"].to(DEV).clone().requires_grad_(True)
    idx, roll, labels = inp["dev"]
    prev = ops.FORCE_VALU_ATTENTION
    ops.FORCE_VALU_ATTENTION = bool(valu)
    try:
        out = ops.window_attn_core(qkv, bias, hs, idx, roll, labels, inp["nH"], WS, inp["cosine"], attn_drop=drop, seed=seed)
        out.backward(to(inp["dout"]))
    finally:
        ops.FORCE_VALU_ATTENTION = prev
    return dict(out=out.detach(), dqkv=qkv.grad, dbias=None if bias is None else bias.grad, dscale=hs.grad if inp["cosine"] else None,
                v=qkv.detach()[:, :, 2 * inp["C"]:], dO=to(inp["dout"]))


def small_result(name, dtype, reserved):
    key = ("run", name, dtype, reserved)
    if key not in _CACHE:
        with reserved_cus(reserved):
            _CACHE[key] = run_core(small_inputs(name), dtype)
    return _CACHE[key]


def check_vs_reference(got, ref, dtype, tag):
    assert_close(got["out"], ref["out"], TOL[dtype], tag + " out")
    assert_close(got["dqkv"], ref["dqkv"], GRAD_TOL[dtype], tag + " dqkv")
    for k in ("dbias", "dscale"):
        if ref[k] is None:
            continue
        assert_close(got[k], ref[k], GRAD_TOL[dtype], f"{tag} {k}")
        # a partial lost on one iteration is a SLOPE, not noise (dhead_scale has nH elements: judged however few they are)
        assert assert_unbiased(got[k], ref[k], f"{tag} {k}", min_elems=1) is not None


# ----------------------------------------------------------------------------- 1. multi-iteration core op against the oracle
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,reserved", SMALL_RUNS)
def test_multi_iteration_core_vs_oracle(name, reserved, dtype):
    c = SMALL[name]
    assert c["B"] * c["N"] * c["C"] * 2 < LARGE_LINE  # the small head groups
    with reserved_cus(reserved):
        assert_multi_iteration(c["windows"], bwd_slots(c["B"], c["N"], c["nH"], dtype), f"{name} backward")
    assert_multi_iteration(c["windows"], fwd_slots(c["nH"], reserved, dtype), f"{name} forward")
    check_vs_reference(small_result(name, dtype, reserved), oracle_small(name, dtype), dtype, f"persistent {name} r{reserved}")


# ----------------------------------------------------------------------------- 2. the slot mapping must not change results
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(SMALL))
def test_slot_mapping_does_not_change_a_bit(name, dtype):
    """Same head group, another window -> slot assignment: every window's arithmetic is independent of the slot that ran it.
    (dbias / dhead_scale change their summation order with the slot count; they are held by the oracle test.)"""
    c = SMALL[name]
    with reserved_cus(0):
        s0 = bwd_slots(c["B"], c["N"], c["nH"], dtype)
    with reserved_cus(128):
        s128 = bwd_slots(c["B"], c["N"], c["nH"], dtype)
    assert s0 != s128 and fwd_slots(c["nH"], 0, dtype) != fwd_slots(c["nH"], 128, dtype)
    assert_multi_iteration(c["windows"], s128, name)
    a, b = small_result(name, dtype, 0), small_result(name, dtype, 128)
    assert torch.equal(a["out"], b["out"])
    assert torch.equal(a["dqkv"], b["dqkv"])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(SMALL))
def test_image_of_the_batched_call_equals_the_single_image_call(name, dtype):
    """Image b of the multi-iteration call is, bit for bit, the call on that image alone, which takes ONE iteration per slot (an
    image has at most 67 windows, a full chip at least 128 slots)."""
    c = SMALL[name]
    inp = small_inputs(name)
    batched = small_result(name, dtype, 128)
    with reserved_cus(128):
        assert_multi_iteration(c["windows"], bwd_slots(c["B"], c["N"], c["nH"], dtype), name)
    with reserved_cus(0):
        per_image = c["N"] // WS
        assert bwd_slots(1, c["N"], c["nH"], dtype) == per_image and fwd_slots(c["nH"], 0, dtype) >= per_image  # (capped at the windows)
        for b in (0, 1, c["B"] - 1):
            single = run_core(inp, dtype, images=slice(b, b + 1))
            assert torch.equal(batched["out"][b:b + 1], single["out"]), b
            assert torch.equal(batched["dqkv"][b:b + 1], single["dqkv"]), b


# ----------------------------------------------------------------------------- 3. grid rounding
# One image of 67 windows on a full chip: 67 slots, and the bf16 grid is rounded up to 8 x ceil(67 / 8) = 72 workgroups per head
# group, whose surplus must return without touching the partials (a dbias partial written by slot 67 would land in the
# dhead_scale partials behind the 67 x nH x Ws^2 dbias words -- hence cosine AND bias).
GRID = {
    "grid67_nH3": _case(1, 3, "nest_roll", 32, True, True, N=N67),
    "grid67_nH4": _case(1, 4, "nest_roll", 32, True, True, N=N67),
    "grid67_nH5": _case(1, 5, "none", 0, True, True, N=N67),
}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(GRID))
def test_grid_rounded_past_the_slot_count(name, dtype):
    L = _L()
    lib, ptr, check = L.lib, L.ptr, L.check
    c = GRID[name]
    inp = small_inputs(name)
    ref = oracle_small(name, dtype)
    B, N, C, nH = c["B"], c["N"], c["C"], c["nH"]
    with reserved_cus(0):
        slots = bwd_slots(B, N, nH, dtype)
        assert slots == c["windows"] == 67 and slots % 8 != 0 and fwd_slots(nH, 0, dtype) >= 67  # both launches: 67 slots
        got = run_core(inp, dtype)
        check_vs_reference(got, ref, dtype, f"rounded grid {name}")
        # the accumulate contract of the C ABI (fp32 path always; bf16 path without HS_ATTN_OVERWRITE_GRADS): dbias and
        # dhead_scale are ADDED to what the buffers hold
        g = torch.Generator().manual_seed(11)
        start_b, start_s = torch.randn(nH, WS, WS, generator=g).to(DEV), torch.randn(nH, generator=g).to(DEV)
        qkv = inp["qkv"].to(DEV).to(dtype)
        dout = inp["dout"].to(DEV).to(dtype)
        bias, hs = inp["bias_t"].to(DEV), inp["hscale"].to(DEV)
        idx, roll, labels = inp["dev"]
        dt = L.dtype_code(dtype)
        out = torch.empty(B, N, C, dtype=dtype, device=DEV)
        lse = torch.empty(B, nH, N, device=DEV)
        check(lib.hs_window_attn_fwd(ptr(qkv), ptr(out), ptr(lse), ptr(bias), ptr(hs), ptr(idx), roll, ptr(labels), B, N, C, nH, WS,
                                     L.HS_ATTN_COSINE, 0.0, 0, dt, None), "fwd")
        assert torch.equal(out, got["out"])
        dqkv = torch.empty_like(qkv)
        dbias, dscale = start_b.clone(), start_s.clone()
        wsp = torch.empty(int(lib.hs_window_attn_bwd_workspace(B, N, C, nH, WS, dt)), device=DEV)
        check(lib.hs_window_attn_bwd(ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(dqkv), ptr(dbias), ptr(dscale), ptr(wsp), ptr(bias),
                                     ptr(hs), ptr(idx), roll, ptr(labels), B, N, C, nH, WS, L.HS_ATTN_COSINE, 0.0, 0, dt, None), "bwd")
    assert torch.equal(dqkv, got["dqkv"])
    added = dict(out=out, dqkv=dqkv, dbias=dbias - start_b, dscale=dscale - start_s)
    check_vs_reference(added, ref, dtype, f"rounded grid {name}, accumulated")
    # against the overwriting call: the start value rides through the <= 17 fp32 additions of the reduction and is subtracted
    # again -- at most 32 roundings at the magnitude of start + gradient
    for k, start in (("dbias", start_b), ("dscale", start_s)):
        floor = 32 * 2.0 ** -24 * float(start.abs().max() + got[k].abs().max())
        assert_close(added[k], got[k], 1e-5, f"accumulated {k} vs written {k}", floor=floor)


# ----------------------------------------------------------------------------- 4. the large head groups (>= 64 MB)
def large_inputs(name):
    """bf16 values on the device (fixed seed), kept for the dropout tests of the same shape."""
    key = ("in", name)
    if key not in _CACHE:
        c = LARGE[name]
        assert c["B"] * c["N"] * c["C"] * 2 >= LARGE_LINE, name  # at or above the line that selects 8 (forward) / 4 (backward) heads
        g = torch.Generator(device=DEV).manual_seed(7)
        qkv = torch.randn(c["B"], c["N"], 3 * c["C"], generator=g, device=DEV).to(BF16)
        bias = torch.randn(c["nH"], WS, WS, generator=g, device=DEV)
        hscale = torch.rand(c["nH"], generator=g, device=DEV) * (8 if c["cosine"] else 0.3) + 0.1
        dout = torch.randn(c["B"], c["N"], c["C"], generator=g, device=DEV).to(BF16)
        dev, host = _tables(c)
        _CACHE[key] = dict(c, qkv=qkv, bias_t=bias, hscale=hscale, dout=dout, dev=dev, host=host)
    return _CACHE[key]


def oracle_large(inp):
    """`_oracle_core` in float64 on the device with plain torch ops and autograd, image by image; no project kernel takes part."""
    idx, labels = (None if t is None else t.to(DEV) for t in inp["host"])
    bias = inp["bias_t"].double().requires_grad_(True)
    hs = inp["hscale"].double().requires_grad_(True)
    outs, dq = [], []
    for b in range(inp["B"]):
        q = inp["qkv"][b:b + 1].double().requires_grad_(True)
        o = _oracle_core(q, bias, hs, idx, labels, inp["nH"], WS, inp["cosine"])
        o.backward(inp["dout"][b:b + 1].double())
        outs.append(o.detach())
        dq.append(q.grad)
    return dict(out=torch.cat(outs), dqkv=torch.cat(dq), dbias=bias.grad, dscale=hs.grad if inp["cosine"] else None)


@pytest.mark.parametrize("name", list(LARGE))
def test_large_head_groups_vs_float64(name):
    inp = large_inputs(name)
    assert inp["B"] * inp["N"] * inp["C"] * 2 >= LARGE_LINE
    ref = oracle_large(inp)
    got = run_core(inp, BF16)
    check_vs_reference(got, ref, BF16, f"large {name}")
    # second opinion, not the reference: the fp32-VALU kernels on the same bf16 values (bounds of tests/test_gpu_fullsize.py)
    valu = run_core(inp, BF16, valu=True)
    assert_close(got["out"], valu["out"], 1e-2, f"large {name} out vs VALU")
    assert_close(got["dqkv"], valu["dqkv"], 3e-2, f"large {name} dqkv vs VALU")
    assert_close(got["dbias"], valu["dbias"], 2e-2, f"large {name} dbias vs VALU")


# ----------------------------------------------------------------------------- 5. dropout across iterations
def _dropout_inputs(name):
    if name in LARGE:
        return large_inputs(name)
    inp = dict(small_inputs(name))
    for k in ("qkv", "dout", "bias_t", "hscale"):  # one upload for the five runs below
        inp[k] = inp[k].to(DEV)
    return inp


@pytest.mark.parametrize("name,dtype", [("roll_nH4", BF16), ("roll_nH4", F32), ("fwd8_roll", BF16), ("bwd4_ring", BF16)],
                         ids=["roll_nH4-bf16", "roll_nH4-f32", "fwd8_roll-bf16", "bwd4_ring-bf16"])
def test_dropout_across_iterations(name, dtype):
    """The mask belongs to the (image, head, query, key), not to the slot's iteration: the MFMA result agrees with the fp32-VALU
    kernels on the same values and seed, does not change by a bit with the slot mapping, and the backward regenerates exactly the
    forward's mask (adjoint identity: out is linear in V for a fixed mask)."""
    inp = _dropout_inputs(name)
    p_drop, seed = 0.3, 20240607
    if name in LARGE:
        assert inp["B"] * inp["N"] * inp["C"] * 2 >= LARGE_LINE
    else:
        with reserved_cus(128):
            assert_multi_iteration(inp["windows"], bwd_slots(inp["B"], inp["N"], inp["nH"], dtype), name)
        assert_multi_iteration(inp["windows"], fwd_slots(inp["nH"], 128, dtype), name)
    with reserved_cus(128):
        a = run_core(inp, dtype, drop=p_drop, seed=seed)
    with reserved_cus(0):
        b = run_core(inp, dtype, drop=p_drop, seed=seed)
        plain = run_core(inp, dtype)
        valu = run_core(inp, dtype, drop=p_drop, seed=seed, valu=True)
    assert not torch.equal(a["out"], plain["out"])
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["dqkv"], b["dqkv"])
    # bf16: the bounds of test_attention_dropout_mask_is_path_independent; fp32: two fp32 implementations of the same sums (the
    # bounds of the fp32 MFMA vs VALU comparison in tests/test_gpu_fullsize.py)
    out_tol, grad_tol, adj_tol = (1e-2, 3e-2, 2e-2) if dtype == BF16 else (1e-5, 1e-4, 1e-4)
    assert_close(a["out"], valu["out"], out_tol, f"dropout {name} out vs VALU")
    assert_close(a["dqkv"], valu["dqkv"], grad_tol, f"dropout {name} dqkv vs VALU")
    terms = a["dO"].double() * a["out"].double()
    lhs = float(terms.sum())
    rhs = float((a["dqkv"][:, :, 2 * inp["C"]:].double() * a["v"].double()).sum())
    # both sides are signed sums of products of values rounded to `dtype`: judged against the noise scale of such a sum (2-norm
    # of the terms), the bounds of test_attention_dropout_statistics_and_adjoint
    noise = float(terms.pow(2).sum().sqrt())
    assert abs(lhs - rhs) <= adj_tol * noise, (lhs, rhs, noise)
    assert torch.isfinite(a["dqkv"].float()).all()


# ----------------------------------------------------------------------------- 6. the module kernel, both forms
# 13 images of 32 windows = 416 windows on the 128 slots left by hs_set_reserved_cus(128): three full rounds and a tail of 32, the
# stride crossing image boundaries (128 = 4 images: the same window of a later image) -- and on 256 slots for the bit-exact twin.
MODULE_B, MODULE_NSIDE = 13, 16
MODULE_CASES = [
    # C, nH, strategy, shift, cosine, bias, ln, residual, qkv_bias
    (128, 4, "ring_shift", 4, True, True, True, True, True),
    (96, 3, "nest_roll", 32, False, True, False, False, True),
    (96, 3, "none", 0, False, False, True, False, False),
    (128, 4, "nest_grid_shift", 32, True, False, False, True, False),
]
MODULE_TRAIN_CASES = [
    # C, nH, strategy, shift, cosine, bias, qkv_bias, v1 (LayerNorm in front + residual behind)
    (128, 4, "ring_shift", 4, True, True, True, True),
    (96, 3, "nest_roll", 32, False, True, True, False),
    (128, 4, "none", 0, False, True, True, True),
    (96, 3, "ring_shift", 4, True, True, True, False),
]


def _module_precondition():
    windows = MODULE_B * 8 * MODULE_NSIDE * MODULE_NSIDE // WS
    assert_multi_iteration(windows, module_slots(128), "module kernel")
    assert windows > module_slots(0)  # the twin at reserved = 0 walks as well, on another mapping


@pytest.mark.parametrize("C,nH,strategy,shift,cosine,use_bias,use_ln,residual,qkv_bias", MODULE_CASES)
def test_module_kernel_multi_iteration(C, nH, strategy, shift, cosine, use_bias, use_ln, residual, qkv_bias):
    _module_precondition()
    with reserved_cus(128):
        y, run = TM.module_kernel_case(C, nH, MODULE_B, MODULE_NSIDE, strategy, shift, cosine, use_bias, use_ln, residual, qkv_bias)
    with reserved_cus(0):
        assert torch.equal(run(), y)


@pytest.mark.parametrize("C,nH,strategy,shift,cosine,use_bias,qkv_bias,v1", MODULE_TRAIN_CASES)
def test_module_train_form_multi_iteration(C, nH, strategy, shift, cosine, use_bias, qkv_bias, v1):
    """Output, every gradient and the saved attention output against the oracle and the four-kernel composition (the bounds of
    test_module_train_form_vs_oracle_and_composition); the output does not change by a bit with the slot mapping."""
    _module_precondition()
    with reserved_cus(128):
        out, run = TM.module_train_form_case(C, nH, MODULE_B, MODULE_NSIDE, strategy, shift, cosine, use_bias, qkv_bias, v1)
    with reserved_cus(0):
        assert torch.equal(run(True)[0], out)


def test_module_train_form_saved_tensors_multi_iteration():
    """LayerNorm(x) and its statistics, qkv, the attention output, lse and norm2 of the walk against the separate kernels."""
    _module_precondition()
    with reserved_cus(128):
        # The saved tensors at the bounds of test_module_train_form_saved_tensors_equal_the_separate_kernels.  `out` against the proj
        # GEMM on the saved attention output: both round an fp32 sum to bf16, and sums taken in another order may land on ADJACENT
        # bf16 values -- one ulp, up to 2^-7 of the tensor's scale for an element of the top binade.  The 4e-3 of the two-image test
        # admits that only below the top binade; with 6.5 x the elements one of the ~2000 of magnitude >= 8 does flip: measured
        # 5.78e-3 = 0.0625 / 10.81, exactly one ulp of [8, 16).  Bound: one ulp, 2^-7 (inside the 1e-2 that holds the output to
        # the composition in test_module_train_form_multi_iteration).
        TM.module_train_form_saved_tensors_case(MODULE_B, out_tol=2.0 ** -7)
