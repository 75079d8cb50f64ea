"""csrc/mlp_fused.hip through its C ABI (hs_mlp_fused_fwd / _bwd / _drop_fwd / _drop_bwd): every form of the kernel over its
persistent tile loop, inside guarded buffers, plus exact probes of the two products and the argument contract.

The kernel is one workgroup per usable CU that walks the 32-token tiles blockIdx.x, + gridDim.x, ... and carries state from one tile
to the next: the double-buffered x / saved-h tiles, the residual rows in registers, and an epilogue that runs one iteration late
(output rows, the kept mlp(x) rows, the post-norm statistics, the output mask and the DropPath factor are all indexed by the
PREVIOUS tile).  tests/test_gpu_mlp_fused.py reaches the loop with the v1 forward and the plain backward only; here

  * the loop cases run 390 tiles (12 480 rows) on 128 workgroups (hs_set_reserved_cus(128)): 3 tiles on every workgroup, 4 on six,
    so both buffers are reused and the deferred epilogue runs inside the loop and behind it.  390 = 30 samples x 13 tiles for the
    DropPath factors; 13 is coprime with 128, so a workgroup's consecutive tiles lie in different samples.  Each loop test asserts
    tiles > 2 grid and tiles % grid != 0 from the library's own reserved-CU count before it launches;
  * every output is a 16-byte-aligned view into a larger allocation whose two guard bands must come back unchanged, pre-filled with
    NaN so that an element the kernel never wrote shows; every row operand (x, dy, saved h, dres) is the first `rows` rows of an
    allocation that goes on with 64 NaN rows, so that a read past the end poisons a result;
  * the toleranced comparisons use the float64 oracle formulas with the kernel's rounding points and TOL[bf16], as
    test_gpu_mlp_fused.py does; the exact probes (structured weights) judge every (token, hidden unit, channel) path on its own
    with a derived per-element bound.

Out of scope: the split into launches below 2 GiB (rows_per_launch / row0 in the kernel's parameters) needs more than 2 M rows and
stays untested; the library has no hook to lower that limit."""
import contextlib
import ctypes
import math

import pytest
import torch

from _util import TOL, assert_close, mask_of, reserved_cus
from test_gpu_mlp_fused import _case, _oracle_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
SENTINEL = 7.0           # guard bands (exact in bf16 and fp32)
TAIL_ROWS = 64           # NaN rows behind every row operand
LOOP_TILES = 390         # 30 samples x 13 tiles
LOOP_ROWS = LOOP_TILES * 32
LOOP_SAMPLES = 30
LOOP_RESERVED = 128      # -> 128 workgroups
# (rows, reserved CUs or None for the default grid, samples for row_scale)
SHAPES = [pytest.param(32, None, 1, id="32"), pytest.param(96, None, 3, id="96"), pytest.param(LOOP_ROWS, LOOP_RESERVED, LOOP_SAMPLES, id="loop")]
SEEDS = (0x1234567890ABCDEF, 0x0FEDCBA987654321)
RAN = []  # (kind of test, tiles, grid) of the launches made here


def _L():
    from heal_swin_amd import _lib
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def _grid(rows, reserved, what):
    """The launch shape of a case: (tiles, grid) from the library's own reserved-CU count.  A loop case must really loop."""
    with (reserved_cus(reserved) if reserved is not None else contextlib.nullcontext()):
        tiles = rows // 32
        grid = min(tiles, 256 - int(_L().lib.hs_get_reserved_cus()))
        if reserved is not None:
            assert tiles > 2 * grid and tiles % grid != 0, f"{what}: {tiles} tiles on {grid} workgroups is not a loop case any more"
        key = (what.split(" C=")[0], tiles, grid)
        if key not in RAN:  # one line per kind of launch in the terminal summary
            from conftest import NOTES
            RAN.append(key)
            NOTES.append(f"mlp_fused loop tests, {key[0]}: {tiles} tiles on {grid} workgroups, {tiles // grid}-{-(-tiles // grid)} tiles per workgroup")
        yield tiles, grid


class Outputs:
    """Output tensors as 16-byte-aligned views into larger allocations: SENTINEL guard bands (two rows and 16 bytes, so the view is
    off the allocator's 256-byte grid) on both sides, NaN inside."""

    def __init__(self):
        self.items = {}

    def new(self, name, shape, dtype=BF):
        n = math.prod(shape)
        width = shape[-1] if len(shape) > 1 else 32
        g = 2 * width + 16 // torch.empty((), dtype=dtype).element_size()
        flat = torch.full((n + 2 * g,), SENTINEL, device=DEV, dtype=dtype)
        view = flat[g:g + n].view(shape)
        view.fill_(NAN)
        assert view.data_ptr() % 16 == 0 and view.is_contiguous()
        self.items[name] = (flat, view, g, n)
        return view

    def problems(self, untouched=False):
        """Guards changed, elements never written (or, after a refused call, any element written)."""
        bad = []
        for name, (flat, view, g, n) in self.items.items():
            lo, hi = int((flat[:g] != SENTINEL).sum()), int((flat[g + n:] != SENTINEL).sum())
            if lo or hi:
                bad.append(f"{name}: {lo} guard elements in front and {hi} behind were overwritten")
            nan = torch.isnan(view)
            if untouched and not bool(nan.all()):
                bad.append(f"{name}: {int((~nan).sum())} elements written by a call that was refused")
            if not untouched and bool(nan.any()):
                rows = torch.nonzero(nan.view(view.shape[0], -1).any(1)).flatten()[:8].tolist()
                bad.append(f"{name}: {int(nan.sum())} elements never written or NaN (first rows {rows})")
        return bad


def _rows(t):
    """A row operand: the first rows of an allocation that continues with TAIL_ROWS rows of NaN."""
    buf = torch.full((t.shape[0] + TAIL_ROWS,) + tuple(t.shape[1:]), NAN, device=t.device, dtype=t.dtype)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


def _judge(tag, outs, checks, exact=()):
    """Every tensor is judged before the test fails: the message names all that are off."""
    bad = outs.problems()
    for a, b, tol, what in checks:
        try:
            assert_close(a, b, tol, f"{tag} {what}")
        except AssertionError as e:
            bad.append(str(e))
    bad += [f"{tag} {what}" for ok, what in exact if not ok]
    assert not bad, "\n".join(bad)


def _gelu64(h):
    return 0.5 * h * (1.0 + torch.erf(h / 2 ** 0.5))


def _gelu_grad64(h):
    return 0.5 * (1.0 + torch.erf(h / 2 ** 0.5)) + h * torch.exp(-h * h / 2) / (2 * math.pi) ** 0.5


# ----------------------------------------------------------------------------- references, computed once per (C, rows)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _fwd_case(C, rows):
    def make():
        t = _case(C, rows, 7 * C + rows)
        t["x"] = _rows(t["x"])
        return t
    return _cached(("case", C, rows), make)


def _oracle_post(t, mh=1.0, mo=1.0, rsv=1.0):
    """v2 placement, float64 with the kernel's rounding points: gelu(h) * mask -> bf16 (operand of fc2), mlp(x) -> bf16 (what the
    LayerNorm reads), out = x + rs * LayerNorm(mask_o * mlp(x))."""
    from oracle import model as OM
    x = t["x"].double()
    h = OM.linear(x, t["w1"].double(), t["b1"].double())
    act = OM.gelu(h) * mh
    m = OM.linear(act.to(BF).double(), t["w2"].double(), t["b2"].double())
    out = x + rsv * OM.layer_norm(m.to(BF).double() * mo, t["ln_w"].double(), t["ln_b"].double())
    return dict(h=h, act=act, m=m, out=out)


def _row_scale(samples):
    """DropPath factors of rate 0.1: every fourth sample (1, 5, 9, ...) dropped, the rest 1 / 0.9."""
    rs = torch.full((samples,), 1.0 / 0.9, device=DEV)
    rs[1::4] = 0.0
    return rs


# ----------------------------------------------------------------------------- C: every form over the loop, against the oracle
SAVE_SETS = {  # v1 forward: which of n / (mean, rstd) / h / act the caller keeps
    "production": dict(n=True, stats=True, h=True, act=False),  # FusedMlpBlockFn with MLP_KEEP_ACT = False
    "full": dict(n=True, stats=True, h=True, act=True),
    "no_n": dict(n=False, stats=True, h=True, act=True),
    "no_stats": dict(n=True, stats=False, h=True, act=True),
    "no_h": dict(n=True, stats=True, h=False, act=True),
}


@pytest.mark.parametrize("keep", list(SAVE_SETS))
@pytest.mark.parametrize("rows,reserved,samples", SHAPES)
@pytest.mark.parametrize("C", [96, 128])
def test_v1_forward_save_sets(C, rows, reserved, samples, keep):
    """out = x + fc2(gelu(fc1(LayerNorm(x)))) with each combination of kept tensors the ABI allows: the production set, the full
    set, and the full set less one of n_out / (mean_out, rstd_out) / h_out."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    t, H, k = _fwd_case(C, rows), 4 * C, SAVE_SETS[keep]
    ref = _cached(("v1", C, rows), lambda: _oracle_fwd(t, True, True))
    o = Outputs()
    out = o.new("out", (rows, C))
    n = o.new("n", (rows, C)) if k["n"] else None
    mean, rstd = (o.new("mean", (rows,), torch.float32), o.new("rstd", (rows,), torch.float32)) if k["stats"] else (None, None)
    h = o.new("h", (rows, H)) if k["h"] else None
    act = o.new("act", (rows, H)) if k["act"] else None
    tag = f"v1 fwd C={C} rows={rows} keep={keep}"
    with _grid(rows, reserved, tag):
        L.check(lib.hs_mlp_fused_fwd(ptr(t["x"]), ptr(t["ln_w"]), ptr(t["ln_b"]), ptr(t["w1"]), ptr(t["b1"]), ptr(t["w2"]), ptr(t["b2"]),
                                     ptr(n), ptr(mean), ptr(rstd), ptr(h), ptr(act), ptr(out), rows, C, H, L.HS_ATTN_RESIDUAL, L.HS_BF16,
                                     _stream()), "hs_mlp_fused_fwd")
    checks = [(out, ref["out"], TOL[BF], "out")]
    checks += [(n, ref["n"], TOL[BF], "LayerNorm(x)")] if k["n"] else []
    checks += [(mean, ref["mean"], 1e-5, "mean"), (rstd, ref["rstd"], 1e-5, "rstd")] if k["stats"] else []
    checks += [(h, ref["h"], TOL[BF], "h")] if k["h"] else []
    checks += [(act, ref["act"], TOL[BF], "gelu(h)")] if k["act"] else []
    _judge(tag, o, checks)


@pytest.mark.parametrize("keep_act", [True, False])
@pytest.mark.parametrize("rows,reserved,samples", SHAPES)
@pytest.mark.parametrize("C", [96, 128])
def test_v2_forward_post_norm(C, rows, reserved, samples, keep_act):
    """HS_ATTN_RESIDUAL | HS_MLP_NORM_AFTER: out = x + LayerNorm(mlp(x)); kept are mlp(x), the statistics of its bf16 rounding
    (judged against the rows the kernel itself stored), h and optionally gelu(h) -- all but h leave in the deferred epilogue."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    t, H = _fwd_case(C, rows), 4 * C
    ref = _cached(("v2", C, rows), lambda: _oracle_post(t))
    o = Outputs()
    out, m, h = o.new("out", (rows, C)), o.new("m", (rows, C)), o.new("h", (rows, H))
    mean, rstd = o.new("mean", (rows,), torch.float32), o.new("rstd", (rows,), torch.float32)
    act = o.new("act", (rows, H)) if keep_act else None
    tag = f"v2 fwd C={C} rows={rows} act={'kept' if keep_act else 'null'}"
    with _grid(rows, reserved, tag):
        L.check(lib.hs_mlp_fused_fwd(ptr(t["x"]), ptr(t["ln_w"]), ptr(t["ln_b"]), ptr(t["w1"]), ptr(t["b1"]), ptr(t["w2"]), ptr(t["b2"]),
                                     ptr(m), ptr(mean), ptr(rstd), ptr(h), ptr(act), ptr(out), rows, C, H,
                                     L.HS_ATTN_RESIDUAL | L.HS_MLP_NORM_AFTER, L.HS_BF16, _stream()), "hs_mlp_fused_fwd")
    md = m.double()
    checks = [(m, ref["m"], TOL[BF], "mlp(x)"), (mean, md.mean(1), 1e-5, "mean"), (rstd, (md.var(1, unbiased=False) + 1e-5).rsqrt(), 1e-5, "rstd"),
              (h, ref["h"], TOL[BF], "h"), (out, ref["out"], TOL[BF], "out")]
    checks += [(act, ref["act"], TOL[BF], "gelu(h)")] if keep_act else []
    _judge(tag, o, checks)


@pytest.mark.parametrize("drop_p,with_path", [(0.1, True), (0.25, False), (0.0, True)])
@pytest.mark.parametrize("rows,reserved,samples", SHAPES)
@pytest.mark.parametrize("C", [96, 128])
def test_drop_forward(C, rows, reserved, samples, drop_p, with_path):
    """hs_mlp_fused_drop_fwd: out = x + rs[sample] * LayerNorm(mask_o * fc2(mask_h * gelu(fc1(x)))) with the generator's own masks
    (mask_of: functions of seed and element index).  The hidden mask is keyed by the CURRENT tile, the output mask and the DropPath
    factor by the PREVIOUS one.  Exact beside the toleranced comparisons: the kept activation is 0 exactly where the hidden mask is
    0 (and nowhere else, where gelu(h) is representable: 0 < |h| <= 8), and a sample with factor 0 returns x bit for bit."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    t, H = _fwd_case(C, rows), 4 * C
    per = rows // samples
    rs = _row_scale(samples) if with_path else None

    def make():
        mh = mask_of(SEEDS[0], drop_p, (rows, H)) if drop_p else 1.0
        mo = mask_of(SEEDS[1], drop_p, (rows, C)) if drop_p else 1.0
        rsv = rs.double().repeat_interleave(per).view(rows, 1) if with_path else 1.0
        return mh, mo, _oracle_post(t, mh, mo, rsv)
    mh, mo, ref = _cached(("drop", C, rows, drop_p, with_path), make)
    o = Outputs()
    out, m, h, act = o.new("out", (rows, C)), o.new("m", (rows, C)), o.new("h", (rows, H)), o.new("act", (rows, H))
    mean, rstd = o.new("mean", (rows,), torch.float32), o.new("rstd", (rows,), torch.float32)
    tag = f"drop fwd C={C} rows={rows} p={drop_p} path={with_path}"
    with _grid(rows, reserved, tag):
        L.check(lib.hs_mlp_fused_drop_fwd(ptr(t["x"]), ptr(t["ln_w"]), ptr(t["ln_b"]), ptr(t["w1"]), ptr(t["b1"]), ptr(t["w2"]), ptr(t["b2"]),
                                          ptr(m), ptr(mean), ptr(rstd), ptr(h), ptr(act), ptr(out), ptr(rs), per, drop_p, SEEDS[0], SEEDS[1],
                                          rows, C, H, L.HS_ATTN_RESIDUAL | L.HS_MLP_NORM_AFTER, L.HS_BF16, _stream()), "hs_mlp_fused_drop_fwd")
    md = m.double() * mo  # the LayerNorm's input: the stored rows behind the output mask
    checks = [(h, ref["h"], TOL[BF], "h"), (act, ref["act"], TOL[BF], "mask_h * gelu(h)"), (m, ref["m"], TOL[BF], "mlp(x)"),
              (mean, md.mean(1), 1e-5, "mean"), (rstd, (md.var(1, unbiased=False) + 1e-5).rsqrt(), 1e-5, "rstd"),
              (out, ref["out"], TOL[BF], "out")]
    exact = []
    if drop_p:
        frac = 1.0 - (mh != 0).double().mean().item()
        exact.append((abs(frac - drop_p) < 0.01 or rows < 1024, f"hidden drop fraction {frac} vs {drop_p}"))
        hk = h.double().abs()
        alive = (mh != 0) & (hk > 0) & (hk <= 8)
        exact.append((bool((act[mh == 0] == 0).all()), "kept activation is not 0 everywhere the hidden mask is 0"))
        exact.append((bool((act[alive] != 0).all()), "kept activation is 0 where the hidden mask keeps a non-zero gelu(h)"))
    if with_path:
        gone = (rs == 0).repeat_interleave(per)
        exact.append((torch.equal(out[gone], t["x"][gone]), "rows of a sample with DropPath factor 0 differ from x"))
        if samples > 1:
            exact.append((bool(gone.any()) and not torch.equal(out[~gone], t["x"][~gone]), "no sample was dropped, or every sample was"))
    _judge(tag, o, checks, exact)


def _bwd_case(C, rows):
    def make():
        t = _case(C, rows, 11 * C + rows)
        g = torch.Generator(device=DEV).manual_seed(5)
        t["dy"] = _rows(torch.randn((rows, C), generator=g, device=DEV).to(BF))
        t["h"] = _rows((torch.randn((rows, 4 * C), generator=g, device=DEV) * 1.5).to(BF))
        t["dres"] = _rows(torch.randn((rows, C), generator=g, device=DEV).to(BF))
        t["w2t"], t["w1t"] = t["w2"].t().contiguous(), t["w1"].t().contiguous()
        t["dact"] = t["dy"].double() @ t["w2"].double()
        t["gp"] = _gelu_grad64(t["h"].double())
        return t
    return _cached(("bwd", C, rows), make)


def _bwd_judge(tag, o, t, dh, dn, mh, with_res, exact=()):
    dh_ref = t["dact"] * t["gp"] * mh
    dn_ref = dh_ref.to(BF).double() @ t["w1"].double()
    if with_res:
        dn_ref = dn_ref + t["dres"].double()
    _judge(tag, o, [(dh, dh_ref, TOL[BF], "dh"), (dn, dn_ref, TOL[BF], "dn")], exact)


@pytest.mark.parametrize("rows,reserved,samples", SHAPES)
@pytest.mark.parametrize("C", [96, 128])
def test_plain_backward_with_dres(C, rows, reserved, samples):
    """dh = (dy W2) * gelu'(h), dn = dh W1 + dres; the dres rows are plain global loads requested one tile ahead of their use."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    t, H = _bwd_case(C, rows), 4 * C
    o = Outputs()
    dh, dn = o.new("dh", (rows, H)), o.new("dn", (rows, C))
    tag = f"bwd C={C} rows={rows} dres"
    with _grid(rows, reserved, tag):
        L.check(lib.hs_mlp_fused_bwd(ptr(t["dy"]), ptr(t["h"]), ptr(t["w2t"]), ptr(t["w1t"]), ptr(t["dres"]), ptr(dh), ptr(dn), rows, C, H,
                                     L.HS_BF16, _stream()), "hs_mlp_fused_bwd")
    _bwd_judge(tag, o, t, dh, dn, 1.0, True)


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("rows,reserved,samples", SHAPES)
@pytest.mark.parametrize("C", [96, 128])
def test_drop_backward(C, rows, reserved, samples, with_res):
    """hs_mlp_fused_drop_bwd: dh = mask_h * (dy W2) * gelu'(h) with the forward's hidden mask (same seed, keyed by the current tile),
    dn = dh W1 (+ dres); dh is exactly 0 where the mask is 0."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    t, H, drop_p = _bwd_case(C, rows), 4 * C, 0.1
    mh = _cached(("mh", rows, H), lambda: mask_of(SEEDS[0], drop_p, (rows, H)))
    o = Outputs()
    dh, dn = o.new("dh", (rows, H)), o.new("dn", (rows, C))
    tag = f"drop bwd C={C} rows={rows} dres={with_res}"
    with _grid(rows, reserved, tag):
        L.check(lib.hs_mlp_fused_drop_bwd(ptr(t["dy"]), ptr(t["h"]), ptr(t["w2t"]), ptr(t["w1t"]), ptr(t["dres"] if with_res else None), ptr(dh),
                                          ptr(dn), drop_p, SEEDS[0], rows, C, H, L.HS_BF16, _stream()), "hs_mlp_fused_drop_bwd")
    exact = [(bool((dh[mh == 0] == 0).all()), "dh is not 0 everywhere the hidden mask is 0"),
             (bool((mh == 0).any()) and float((dh[mh != 0] != 0).double().mean()) > 0.99, "the mask drops nothing, or dh is 0 where it keeps")]
    _bwd_judge(tag, o, t, dh, dn, mh, with_res, exact)


# ----------------------------------------------------------------------------- D: exact probes of the two products
def probe_maps(C, device):
    """Index structure of the probes.
    ch[j]: the one channel hidden unit j reads in product 1 -- a bijection inside each block of C units (5 is coprime with 96 and
        128), shifted per block, so every channel feeds four hidden units.
    sup[c, 0..3]: the four hidden units channel c reads in product 2.  The units are listed in the order 64 (t % NW) + t / NW, which
        cycles through the NW = C / 16 waves' 64-wide column blocks of product 1; channel c takes four consecutive entries of that list
        (its group permuted by 7 c + 3), hence four different waves' blocks and four different 32-wide k-steps of product 2, and the C
        supports partition the 4 C units."""
    H, NW = 4 * C, C // 16
    j = torch.arange(H, device=device)
    ch = (5 * (j % C) + 7 * (j // C)) % C
    order = 64 * (j % NW) + j // NW
    c = torch.arange(C, device=device)
    k = torch.arange(4, device=device)
    sup = order[(4 * ((7 * c + 3) % C))[:, None] + k]
    rot = (c[:, None] + k) % 4  # which of the four distinct powers of two each member gets
    assert torch.equal(torch.bincount(ch, minlength=C), torch.full((C,), 4, device=device))
    assert torch.equal(sup.flatten().sort().values, j)
    for width in (32, 64):
        blk = (sup // width).sort(1).values
        assert bool((blk[:, 1:] != blk[:, :-1]).all()), f"a support has two units in one {width}-wide block"
    return ch, sup, rot


def _dense(C, ch, vals, sup, pw, device):
    """[4C, C] one-hot rows (A operand of product 1) and [C, 4C] four-term rows (A operand of product 2), bf16."""
    H = 4 * C
    wa = torch.zeros((H, C), device=device, dtype=torch.float64)
    wa[torch.arange(H, device=device), ch] = vals
    wb = torch.zeros((C, H), device=device, dtype=torch.float64)
    wb.scatter_(1, sup, pw)
    assert torch.equal(wa.to(BF).double(), wa) and torch.equal(wb.to(BF).double(), wb)
    return wa.to(BF), wb.to(BF)


def forward_probe_inputs(C, rows, residual, device):
    """x multiples of 1/4 in [-4, 4]; W1 one-hot with values from {1, -1, 0.5, -0.5, 2}; b1 multiples of 1/8 in [-1, 1]: h = w x + b1
    is a multiple of 1/8 with |h| <= 9, exact in bf16 (72 < 2^7).  W2 rows: weights {2, 1, 1/2, 1/4} on the four units of the
    support.  b2 multiples of 1/8 in [1, 2] without the residual and [5, 6] with it: gelu >= -0.17 bounds the product-2 sum below by
    -0.17 * 3.75 = -0.64, so out >= 0.36 (without) and >= -4 + 5 - 0.64 = 0.36 (with): no cancellation, no |out| below 2^-6."""
    g = torch.Generator(device=device).manual_seed(1000 * C + rows + int(residual))
    H = 4 * C
    ch, sup, rot = probe_maps(C, device)
    x = torch.randint(-16, 17, (rows, C), generator=g, device=device).double() / 4
    vals = torch.tensor([1.0, -1.0, 0.5, -0.5, 2.0], device=device, dtype=torch.float64)[torch.randint(0, 5, (H,), generator=g, device=device)]
    b1 = torch.randint(-8, 9, (H,), generator=g, device=device).double() / 8
    pw = 2.0 ** (1 - rot).double()
    b2 = (5.0 if residual else 1.0) + torch.randint(0, 9, (C,), generator=g, device=device).double() / 8
    w1, w2 = _dense(C, ch, vals, sup, pw, device)
    assert torch.equal(x.to(BF).double(), x)
    return dict(x=x.to(BF), w1=w1, w2=w2, b1=b1.float(), b2=b2.float(), ch=ch, vals=vals, sup=sup, pw=pw)


def backward_probe_inputs(C, rows, device):
    """Integer dy in [-3, 3]; W2^T one-hot with values from {1, -1, 2, -2, 4}: dact = w dy is an integer, |dact| <= 12, exact.
    W1^T rows: weights {8, 4, 2, 1} on the four units of the support.  Saved h: multiples of 1/8 in [-4, 4], drawn per element from
    [-0.625, 4] (gelu' >= 0.06 > 0) or [-2.75, -0.875] (gelu' <= -0.022 < 0) such that sign(dact gelu'(h)) is one sign s per TOKEN;
    dres = s * (multiple of 1/4 in [1/4, 4]).  All terms of a dn element then share a sign: dn is exactly 0 (every dy read is 0, no
    dres) or |dn| >= 1 * 1 * 1 * 0.022 > 2^-6 -- the float64 reference has no cancellation."""
    g = torch.Generator(device=device).manual_seed(2000 * C + rows)
    H = 4 * C
    ch, sup, rot = probe_maps(C, device)
    dy = torch.randint(-3, 4, (rows, C), generator=g, device=device).double()
    vals = torch.tensor([1.0, -1.0, 2.0, -2.0, 4.0], device=device, dtype=torch.float64)[torch.randint(0, 5, (H,), generator=g, device=device)]
    pw = 2.0 ** (3 - rot).double()
    dact = dy[:, ch] * vals
    s = (2 * torch.randint(0, 2, (rows, 1), generator=g, device=device) - 1).double()
    h_pos = torch.randint(-5, 33, (rows, H), generator=g, device=device).double() / 8
    h_neg = torch.randint(-22, -6, (rows, H), generator=g, device=device).double() / 8
    h = torch.where(torch.sign(dact) * s >= 0, h_pos, h_neg)
    dres = s * torch.randint(1, 17, (rows, C), generator=g, device=device).double() / 4
    w2t, w1t = _dense(C, ch, vals, sup, pw, device)
    assert torch.equal(h.to(BF).double(), h) and torch.equal(dres.to(BF).double(), dres)
    return dict(dy=dy.to(BF), h=h.to(BF), dres=dres.to(BF), w2t=w2t, w1t=w1t, dact=dact, sup=sup, pw=pw)


def _product2_bound(ref, terms):
    """One bf16 rounding of the result, |v| 2^-8 (half an ulp of 8 significant bits), plus 5 fp32 roundings of partial sums that
    never exceed the sum of the terms' magnitudes (four products and the bias / residual rows): 5 * 2^-24 * sum|terms|.  Elements
    below 2^-6 are judged against the additive term alone."""
    return torch.where(ref.abs() >= 2.0 ** -6, ref.abs() * 2.0 ** -8, torch.zeros_like(ref)) + 5 * 2.0 ** -24 * terms


def _worst(err, bound):
    ex = err - bound
    i = int(ex.argmax())
    return f"worst excess {float(ex.flatten()[i]):.3e} at row {i // err.shape[1]}, column {i % err.shape[1]} " \
           f"(error {float(err.flatten()[i]):.3e}, bound {float(bound.flatten()[i]):.3e}); {int((ex > 0).sum())} of {err.numel()} elements over"


PROBE_SHAPES = [pytest.param(64, None, id="64"), pytest.param(LOOP_ROWS, LOOP_RESERVED, id="loop")]


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("rows,reserved", PROBE_SHAPES)
@pytest.mark.parametrize("C", [96, 128])
def test_forward_products_exact_probe(C, rows, reserved, residual):
    """Structured weights (forward_probe_inputs), no LayerNorm, so every (token, hidden unit, channel) path is judged on its own:
      h      = W1[j, ch(j)] x[ch(j)] + b1[j] is exactly representable: torch.equal;
      act    within 2^-8 |gelu64(h)| + 4e-6: one bf16 rounding plus twice the 2e-6 test_gelu_matches_erf_gelu enforces for hs_gelu.h;
      out    against float64 arithmetic on the act the kernel stored (the operand product 2 reads), b2 and x, within
             _product2_bound: a lost k-step, a swapped fragment, a wrong bias slot or a wrong residual row moves an element by at
             least 1/4 of an activation or 1/8 of a bias step.
    The inputs keep out >= 0.36 (docstring of forward_probe_inputs), so the bound is never judged at a cancelled value."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    H = 4 * C
    p = forward_probe_inputs(C, rows, residual, DEV)
    x = _rows(p["x"])
    o = Outputs()
    out, h, act = o.new("out", (rows, C)), o.new("h", (rows, H)), o.new("act", (rows, H))
    tag = f"fwd probe C={C} rows={rows} residual={residual}"
    with _grid(rows, reserved, tag):
        L.check(lib.hs_mlp_fused_fwd(ptr(x), None, None, ptr(p["w1"]), ptr(p["b1"]), ptr(p["w2"]), ptr(p["b2"]), None, None, None, ptr(h),
                                     ptr(act), ptr(out), rows, C, H, L.HS_ATTN_RESIDUAL if residual else 0, L.HS_BF16, _stream()),
                "hs_mlp_fused_fwd")
    bad = o.problems()
    x64 = x.double()
    h_ref = x64[:, p["ch"]] * p["vals"] + p["b1"].double()
    assert torch.equal(h_ref.to(BF).double(), h_ref)
    if not torch.equal(h, h_ref.to(BF)):
        bad.append(f"{tag} h: {int((h != h_ref.to(BF)).sum())} elements differ from the exact value")
    g64 = _gelu64(h_ref)
    err, bound = (act.double() - g64).abs(), g64.abs() * 2.0 ** -8 + 4e-6
    if not bool((err <= bound).all()):
        bad.append(f"{tag} act: {_worst(err, bound)}")
    terms = act.double()[:, p["sup"]] * p["pw"]  # [rows, C, 4]
    ref = terms.sum(-1) + p["b2"].double() + (x64 if residual else 0.0)
    mag = terms.abs().sum(-1) + p["b2"].double().abs() + (x64.abs() if residual else 0.0)
    if float(ref.abs().min()) < 2.0 ** -6:
        bad.append(f"{tag}: the reference reaches |out| = {float(ref.abs().min()):.3e} < 2^-6, the inputs were to exclude that")
    err, bound = (out.double() - ref).abs(), _product2_bound(ref, mag)
    if not bool((err <= bound).all()):
        bad.append(f"{tag} out: {_worst(err, bound)}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("rows,reserved", PROBE_SHAPES)
@pytest.mark.parametrize("C", [96, 128])
def test_backward_products_exact_probe(C, rows, reserved, with_res):
    """The transposed probe (backward_probe_inputs): dact = W2^T[j, ch(j)] dy[ch(j)] is an exact integer, so
      dh     within 2^-8 |v| + 4e-6 |dact| of v = dact gelu'64(h): one bf16 rounding, plus |dact| times twice the 2e-6 that
             test_gelu_matches_erf_gelu enforces for GELU' (the fp32 product's own rounding, 6e-8 |v|, is inside that);
      dn     against float64 arithmetic on the dh the kernel stored through the four-term W1^T rows, plus dres, within
             _product2_bound.
    All terms of a dn element share a sign (docstring of backward_probe_inputs): an element is exactly 0 or above 2^-6."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    H = 4 * C
    p = backward_probe_inputs(C, rows, DEV)
    dy, hs, dres = _rows(p["dy"]), _rows(p["h"]), _rows(p["dres"]) if with_res else None
    o = Outputs()
    dh, dn = o.new("dh", (rows, H)), o.new("dn", (rows, C))
    tag = f"bwd probe C={C} rows={rows} dres={with_res}"
    with _grid(rows, reserved, tag):
        L.check(lib.hs_mlp_fused_bwd(ptr(dy), ptr(hs), ptr(p["w2t"]), ptr(p["w1t"]), ptr(dres), ptr(dh), ptr(dn), rows, C, H, L.HS_BF16,
                                     _stream()), "hs_mlp_fused_bwd")
    bad = o.problems()
    v = p["dact"] * _gelu_grad64(hs.double())
    err, bound = (dh.double() - v).abs(), v.abs() * 2.0 ** -8 + 4e-6 * p["dact"].abs()
    if not bool((err <= bound).all()):
        bad.append(f"{tag} dh: {_worst(err, bound)}")
    terms = dh.double()[:, p["sup"]] * p["pw"]
    ref = terms.sum(-1) + (dres.double() if with_res else 0.0)
    mag = terms.abs().sum(-1) + (dres.double().abs() if with_res else 0.0)
    small = (ref != 0) & (ref.abs() < 2.0 ** -6)
    if bool(small.any()):
        bad.append(f"{tag}: {int(small.sum())} reference elements lie in (0, 2^-6), the inputs were to exclude that")
    err, bound = (dn.double() - ref).abs(), _product2_bound(ref, mag)
    if not bool((err <= bound).all()):
        bad.append(f"{tag} dn: {_worst(err, bound)}")
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------- E: argument contract
def _contract_fwd(drop, rows=96, **kw):
    """One refused forward call at C = 128: returns (status, outputs).  Keyword arguments replace single arguments of a valid call."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    C, H = 128, 512
    t = _fwd_case(C, rows)
    o = Outputs()
    a = dict(g=t["ln_w"], b=t["ln_b"], n=o.new("n", (rows, C)), mean=o.new("mean", (rows,), torch.float32),
             rstd=o.new("rstd", (rows,), torch.float32), h=o.new("h", (rows, H)), act=o.new("act", (rows, H)), out=o.new("out", (rows, C)),
             rs=torch.ones(3, device=DEV), per=32, p=0.1, flags=L.HS_ATTN_RESIDUAL | (L.HS_MLP_NORM_AFTER if drop else 0))
    a.update(kw)
    head = (ptr(t["x"]), ptr(a["g"]), ptr(a["b"]), ptr(t["w1"]), ptr(t["b1"]), ptr(t["w2"]), ptr(t["b2"]), ptr(a["n"]), ptr(a["mean"]),
            ptr(a["rstd"]), ptr(a["h"]), ptr(a["act"]), ptr(a["out"]))
    if drop:
        rc = lib.hs_mlp_fused_drop_fwd(*head, ptr(a["rs"]), a["per"], a["p"], SEEDS[0], SEEDS[1], rows, C, H, a["flags"], L.HS_BF16, _stream())
    else:
        rc = lib.hs_mlp_fused_fwd(*head, rows, C, H, a["flags"], L.HS_BF16, _stream())
    torch.cuda.synchronize()
    return rc, o


CONTRACT_FWD = {
    "drop_p=-0.1": dict(drop=True, p=-0.1),
    "drop_p=1.0": dict(drop=True, p=1.0),
    "drop form without HS_MLP_NORM_AFTER": dict(drop=True, flags=4),
    "rows_per_sample=48 (no multiple of 32)": dict(drop=True, per=48),
    "rows_per_sample=64 (does not divide 96 rows)": dict(drop=True, per=64),
    "mean_out without rstd_out": dict(drop=False, rstd=None),
    "rstd_out without mean_out": dict(drop=False, mean=None),
    "ln_gamma without ln_beta": dict(drop=False, b=None),
    "ln_beta without ln_gamma": dict(drop=False, g=None),
    "HS_MLP_NORM_AFTER without gamma": dict(drop=False, flags=4 | 16, g=None, b=None),
    "HS_MLP_NORM_AFTER without gamma, drop form": dict(drop=True, g=None, b=None),
    "rows=48": dict(drop=False, rows=48),
    "rows=48, drop form": dict(drop=True, rows=48, rs=None),
}


@pytest.mark.parametrize("case", list(CONTRACT_FWD))
def test_forward_argument_contract(case):
    """Every refused forward call returns a status other than HS_OK and writes nothing."""
    assert (_L().HS_ATTN_RESIDUAL, _L().HS_MLP_NORM_AFTER) == (4, 16)
    rc, o = _contract_fwd(**CONTRACT_FWD[case])
    bad = o.problems(untouched=True)
    assert rc != 0 and not bad, f"{case}: status {rc}\n" + "\n".join(bad)


@pytest.mark.parametrize("case,drop,drop_p,rows", [("drop_p=-0.1", True, -0.1, 96), ("drop_p=1.0", True, 1.0, 96), ("rows=48", False, 0.0, 48),
                                                   ("rows=48, drop form", True, 0.1, 48)])
def test_backward_argument_contract(case, drop, drop_p, rows):
    L = _L()
    lib, ptr = L.lib, L.ptr
    C, H = 128, 512
    t = _bwd_case(C, rows)
    o = Outputs()
    dh, dn = o.new("dh", (rows, H)), o.new("dn", (rows, C))
    head = (ptr(t["dy"]), ptr(t["h"]), ptr(t["w2t"]), ptr(t["w1t"]), ptr(t["dres"]), ptr(dh), ptr(dn))
    if drop:
        rc = lib.hs_mlp_fused_drop_bwd(*head, drop_p, SEEDS[0], rows, C, H, L.HS_BF16, _stream())
    else:
        rc = lib.hs_mlp_fused_bwd(*head, rows, C, H, L.HS_BF16, _stream())
    torch.cuda.synchronize()
    bad = o.problems(untouched=True)
    assert rc != 0 and not bad, f"{case}: status {rc}\n" + "\n".join(bad)
