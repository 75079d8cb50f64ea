"""Operator-level tests of the weight-gradient kernels (csrc/linear_wgrad.hip): every stage count around the 3- and 4-stage rings,
ragged last stages and slices, partial tiles, column blocks with hostile neighbours, groups and the register-staged fallback, at the
smallest shapes where each can go wrong.

EXACT, not toleranced: the operands are integers drawn from {-3 ... 3} (exact in bf16 and fp32), so every partial sum is an integer
of magnitude <= 9 * rows <= 9 * 1025 < 2^24 and every fp32 accumulation is exact in any order: dW must EQUAL dY^T X computed in
float64, and dbias the column sums.  A wrong token, a stage read twice or a lost tail row changes an integer.  (The GELU-operand
entry is not integer-valued: it keeps the reference and bounds of test_gpu_mlp_fused.py::test_linear_wgrad_gelu_equals_wgrad_of_gelu.)

Sentinels: the workspace continues with 1024 NaN floats that must stay NaN; dw and dbias are views into larger buffers whose other
elements must stay untouched; dY and X are the first `rows` rows of allocations that continue with 64 rows of NaN, so a kernel that
reads past its slice poisons an integer result (it does not fault).

Rows: up to 512 rows are one token slice.  bf16 stages hold 32 tokens: rows 1 ... 161 give 1 ... 6 stages (fewer than the prologue
issues, one full trip of the 3- and of the 4-stage ring, the first stage of the second trip of each, every branch of the vmcnt
ladder, a one-token last stage); 513 = 2 slices of 288 rows, the last with 225; 1025 = 3 slices of 352, the last with 321.  fp32
stages hold 16 tokens."""
import ctypes
import functools
import os
import subprocess
import sys

import pytest
import torch

from _util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64          # guard elements on both sides of dw / dbias (a multiple of 4: the destinations stay 16-byte aligned)
GUARD = 12345.0   # what the guard elements hold
TAIL = 64         # NaN rows behind the operands

ROWS_BF16 = [1, 32, 33, 64, 65, 96, 97, 128, 129, 161, 513, 1025]
ROWS_F32 = [1, 16, 17, 33, 48, 49, 65, 513]
# kernel -> (hs_linear_wgrad_group_variant, shapes (n_out, k_in))
BF16_SHAPES = {
    "256x256": (1, [(256, 256), (520, 256)]),          # n >= 512, no multiple of 256: the last n tile has 8 live rows
    "256x128": (2, [(256, 128), (520, 136)]),
    "128x128": (3, [(128, 128), (96, 288), (12, 40)]),  # n_out % 8 == 4 (the 12-class head): LDS-DMA path only
}
BF16_CASES = [pytest.param(v, n, k, r, id=f"{kern}-{n}x{k}-rows{r}") for kern, (v, shapes) in BF16_SHAPES.items() for n, k in shapes
              for r in ROWS_BF16]


def _L():
    from heal_swin_amd import _lib
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ints(shape, g):
    return torch.randint(-3, 4, shape, generator=g, device=DEV).float()


def _with_tail(m, cols=None, col0=0):
    """m as the first rows (and the columns from col0) of an allocation that is NaN everywhere else; returns (allocation, view)."""
    rows, width = m.shape
    buf = torch.full((rows + TAIL, cols or width), float("nan"), dtype=m.dtype, device=DEV)
    buf[:rows, col0:col0 + width] = m
    return buf, buf[:rows, col0:col0 + width]


@functools.lru_cache(maxsize=None)
def _operands(rows, n_out, k_in, dtype):
    """Integer operands behind NaN rows and their exact products, made once per shape and never changed."""
    g = torch.Generator(device=DEV).manual_seed(1000 * rows + n_out + k_in)
    dy, x = _ints((rows, n_out), g).to(dtype), _ints((rows, k_in), g).to(dtype)
    ref_w = (dy.double().t() @ x.double()).float()
    ref_b = dy.double().sum(0).float()
    return _with_tail(dy)[0], _with_tail(x)[0], ref_w, ref_b


class _Dest:
    """dw / dbias as views into larger buffers, preset to integers for accumulate = 1."""

    def __init__(self, n_out, k_in, bias, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.wbuf = torch.full((n_out * k_in + 2 * PAD,), GUARD, device=DEV)
        self.bbuf = torch.full((n_out + 2 * PAD,), GUARD, device=DEV)
        self.dw = self.wbuf[PAD:PAD + n_out * k_in].view(n_out, k_in)
        self.db = self.bbuf[PAD:PAD + n_out] if bias else None
        self.dw.copy_(_ints((n_out, k_in), g))
        self.bbuf[PAD:PAD + n_out] = _ints((n_out,), g)
        self.base_w, self.base_b = self.dw.clone(), self.bbuf[PAD:PAD + n_out].clone()

    def check(self, ref_w, ref_b, acc, what):
        assert torch.equal(self.dw, ref_w + self.base_w if acc else ref_w), f"{what}: dw"
        if self.db is not None:
            assert torch.equal(self.db, ref_b + self.base_b if acc else ref_b), f"{what}: dbias"
        else:
            assert torch.equal(self.bbuf[PAD:-PAD], self.base_b), f"{what}: dbias written without a bias"
        for buf in (self.wbuf, self.bbuf):
            assert bool((buf[:PAD] == GUARD).all()) and bool((buf[-PAD:] == GUARD).all()), f"{what}: wrote beside dw / dbias"


def _workspace(floats):
    return torch.full((floats + 1024,), float("nan"), dtype=torch.float32, device=DEV)


def _check_guard(ws, floats, what):
    assert bool(torch.isnan(ws[floats:]).all()), f"{what}: wrote behind its workspace"


def _run_exact(rows, n_out, k_in, dtype, bias=True, acc=0, what=""):
    L = _L()
    ybuf, xbuf, ref_w, ref_b = _operands(rows, n_out, k_in, dtype)
    d = _Dest(n_out, k_in, bias, rows + acc)
    nws = int(L.lib.hs_linear_wgrad_workspace(rows, n_out, k_in))
    ws = _workspace(nws)
    L.check(L.lib.hs_linear_wgrad(L.ptr(ybuf), L.ptr(xbuf), L.ptr(d.dw), L.ptr(d.db), L.ptr(ws), rows, n_out, k_in, acc,
                                  L.dtype_code(dtype), _stream()), "hs_linear_wgrad")
    torch.cuda.synchronize()
    d.check(ref_w, ref_b, acc, what or f"rows {rows} {n_out}x{k_in} bias {bias} acc {acc}")
    _check_guard(ws, nws, what)


@pytest.mark.parametrize("variant,n_out,k_in,rows", BF16_CASES)
def test_bf16_exact_at_every_stage_count(variant, n_out, k_in, rows):
    L = _L()
    assert int(L.lib.hs_linear_wgrad_group_variant(rows, n_out, k_in, L.HS_BF16)) == variant
    _run_exact(rows, n_out, k_in, BF)


@pytest.mark.parametrize("n_out,k_in", [(128, 128), (100, 72)])
@pytest.mark.parametrize("rows", ROWS_F32)
def test_fp32_exact_at_every_stage_count(rows, n_out, k_in):
    _run_exact(rows, n_out, k_in, torch.float32)


@pytest.mark.parametrize("kernel,n_out,k_in,dtype", [("256x256", 520, 256, BF), ("256x128", 520, 136, BF), ("128x128", 96, 288, BF),
                                                     ("128x128_head", 12, 40, BF), ("fp32", 100, 72, torch.float32)])
def test_bias_and_accumulate_cross_on_every_kernel(kernel, n_out, k_in, dtype):
    for rows in (97, 513):
        for bias in (True, False):
            for acc in (0, 1):
                _run_exact(rows, n_out, k_in, dtype, bias, acc)


@pytest.mark.parametrize("rows", [33, 97, 513])
@pytest.mark.parametrize("n_out,k_in", [(128, 128), (96, 288)])
def test_gelu_operand_on_the_128_tile(rows, n_out, k_in):
    """Reference and bounds of test_gpu_mlp_fused.py::test_linear_wgrad_gelu_equals_wgrad_of_gelu: float64 with the oracle's gelu on the
    same bf16 h at 3e-3, dbias at 1e-3."""
    from oracle import model as OM
    L = _L()
    assert L.lib.hs_linear_wgrad_gelu_supported(rows, n_out, k_in, L.HS_BF16)
    assert int(L.lib.hs_linear_wgrad_group_variant(rows, n_out, k_in, L.HS_BF16)) == 3
    g = torch.Generator(device=DEV).manual_seed(rows)
    dy = torch.randn((rows, n_out), generator=g, device=DEV).to(BF)
    h = (torch.randn((rows, k_in), generator=g, device=DEV) * 1.5).to(BF)
    ybuf, xbuf = _with_tail(dy)[0], _with_tail(h)[0]
    wbuf, bbuf = torch.full((n_out * k_in + 2 * PAD,), GUARD, device=DEV), torch.full((n_out + 2 * PAD,), GUARD, device=DEV)
    dw, db = wbuf[PAD:-PAD].view(n_out, k_in), bbuf[PAD:-PAD]
    nws = int(L.lib.hs_linear_wgrad_workspace(rows, n_out, k_in))
    ws = _workspace(nws)
    L.check(L.lib.hs_linear_wgrad_gelu(L.ptr(ybuf), L.ptr(xbuf), L.ptr(dw), L.ptr(db), L.ptr(ws), rows, n_out, k_in, 0, L.HS_BF16,
                                       _stream()), "hs_linear_wgrad_gelu")
    ref = dy.double().t() @ OM.gelu(h.double()).to(BF).double()
    assert_close(dw, ref, 3e-3, f"wgrad_gelu {rows}x{n_out}x{k_in} dW")
    assert_close(db, dy.double().sum(0), 1e-3, f"wgrad_gelu {rows}x{n_out}x{k_in} db")
    for buf in (wbuf, bbuf):
        assert bool((buf[:PAD] == GUARD).all()) and bool((buf[-PAD:] == GUARD).all())
    _check_guard(ws, nws, "hs_linear_wgrad_gelu")


@pytest.mark.parametrize("rows", [97, 513])
@pytest.mark.parametrize("n_out,k_in", [(96, 288), (128, 128)])
def test_column_blocks_with_nan_neighbours(rows, n_out, k_in):
    """hs_linear_wgrad_ld on the middle block of a [rows, 3 n_out] and the last block of a [rows, 3 k_in] matrix whose other blocks are
    NaN: a tile that overhangs the operand's columns reads its neighbours into accumulators that are never stored."""
    L = _L()
    g = torch.Generator(device=DEV).manual_seed(7 * rows + n_out)
    dy, x = _ints((rows, n_out), g).to(BF), _ints((rows, k_in), g).to(BF)
    ybuf, _ = _with_tail(dy, 3 * n_out, n_out)
    xbuf, _ = _with_tail(x, 3 * k_in, 2 * k_in)
    d = _Dest(n_out, k_in, True, rows)
    nws = int(L.lib.hs_linear_wgrad_workspace(rows, n_out, k_in))
    ws = _workspace(nws)
    L.check(L.lib.hs_linear_wgrad_ld(L.ptr(ybuf), 3 * n_out, n_out, L.ptr(xbuf), 3 * k_in, 2 * k_in, L.ptr(d.dw), L.ptr(d.db), L.ptr(ws),
                                     rows, n_out, k_in, 1, _stream()), "hs_linear_wgrad_ld")
    torch.cuda.synchronize()
    d.check((dy.double().t() @ x.double()).float(), dy.double().sum(0).float(), 1, "hs_linear_wgrad_ld")
    _check_guard(ws, nws, "hs_linear_wgrad_ld")


# (rows, [(n_out, k_in, bias)], one launch expected)
GROUPS = {
    "128tile_triple": (97, [(128, 128, True), (96, 288, False), (24, 40, True)], True),
    "256tile_pair": (129, [(256, 256, True), (512, 256, True)], True),
    "mixed_tiles_launch_alone": (97, [(256, 256, True), (128, 128, True), (512, 128, False)], False),
}


@pytest.mark.parametrize("name", list(GROUPS))
def test_groups_exact(name):
    L = _L()
    rows, members, one_launch = GROUPS[name]
    variants = {int(L.lib.hs_linear_wgrad_group_variant(rows, n, k, L.HS_BF16)) for n, k, _ in members}
    assert (len(variants) == 1 and 0 not in variants) == one_launch, variants
    made, problems = [], []
    for i, (n_out, k_in, bias) in enumerate(members):
        ybuf, xbuf, ref_w, ref_b = _operands(rows, n_out, k_in, BF)
        d, acc = _Dest(n_out, k_in, bias, rows + i), i & 1
        made.append((d, ref_w, ref_b, acc))
        problems.append((ybuf, xbuf, d.dw, d.db, n_out, k_in, acc, False))
    arr = L.wgrad_problems(problems)
    nws = int(L.lib.hs_linear_wgrad_group_workspace(arr, len(members), rows, L.HS_BF16))
    assert nws > 0
    ws = _workspace(nws)
    L.check(L.lib.hs_linear_wgrad_group(arr, len(members), L.ptr(ws), rows, L.HS_BF16, _stream()), "hs_linear_wgrad_group")
    torch.cuda.synchronize()
    for i, (d, ref_w, ref_b, acc) in enumerate(made):
        d.check(ref_w, ref_b, acc, f"{name} member {i}")
    _check_guard(ws, nws, name)


def _fallback_child():
    """Runs in the child process of the test below, where HS_WGRAD_VARIANT=0 selects the register-staged kernels."""
    L = _L()
    for n_out, k_in in [(128, 128), (96, 288), (256, 128)]:
        for rows in (1, 33, 65, 513):
            assert int(L.lib.hs_linear_wgrad_group_variant(rows, n_out, k_in, L.HS_BF16)) == 0
            _run_exact(rows, n_out, k_in, BF, bias=True, acc=rows & 1)
    _run_exact(65, 96, 288, BF, bias=False, acc=0)
    print("fallback exact")


def test_register_staged_fallback_exact():
    """HS_WGRAD_VARIANT is read once per process, so the register-staged kernels (both tile heights) run in one fresh child."""
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_wgrad_kernels as t; t._fallback_child()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HS_WGRAD_VARIANT="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fallback exact" in r.stdout, r.stdout + r.stderr
