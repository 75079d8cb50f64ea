"""The small streaming kernels every training step runs through -- csrc/gelu.hip, split3.hip, shift_rows.hip, rel_bias.hip -- at the
code paths their first tests never reached, through the C ABI, element by element against a float64 / bit-exact reference:

  * the capped-grid pass: grids stop at 4096 workgroups of 256 threads (1 048 576 vectors) and loop; every kernel runs past it;
  * tails (n % 8 bf16, n % 4 fp32, n < one vector), with and without dropout;
  * the dropout mask against the HOST reference of the rule (tests/_mask_ref.py), exactly -- not against another kernel;
  * hs_split_bf16x3 in both modes against torch, bit for bit;
  * hs_gather_rows: the 16-byte kernel with tables and rolls, both kernels past their cap, the fallback from the pointer;
  * rel_bias.hip: empty and long runs, more than 48 batched jobs, more than 64 heads, bad jobs behind the first chunk.

Value bound (GELU, residual_drop):  |got - ref| <= r |ref| + 2e-6 s,  r = 2^-8 (bf16: the rounding of the result -- half an ulp is
2^-8 of the value at the bottom of a binade) or 2^-21 (fp32: a handful of roundings), s = 1 / (1 - p) forward, |dy| / (1 - p) backward; 2e-6 is the absolute error test_gelu_matches_erf_gelu pins for the polynomial.
Measured on an MI355X, as the largest fraction of its bound that any element used: see the docstrings of the tests.
Inputs keep |x|, |dy| >= 0.1, so an output is zero exactly where the element was dropped."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _mask_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SEED = (7 << 32) | 9  # both key words in use
SENTINEL = 7.0
R_TOL = {BF: 2.0 ** -8, F32: 2.0 ** -21}
VEC = {BF: 8, F32: 4}
CAP = 4096 * 256  # vectors (or bytes, for the byte gather) one pass of a capped grid covers
LN100_F32 = float(np.float32(math.log(100.0)))  # the clamp as the kernels hold it

USED = {}  # what -> largest err / bound seen


@pytest.fixture(scope="module", autouse=True)
def _report_measured_bounds():
    """The largest fraction of each value bound that this module's tests used goes into the session summary."""
    yield
    from conftest import NOTES
    for key in sorted(USED):
        NOTES.append(f"stream kernels, {key}: worst element at {USED[key]:.3f} of |got - ref| <= r |ref| + 2e-6 s")


def _L():
    from heal_swin_amd import _lib
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(status, what):
    _L().check(status, what)


def _no_epoch():
    _L().lib.hs_set_seed_epoch(None)


_HOST_KEEP = {}


def host_keep(n, p, seed=SEED, epoch=0):
    """The host reference's keep mask of elements 0 ... n - 1 as a bool tensor on the device (computed once per (p, seed, epoch) at the
    largest n asked for; shared and never written)."""
    if p == 0.0:
        return torch.ones(n, dtype=torch.bool, device=DEV)
    key = (p, seed, epoch)
    m = _HOST_KEEP.get(key)
    if m is None or m.numel() < n:
        m = torch.from_numpy(MR.keep(np.arange(n, dtype=np.uint64), p, seed, epoch)).to(DEV)
        _HOST_KEEP[key] = m
    return m[:n]


def away_from_zero(n, gen_seed, dtype, lo=0.1, hi=4.0):
    """+-[lo, hi) uniformly, rounded to dtype."""
    g = torch.Generator(device=DEV).manual_seed(gen_seed)
    mag = lo + (hi - lo) * torch.rand(n, generator=g, device=DEV)
    sign = torch.where(torch.rand(n, generator=g, device=DEV) < 0.5, -1.0, 1.0)
    return (sign * mag).to(dtype)


def padded(n, dtype, extra=32):
    """(buffer, its first n elements): the buffer is filled with SENTINEL, `extra` elements behind the view catch a store past n."""
    buf = torch.full((n + extra,), SENTINEL, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[:n]


def slack_intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def check_bound(got, ref, r, s, what, key):
    """|got - ref| <= r |ref| + 2e-6 s on every element (float64, on the device); records the largest fraction of the bound used."""
    err = (got.double() - ref).abs()
    bound = r * ref.abs() + 2e-6 * s
    used = float((err / bound).max())
    USED[key] = max(USED.get(key, 0.0), used)
    print(f"{what}: worst element uses {used:.3f} of its bound")
    assert used <= 1.0, f"{what}: an element is at {used:.3f} of its bound (r = {r}, 2e-6 s)"


# ----------------------------------------------------------------------------- hs_gelu_fwd / hs_gelu_bwd
GELU_SIZES = {
    (BF, "tails"): [8 * 33 + r for r in range(8)] + [1, 5, 7],
    (F32, "tails"): [4 * 33 + r for r in range(4)] + [1, 3],
    (BF, "capped"): [8_388_608 + 8_000 + 5],
    (F32, "capped"): [4_194_304 + 4_000 + 3],
}


def _gelu_pair(n, p, dtype, seed=SEED):
    L = _L()
    x, dy = away_from_zero(n, 11 + n, dtype), away_from_zero(n, 13 + n, dtype, hi=2.0)
    ybuf, y = padded(n, dtype)
    dxbuf, dx = padded(n, dtype)
    dt = L.dtype_code(dtype)
    _ok(L.lib.hs_gelu_fwd(L.ptr(x), L.ptr(y), n, p, seed, dt, _stream()), "hs_gelu_fwd")
    _ok(L.lib.hs_gelu_bwd(L.ptr(dy), L.ptr(x), L.ptr(dx), n, p, seed, dt, _stream()), "hs_gelu_bwd")
    torch.cuda.synchronize()
    assert slack_intact(ybuf, n) and slack_intact(dxbuf, n), f"n = {n}: a store past the end"
    return x, dy, y, dx


@pytest.mark.parametrize("which", ["tails", "capped"])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_gelu_fwd_bwd_mask_and_values(dtype, p, which):
    """Vector loop, second pass of the capped grid and the scalar tail, forward and backward, against float64 erf GELU x the host mask
    x fp32(1 / (1 - p)).  The zero pattern equals the host mask exactly, in the backward too (it regenerates the forward's mask).
    Measured (MI355X), largest fraction of the bound used: bf16 0.993 forward / 0.995 backward (round-to-nearest alone reaches 2^-8 of the
    value at the bottom of a binade); fp32 0.350 forward / 0.372 backward."""
    _no_epoch()
    scale = MR.keep_scale(p) if p > 0 else 1.0
    for n in GELU_SIZES[(dtype, which)]:
        x, dy, y, dx = _gelu_pair(n, p, dtype)
        keep = host_keep(n, p)
        assert torch.equal(y != 0, keep), f"n = {n}: forward zero pattern is not the host mask"
        assert torch.equal(dx != 0, keep), f"n = {n}: backward zero pattern is not the host mask"
        x64, dy64, m = x.double(), dy.double(), keep.double() * scale
        name = "bf16" if dtype == BF else "fp32"
        check_bound(y, gelu64(x64) * m, R_TOL[dtype], 1.0 / (1.0 - p), f"gelu fwd {name} p={p} n={n}", f"gelu fwd {name}")
        check_bound(dx, dy64 * dgelu64(x64) * m, R_TOL[dtype], dy64.abs() / (1.0 - p), f"gelu bwd {name} p={p} n={n}", f"gelu bwd {name}")


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_gelu_drop_everything_gives_exact_zeros(dtype):
    _no_epoch()
    for n in (VEC[dtype] * 33 + VEC[dtype] - 1, 3):
        _, _, y, dx = _gelu_pair(n, 1.0, dtype)
        assert bool((y == 0).all()) and bool((dx == 0).all())


@pytest.mark.parametrize("rows,width", [(37, 24), (1000, 264), (5, 3)])
def test_mask_helper_is_the_host_reference(rows, width):
    """`_util.mask_of` -- what the LayerNorm, GEMM-epilogue, fused-MLP and split3 mask tests compare against -- anchored to the rule."""
    from _util import mask_of
    _no_epoch()
    for p, seed in ((0.25, SEED), (0.1, 42), (0.5, 0)):
        got = mask_of(seed, p, (rows, width))
        ref = host_keep(rows * width, p, seed).view(rows, width).double() / (1.0 - p)
        assert torch.equal(got, ref), (p, seed)


def test_registered_epoch_counter_enters_as_the_seed_offset():
    """hs_set_seed_epoch with a counter of 3: GELU, residual_drop and gelu_split3 (one translation unit, one pointer) draw keep(..., epoch=3)."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    p, n, rows, k = 0.25, 8 * 33 + 5, 11, 12
    counter = torch.tensor([3], dtype=torch.int64, device=DEV)
    _no_epoch()
    x = away_from_zero(n, 5, BF)
    xs = away_from_zero(rows * k, 6, F32).view(rows, k)
    y, out, o3 = torch.empty_like(x), torch.empty(264, dtype=BF, device=DEV), torch.empty(rows, 3 * k, dtype=BF, device=DEV)
    _ok(lib.hs_set_seed_epoch(ptr(counter)), "hs_set_seed_epoch")
    try:
        _ok(lib.hs_gelu_fwd(ptr(x), ptr(y), n, p, SEED, L.HS_BF16, _stream()), "hs_gelu_fwd")
        _ok(lib.hs_residual_drop(None, ptr(x), ptr(out), None, 264, 264, p, SEED, L.HS_BF16, _stream()), "hs_residual_drop")
        _ok(lib.hs_gelu_split3(None, ptr(xs), ptr(o3), rows, k, p, SEED, _stream()), "hs_gelu_split3")
        torch.cuda.synchronize()
    finally:
        _no_epoch()
    keep3 = host_keep(n, p, SEED, epoch=3)
    assert not torch.equal(keep3, host_keep(n, p, SEED))
    assert torch.equal(y != 0, keep3)
    assert torch.equal(out != 0, keep3[:264])
    assert torch.equal(o3[:, :k] != 0, keep3[:rows * k].view(rows, k))
    _ok(lib.hs_gelu_fwd(ptr(x), ptr(y), n, p, SEED, L.HS_BF16, _stream()), "hs_gelu_fwd")
    assert torch.equal(y != 0, host_keep(n, p, SEED)), "clearing the counter restores the plain seed"


# ----------------------------------------------------------------------------- hs_residual_drop
ROW_SCALE = [1.25, 0.0, 0.5, 2.0, 1.0]
RESID_EPS = {(BF, "small"): 264, (F32, "small"): 132, (BF, "capped"): 1_680_000, (F32, "capped"): 840_000}


@pytest.mark.parametrize("which", ["small", "capped"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_residual_drop_per_sample_scale_and_mask(dtype, which):
    """out = x + rs * mask * t / (1 - p) over 5 samples with their own row_scale; the capped shapes put the end of the last sample in the
    second pass of the grid.  x == NULL shows the mask itself (zero where dropped or rs = 0); with x a flipped mask is an error of at
    least 0.5 * 0.5 * 4 / 3 = 0.33 against a bound below 0.03.  Measured (MI355X), largest fraction of the bound used: bf16 0.996, fp32 0.107."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    _no_epoch()
    eps = RESID_EPS[(dtype, which)]
    n = 5 * eps
    assert eps % VEC[dtype] == 0 and (which == "small" or n // VEC[dtype] > CAP)
    dt = L.dtype_code(dtype)
    x, t = away_from_zero(n, 21, dtype, hi=2.0), away_from_zero(n, 22, dtype, lo=0.5, hi=2.0)
    rs = torch.tensor(ROW_SCALE, device=DEV)
    rs_elem = rs.double().repeat_interleave(eps)
    name = "bf16" if dtype == BF else "fp32"
    for p, with_x, with_rs in ((0.25, False, True), (0.25, True, True), (0.25, True, False), (0.25, False, False), (0.0, True, True)):
        keep = host_keep(n, p)
        buf, out = padded(n, dtype)
        _ok(lib.hs_residual_drop(ptr(x) if with_x else None, ptr(t), ptr(out), ptr(rs) if with_rs else None, eps if with_rs else n, n, p, SEED,
                                 dt, _stream()), "hs_residual_drop")
        torch.cuda.synchronize()
        assert slack_intact(buf, n)
        scale = MR.keep_scale(p) if p > 0 else 1.0
        r64 = rs_elem if with_rs else torch.ones((), dtype=torch.float64, device=DEV)
        branch = r64 * keep.double() * scale * t.double()
        if not with_x:
            assert torch.equal(out != 0, keep & (r64 != 0)), f"p={p} rs={with_rs}: zero pattern is not the host mask"
        check_bound(out, (x.double() if with_x else 0.0) + branch, R_TOL[dtype], 1.0 / (1.0 - p),
                    f"residual_drop {name} {which} p={p} x={with_x} rs={with_rs}", f"residual_drop {name}")


# ----------------------------------------------------------------------------- hs_split_bf16x3
SPLIT_SHAPES = [(1, 4), (777, 264), (3, 12), (4099, 1028)]


def _wide_range(rows, k, gen_seed):
    """randn * 2^e, e uniform in [-60, 60), with +-0 in the first elements: no infinity, NaN or subnormal (their lo is not defined)."""
    g = torch.Generator(device=DEV).manual_seed(gen_seed)
    e = torch.randint(-60, 60, (rows, k), generator=g, device=DEV)
    x = torch.randn(rows, k, generator=g, device=DEV) * torch.exp2(e.float())
    x.view(-1)[0], x.view(-1)[1] = 0.0, -0.0
    assert bool(torch.isfinite(x).all()) and float(x[x != 0].abs().min()) > 2.0 ** -100
    return x


@pytest.mark.parametrize("rows,k", SPLIT_SHAPES)
@pytest.mark.parametrize("mode", [0, 1])
def test_split_bf16x3_bits(mode, rows, k):
    """[hi | hi | lo] (mode 0) and [hi | lo | hi] (mode 1) bit for bit against torch: hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in
    fp32), and |x - hi - lo| <= 2^-17 |x| as the header states; (4099, 1028) is past the capped grid."""
    L = _L()
    assert rows * (k // 4) > CAP or (rows, k) != SPLIT_SHAPES[-1]
    x = _wide_range(rows, k, rows + k)
    buf, flat = padded(rows * 3 * k, BF)
    out = flat.view(rows, 3 * k)
    _ok(L.lib.hs_split_bf16x3(L.ptr(x), L.ptr(out), rows, k, mode, _stream()), "hs_split_bf16x3")
    torch.cuda.synchronize()
    assert slack_intact(buf, rows * 3 * k)
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    ref = torch.cat([hi, hi, lo] if mode == 0 else [hi, lo, hi], dim=1)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    got_hi, got_lo = out[:, :k].double(), out[:, (2 * k if mode == 0 else k):(3 * k if mode == 0 else 2 * k)].double()
    assert bool(((x.double() - got_hi - got_lo).abs() <= 2.0 ** -17 * x.double().abs()).all())


# ----------------------------------------------------------------------------- hs_gelu_split3
@pytest.mark.parametrize("rows,k", [(777, 12), (4099, 1028)])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_gelu_split3_mask_and_values(bwd, p, rows, k):
    """GELU (or dy GELU') x mask written as [hi | hi | lo]: mask exact against the host reference at element row * k + col (k = 12: rows
    start alternately in the first and the second half of a chunk; (4099, 1028): past the capped grid), both hi blocks the same bits,
    |hi + lo - ref| <= 2^-16 |ref| + 2e-6 s.  Measured (MI355X), largest fraction of the bound used: 0.489 forward, 0.474 backward."""
    L = _L()
    _no_epoch()
    n = rows * k
    x = away_from_zero(n, 31, F32).view(rows, k)
    dy = away_from_zero(n, 32, F32, hi=2.0).view(rows, k)
    buf, flat = padded(3 * n, BF)
    out = flat.view(rows, 3 * k)
    _ok(L.lib.hs_gelu_split3(L.ptr(dy) if bwd else None, L.ptr(x), L.ptr(out), rows, k, p, SEED, _stream()), "hs_gelu_split3")
    torch.cuda.synchronize()
    assert slack_intact(buf, 3 * n)
    keep = host_keep(n, p).view(rows, k)
    hi, hi2, lo = out[:, :k], out[:, k:2 * k], out[:, 2 * k:]
    assert torch.equal(hi != 0, keep), "zero pattern is not the host mask"
    assert torch.equal(hi.view(torch.int16), hi2.view(torch.int16))
    m = keep.double() * (MR.keep_scale(p) if p > 0 else 1.0)
    x64, dy64 = x.double(), dy.double()
    ref = dy64 * dgelu64(x64) * m if bwd else gelu64(x64) * m
    s = dy64.abs() / (1.0 - p) if bwd else 1.0 / (1.0 - p)
    what = f"gelu_split3 {'bwd' if bwd else 'fwd'}"
    check_bound(hi.double() + lo.double(), ref, 2.0 ** -16, s, f"{what} p={p} ({rows}, {k})", what)


# ----------------------------------------------------------------------------- hs_gather_rows
def _bytes(b, n, row_bytes, gen_seed):
    g = torch.Generator(device=DEV).manual_seed(gen_seed)
    return torch.randint(0, 256, (b, n, row_bytes), generator=g, device=DEV, dtype=torch.uint8)


def _perm(n, gen_seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(gen_seed)).to(torch.int32).to(DEV)


def at_offset(t, e):
    """t inside a larger allocation, e elements behind a 256-byte-aligned base, with slack on both sides."""
    per = 256 // t.element_size()
    buf = torch.zeros(2 * per + t.numel() + 64, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 256 == 0
    v = buf[per + e:per + e + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (e * t.element_size()) % 16
    return v


def _gather(x, idx, roll, out=None):
    """hs_gather_rows into a sentinel-padded buffer (or `out`); returns the [B, N, row_bytes] result."""
    L = _L()
    b, n, rb = x.shape
    if out is None:
        buf, flat = padded(x.numel(), torch.uint8)
        out = flat.view(x.shape)
    else:
        buf = None
    _ok(L.lib.hs_gather_rows(L.ptr(x), L.ptr(out), L.ptr(idx), roll, b, n, rb, _stream()), "hs_gather_rows")
    torch.cuda.synchronize()
    assert buf is None or slack_intact(buf, x.numel())
    return out


def _gather_ref(x, idx, roll):
    return x[:, idx.long()] if idx is not None else torch.roll(x, -roll, dims=1)


@pytest.mark.parametrize("row_bytes", [16, 48, 96])
def test_gather_rows_vector_kernel_tables_and_rolls(row_bytes):
    b, n = 3, 1001
    x = _bytes(b, n, row_bytes, row_bytes)
    assert x.data_ptr() % 16 == 0
    idx = _perm(n, 1)
    assert torch.equal(_gather(x, idx, 0), _gather_ref(x, idx, 0))
    for roll in (0, 1, n - 1):
        assert torch.equal(_gather(x, None, roll), _gather_ref(x, None, roll)), f"roll {roll}"


@pytest.mark.parametrize("b,n,row_bytes", [(3, 350_003, 16), (2, 100_003, 6)], ids=["vector", "bytes"])
def test_gather_rows_past_the_capped_grid(b, n, row_bytes):
    assert b * n * (row_bytes // 16 if row_bytes % 16 == 0 else row_bytes) > CAP
    x = _bytes(b, n, row_bytes, n)
    idx = _perm(n, 2)
    assert torch.equal(_gather(x, idx, 0), _gather_ref(x, idx, 0))
    assert torch.equal(_gather(x, None, n - 1), _gather_ref(x, None, n - 1))


def test_gather_rows_falls_back_from_the_pointer():
    """row_bytes % 16 == 0 but x (then out) 4 bytes behind an aligned base: the byte kernel moves the same bits."""
    b, n, rb = 3, 1001, 32
    x = _bytes(b, n, rb, 7)
    idx = _perm(n, 3)
    for roll, table in ((0, idx), (n - 1, None)):
        ref = _gather_ref(x, table, roll)
        assert torch.equal(_gather(at_offset(x, 4), table, roll), ref)
        out = at_offset(torch.full_like(x, 7), 4)
        assert torch.equal(_gather(x, table, roll, out=out), ref)


def test_nest_roll_shift_reaches_the_vector_kernel():
    """NestRollShift on 8 fp32 channels (32-byte rows): shift = the oracle's index table, shift_back restores the input."""
    from heal_swin_amd.models_torch import hp_shifting as S
    from oracle import tables as T
    n, ws = 8 * 16 * 16, 16
    x = torch.randn(2, n, 8, device=DEV)
    assert x.data_ptr() % 16 == 0
    for shift in (8, 1, 15):  # (shift_back rolls by n - shift)
        sh = S.NestRollShift(shift, n, ws)
        idx = torch.from_numpy(np.asarray(T.nest_roll_shift(n, ws, shift)[0])).long().to(DEV)
        xs = sh.shift(x)
        assert torch.equal(xs, x[:, idx])
        assert torch.equal(sh.shift_back(xs), x)


# ----------------------------------------------------------------------------- rel_bias.hip
def parr(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def iarr(v):
    return (ctypes.c_int * len(v))(*v)


def _rel_index(ws, rows_used, table_rows, one_row, gen_seed=0):
    """A hand-made rel_idx [ws^2] into `table_rows` rows of which at most the first `rows_used` occur, its stable argsort and run offsets."""
    g = torch.Generator().manual_seed(gen_seed + ws)
    rel = torch.full((ws * ws,), 3, dtype=torch.int64) if one_row else torch.randint(0, rows_used, (ws * ws,), generator=g)
    rel = rel.to(DEV)
    order = torch.argsort(rel, stable=True).to(torch.int32)
    counts = torch.bincount(rel, minlength=table_rows)
    offs = torch.cat([torch.zeros(1, dtype=torch.long, device=DEV), counts.cumsum(0)]).to(torch.int32)
    assert bool((counts == 0).any())
    return rel.to(torch.int32), order, offs, counts


def _ints(shape, gen_seed):
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(gen_seed)).float().to(DEV)


def _scatter_ref(dbias, rel, table_rows):
    nh = dbias.shape[0]
    return torch.zeros(table_rows, nh, dtype=torch.float64, device=DEV).index_add_(0, rel.long(), dbias.double().reshape(nh, -1).t())


@pytest.mark.parametrize("one_row", [False, True], ids=["random", "one_row"])
@pytest.mark.parametrize("ws", [5, 16, 64])
def test_rel_bias_scatter_kernels_exact_with_empty_and_long_runs(ws, one_row):
    """Integer-valued dbias in [-8, 8]: every sum is exact, so the scan kernel (64 and 256 threads), the sorted kernel and the sorted-add
    kernel equal a float64 index_add bit for bit -- with table rows that no entry names (0 after an overwrite, unchanged after an add)
    and, for `one_row`, one run of ws^2 entries (4096 at ws = 64: longer than the 16 lanes x 4 of an unrolled round)."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    nh, rows_used = 3, min(ws * ws, 40)
    table_rows = rows_used + 7
    rel, order, offs, counts = _rel_index(ws, rows_used, table_rows, one_row)
    dbias = _ints((nh, ws, ws), ws)
    ref = _scatter_ref(dbias, rel, table_rows)
    empty = counts == 0
    old = _ints((table_rows, nh), 99) + 100.0
    scan, srt, add = torch.full_like(old, SENTINEL), torch.full_like(old, SENTINEL), old.clone()
    _ok(lib.hs_rel_bias_scatter_grad(ptr(dbias), ptr(rel), ptr(scan), table_rows, nh, ws, _stream()), "scatter")
    _ok(lib.hs_rel_bias_scatter_grad_sorted(ptr(dbias), ptr(order), ptr(offs), ptr(srt), table_rows, nh, ws, _stream()), "scatter_sorted")
    _ok(lib.hs_rel_bias_scatter_grad_sorted_add(ptr(dbias), ptr(order), ptr(offs), ptr(add), table_rows, nh, ws, _stream()), "scatter_sorted_add")
    assert torch.equal(scan.double(), ref) and torch.equal(srt.double(), ref)
    assert torch.equal(add.double(), ref + old.double())
    assert bool((scan[empty] == 0).all()) and bool((srt[empty] == 0).all()) and torch.equal(add[empty], old[empty])


HEAD_CYCLE = [1, 3, 6, 12, 24, 2]


@pytest.mark.parametrize("count", [49, 97])
def test_batched_rel_bias_and_head_scale_past_one_chunk(count):
    """More jobs than one launch holds (48): gather (first_head runs on across chunks), scatter (mixed accumulate flags) and head scale equal
    the per-job entry points bit for bit; gather equals table[rel_idx][:, h], scatter the float64 index_add, bit for bit."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    ws, table_rows = 16, 47
    ws2 = ws * ws
    rel, order, offs, _ = _rel_index(ws, 40, table_rows, False, gen_seed=count)
    heads = [HEAD_CYCLE[j % len(HEAD_CYCLE)] for j in range(count)]
    acc = [1 if (j % 3 == 1 or j == 48) else 0 for j in range(count)]  # (differs from job 0 in both chunks)
    assert acc[0] == 0 and acc[1] == 1 and acc[48] == 1
    g = torch.Generator().manual_seed(count)
    # gather
    tables = [torch.randn(table_rows, h, generator=g).to(DEV) for h in heads]
    total = sum(heads)
    bias = torch.full((total + 1, ws2), SENTINEL, device=DEV)
    _ok(lib.hs_rel_bias_gather_many(parr(tables), iarr(heads), count, ptr(rel), ptr(bias), table_rows, ws, _stream()), "gather_many")
    assert bool((bias[total] == SENTINEL).all())
    first = 0
    for j, (t, h) in enumerate(zip(tables, heads)):
        one = torch.full((h, ws2), SENTINEL, device=DEV)
        _ok(lib.hs_rel_bias_gather(ptr(t), ptr(rel), ptr(one), table_rows, h, ws, _stream()), "gather")
        assert torch.equal(one, t[rel.long()].t()), j
        assert torch.equal(bias[first:first + h], one), j
        first += h
    # scatter
    dbias = [_ints((h, ws2), 1000 + j) for j, h in enumerate(heads)]
    old = [_ints((table_rows, h), 2000 + j) + 50.0 for j, h in enumerate(heads)]
    many = [o.clone() for o in old]
    _ok(lib.hs_rel_bias_scatter_grad_sorted_many(parr(dbias), parr(many), iarr(heads), iarr(acc), count, ptr(order), ptr(offs), table_rows, ws,
                                                 _stream()), "scatter_many")
    for j, h in enumerate(heads):
        one = old[j].clone()
        fn = lib.hs_rel_bias_scatter_grad_sorted_add if acc[j] else lib.hs_rel_bias_scatter_grad_sorted
        _ok(fn(ptr(dbias[j]), ptr(order), ptr(offs), ptr(one), table_rows, h, ws, _stream()), "scatter")
        ref = _scatter_ref(dbias[j], rel, table_rows) + (old[j].double() if acc[j] else 0.0)
        assert torch.equal(one.double(), ref), j
        assert torch.equal(many[j], one), j
    # head scale, forward then backward
    ls = [(torch.randn(h, generator=g) * 2 + 3).to(DEV) for h in heads]  # some beyond ln 100
    ds = [torch.randn(h, generator=g).to(DEV) for h in heads]
    scale = [torch.full((h,), SENTINEL, device=DEV) for h in heads]
    dls = [torch.full((h,), SENTINEL, device=DEV) for h in heads]
    _ok(lib.hs_cos_head_scale_many(parr(ls), None, parr(scale), iarr(heads), None, count, _stream()), "scale_many")
    _ok(lib.hs_cos_head_scale_many(parr(ls), parr(ds), parr(dls), iarr(heads), iarr(acc), count, _stream()), "scale_many bwd")
    for j, h in enumerate(heads):
        s1, d1 = torch.full((h,), SENTINEL, device=DEV), torch.full((h,), SENTINEL, device=DEV)
        _ok(lib.hs_cos_head_scale_fwd(ptr(ls[j]), ptr(s1), h, _stream()), "scale_fwd")
        _ok(lib.hs_cos_head_scale_bwd(ptr(ls[j]), ptr(ds[j]), ptr(d1), h, acc[j], _stream()), "scale_bwd")
        assert torch.equal(scale[j], s1) and torch.equal(dls[j], d1), j
    _check_head_scale(torch.cat(ls), torch.cat(ds), torch.cat(scale), torch.cat([d - a * SENTINEL for d, a in zip(dls, acc)]), f"many {count}")


def _check_head_scale(ls, ds, scale, dls, what):
    """exp(min(l, ln 100)) and d * scale * [l <= ln 100] in float64, at 1e-6 of the tensor's scale (the bound of
    test_cos_head_scale_matches_the_torch_formula); beyond the clamp the gradient is exactly 0."""
    from _util import assert_close
    l64 = ls.double()
    ref = torch.exp(torch.clamp(l64, max=math.log(100.0)))
    on = l64 <= LN100_F32
    assert_close(scale, ref, 1e-6, f"cos_head_scale {what}")
    assert_close(dls, torch.where(on, ds.double() * ref, torch.zeros_like(ref)), 1e-6, f"cos_head_scale bwd {what}")
    assert bool((dls[~on] == 0).all())


@pytest.mark.parametrize("heads", [65, 130])
def test_cos_head_scale_more_heads_than_one_workgroup(heads):
    L = _L()
    lib, ptr = L.lib, L.ptr
    g = torch.Generator().manual_seed(heads)
    ls = torch.randn(heads, generator=g) * 2 + 3
    ls[0], ls[63], ls[1], ls[heads - 1] = LN100_F32, LN100_F32, 5.0, 5.0  # on the clamp; beyond it, in the first and the last workgroup
    ls, ds = ls.to(DEV), torch.randn(heads, generator=g).to(DEV)
    bscale, scale = padded(heads, F32)
    bd, dls = padded(heads, F32)
    _ok(lib.hs_cos_head_scale_fwd(ptr(ls), ptr(scale), heads, _stream()), "scale_fwd")
    _ok(lib.hs_cos_head_scale_bwd(ptr(ls), ptr(ds), ptr(dls), heads, 0, _stream()), "scale_bwd")
    acc = torch.full((heads,), 2.0, device=DEV)
    _ok(lib.hs_cos_head_scale_bwd(ptr(ls), ptr(ds), ptr(acc), heads, 1, _stream()), "scale_bwd add")
    torch.cuda.synchronize()
    assert slack_intact(bscale, heads) and slack_intact(bd, heads)
    _check_head_scale(ls, ds, scale, dls, f"{heads} heads")
    assert float(dls[1]) == 0.0 and float(dls[heads - 1]) == 0.0 and float(dls[0]) != 0.0 and float(dls[63]) != 0.0
    assert torch.equal(acc, dls + 2.0)


def test_cos_head_scale_many_with_a_full_workgroup_job():
    """The batched form gives a job one 64-lane workgroup: a job of exactly 64 heads (the entry point's limit) between two small ones."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    heads = [3, 64, 2]
    g = torch.Generator().manual_seed(64)
    ls = [(torch.randn(h, generator=g) * 2 + 3) for h in heads]
    ls[1][0], ls[1][63], ls[1][1] = LN100_F32, LN100_F32, 5.0
    ls = [t.to(DEV) for t in ls]
    ds = [torch.randn(h, generator=g).to(DEV) for h in heads]
    bufs = [padded(h, F32) for h in heads]
    dbufs = [padded(h, F32) for h in heads]
    _ok(lib.hs_cos_head_scale_many(parr(ls), None, parr([v for _, v in bufs]), iarr(heads), None, 3, _stream()), "scale_many")
    _ok(lib.hs_cos_head_scale_many(parr(ls), parr(ds), parr([v for _, v in dbufs]), iarr(heads), iarr([0, 0, 0]), 3, _stream()), "scale_many bwd")
    torch.cuda.synchronize()
    for (b, _), (db, _), h in zip(bufs, dbufs, heads):
        assert slack_intact(b, h) and slack_intact(db, h)
    _check_head_scale(torch.cat(ls), torch.cat(ds), torch.cat([v for _, v in bufs]), torch.cat([v for _, v in dbufs]), "job of 64 heads")
    assert float(dbufs[1][1][1]) == 0.0


@pytest.mark.parametrize("entry", ["gather_null_table", "gather_no_heads", "scatter_null_dbias", "scale_65_heads", "scale_null_out"])
def test_batched_forms_refuse_a_bad_job_before_any_launch(entry):
    """60 jobs, job 50 (second chunk of 48) bad: HS_ERR_INVALID_ARG, and the outputs of jobs 0 ... 47 -- the chunk that used to be
    launched before the bad job was looked at -- still hold their sentinel."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    count, bad, ws, table_rows = 60, 50, 5, 20
    ws2 = ws * ws
    rel, order, offs, _ = _rel_index(ws, 12, table_rows, False)
    heads = [HEAD_CYCLE[j % len(HEAD_CYCLE)] for j in range(count)]
    if entry.startswith("gather"):
        tables = [torch.randn(table_rows, h, device=DEV) for h in heads]
        if entry == "gather_null_table":
            tables[bad] = None
        else:
            heads[bad] = 0
        outs = [torch.full((sum(heads), ws2), SENTINEL, device=DEV)]
        status = lib.hs_rel_bias_gather_many(parr(tables), iarr(heads), count, ptr(rel), ptr(outs[0]), table_rows, ws, _stream())
    elif entry.startswith("scatter"):
        dbias = [_ints((h, ws2), j) for j, h in enumerate(heads)]
        dbias[bad] = None
        outs = [torch.full((table_rows, h), SENTINEL, device=DEV) for h in heads]
        status = lib.hs_rel_bias_scatter_grad_sorted_many(parr(dbias), parr(outs), iarr(heads), iarr([j % 2 for j in range(count)]), count, ptr(order),
                                                          ptr(offs), table_rows, ws, _stream())
    else:
        if entry == "scale_65_heads":
            heads[bad] = 65
        ls = [torch.zeros(h, device=DEV) for h in heads]
        outs = [torch.full((h,), SENTINEL, device=DEV) for h in heads]
        args = list(outs)
        if entry == "scale_null_out":
            args[bad] = None
        status = lib.hs_cos_head_scale_many(parr(ls), None, parr(args), iarr(heads), None, count, _stream())
    torch.cuda.synchronize()
    assert status == 1, (status, lib.hs_last_error().decode())  # HS_ERR_INVALID_ARG
    assert f"job {bad}" in lib.hs_last_error().decode()
    with pytest.raises(AssertionError):
        L.check(status, entry)
    for o in outs:
        assert bool((o == SENTINEL).all()), "a chunk was launched before the bad job was refused"
