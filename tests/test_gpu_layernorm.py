"""The LayerNorm kernels (csrc/layernorm.hip) at operator level: the persistent row loops, every lane shape, every dispatch path.

Every reference is the plain formula in torch float64 on inputs rounded to the kernel's dtype (`x.to(dtype).double()`, fp32 gamma /
beta, eps 1e-5, autograd for the gradients), evaluated on the device; outputs are held to TOL[dtype], gradients to GRAD_TOL[dtype]
on max|a - b| / max|b|, the saved row statistics to 1e-5 of their scale.

Dispatch of ln_fwd_impl / ln_bwd_impl (`fwd_path` / `bwd_path`, whose enumerators are the rows' names).  `vector`: width % 8 == 0
(bf16) / width % 4 == 0 (fp32); `extras`: row_scale or drop_p; `lo`: the compensated stream operands.  Every parametrised case
below carries in its id the (lanes per row, chunks per lane) shape that `with_shape` picks and the row of this table it is meant
to reach.

  # forward
  #   fwd-fast-plain   layernorm_fwd_fast_kernel<EX = false>   vector, no extras, no lo                (plain, residual, add, passthrough)
  #   fwd-fast-EX      layernorm_fwd_fast_kernel<EX = true>    bf16 vector, extras, no add operand, no lo        (v2 forms with extras)
  #   fwd-general-vec  layernorm_fwd_kernel<VEC = 8 / 4>       vector and: add + extras, or lo, or fp32 + extras
  #   fwd-general-elem layernorm_fwd_kernel<VEC = 1>           every other width up to 1024
  # backward
  #   bwd-fast-bf16    layernorm_bwd_fast_kernel<bf16_t>       bf16 vector, no extras (with or without the second gradient)
  #   bwd-fast-fp32    layernorm_bwd_fast_kernel<float>        fp32 vector, no extras
  #   bwd-fast-EX      layernorm_bwd_fast_kernel<EX = true>    bf16 vector, extras, v2 form
  #   bwd-general-v1   layernorm_bwd_kernel, v1_mode = 1       add form with extras (dadd_out), element-wise add / passthrough form
  #   bwd-general      layernorm_bwd_kernel, v1_mode = 0       fp32 v2 form with extras, element-wise plain / residual form
  # parameter reduce (dgamma / dbeta from the per-workgroup partial rows)
  #   reduce-now       reduce_now (csrc/reduce_many.hip)       width % 4 == 0
  #   reduce-deferred  reduce_defer + hs_reduce_flush          width % 4 == 0 with HS_ACC_DEFER
  #   reduce-kernel    layernorm_param_reduce_kernel           width % 4 != 0

Families:  A  more rows than two resident rounds (the prefetch hand-over, the ragged last round, dgamma / dbeta across rounds),
with row slices run alone reproducing the large run bit for bit;  B  every lane shape, small and ragged, and the width limits;
C  the element-wise parameter reduce over 130 partial rows;  D  dropout / DropPath forms against float64 with the generator's own
mask;  E  `sample_of` exactly, at sample boundaries and across 2^24 rows.

Out of scope: the `rows * width * bytes >= 2^32` fallback from the fast to the general kernels needs 4 GiB operands and is left to
the full-size tests."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from _util import GRAD_TOL, TOL, assert_close, mask_of, reserved_cus, worst

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NAME = {BF16: "bf16", F32: "fp32"}
VEC = {BF16: 8, F32: 4}
HS_ERR_UNSUPPORTED = 2
RS6 = [0.0, 2.0, 0.5, 2.0, 0.5, 1.25]  # DropPath factors of six samples: a row that reads its neighbour's is off by a factor of four
P_DROP, SEED = 0.2, 0x51F15EED0BADC0DE  # 1 / (1 - p) = 1.25 is exact in bf16


def _L():
    from heal_swin_amd import _lib
    return _lib


def _ops():
    from heal_swin_amd import ops
    return ops


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module", autouse=True)
def _family_report():
    yield
    import conftest
    for fam in "ABCD":
        s, r, e = worst(f"ln/{fam} ")
        conftest.NOTES.append(f"LayerNorm kernels, family {fam}: worst max|a-b|/max|b| {s:.2e} (rms {r:.2e}, elem99.9 {e:.2e}) against float64")
    if STREAM_SLACK:
        conftest.NOTES.append(f"LayerNorm kernels, family D, compensated stream: hi + lo within {worst('ln/stream-sum ')[0]:.2e} of the float64 sum's scale "
                              f"(bound 2^-16 = {2.0 ** -16:.2e}); {sum(n for n, _ in STREAM_SLACK)} of {sum(m for _, m in STREAM_SLACK)} elements of hi "
                              "are a neighbour of the bf16 rounding of the float64 sum (fp32 evaluation near a rounding tie)")
    conftest.NOTES.append(f"LayerNorm kernels, family E: {E_ROWS[0]} rows in {E_ROWS[1]} launches compared exactly with row_scale[row // rows_per_sample]: "
                          f"{E_ROWS[2]} rows differ")


# ----------------------------------------------------------------------------- the dispatch, mirrored for planning and for the ids
def lane_shape(dtype, width):
    """(vector width, lanes per row, chunks per lane) of `with_shape`."""
    vec = VEC[dtype] if width % VEC[dtype] == 0 else 1
    chunks = width // vec
    for cap, shape in ((2, (2, 1)), (4, (4, 1)), (8, (8, 1)), (16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (128, (64, 2)), (256, (64, 4)),
                       (512, (64, 8)), (1024, (64, 16))):
        if chunks <= cap:
            assert shape != (64, 16) or vec == 1
            return (vec,) + shape
    raise AssertionError(f"width {width} is outside what with_shape places")


def route(dtype, width, form, extras=False, lo=False, deferred=False):
    """The rows of the dispatch table (module docstring) that a call reaches: forward kernel, backward kernel, parameter reduce."""
    vec, lpr, iters = lane_shape(dtype, width)
    v1 = form in ("add", "passthrough")
    if vec == 1:
        fwd = "fwd-general-elem"
    elif not extras and not lo:
        fwd = "fwd-fast-plain"
    elif extras and not lo and form != "add" and dtype == BF16:
        fwd = "fwd-fast-EX"
    else:
        fwd = "fwd-general-vec"
    if vec > 1 and not extras:
        bwd = "bwd-fast-" + NAME[dtype]
    elif vec > 1 and extras and not v1 and dtype == BF16:
        bwd = "bwd-fast-EX"
    else:
        bwd = "bwd-general-v1" if v1 else "bwd-general"
    red = "reduce-kernel" if width % 4 else ("reduce-deferred" if deferred else "reduce-now")
    return f"({lpr},{iters})", fwd, bwd, red


def case_id(dtype, width, form, **kw):
    return "-".join((NAME[dtype], f"w{width}", form) + route(dtype, width, form, **kw))


# ----------------------------------------------------------------------------- inputs, the kernels, the float64 formula
def make_inputs(dtype, rows, width, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def rn(*shape):
        return torch.randn(shape, generator=g, device=DEV)
    return SimpleNamespace(
        x=(rn(rows, width) * 3 + 1.5 + rn(rows, 1)).to(dtype), r=rn(rows, width).to(dtype), dy=rn(rows, width).to(dtype),
        d2=rn(rows, width).to(dtype), gamma=1 + 0.3 * rn(width), beta=0.2 * rn(width))


def cut(t, lo, hi):
    """Rows lo .. hi - 1 as inputs of their own (views: the caller picks `lo` so that they start on a 16-byte boundary)."""
    s = SimpleNamespace(x=t.x[lo:hi], r=t.r[lo:hi], dy=t.dy[lo:hi], d2=t.d2[lo:hi], gamma=t.gamma, beta=t.beta)
    assert s.x.data_ptr() % 16 == 0 and s.x.is_contiguous()
    return s


def run_ops(form, t, row_scale=None, drop_p=0.0, seed=None):
    """The four forms through the autograd ops.  plain / residual: y = [r +] rs LN(drop(x));  add: s = x + rs drop(r), y = LN(s) with
    gradients arriving on s (d2) and y (dy);  passthrough: (LN(x), alias of x) with the alias gradient d2 fed in."""
    ops = _ops()
    x, r = t.x.clone().requires_grad_(True), t.r.clone().requires_grad_(True)
    g, b = t.gamma.clone().requires_grad_(True), t.beta.clone().requires_grad_(True)
    out = {}
    if form in ("plain", "residual"):
        out["y"] = ops.layer_norm(x, g, b, r if form == "residual" else None, row_scale=row_scale, drop_p=drop_p, seed=seed)
        out["y"].backward(t.dy)
    elif form == "add":
        out["s"], out["y"] = ops.add_layer_norm(x, r, g, b, row_scale=row_scale, drop_p=drop_p, seed=seed)
        torch.autograd.backward([out["s"], out["y"]], [t.d2, t.dy])
    else:
        assert form == "passthrough" and row_scale is None and not drop_p
        out["y"], alias = ops.layer_norm_passthrough(x, g, b)
        torch.autograd.backward([out["y"], alias], [t.dy, t.d2])
    out = {k: v.detach() for k, v in out.items()}
    out.update(dx=x.grad, dgamma=g.grad, dbeta=b.grad)
    if form in ("residual", "add"):
        out["dr"] = r.grad
    return out


def c_forward(form, t):
    """hs_layernorm_fwd / hs_add_layernorm_fwd called directly: (y, mean, rstd) -- the statistics the backward is handed."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    rows, width = t.x.shape
    y, s = torch.empty_like(t.x), torch.empty_like(t.x)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    dt = L.dtype_code(t.x.dtype)
    if form == "add":
        L.check(lib.hs_add_layernorm_fwd(ptr(t.x), ptr(t.r), ptr(t.gamma), ptr(t.beta), ptr(s), ptr(y), ptr(mean), ptr(rstd), rows, width, dt,
                                         _stream()), "hs_add_layernorm_fwd")
    else:
        L.check(lib.hs_layernorm_fwd(ptr(t.x), ptr(t.r) if form == "residual" else None, ptr(t.gamma), ptr(t.beta), ptr(y), ptr(mean),
                                     ptr(rstd), rows, width, dt, _stream()), "hs_layernorm_fwd")
    return y, mean, rstd


def ln64(x, g, b):
    mu = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    return (x - mu) * rstd * g + b, mu.detach().flatten(), rstd.detach().flatten()


def reference(form, t, M=1.0, rsv=1.0):
    """float64 autograd on the explicit formula.  M: the dropout multiplier per element (mask / (1 - p)), rsv: the DropPath factor
    per row as a column."""
    dt = t.x.dtype
    x, r = t.x.double().requires_grad_(True), t.r.double().requires_grad_(True)
    g, b = t.gamma.double().requires_grad_(True), t.beta.double().requires_grad_(True)
    dy, d2 = t.dy.double(), t.d2.double()
    out = {}
    if form == "add":
        s = x + rsv * M * r
        stored = s + (s.detach().to(dt).double() - s.detach())  # the kernel normalises the sum as it is stored
        y, mean, rstd = ln64(stored, g, b)
        out["s"] = s.detach()
        loss = (s * d2).sum() + (y * dy).sum()
    else:
        n, mean, rstd = ln64(M * x, g, b)
        y = rsv * n + (r if form == "residual" else 0.0)
        loss = (y * dy).sum() + ((x * d2).sum() if form == "passthrough" else 0.0)
    loss.backward()
    out.update(y=y.detach(), mean=mean, rstd=rstd, dx=x.grad, dgamma=g.grad, dbeta=b.grad)
    if form in ("residual", "add"):
        out["dr"] = r.grad
    return out


def compare(tag, got, ref, dtype):
    for k in ("y", "s"):
        if k in got:
            assert_close(got[k], ref[k], TOL[dtype], f"{tag} {k}")
    for k in ("dx", "dr", "dgamma", "dbeta"):
        if k in got:
            assert_close(got[k], ref[k], GRAD_TOL[dtype], f"{tag} {k}")


# ============================================================================= A. multi-round
def plan_rows(lpr, bound, multiple_of=1):
    """rows = 2 R + tail with R = bound x 4 waves x rows per wave (one round of the largest launch the kernel may make); the tail ends
    inside a wave's row group and inside a workgroup."""
    rpw = 64 // lpr
    rows = 2 * bound * 4 * rpw + (4 * rpw + rpw // 2 + 1 if rpw > 1 else 3)
    while rows % multiple_of or rows % (4 * rpw) == 0 or (rpw > 1 and rows % rpw == 0):
        rows += 1
    return rows


def assert_plan(rows, lpr, bound, what):
    """The launch has at most `bound` workgroups of 4 waves x rpw rows: then some wave makes at least three passes, the last
    workgroup of the last round is partly filled and (rpw > 1) so is its last live wave."""
    rpw = 64 // lpr
    assert rows > 2 * bound * 4 * rpw, f"{what}: {rows} rows do not exceed two rounds of {bound} workgroups x {4 * rpw} rows"
    assert rows % (4 * rpw) != 0, f"{what}: {rows} rows end on a workgroup boundary"
    assert rpw == 1 or rows % rpw != 0, f"{what}: {rows} rows end on a wave's row-group boundary"


def launch_bounds(reserved):
    """(forward, backward) upper bounds of the fast kernels' grids: a 256-thread workgroup puts one wave on each SIMD, a SIMD holds
    at most 8: usable CUs x 8 workgroups, the backward capped at kBwdMaxBlocks = 2048.  These are the test's own bounds, not the
    library's grids (which cannot be read from here): the assertion below only checks that the reservation took effect, and the
    planning assertions hold the row count against these bounds, so that a launch rule which outgrows them has to change this test."""
    usable = 256 - int(_L().lib.hs_get_reserved_cus())
    assert usable == 256 - reserved
    return usable * 8, min(2048, usable * 8)


FORMS = ("plain", "residual", "add", "passthrough")
A_CASES = ([(BF16, w, 128) for w in (16, 96, 192, 512, 768, 1536)] + [(F32, w, 128) for w in (8, 48, 256, 768, 1024)]
           + [(BF16, 96, 0), (F32, 256, 0)])  # reserved 0: 256 usable CUs, the other row -> wave mapping


@pytest.mark.parametrize("dtype,width,reserved,form", [
    pytest.param(d, w, res, f, id=f"reserved{res}-" + case_id(d, w, f)) for d, w, res in A_CASES for f in FORMS])
def test_multi_round_vs_float64_and_row_slices_bit_exact(dtype, width, reserved, form):
    """More rows than two resident rounds of the fast kernels.  Second assertion: rows are independent and the instantiation depends
    on width, dtype and form only, so a contiguous slice of the input run alone reproduces the large run's y, dx, mean and rstd for
    those rows bit for bit -- a prefetch that hands a wave another row's chunk fails this exactly."""
    _, lpr, _ = lane_shape(dtype, width)
    rpw = 64 // lpr
    with reserved_cus(reserved):
        fwd_bound, bwd_bound = launch_bounds(reserved)
        rows = plan_rows(lpr, max(fwd_bound, bwd_bound))
        tag = f"ln/A {NAME[dtype]} {rows}x{width} reserved {reserved} {form}"
        assert_plan(rows, lpr, fwd_bound, tag + " forward")
        assert_plan(rows, lpr, bwd_bound, tag + " backward")
        t = make_inputs(dtype, rows, width, 1000 * width + reserved)
        got, ref = run_ops(form, t), reference(form, t)
        compare(tag, got, ref, dtype)
        y_c, mean, rstd = c_forward(form, t)
        assert torch.equal(y_c, got["y"])
        assert_close(mean, ref["mean"], 1e-5, tag + " mean")
        assert_close(rstd, ref["rstd"], 1e-5, tag + " rstd")
        del ref
        one_round = fwd_bound * 4 * rpw
        second = one_round + 8 * (3 * rpw + 1)  # inside the second round, not on a workgroup boundary; row offsets are multiples of 8
        for lo, hi in ((second, second + 9 * rpw + rpw // 2 + 1), ((2 * one_round - 8) // 8 * 8, rows)):
            sub = cut(t, lo, hi)
            alone = run_ops(form, sub)
            for k in ("y", "s", "dx", "dr"):
                if k in got:
                    assert torch.equal(alone[k], got[k][lo:hi]), f"{tag}: {k} of rows {lo}..{hi} run alone differs from the large run"
            y_s, mean_s, rstd_s = c_forward(form, sub)
            assert torch.equal(y_s, got["y"][lo:hi]) and torch.equal(mean_s, mean[lo:hi]) and torch.equal(rstd_s, rstd[lo:hi]), (
                f"{tag}: y / mean / rstd of rows {lo}..{hi} run alone differ from the large run")


@pytest.mark.parametrize("dtype,width", [pytest.param(d, w, id=case_id(d, w, "add", extras=True)) for d, w in ((BF16, 16), (F32, 8))])
def test_multi_round_general_kernels_vs_float64(dtype, width):
    """The general kernels behind their own caps (4096 workgroups forward with the prefetch of ITERS == 1, `bwd_blocks` <= 2048
    backward): the add form with a DropPath factor, s = a + rs b, y = LN(s), gradients on both outputs (dadd_out = rs g)."""
    _, lpr, _ = lane_shape(dtype, width)
    rows = plan_rows(lpr, 4096, multiple_of=len(RS6))
    tag = f"ln/A general {NAME[dtype]} {rows}x{width} add + row_scale"
    assert_plan(rows, lpr, 4096, tag + " forward")
    assert_plan(rows, lpr, 2048, tag + " backward")
    assert rows // 48 >= 2048  # bwd_blocks: rows / 48 workgroups, capped
    t = make_inputs(dtype, rows, width, 77 + width)
    rs = torch.tensor(RS6, device=DEV)
    rsv = rs.double().repeat_interleave(rows // len(RS6))[:, None]
    compare(tag, run_ops("add", t, row_scale=rs), reference("add", t, rsv=rsv), dtype)


# ============================================================================= B. every lane shape
B_WIDTHS = {
    (BF16, "partly"): (8, 24, 40, 96, 192, 384, 768, 1536, 3072), (BF16, "full"): (16, 32, 64, 128, 256, 512, 1024, 2048, 4096),
    (F32, "partly"): (4, 12, 20, 48, 96, 192, 384, 768, 1536), (F32, "full"): (8, 16, 32, 64, 128, 256, 512, 1024, 2048),
    (BF16, "elem"): (2, 3, 6, 12, 20, 50, 100, 250, 500, 1023), (F32, "elem"): (2, 3, 6, 10, 18, 50, 101, 250, 501, 1023),
}
B_CASES = [(d, w, f) for (d, fill), ws in B_WIDTHS.items() for w in ws for f in (("plain", "residual") if fill == "full" else ("plain", "residual", "add"))]


def test_lane_shape_sweep_covers_every_shape():
    """Every (lanes per row, chunks per lane) that with_shape can return is in the sweep, for both vector paths and the element-wise one."""
    vector = {(2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8)}
    for d in (BF16, F32):
        assert {lane_shape(d, w)[1:] for w in B_WIDTHS[d, "partly"]} == vector and {lane_shape(d, w)[1:] for w in B_WIDTHS[d, "full"]} == vector
        assert all(lane_shape(d, w)[0] == VEC[d] for fill in ("partly", "full") for w in B_WIDTHS[d, fill])
        assert {lane_shape(d, w)[1:] for w in B_WIDTHS[d, "elem"]} == vector | {(64, 16)} and all(lane_shape(d, w)[0] == 1 for w in B_WIDTHS[d, "elem"])


@pytest.mark.parametrize("dtype,width,form", [pytest.param(d, w, f, id=case_id(d, w, f)) for d, w, f in B_CASES])
def test_every_lane_shape_small_and_ragged(dtype, width, form):
    """Several workgroups, a ragged last wave and a ragged last row group at every lane shape; partly filled widths leave lanes
    without a chunk (`c < nchunk` false somewhere)."""
    _, lpr, _ = lane_shape(dtype, width)
    rpw = 64 // lpr
    rows = 5 * (4 * rpw) + rpw + 1
    t = make_inputs(dtype, rows, width, 31 * width + rows)
    compare(f"ln/B {NAME[dtype]} {rows}x{width} {form}", run_ops(form, t), reference(form, t), dtype)


@pytest.mark.parametrize("dtype,width", [(BF16, 4096 + 8), (F32, 2048 + 4), (BF16, 1025), (F32, 1025)], ids=[
    "bf16-w4104-past-fwd-fast-plain-bwd-fast-bf16", "fp32-w2052-past-fwd-fast-plain-bwd-fast-fp32",
    "bf16-w1025-past-fwd-general-elem-bwd-general", "fp32-w1025-past-fwd-general-elem-bwd-general"])
def test_width_limits_are_unsupported_and_write_nothing(dtype, width):
    """One chunk past the widest shape of the table row named in the id: no kernel is launched, nothing is written."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    rows, dt = 9, L.dtype_code(dtype)
    t = make_inputs(dtype, rows, width, width)
    sent = 12345.0
    y, dx = torch.full_like(t.x, sent), torch.full_like(t.x, sent)
    mean, rstd = torch.full((rows,), sent, device=DEV), torch.full((rows,), sent, device=DEV)
    dg, db = torch.full((width,), sent, device=DEV), torch.full((width,), sent, device=DEV)
    ws = torch.full((int(lib.hs_layernorm_bwd_workspace(rows, width)),), sent, device=DEV)
    assert lib.hs_layernorm_fwd(ptr(t.x), None, ptr(t.gamma), ptr(t.beta), ptr(y), ptr(mean), ptr(rstd), rows, width, dt, _stream()) == HS_ERR_UNSUPPORTED
    good_mean, good_rstd = torch.zeros(rows, device=DEV), torch.ones(rows, device=DEV)
    assert lib.hs_layernorm_bwd(ptr(t.dy), ptr(t.x), ptr(t.gamma), ptr(good_mean), ptr(good_rstd), ptr(dx), ptr(dg), ptr(db), ptr(ws), 0, rows,
                                width, dt, _stream()) == HS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for name, buf in (("y", y), ("mean", mean), ("rstd", rstd), ("dx", dx), ("dgamma", dg), ("dbeta", db), ("workspace", ws)):
        assert bool((buf == sent).all()), f"{name} was written by a call that returned HS_ERR_UNSUPPORTED"
    # the ops size their workspace with hs_layernorm_bwd_workspace and call the same entry points: they raise, no eager fall-back
    with pytest.raises(RuntimeError, match="UNSUPPORTED|too large"):
        _ops().layer_norm(t.x, t.gamma, t.beta)
    with pytest.raises(RuntimeError, match="UNSUPPORTED|too large"):
        _ops().add_layer_norm(t.x, t.r, t.gamma, t.beta)


# ============================================================================= C. parameter reduce over many partial rows
C_ROWS = 48 * 130 + 7  # bwd_blocks: 130 workgroups = 130 partial rows, two full strides of 64 and a remainder


@pytest.mark.parametrize("dtype,width,deferred", [
    pytest.param(d, w, q, id=case_id(d, w, "plain", deferred=q))
    for d, w, q in ((BF16, 50, False), (F32, 101, False), (F32, 1023, False), (BF16, 100, False), (BF16, 100, True))])
def test_param_reduce_over_many_partial_rows(dtype, width, deferred):
    """dgamma / dbeta of the element-wise backward from 130 partial rows against float64, and accumulate = 1 bit-equal to
    overwrite-then-add; widths % 4 != 0 take layernorm_param_reduce_kernel, width 100 the two routes of csrc/reduce_many.hip."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    rows, dt = C_ROWS, L.dtype_code(dtype)
    assert rows // 48 == 130 and lane_shape(dtype, width)[0] == 1
    t = make_inputs(dtype, rows, width, width)
    ref = reference("plain", t)
    _, mean, rstd = c_forward("plain", t)
    ws = torch.empty(int(lib.hs_layernorm_bwd_workspace(rows, width)), device=DEV)
    dx = torch.empty_like(t.x)
    start_g, start_b = torch.randn(width, device=DEV), torch.randn(width, device=DEV)
    flag = L.HS_ACC_DEFER if deferred else 0

    def bwd(dg, db, acc):
        L.check(lib.hs_layernorm_bwd(ptr(t.dy), ptr(t.x), ptr(t.gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dg), ptr(db), ptr(ws), acc | flag,
                                     rows, width, dt, _stream()), "hs_layernorm_bwd")
        if deferred:
            assert int(lib.hs_reduce_pending(_stream())) == 1
            L.check(lib.hs_reduce_flush(_stream()), "hs_reduce_flush")
    dg0, db0 = torch.full((width,), 7.0, device=DEV), torch.full((width,), 7.0, device=DEV)
    bwd(dg0, db0, 0)
    tag = f"ln/C {NAME[dtype]} {rows}x{width}" + (" deferred" if deferred else "")
    assert_close(dg0, ref["dgamma"], GRAD_TOL[dtype], tag + " dgamma")
    assert_close(db0, ref["dbeta"], GRAD_TOL[dtype], tag + " dbeta")
    assert_close(dx, ref["dx"], GRAD_TOL[dtype], tag + " dx")
    dg1, db1 = start_g.clone(), start_b.clone()
    bwd(dg1, db1, 1)
    assert torch.equal(dg1, start_g + dg0) and torch.equal(db1, start_b + db0)


# ============================================================================= D. stochastic forms with known masks
def stochastic_args(kind, rows, width):
    """(row_scale, drop_p, float64 mask multiplier, float64 DropPath column) for kind in rs / p / both."""
    rs = torch.tensor(RS6, device=DEV) if kind in ("rs", "both") else None
    p = P_DROP if kind in ("p", "both") else 0.0
    M = mask_of(SEED, p, (rows, width)) if p else 1.0
    rsv = rs.double().repeat_interleave(rows // len(RS6))[:, None] if rs is not None else 1.0
    return rs, p, M, rsv


@pytest.mark.parametrize("dtype,width", [pytest.param(d, w, id=case_id(d, w, "add", extras=True)) for d, w in ((BF16, 96), (BF16, 100), (F32, 48))])
def test_mask_is_a_function_of_seed_and_element_index(dtype, width):
    """The mask read off hs_gelu_fwd (bf16, flat) is the mask of the LayerNorm kernels: read off the v1 form s = a + M b with a = 0,
    b = 1 in this dtype and at this width (vector and element-wise kernels)."""
    L = _L()
    lib, ptr = L.lib, L.ptr
    rows = 37
    a, b = torch.zeros((rows, width), device=DEV, dtype=dtype), torch.ones((rows, width), device=DEV, dtype=dtype)
    s, y = torch.empty_like(a), torch.empty_like(a)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    gamma, beta = torch.ones(width, device=DEV), torch.zeros(width, device=DEV)
    L.check(lib.hs_add_layernorm_drop_fwd(ptr(a), ptr(b), ptr(gamma), ptr(beta), ptr(s), ptr(y), ptr(mean), ptr(rstd), None, 1, P_DROP, SEED,
                                          rows, width, L.dtype_code(dtype), _stream()), "hs_add_layernorm_drop_fwd")
    M = mask_of(SEED, P_DROP, (rows, width))
    assert torch.equal(s.double(), M)
    dropped = float((M == 0).double().mean())
    assert 0.5 * P_DROP < dropped < 1.5 * P_DROP, dropped  # (a mask that drops nothing would make the tests below vacuous)
    assert not torch.equal(mask_of(SEED + 1, P_DROP, (rows, width)), M)


RPS = (48, 100, 3)
KINDS = ("rs", "p", "both")


@pytest.mark.parametrize("rows_per_sample", RPS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,width,form", [
    pytest.param(d, w, f, id=case_id(d, w, f, extras=True)) for d, w in ((BF16, 96), (BF16, 192), (BF16, 768), (F32, 192)) for f in ("plain", "residual")])
def test_stochastic_v2_vs_float64(dtype, width, form, kind, rows_per_sample):
    """y = [res +] rs LN(mask x) and its backward (dy_eff = rs dy, dx = mask LN_bwd) with the generator's own mask."""
    rows = len(RS6) * rows_per_sample
    t = make_inputs(dtype, rows, width, width + rows)
    rs, p, M, rsv = stochastic_args(kind, rows, width)
    compare(f"ln/D v2 {NAME[dtype]} {rows}x{width} {form} {kind}", run_ops(form, t, rs, p, SEED), reference(form, t, M, rsv), dtype)


@pytest.mark.parametrize("form", ["plain", "residual"])
def test_stochastic_v2_multi_round_vs_float64(form):
    """The EX instantiations of both fast kernels past two resident rounds (planned as in family A)."""
    dtype, width, reserved = BF16, 96, 128
    _, lpr, _ = lane_shape(dtype, width)
    with reserved_cus(reserved):
        fwd_bound, bwd_bound = launch_bounds(reserved)
        rows = plan_rows(lpr, max(fwd_bound, bwd_bound), multiple_of=len(RS6))
        tag = f"ln/D v2 multi-round bf16 {rows}x{width} {form}"
        assert_plan(rows, lpr, fwd_bound, tag + " forward")
        assert_plan(rows, lpr, bwd_bound, tag + " backward")
        t = make_inputs(dtype, rows, width, 5)
        rs, p, M, rsv = stochastic_args("both", rows, width)
        compare(tag, run_ops(form, t, rs, p, SEED), reference(form, t, M, rsv), dtype)


@pytest.mark.parametrize("rows_per_sample", RPS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,width", [pytest.param(d, w, id=case_id(d, w, "add", extras=True)) for d, w in ((BF16, 128), (BF16, 768), (F32, 96))])
def test_stochastic_v1_vs_float64(dtype, width, kind, rows_per_sample):
    """s = a + rs mask b, y = LN(round(s)), gradients on both outputs: da = g, db = rs mask g (the dadd_out path)."""
    rows = len(RS6) * rows_per_sample
    t = make_inputs(dtype, rows, width, 3 * width + rows)
    rs, p, M, rsv = stochastic_args(kind, rows, width)
    compare(f"ln/D v1 {NAME[dtype]} {rows}x{width} {kind}", run_ops("add", t, rs, p, SEED), reference("add", t, M, rsv), dtype)


STREAM_SLACK = []  # (elements of hi that are a neighbour of the rounded float64 sum, elements) per stream case, for the report
E_ROWS = [0, 0, 0]  # family E: rows compared exactly, launches, rows that differed


def assert_rounds_to_bf16(hi, exact, mag, what):
    """`hi` is the bf16 rounding of `exact` (float64).  The kernel forms the sum in fp32, so an element whose exact sum lies next to
    a bf16 rounding tie may land on the neighbour: each element is allowed the fp32 evaluation error of its own operands and no
    more.  `mag` is the sum of the magnitudes of the element's terms; the path to one element makes at most about 30 fp32 roundings
    (8 serial adds and 6 butterfly steps for each of the two row statistics, the reciprocal square root, the affine map, the two
    factors and the adds), each at most 2^-24 of `mag`: 64 x 2^-24 = 2^-18 of `mag` covers them twice.  That is 2^-9 of a bf16 ulp
    of an element as large as its terms: about one element in 250 lies near enough to a tie to use it."""
    slack = 2.0 ** -18 * mag
    low, high = (exact - slack).to(BF16), (exact + slack).to(BF16)
    bad = (hi < low) | (hi > high)
    STREAM_SLACK.append((int((hi != exact.to(BF16)).sum()), hi.numel()))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements of hi are not the bf16 rounding of the float64 sum"


@pytest.mark.parametrize("rows_per_sample", RPS)
@pytest.mark.parametrize("form", [pytest.param(f, id=case_id(BF16, 512, f, extras=True, lo=True)) for f in ("residual", "add")])
def test_compensated_stream_with_droppath_and_dropout(form, rows_per_sample):
    """layer_norm_stream / add_layer_norm_stream with row_scale and drop_p (the model's train-mode residual stream): hi is the bf16
    rounding of the float64 sum, hi + lo follows it to 2^-16 of its scale (one bf16 rounding of the remainder: 2^-9 of 2^-9), and the
    gradients are those of the plain stochastic call with the same seed.  Residual form: bit for bit -- the backward is the same
    call on the same x and dy, and the general forward kernel that carries the stream computes the row statistics with the fast
    kernel's arithmetic in the fast kernel's order.  Add form: the stream's y is the LN of the un-rounded sum and lo_in moves that
    sum, so the saved statistics and the stored s differ from the plain call's by a bf16 rounding of s and the gradients agree
    to GRAD_TOL only."""
    ops = _ops()
    dtype, width = BF16, 512
    rows = len(RS6) * rows_per_sample
    t = make_inputs(dtype, rows, width, 9 + rows)
    rs, p, M, rsv = stochastic_args("both", rows, width)
    lo_in = (t.d2.float() * 2.0 ** -10).to(BF16)  # a remainder of the incoming stream
    x, r = t.x.clone().requires_grad_(True), t.r.clone().requires_grad_(True)
    g, b = t.gamma.clone().requires_grad_(True), t.beta.clone().requires_grad_(True)
    tag = f"ln/D stream {form} {rows}x{width}"
    if form == "residual":  # y + y_lo = (r + r_lo) + rs LN(mask x)
        hi, lo = ops.layer_norm_stream(x, g, b, r, res_lo=lo_in, row_scale=rs, drop_p=p, seed=SEED)
        g64, b64, mx = t.gamma.double(), t.beta.double(), M * t.x.double()
        n, mu, rstd = ln64(mx, g64, b64)
        xhat = ((mx - mu[:, None]) * rstd[:, None]).abs()
        exact = t.r.double() + lo_in.double() + rsv * n
        # (an error of the row statistics moves an element by |gamma| (|xhat| + 1) times that error, whatever the element's own size)
        mag = t.r.double().abs() + lo_in.double().abs() + rsv * (g64.abs() * (2 * xhat + 1) + b64.abs())
        hi.backward(t.dy)
    else:                   # s + s_lo = (x + x_lo) + rs mask r,  y = LN of the un-rounded sum
        hi, y, lo = ops.add_layer_norm_stream(x, lo_in, r, g, b, row_scale=rs, drop_p=p, seed=SEED)
        exact = t.x.double() + lo_in.double() + rsv * M * t.r.double()
        mag = t.x.double().abs() + lo_in.double().abs() + (rsv * M * t.r.double()).abs()
        assert_close(y, ln64(exact, t.gamma.double(), t.beta.double())[0], TOL[dtype], tag + " y")
        torch.autograd.backward([hi, y], [t.d2, t.dy])
    assert not lo.requires_grad
    assert_rounds_to_bf16(hi.detach(), exact, mag, tag)
    assert_close(hi.detach().double() + lo.double(), exact, 2.0 ** -16, f"ln/stream-sum {form} {rows}x{width} hi + lo")
    plain = run_ops(form, t, rs, p, SEED)
    for k, v in (("dx", x.grad), ("dr", r.grad), ("dgamma", g.grad), ("dbeta", b.grad)):
        if form == "residual":
            assert torch.equal(v, plain[k]), f"{tag}: {k} differs from the plain stochastic call's"
        else:
            assert_close(v, plain[k], GRAD_TOL[dtype], f"{tag} {k} vs the plain stochastic call")


# ============================================================================= E. sample_of, exactly
def _sample_of_case(dtype, width, rows_per_sample, samples):
    rows = samples * rows_per_sample
    rs = (1 + torch.arange(samples, device=DEV) % 255).float()  # exact in bf16
    # (gamma = 0: the values of x do not reach y; the large cases skip the random fill)
    x = torch.randn((rows, width), device=DEV, dtype=dtype) if rows * width <= 1 << 24 else torch.zeros((rows, width), device=DEV, dtype=dtype)
    with torch.no_grad():
        y = _ops().layer_norm(x, torch.zeros(width, device=DEV), torch.ones(width, device=DEV), row_scale=rs)
    del x
    want = rs.to(dtype).repeat_interleave(rows_per_sample)[:, None].expand(rows, width)
    E_ROWS[0] += rows
    E_ROWS[1] += 1
    if not torch.equal(y, want):
        bad = (y != want).any(1).nonzero().flatten()
        E_ROWS[2] += int(bad.numel())
        raise AssertionError(f"{int(bad.numel())} rows of {rows} read another sample's factor (rows_per_sample {rows_per_sample}); first rows {bad[:8].tolist()}")


@pytest.mark.parametrize("rows_per_sample", [1, 3, 7, 48, 100, 768, 12 * 1024 + 3])
@pytest.mark.parametrize("dtype,width", [pytest.param(d, w, id=case_id(d, w, "plain", extras=True)) for d, w in ((BF16, 8), (F32, 4))])
def test_sample_of_is_exact_at_sample_boundaries(dtype, width, rows_per_sample):
    """gamma = 0, beta = 1, drop_p = 0: every element of row i is row_scale[i // rows_per_sample]."""
    _sample_of_case(dtype, width, rows_per_sample, 300)


@pytest.mark.parametrize("rows_per_sample", [3, 11])
@pytest.mark.parametrize("dtype,width", [pytest.param(d, w, id=case_id(d, w, "plain", extras=True)) for d, w in ((BF16, 8), (F32, 4))])
def test_sample_of_is_exact_where_the_float_quotient_is_off_by_one(dtype, width, rows_per_sample):
    """With 300 samples the quotient stays small and the float product truncates to it without help.  The repairs of sample_of
    are needed once row x (1 / rows_per_sample as the fp32 reciprocal gives it) lands on the wrong side of a whole number, which
    takes rows from about 2^23 on: so as many whole samples as fit below 2^24 rows, the float branch to its end.  A reciprocal
    that comes out too large gives the last row of a sample the next sample's quotient (the downward repair), one that comes
    out too small leaves the first row of a sample one short (the upward repair).  Which it is depends on the divisor and on
    the hardware's reciprocal, which is good to one ulp and not correctly rounded: 1 / 11 comes out too large on gfx950 (without
    the downward repair 0.48 M of these rows read their neighbour's factor, from row 11534346 on), 1 / 3 does not."""
    samples = (2 ** 24 - 1) // rows_per_sample
    assert 2 ** 24 - rows_per_sample <= samples * rows_per_sample < 2 ** 24
    _sample_of_case(dtype, width, rows_per_sample, samples)


def test_sample_of_is_exact_on_both_sides_of_2_pow_24_rows():
    """The float-reciprocal branch up to row 2^24 - 1 and the division branch from 2^24 on, in one launch of the fast EX kernel
    (256 MiB per tensor: below the 4 GiB switch to the general kernel)."""
    rps = 48
    samples = -(-(2 ** 24 + 1000) // rps)
    assert samples * rps > 2 ** 24 + 900 and samples * rps * 8 * 2 < 2 ** 32
    _sample_of_case(BF16, 8, rps, samples)
