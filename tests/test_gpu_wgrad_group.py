"""Grouped weight gradients (`hs_linear_wgrad_group`, include/healswin.h): several Linear layers over the same token rows in one
launch must give what the single-problem entry points give.  The slice count of a group differs from a single launch's, so the
summation order over the token slices differs and bit-equality is not required: the bound is the one
tests/test_gpu_kernels.py::test_linear_wgrad_vs_fp32 uses against the fp32 product,
    |dW - ref| <= 2e-4 * max(1, max|ref|) * max(1, sqrt(rows / 4096)),    |db - ref| <= 2e-4 * max(1, max|ref|),
here with the single entry point's result as `ref`."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from heal_swin_amd import _lib
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _single(L, dy, x, dw, db, acc, gelu):
    rows, n_out, k_in = dy.shape[0], dy.shape[1], x.shape[1]
    ws = torch.empty(int(L.lib.hs_linear_wgrad_workspace(rows, n_out, k_in)), dtype=torch.float32, device=DEV)
    fn = L.lib.hs_linear_wgrad_gelu if gelu else L.lib.hs_linear_wgrad
    L.check(fn(L.ptr(dy), L.ptr(x), L.ptr(dw), L.ptr(db), L.ptr(ws), rows, n_out, k_in, acc, L.HS_BF16, _stream()), "single")
    return ws


def _check(rows, got, ref, what):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    bound = 2e-4 * max(1.0, scale) * (max(1.0, (rows / 4096) ** 0.5) if what == "dw" else 1.0)
    print(f"{what}: err {err:.3e} bound {bound:.3e} scale {scale:.3e}")
    assert err <= bound, (what, err, bound)


# (rows, [(n_out, k_in, bias, gelu)], one launch expected)
CASES = {
    "pair_fc2_fc1_256tile": (33000, [(512, 2048, True, False), (2048, 512, True, False)], True),
    "pair_proj_qkv_256tile": (40001, [(512, 512, True, False), (1536, 512, True, False)], True),
    "triple_256tile_ragged": (7777, [(256, 256, True, False), (768, 256, False, False), (1024, 256, True, False)], True),
    "quad_256tile": (20000, [(256, 256, True, False), (768, 256, True, False), (256, 1024, True, False), (1024, 256, True, False)], True),
    "pair_128tile_gelu": (5003, [(128, 512, True, True), (128, 128, True, False)], True),
    "quad_128tile_gelu_ragged": (777, [(96, 288, True, False), (96, 384, True, True), (128, 128, False, False), (24, 40, True, False)], True),
    "pair_256x128_tile": (9000, [(512, 128, True, False), (768, 128, True, False)], True),
    "mixed_tiles_launch_alone": (6000, [(512, 512, True, False), (128, 128, True, False), (128, 512, True, True)], False),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("deferred", [False, True])
def test_group_equals_single_problem_entry_points(name, acc, deferred):
    L = _lib()
    lib = L.lib
    rows, members, one_launch = CASES[name]
    g = torch.Generator(device=DEV).manual_seed(rows + len(members))
    variants = {int(lib.hs_linear_wgrad_group_variant(rows, n, k, L.HS_BF16)) for n, k, _, _ in members}
    assert (len(variants) == 1 and 0 not in variants) == one_launch, variants
    ops_in, refs, outs = [], [], []
    for n_out, k_in, bias, gelu in members:
        dy = torch.randn((rows, n_out), generator=g, device=DEV).to(torch.bfloat16)
        x = torch.randn((rows, k_in), generator=g, device=DEV).to(torch.bfloat16)
        base_w = torch.randn((n_out, k_in), generator=g, device=DEV)
        base_b = torch.randn(n_out, generator=g, device=DEV) if bias else None
        rw, rb = base_w.clone(), (base_b.clone() if bias else None)
        _single(L, dy, x, rw, rb, acc, gelu)
        refs.append((rw, rb))
        dw, db = base_w.clone(), (base_b.clone() if bias else None)
        outs.append((dw, db, base_w))
        ops_in.append((dy, x, dw, db, n_out, k_in, acc | (L.HS_ACC_DEFER if deferred else 0), gelu))
    arr = L.wgrad_problems(ops_in)
    nws = int(lib.hs_linear_wgrad_group_workspace(arr, len(members), rows, L.HS_BF16))
    assert nws > 0
    ws = torch.full((nws + 1024,), float("nan"), dtype=torch.float32, device=DEV)  # (a guard zone behind the workspace)
    L.check(lib.hs_linear_wgrad_group(arr, len(members), L.ptr(ws), rows, L.HS_BF16, _stream()), "hs_linear_wgrad_group")
    if deferred:
        assert int(lib.hs_reduce_pending(_stream())) == len(members)  # one queued sum per problem
        if not acc:
            assert all(torch.equal(dw, base) for dw, _, base in outs), "a deferred call must not touch the gradient before the flush"
        L.check(lib.hs_reduce_flush(_stream()), "hs_reduce_flush")
    assert int(lib.hs_reduce_pending(_stream())) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nws:]).all()), "the launch wrote behind its workspace"
    for (dw, db, _), (rw, rb) in zip(outs, refs):
        _check(rows, dw, rw, "dw")
        if db is not None:
            _check(rows, db, rb, "db")


def test_group_of_one_is_the_single_entry_point_bit_for_bit():
    L = _lib()
    rows, n_out, k_in = 33000, 512, 2048
    g = torch.Generator(device=DEV).manual_seed(3)
    dy = torch.randn((rows, n_out), generator=g, device=DEV).to(torch.bfloat16)
    x = torch.randn((rows, k_in), generator=g, device=DEV).to(torch.bfloat16)
    rw, rb = torch.zeros((n_out, k_in), device=DEV), torch.zeros(n_out, device=DEV)
    _single(L, dy, x, rw, rb, 0, False)
    dw, db = torch.ones_like(rw), torch.ones_like(rb)
    arr = L.wgrad_problems([(dy, x, dw, db, n_out, k_in, 0, False)])
    ws = torch.empty(int(L.lib.hs_linear_wgrad_group_workspace(arr, 1, rows, L.HS_BF16)), dtype=torch.float32, device=DEV)
    L.check(L.lib.hs_linear_wgrad_group(arr, 1, L.ptr(ws), rows, L.HS_BF16, _stream()), "hs_linear_wgrad_group")
    assert torch.equal(dw, rw) and torch.equal(db, rb)


def test_parked_problem_without_a_partner_lands_at_flush_reductions():
    """The op layer parks the first Linear of a pair; when no second one comes, flush_reductions launches it alone."""
    from heal_swin_amd import ops
    from heal_swin_amd.ops import gemm, runtime
    L = _lib()
    rows, n_out, k_in = 20000, 512, 512
    g = torch.Generator(device=DEV).manual_seed(11)
    dy = torch.randn((rows, n_out), generator=g, device=DEV).to(torch.bfloat16)
    x = torch.randn((rows, k_in), generator=g, device=DEV).to(torch.bfloat16)
    rw, rb = torch.zeros((n_out, k_in), device=DEV), torch.zeros(n_out, device=DEV)
    _single(L, dy, x, rw, rb, 1, False)
    dw, db = torch.zeros_like(rw), torch.zeros_like(rb)
    gemm._wgrad_grouped((dy, x, dw, db, n_out, k_in, 1 | L.HS_ACC_DEFER, False))
    s = torch.cuda.current_stream().cuda_stream
    assert s in runtime._PARKED and int(L.lib.hs_reduce_pending(_stream())) == 0
    assert not bool(dw.any()), "nothing is launched while the problem is parked"
    ops.flush_reductions()
    assert s not in runtime._PARKED and int(L.lib.hs_reduce_pending(_stream())) == 0
    assert torch.equal(dw, rw) and torch.equal(db, rb)  # launched alone: the single entry point's launch and sum


def test_parked_problems_pair_up_and_a_mismatch_is_launched_alone():
    from heal_swin_amd import ops
    from heal_swin_amd.ops import gemm, runtime
    L = _lib()
    g = torch.Generator(device=DEV).manual_seed(12)
    made = []
    for rows, n_out, k_in in ((20000, 512, 2048), (20000, 2048, 512), (5000, 1024, 1024), (20000, 512, 512)):
        dy = torch.randn((rows, n_out), generator=g, device=DEV).to(torch.bfloat16)
        x = torch.randn((rows, k_in), generator=g, device=DEV).to(torch.bfloat16)
        rw, rb = torch.zeros((n_out, k_in), device=DEV), torch.zeros(n_out, device=DEV)
        _single(L, dy, x, rw, rb, 1, False)
        dw, db = torch.zeros_like(rw), torch.zeros_like(rb)
        gemm._wgrad_grouped((dy, x, dw, db, n_out, k_in, 1 | L.HS_ACC_DEFER, False))
        made.append((rows, dw, db, rw, rb))
    # the first two paired; the third (other rows) parked, then launched alone when the fourth came; the fourth is parked
    assert int(L.lib.hs_reduce_pending(_stream())) == 3 and torch.cuda.current_stream().cuda_stream in runtime._PARKED
    ops.flush_reductions()
    for rows, dw, db, rw, rb in made:
        _check(rows, dw, rw, "dw")
        _check(rows, db, rb, "db")
