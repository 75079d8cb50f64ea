"""hs_gemm_nt across MULTI-TILE persistent workgroups: the state carried from one output tile to the next.

A workgroup of hs_gemm_nt walks the tiles id0, id0 + stride, id0 + 2 stride, ... (stride = workgroups per XCD, 32 minus
hs_set_reserved_cus() / 8) as ONE stream of k-steps whose DMA issue cursor runs NSTAGE - 1 steps ahead of the compute cursor,
so a tile's operands -- and, on the 256-row tiles, its bias (LDS slots written when the issue cursor enters the tile) -- are
fetched while earlier tiles are still being computed or written out.  The cases here put every workgroup on >= 3 tiles whose
column blocks differ from one tile to the next (tiles_n coprime with the stride), with k on both sides of nk = NSTAGE - 1 k-steps,
under three strides, the two 256-row tile variants and the built-in choice, every epilogue, dropout on and off, and a strided A.

Reference: the float64 product of the same bf16 operands on the GPU, with the epilogue formulas of include/healswin.h
(HS_EPI_*).  A failing comparison names the wrong (tm, tn) tiles, where they sit in their workgroup's tile sequence, and whose
column block's bias explains the error."""
import pytest
import torch

from _util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
M_ROWS = 100003  # 391 row blocks of 256, the last one partial: >= 4 tiles per workgroup at tiles_n = 3 and stride 32
TILE = {1: (128, 128), 2: (256, 128), 3: (256, 256)}
# Candidate widths per forced variant (tiles_n 3, 3, 5, 7 and a ragged 7 at BN = 128; 3, 5, 7 and a ragged 7 at BN = 256).  The
# built-in choice (0) gets the model's stage-0 widths too (qkv 288, fc1 384: the 256 x 128 tile when k is not a multiple of 64).
# A case takes the widths whose tile grid reaches the regime under its stride (_Layout.reaches), in turn over the k classes; stride 30
# shares the factors 2, 3 and 5 with tiles_n, so it runs the 7-column-block widths.
NS = {2: [288, 384, 640, 896, 872], 3: [768, 1280, 1792, 1736], 0: [288, 384, 640, 896, 1280, 1792]}
# (k, k2): k-step counts nk = 1, 1, 2, 2, 3 with one segment (k = 16: the K-tail, non-FAST path), 1 + 1, 1 + 1 with a full
# second segment, and 2 + 1 with two segments
KS = [(16, 0), (64, 0), (96, 0), (128, 0), (192, 0), (32, 32), (64, 64), (96, 32)]
RESERVED = [0, 8, 16]  # strides 32, 31, 30 workgroups per XCD


def _lib():
    from heal_swin_amd import _lib
    return _lib


def _gemm(a, b, bias=None, epi=0, aux=None, a2=None, b2=None, p=0.0, seed=0):
    """hs_gemm_nt through the C ABI (as tests/test_gpu_gemm.py::_gemm), a and a2 with their own row strides."""
    L = _lib()
    m, k = a.shape
    n = b.shape[0]
    c = torch.empty((m, n), dtype=BF, device=a.device)
    if epi == L.HS_EPI_GELU:
        aux = torch.empty((m, n), dtype=BF, device=a.device)
    k2 = 0 if a2 is None else a2.shape[1]
    L.check(L.lib.hs_gemm_nt(L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), k, L.ptr(a2), 0 if a2 is None else a2.stride(0), L.ptr(b2),
                             0 if b2 is None else b2.stride(0), k2, L.ptr(bias), L.ptr(c), L.ptr(aux), m, n, epi, p, seed, L.HS_BF16,
                             L.stream_ptr(a.device)), "hs_gemm_nt")
    return c, aux


def _variant(forced, m, n, k, k2, epi):
    """The tile variant hs_gemm_nt launches under hs_gemm_nt_set_tile(forced) (asked of the library, so that the case knows its
    tile grid); leaves the built-in choice set."""
    L = _lib()
    L.lib.hs_gemm_nt_set_tile(forced)
    try:
        return int(L.lib.hs_gemm_nt_tile_variant(m, n, k, k2, epi))
    finally:
        L.lib.hs_gemm_nt_set_tile(0)


class _Layout:
    """Tile grid and tile -> workgroup assignment of one launch (launch_tile in csrc/gemm_nt.hip)."""

    def __init__(self, variant, m, n, reserved):
        self.variant = variant
        self.bm, self.bn = TILE[variant]
        self.tiles_m, self.tiles_n = -(-m // self.bm), -(-n // self.bn)
        tiles = self.tiles_m * self.tiles_n
        self.per_xcd = -(-tiles // 8)
        self.stride = min(self.per_xcd, (32 - reserved // 8) * (2 if variant == 1 else 1))

    def position(self, tm, tn):
        """(ordinal of the tile in its workgroup's sequence, id of the workgroup's first tile)"""
        tid = tm * self.tiles_n + tn
        x = tid // self.per_xcd
        id0 = x * self.per_xcd + (tid - x * self.per_xcd) % self.stride
        return (tid - id0) // self.stride, id0

    def reaches(self):
        """every workgroup of a full XCD computes >= 3 tiles, and a workgroup's tiles 0 and 2 (and 1 and 3) lie in different column
        blocks: a tile state (a bias slot) shared by tiles j and j + 2 shows as a wrong column block's values"""
        return self.per_xcd >= 3 * self.stride and (2 * self.stride) % self.tiles_n != 0


def _tile_report(got, ref, lay, bias=None, worst=6):
    """The (tm, tn) tiles with the largest error, their place in the workgroup's tile sequence, and (bias epilogues) the column
    block whose bias the error matches best."""
    m, n = ref.shape
    d = (got.to(torch.float64) - ref).abs()
    pad = torch.nn.functional.pad(d, (0, lay.tiles_n * lay.bn - n, 0, lay.tiles_m * lay.bm - m))
    per_tile = pad.view(lay.tiles_m, lay.bm, lay.tiles_n, lay.bn).amax(dim=(1, 3))
    bad = int((per_tile > 0.05 * float(ref.abs().max())).sum())
    vals, idx = per_tile.flatten().topk(min(worst, per_tile.numel()))
    bpad = None
    if bias is not None:
        bpad = torch.nn.functional.pad(bias.to(torch.float64), (0, lay.tiles_n * lay.bn - n)).view(lay.tiles_n, lay.bn)
    lines = [f"  variant {lay.variant} ({lay.bm} x {lay.bn}), tiles {lay.tiles_m} x {lay.tiles_n}, stride {lay.stride}: "
             f"{bad} tiles off by > 5 % of the scale; the worst:"]
    for v, i in zip(vals.tolist(), idx.tolist()):
        tm, tn = divmod(i, lay.tiles_n)
        ordinal, id0 = lay.position(tm, tn)
        line = (f"    tile (tm {tm}, tn {tn}): max err {v:.3e}; tile #{ordinal} of its workgroup, whose first tile has tn "
                f"{id0 % lay.tiles_n}")
        if bpad is not None:
            r0, c0 = tm * lay.bm, tn * lay.bn
            r1, c1 = min(r0 + lay.bm, m), min(c0 + lay.bn, n)
            shift = (got[r0:r1, c0:c1].to(torch.float64) - ref[r0:r1, c0:c1]).mean(0)  # the bias error is the same on every row
            own = bpad[tn, : c1 - c0]
            fit = [float((shift - (bpad[j, : c1 - c0] - own)).abs().max()) for j in range(lay.tiles_n)]
            j = min(range(lay.tiles_n), key=fit.__getitem__)
            line += f"; the error matches the bias of column block tn {j} (residual {fit[j]:.2e})"
        lines.append(line)
    return "\n".join(lines)


def _check(bad, got, ref, tol, what, lay, bias=None):
    """assert_close, but collected: every comparison of the case is judged before the test fails."""
    try:
        assert_close(got, ref, tol, what)
    except AssertionError as e:
        bad.append(f"{e}\n{_tile_report(got, ref, lay, bias)}")


def _dgelu(x):
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


def _keep(m, n, p, seed):
    """keep mask of the (seed, element index) generator, from the standalone GELU kernel on pre-activations where gelu != 0"""
    from heal_swin_amd import ops
    return ops.GeluDropoutFn.apply(torch.full((m, n), 3.0, device=DEV, dtype=BF), p, seed) != 0


@pytest.mark.parametrize("reserved", RESERVED)
@pytest.mark.parametrize("k,k2", KS, ids=[f"k{k}+{k2}" if k2 else f"k{k}" for k, k2 in KS])
@pytest.mark.parametrize("tile", [2, 3, 0])
def test_gemm_nt_multi_tile_workgroups_vs_fp64(tile, k, k2, reserved):
    L = _lib()
    ki, ri = KS.index((k, k2)), RESERVED.index(reserved)
    m = M_ROWS
    epis = (L.HS_EPI_BIAS, L.HS_EPI_GELU, L.HS_EPI_DGELU, L.HS_EPI_RESID)
    ns = [n for n in NS[tile] if all(_Layout(_variant(tile, m, n, k, k2, e), m, n, reserved).reaches() for e in epis)]
    assert ns, (tile, k, k2, reserved)
    n = ns[ki % len(ns)]
    lays = {e: _Layout(_variant(tile, m, n, k, k2, e), m, n, reserved) for e in epis}
    g = torch.Generator(device=DEV).manual_seed(1000 * ki + 10 * ri + tile)
    kt = k + k2
    # A: a column slice of a wider buffer (lda = k + 8) for the BIAS and RESID launches, a contiguous copy for the others
    a_wide = torch.randn((m, k + 8), generator=g, device=DEV).to(BF)
    a_s = a_wide[:, :k]
    a = a_s.contiguous()
    a2 = torch.randn((m, k2), generator=g, device=DEV).to(BF) if k2 else None
    w = (torch.randn((n, kt), generator=g, device=DEV) * kt ** -0.5).to(BF)
    b, b2 = (w[:, :k], w[:, k:]) if k2 else (w, None)
    bias = torch.randn(n, generator=g, device=DEV)  # O(1): the bias of a wrong column block is an O(1) error
    ref = a.double() @ b.double().t()
    if k2:
        ref += a2.double() @ b2.double().t()
    bias64 = bias.double()
    hb = ref + bias64

    prev_reserved = int(L.lib.hs_get_reserved_cus())
    bad = []
    try:
        L.check(L.lib.hs_set_reserved_cus(reserved), "hs_set_reserved_cus")
        L.lib.hs_gemm_nt_set_tile(tile)
        tag = f"gemm_nt stream tile={tile} m={m} n={n} k={k}+{k2} reserved={reserved}"

        # BIAS (strided A), twice: no atomics, so two launches agree to the bit
        lay = lays[L.HS_EPI_BIAS]
        c, _ = _gemm(a_s, b, bias, a2=a2, b2=b2)
        _check(bad, c, hb, 6e-3, tag + " bias (lda = k + 8)", lay, bias64)
        c2, _ = _gemm(a_s, b, bias, a2=a2, b2=b2)
        if not torch.equal(c, c2):
            bad.append(f"{tag} bias: two identical launches differ in {int((c != c2).sum())} elements")
        del c, c2

        # GELU, p = 0: h and gelu(h)
        lay = lays[L.HS_EPI_GELU]
        h, act = _gemm(a, b, bias, epi=L.HS_EPI_GELU, a2=a2, b2=b2)
        _check(bad, h, hb, 6e-3, tag + " gelu: h", lay, bias64)
        gref = torch.nn.functional.gelu(hb)
        _check(bad, act, gref, 6e-3, tag + " gelu: act", lay)
        del h, act

        # GELU, p = 0.25: h, the mask (keyed on the global element index: the standalone kernel's on the returned h), the survivors
        p, seed = 0.25, 0x5EED0000 + 97 * ki + ri
        h, act = _gemm(a, b, bias, epi=L.HS_EPI_GELU, a2=a2, b2=b2, p=p, seed=seed)
        _check(bad, h, hb, 6e-3, tag + " gelu p=0.25: h", lay, bias64)
        from heal_swin_amd import ops
        plain = ops.GeluDropoutFn.apply(h, p, seed)
        if not torch.equal(act == 0, plain == 0):
            bad.append(f"{tag} gelu p=0.25: dropout mask differs from hs_gelu_fwd's in {int(((act == 0) != (plain == 0)).sum())} elements")
        keep = plain != 0
        del plain
        _check(bad, act, gref * keep / (1 - p), 1e-2, tag + " gelu p=0.25: act", lay)
        h2, act2 = _gemm(a, b, bias, epi=L.HS_EPI_GELU, a2=a2, b2=b2, p=p, seed=seed)
        if not (torch.equal(h, h2) and torch.equal(act, act2)):
            bad.append(f"{tag} gelu p=0.25: two identical launches differ")
        del h, act, h2, act2, gref

        # DGELU, p = 0 and 0.25 (no bias: c = acc * mask * gelu'(aux))
        lay = lays[L.HS_EPI_DGELU]
        hs = (torch.randn((m, n), generator=g, device=DEV) * 1.5).to(BF)
        dref = ref * _dgelu(hs.double())
        d, _ = _gemm(a, b, None, epi=L.HS_EPI_DGELU, aux=hs, a2=a2, b2=b2)
        _check(bad, d, dref, 8e-3, tag + " dgelu", lay)
        keep = _keep(m, n, p, seed)
        d, _ = _gemm(a, b, None, epi=L.HS_EPI_DGELU, aux=hs, a2=a2, b2=b2, p=p, seed=seed)
        # (judged where |reference| > 1e-3: an accumulator that cancels to 0 in fp32 carries no mask bit)
        off = int((((d != 0) != keep) & (dref.abs() > 1e-3)).sum())
        if off:
            bad.append(f"{tag} dgelu p=0.25: dropout mask differs from hs_gelu_fwd's in {off} elements")
        _check(bad, d, dref * keep / (1 - p), 1e-2, tag + " dgelu p=0.25", lay)
        del hs, dref, d, keep

        # RESID (strided A): c = acc + bias + aux
        lay = lays[L.HS_EPI_RESID]
        res = torch.randn((m, n), generator=g, device=DEV).to(BF)
        r, _ = _gemm(a_s, b, bias, epi=L.HS_EPI_RESID, aux=res, a2=a2, b2=b2)
        _check(bad, r, hb + res.double(), 6e-3, tag + " resid (lda = k + 8)", lay, bias64)
    finally:
        L.lib.hs_gemm_nt_set_tile(0)
        L.lib.hs_set_reserved_cus(prev_reserved)
    assert not bad, "\n".join(bad)


def test_stage0_block_full_size_random_biases_through_hs_gemm_nt_vs_oracle():
    """HEAL-SWIN-T stage 0 at full size (C 96, 3 heads, window 64, nest_roll 32, 8 base pixels, nside 128: 131 072 tokens, one
    image) with random Linear biases and LayerNorm affines, qkv / proj / fc1 + GELU / fc2 and their input gradients all through
    hs_gemm_nt (own GEMM forced, fused MLP and fused training attention off, no tuner): qkv (n 288) and fc1 (n 384) run the
    256 x 128 tile with nk = 2 and tiles_n = 3 over 6 tiles per workgroup.  Against oracle.model.swin_block in float64 on the GPU."""
    from heal_swin_amd import ops
    from heal_swin_amd.models_torch import swin_hp_transformer as M
    from oracle import model as OM
    from oracle import tables as T
    from _util import GRAD_TOL, TOL, assert_unbiased
    C, nH, N, bp, ws, shift = 96, 3, 131072, 8, 64, 32
    torch.manual_seed(29)
    blk = M.SwinTransformerBlock(C, N, bp, nH, window_size=ws, shift_size=shift, shift_strategy="nest_roll", rel_pos_bias="flat")
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.normal_(0, 0.02)  # (as tests/test_gpu_baseline_configs.py)
            elif name.startswith("norm") and name.endswith(".weight"):
                p.uniform_(0.5, 1.5)
            elif name.endswith(".bias"):
                p.normal_(0, 0.5)
    sd = {k: v.detach().to(DEV, torch.float64).requires_grad_(True) for k, v in blk.state_dict().items() if v.is_floating_point() and not k.endswith("attn_mask")}
    blk = blk.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn((1, N, C), generator=g, device=DEV).to(BF)
    dy = torch.randn((1, N, C), generator=g, device=DEV).to(BF)

    prev = (ops.OWN_GEMM, ops.FUSED_MLP, ops.FUSED_ATTN_MODULE_TRAIN, ops.GEMM_TUNE)
    try:
        ops.OWN_GEMM, ops.FUSED_MLP, ops.FUSED_ATTN_MODULE_TRAIN, ops.GEMM_TUNE = "1", False, False, False
        xg = x.clone().requires_grad_(True)
        y = blk(xg)
        y.backward(dy)
        torch.cuda.synchronize()
    finally:
        ops.OWN_GEMM, ops.FUSED_MLP, ops.FUSED_ATTN_MODULE_TRAIN, ops.GEMM_TUNE = prev

    sh = OM.Shifter("nest_roll", N, bp, ws, shift)
    sh.idx, sh.inv = sh.idx.to(DEV), sh.inv.to(DEV)
    mask = sh.attn_mask().to(DEV, torch.float64)
    sh.attn_mask = lambda: mask
    rel = torch.from_numpy(T.rel_pos_index(ws)).to(DEV)
    xo = x.double().requires_grad_(True)
    yo = OM.swin_block(xo, sd, "", nH, ws, sh, rel, False, False)
    yo.backward(dy.double())
    tag = "stage-0 block full size, random biases, hs_gemm_nt"
    assert_close(y, yo.detach(), TOL[BF], tag + " y")
    assert_close(xg.grad, xo.grad, GRAD_TOL[BF], tag + " dx")
    assert_unbiased(xg.grad, xo.grad, tag + " dx")
    for name, p in blk.named_parameters():
        # (the relative-position table's gradient is a cancelling sum of bf16-rounded terms: the 5e-2 bound of
        # tests/test_gpu_model.py::_check_grads_own_scale for that family)
        tol = 5e-2 if name.endswith("relative_position_bias_table") else GRAD_TOL[BF]
        assert_close(p.grad, sd[name].grad, tol, f"{tag} grad {name}")
        assert_unbiased(p.grad, sd[name].grad, f"{tag} grad {name}")
