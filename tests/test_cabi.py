"""The C-ABI library loads and exports every symbol include/healswin.h declares; host-side entry points (no GPU needed)
match the golden vectors captured from the reference bit-exactly."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from _golden import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import _lib
    return _lib


def header_symbols():
    src = open(os.path.join(ROOT, "include", "healswin.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hs_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(L):
    lib = ctypes.CDLL(L.LIB_PATH)
    declared = header_symbols()
    assert len(declared) >= 20
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, missing
    # and the Python binding covers exactly the declared set
    assert sorted(L.EXPORTED_SYMBOLS) == declared


def test_depth_sum_indices_match_the_header(L):
    """depth_evaluation's NSUMS and S_* (read at every compute()) restate HS_DEPTH_NSUMS and HS_DS_* of the header."""
    from heal_swin_amd import depth_evaluation as D

    src = open(os.path.join(ROOT, "include", "healswin.h")).read()
    defines = {name: int(value) for name, value in re.findall(r"^#define (HS_DS_[A-Z0-9_]+|HS_DEPTH_NSUMS) (\d+)\b", src, flags=re.M)}
    mine = {name: getattr(D, name) for name in dir(D) if re.fullmatch(r"S_[A-Z0-9_]+", name)}
    assert len(defines) == 15 and {"HS_DS_" + name[2:]: value for name, value in mine.items()} == {
        k: v for k, v in defines.items() if k != "HS_DEPTH_NSUMS"}
    assert D.NSUMS == defines["HS_DEPTH_NSUMS"] == D.S_RANGE + 2 * D.MAX_RANGES


def test_version_and_status_strings(L):
    assert "gfx950" in L.version()
    assert L.lib.hs_status_string(0) == b"ok"
    assert L.device_count() >= 0


def test_host_tables_match_golden(L):
    z = load("tables")
    for ws in (4, 16, 64, 256):
        assert np.array_equal(L.nest_win_idcs(ws), z[f"nest_win_idcs/{ws}"])
    for ws in (4, 16, 64):
        assert np.array_equal(L.rel_pos_index(ws), z[f"rel_pos_index/{ws}"].astype(np.int64))
    for (n, ws, s) in ((64, 16, 8), (1024, 16, 8), (2048, 64, 32), (512, 4, 2)):
        idx, inv, lab = L.build_nest_roll_shift(n, ws, s)
        assert np.array_equal(idx, z[f"nest_roll/{n}_{ws}_{s}/idx"]) and np.array_equal(inv, z[f"nest_roll/{n}_{ws}_{s}/inv"])
        assert sha(L.attn_mask_from_labels(lab, ws)) == str(z[f"nest_roll/{n}_{ws}_{s}/mask_sha"])
    for ns in (4, 8, 16, 32, 64, 128):
        for ws in (16, 64):
            if ws > ns * ns:
                continue
            idx, inv, lab = L.build_nest_grid_shift(ns, 8, ws)
            h = [str(x) for x in z[f"nest_grid/{ns}_{ws}/sha"]]
            assert [sha(idx.astype(np.int64)), sha(inv.astype(np.int64)), sha(lab.astype(np.int64))] == h[:3]
            assert sha(L.attn_mask_from_labels(lab, ws)) == h[3]
            for s in (4, ws // 2):
                idx, inv, lab = L.build_ring_shift(ns, 8, ws, s)
                h = [str(x) for x in z[f"ring/{ns}_{ws}_{s}/sha"]]
                assert [sha(idx.astype(np.int64)), sha(inv.astype(np.int64)), sha(lab.astype(np.int64))] == h[:3]
                assert sha(L.attn_mask_from_labels(lab, ws).astype(np.int64)) == h[3]


def test_healpix_known_answers_via_cabi(L):
    assert L.nest2ring(2, np.arange(10)).tolist() == [13, 5, 4, 0, 15, 7, 6, 1, 17, 9]
    assert L.ring2nest(2, np.arange(10)).tolist() == [3, 7, 11, 15, 2, 1, 6, 5, 10, 9]
    assert int(L.nest2ring(16, [1130])[0]) == 1504 and int(L.ring2nest(16, [1504])[0]) == 1130
    for ns in (1, 4, 64, 256):
        a = np.arange(12 * ns * ns)
        assert np.array_equal(L.ring2nest(ns, L.nest2ring(ns, a)), a)


def test_error_conventions(L):
    with pytest.raises(AssertionError):  # reference: assert base_pix == 8 (hp_shifting.py:78)
        L.build_nest_grid_shift(8, 12, 16)
    with pytest.raises(AssertionError):
        L.build_ring_shift(8, 4, 16, 4)
    with pytest.raises(AssertionError):
        L.nest2ring(3, [0])
    with pytest.raises(AssertionError):
        L.nest_win_idcs(8)  # not 4^k
    # device entry points fail loudly (no silent CPU fallback): no device in this container, or bad arguments
    st = L.lib.hs_layernorm_fwd(None, None, None, None, None, None, None, 4, 8, 0, None)
    assert st != 0 and L.lib.hs_last_error()


def _scratch(L, nbytes=4 << 20):
    """(keep-alive, address) of 4 MiB every pointer of a refused call may name: on the device where there is one, else on the host
    (16-byte aligned either way).  A refusal reads none of it."""
    if L.device_count() > 0:
        import torch
        t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        return t, t.data_ptr()
    buf = ctypes.create_string_buffer(nbytes + 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _patch_calls(L, p, shape, kind, accumulate=0):
    """(forward status, backward status) of a patch operator with every pointer at `p`"""
    P = ctypes.c_void_p(p)
    if kind == "merge":
        return (L.lib.hs_patch_merge_fwd(*[P] * 8, *shape, L.HS_BF16, None), L.lib.hs_patch_merge_bwd(*[P] * 13, accumulate, *shape, L.HS_BF16, None))
    return (L.lib.hs_patch_expand_fwd(*[P] * 8, *shape, L.HS_BF16, None), L.lib.hs_patch_expand_bwd(*[P] * 13, accumulate, *shape, L.HS_BF16, None))


def _chain_call(L, p, accumulate=0, n_tokens=128, roll=0, C=96):
    P = ctypes.c_void_p(p)
    return L.lib.hs_window_attn_module_bwd_chain(*[P] * 14, roll, *[P] * 11, accumulate, 1, n_tokens, C, C // 32, 64, L.HS_ATTN_RESIDUAL, L.HS_BF16, None)


def test_operator_backwards_refuse_a_deferring_accumulate(L):
    """hs_patch_merge_bwd, hs_patch_expand_bwd and hs_window_attn_module_bwd_chain chain kernels that share one workspace, so they
    take accumulate = 0 / 1 only: HS_ACC_DEFER (2, 3) and anything else is HS_ERR_INVALID_ARG, decided on the host."""
    keep, p = _scratch(L)
    for accumulate in (2, 3, -1, 4):
        for st in (_patch_calls(L, p, (64, 32, 64), "merge", accumulate)[1], _patch_calls(L, p, (64, 64, 128, 4), "expand", accumulate)[1],
                   _chain_call(L, p, accumulate)):
            msg = L.lib.hs_last_error().decode()
            assert st == 1 and "accumulate must be 0" in msg and "HS_ACC_DEFER" in msg, (accumulate, st, msg)
    assert L.lib.hs_reduce_pending(None) == 0
    del keep


def test_operator_forward_and_backward_refuse_the_same_shapes(L):
    """What one chained kernel would refuse is refused by both directions, with one status, before the first launch."""
    keep, p = _scratch(L)
    for kind, shape in (("merge", (16, 6, 12)),        # backward hs_gemm_nt: k = dim_out = 12
                        ("merge", (16, 8, 20)),
                        ("merge", (16, 7, 16)),        # odd dim (the reference's 4-sibling view needs none, the 16-byte rows do)
                        ("merge", (4, 1026, 16)),      # LayerNorm over 4104 > 4096 columns
                        ("expand", (16, 8, 12, 4)),    # backward hs_gemm_nt: k = dim_exp = 12
                        ("expand", (16, 12, 24, 4)),   # forward hs_gemm_nt: k = dim = 12
                        ("expand", (16, 8, 24, 5)),    # children does not divide dim_exp
                        ("expand", (4, 8, 8240, 8))):  # LayerNorm over 1030 columns: no multiple of 8 and > 1024
        for accumulate in (0, 1):
            st_f, st_b = _patch_calls(L, p, shape, kind, accumulate)
            assert st_f == st_b and st_f in (1, 2), (kind, shape, st_f, st_b, L.lib.hs_last_error())
    for kw in (dict(n_tokens=96), dict(roll=128), dict(roll=-1), dict(n_tokens=0), dict(C=64)):
        assert _chain_call(L, p, **kw) in (1, 2), kw
    del keep


def test_model_mirrors_reference_surface(L):
    import torch
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch import hp_shifting, hp_windowing
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys
    from _golden import MODEL_CASES, case, model_cfg_spec, state_dict

    for name in MODEL_CASES:
        cfg, spec = model_cfg_spec(name)
        m = SwinHPTransformerSys(SwinHPTransformerConfig(**cfg), DataSpec(**spec))
        ref = state_dict(case("models", "model/" + name))
        mine = m.state_dict()
        assert set(mine) == set(ref)
        for k, v in ref.items():
            assert mine[k].shape == v.shape and mine[k].dtype == v.dtype, k
            if k.endswith(("attn_mask", "relative_position_index")):
                assert torch.equal(mine[k], v), k
        m.load_state_dict(ref, strict=True)
    assert m.no_weight_decay() == {"absolute_pos_embed"} and m.no_weight_decay_keywords() == {"relative_position_bias_table"}
    c = SwinHPTransformerConfig()
    assert (c.patch_size, c.window_size, c.shift_size, c.shift_strategy, c.embed_dim, c.drop_path_rate) == (4, 4, 2, "nest_roll", 96, 0.1)
    # views and tables of hp_windowing
    x = torch.arange(2 * 32 * 3).reshape(2, 32, 3)
    w = hp_windowing.window_partition(x, 16)
    assert w.shape == (4, 16, 3) and torch.equal(hp_windowing.window_reverse(w, 16, 32), x)
    assert hp_windowing.get_nest_win_idcs(16).tolist() == [[5, 4, 1, 0], [7, 6, 3, 2], [13, 12, 9, 8], [15, 14, 11, 10]]
    with pytest.raises(AssertionError):
        hp_windowing.window_partition(x, 12)
    assert hp_shifting.NoShift().get_mask() is None
    # the product refuses CPU tensors instead of falling back
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, spec["dim_in"]))
