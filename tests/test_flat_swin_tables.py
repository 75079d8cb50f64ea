"""Host tables of the flat Swin-UNet (csrc/flat_tables.cpp) and the module's construction, against the reference's own windows,
masks, relative-position index and state-dict layout (tests/golden/flat_swin.npz).  CPU only."""
import hashlib
import json

import numpy as np
import pytest
import torch

from _flat_cases import FLAT_TABLE_CASES, PAPER_CFG, PAPER_SPEC
from _golden import load


def _tile(Ht, Wt, w):
    T = w
    while Ht % (2 * T) == 0 and Wt % (2 * T) == 0:
        T *= 2
    return T


def _compact(v):
    v = v & 0x55555555
    v = (v | (v >> 1)) & 0x33333333
    v = (v | (v >> 2)) & 0x0F0F0F0F
    v = (v | (v >> 4)) & 0x00FF00FF
    return (v | (v >> 8)) & 0x0000FFFF


@pytest.mark.parametrize("Ht,Wt,T", [(8, 12, 4), (16, 24, 8), (32, 64, 32), (320, 384, 64), (4, 4, 2)])
def test_zorder_is_bijection_with_morton_tiles(Ht, Wt, T):
    from heal_swin_amd import _lib
    z_of_rm, rm_of_z = _lib.flat_zorder(Ht, Wt, T)
    assert np.array_equal(np.sort(z_of_rm), np.arange(Ht * Wt))
    assert np.array_equal(rm_of_z[z_of_rm], np.arange(Ht * Wt))
    z = np.arange(Ht * Wt)
    tile, m = z // (T * T), z % (T * T)
    h = (tile // (Wt // T)) * T + _compact(m)
    w = (tile % (Wt // T)) * T + _compact(m >> 1)
    assert np.array_equal(rm_of_z, h * Wt + w)
    # the reference's PatchMerging concat order (0::2,0::2), (1::2,0::2), (0::2,1::2), (1::2,1::2): 4 consecutive tokens
    hh, ww = rm_of_z // Wt, rm_of_z % Wt
    q = np.arange(0, Ht * Wt, 4)
    for k, (dr, dc) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
        assert np.array_equal(hh[q + k], hh[q] + dr) and np.array_equal(ww[q + k], ww[q] + dc)


@pytest.mark.parametrize("Ht,Wt,w,s", FLAT_TABLE_CASES)
def test_shift_tables_reproduce_reference_windows_and_mask(Ht, Wt, w, s):
    from heal_swin_amd import _lib
    g = load("flat_swin")
    key = f"table/{Ht}x{Wt}_w{w}_s{s}"
    T = _tile(Ht, Wt, w)
    idx, inv, lab = _lib.build_flat_shift(Ht, Wt, T, w, s)
    assert np.array_equal(inv[idx], np.arange(Ht * Wt))
    _, rm_of_z = _lib.flat_zorder(Ht, Wt, T)
    cell = rm_of_z  # shifted-frame cell of every Z position
    h, x = cell // Wt, cell % Wt
    ref_win = (h // w) * (Wt // w) + x // w
    ref_pos = (h % w) * w + x % w
    windows = g[key + "/windows"]
    # content: shifted position j holds the token the reference puts at (window, position)
    assert np.array_equal(windows[ref_win, ref_pos], rm_of_z[idx])
    # every window is w*w consecutive Z positions, in-window order = Morton with the row bit least significant
    j = np.arange(Ht * Wt)
    assert np.array_equal(ref_win.reshape(-1, w * w), np.repeat(ref_win[::w * w], w * w).reshape(-1, w * w))
    loc = j % (w * w)
    assert np.array_equal(ref_pos, _compact(loc) * w + _compact(loc >> 1))
    # mask: labels differ -> -100, for every entry of the reference's dense mask (hash) and of our own dense buffer
    n = w * w
    ours = np.zeros(tuple(g[key + "/mask_shape"]), np.float32)
    lw = lab.reshape(-1, n)
    pw = ref_pos.reshape(-1, n)
    for k, win in enumerate(ref_win[::n]):
        m = np.where(lw[k][:, None] != lw[k][None, :], -100.0, 0.0).astype(np.float32)
        ours[win][np.ix_(pw[k], pw[k])] = m
    assert hashlib.sha256(ours.tobytes()).hexdigest() == str(g[key + "/mask_sha"])
    dense = _lib.flat_attn_mask(Ht, Wt, w, s)
    assert np.array_equal(dense, ours)
    nz = g[key + "/mask_nonzero_windows"]
    assert np.array_equal(np.flatnonzero(dense.reshape(dense.shape[0], -1).any(1)), nz)
    assert np.array_equal(dense[nz[0]], g[key + "/mask_first_nonzero"].astype(np.float32))


@pytest.mark.parametrize("w", [2, 4, 8, 16])
def test_rel_pos_index(w):
    from heal_swin_amd import _lib
    rm, z = _lib.flat_rel_pos_index(w)
    assert np.array_equal(rm, load("flat_swin")[f"relpos/{w}"].astype(np.int64))
    pos = _compact(np.arange(w * w)) * w + _compact(np.arange(w * w) >> 1)  # row-major position of each Z position
    assert np.array_equal(z, rm[np.ix_(pos, pos)])


def _build(cfg, spec):
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_transformer import SwinTransformerConfig, SwinTransformerSys
    return SwinTransformerSys(SwinTransformerConfig(**cfg), DataSpec(**spec))


def test_paper_model_state_dict_layout():
    ref = json.loads(str(load("flat_swin")["paper/keys"]))
    sd = _build(dict(PAPER_CFG), dict(PAPER_SPEC)).state_dict()
    got = {k: [list(v.shape), str(v.dtype)] for k, v in sd.items()}
    assert set(got) == {k for k, _, _ in ref}
    for k, shape, dtype in ref:
        assert got[k] == [shape, dtype], k


def test_paper_model_buffers_match_reference_rules():
    m = _build(dict(PAPER_CFG), dict(PAPER_SPEC))
    blk = m.layers[0].blocks[1]
    assert blk._shifted and blk.window_size == 64 and blk.shift_size == 2
    last = m.layers[3].blocks[1]  # 20 x 24 tokens: no clamp at window 8
    assert last._shifted
    assert torch.equal(m.layers[0].blocks[0].attn.relative_position_index,
                       torch.from_numpy(load("flat_swin")["relpos/8"].astype(np.int64)))


SPEC = dict(dim_in=(64, 64), f_in=3, f_out=4, base_pix=None, class_names=[])


@pytest.mark.parametrize("cfg,what", [
    (dict(window_size=(4, 8), patch_size=2, depths=[2, 2], num_heads=[1, 2], embed_dim=16), "square"),
    (dict(window_size=6, patch_size=2, depths=[1], num_heads=[1], embed_dim=16, _dim_in=(48, 48)), "w\\^2"),
    (dict(window_size=4, patch_size=(2, 4), depths=[1], num_heads=[1], embed_dim=16), "patch"),
    (dict(window_size=4, patch_size=2, shift_size=(1, 2), depths=[2], num_heads=[1], embed_dim=16), "shift"),
    (dict(window_size=4, patch_size=2, depths=[2, 2], num_heads=[1, 2], embed_dim=16, final_upsample="other"), "final_upsample"),
])
def test_unsupported_configs_raise_not_implemented(cfg, what):
    cfg = dict(cfg)
    spec = dict(SPEC, dim_in=cfg.pop("_dim_in", SPEC["dim_in"]))
    with pytest.raises(NotImplementedError, match=what):
        _build(cfg, spec)


def test_non_square_clamped_window_raises_not_implemented():
    # 3 stages, window 8 at 64 x 128: the last stage is 8 x 16 tokens, the reference clamps the window to that (non-square) size
    spec = dict(SPEC, dim_in=(64, 128))
    with pytest.raises(NotImplementedError, match="clamping"):
        _build(dict(window_size=8, patch_size=2, depths=[2, 2, 2], num_heads=[1, 2, 4], embed_dim=32), spec)


@pytest.mark.parametrize("dim_in,cfg", [
    ((60, 64), dict(window_size=4, patch_size=2, depths=[2, 2], num_heads=[1, 2], embed_dim=16)),
    ((64, 72), dict(window_size=8, patch_size=2, depths=[2, 2], num_heads=[1, 2], embed_dim=16)),
    ((64, 64), dict(window_size=4, patch_size=2, shift_size=4, depths=[2, 2], num_heads=[1, 2], embed_dim=16)),
])
def test_reference_invalid_sizes_raise_assertion(dim_in, cfg):
    with pytest.raises(AssertionError):
        _build(cfg, dict(SPEC, dim_in=dim_in))


def test_golden_cases_build_with_reference_buffers():
    from _flat_cases import FLAT_MODEL_CASES, flat_cfg_spec
    g = load("flat_swin")
    for name in FLAT_MODEL_CASES:
        cfg, spec = flat_cfg_spec(name)
        sd = _build(cfg, spec).state_dict()
        pre = f"model/{name}/buf/"
        bufs = {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}
        assert bufs and set(bufs) == {k for k in sd if k.endswith(("attn_mask", "relative_position_index"))}, name
        for k, a in bufs.items():
            assert np.array_equal(sd[k].numpy(), a.astype(sd[k].numpy().dtype)), (name, k)
