"""Host-side checks of the depth step on the decoder tail (no GPU needed): `hs_expand_ln_head_depth_step_fwd` is declared, exported
and bound and refuses bad arguments before any launch, and both models have `forward_depth_step`, whose argument errors are raised
before any device work."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "hs_expand_ln_head_depth_step_fwd"


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import _lib
    return _lib


def test_symbol_is_declared_exported_and_bound(L):
    src = open(os.path.join(ROOT, "include", "healswin.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(L.LIB_PATH), SYMBOL)
    assert SYMBOL in L.EXPORTED_SYMBOLS and hasattr(L.lib, SYMBOL)


def _call(L, xn=16, target=16, parts=16, kind=1, delta=1.0, n_out=1, flags=0, transform=0, use_logvar=0, ranges=None, n_ranges=0,
          mparts=16, state=16, preds=16, logvar=None, tokens=64, width=128):
    # the non-null pointers are never dereferenced: every case below is refused before the launch
    rng = (ctypes.c_float * 32)() if ranges is None else ranges
    return L.lib.hs_expand_ln_head_depth_step_fwd(xn, None, 16, 16, 16, target, kind, delta, n_out, None, None, None, None, parts, flags,
                                                  transform, 0.0, 1.0, use_logvar, 0.0, ctypes.addressof(rng), n_ranges, mparts, state, preds,
                                                  logvar, tokens, width, 4, L.HS_BF16, None)


def test_argument_errors_are_refused_before_any_launch(L):
    INVALID, UNSUPPORTED, MISALIGNED = 1, 2, _misaligned_code()
    assert _call(L, xn=None) == INVALID
    assert _call(L, target=None) == INVALID
    assert _call(L, parts=None) == INVALID
    assert _call(L, tokens=0) == INVALID
    # depth_head_ok: an unknown kind, Huber on two channels or with delta <= 0, the log variance on one channel, three channels
    assert _call(L, kind=9) == INVALID
    assert _call(L, kind=2, n_out=2) == INVALID
    assert _call(L, kind=2, delta=0.0) == INVALID
    assert _call(L, kind=3, n_out=1) == INVALID
    assert _call(L, kind=0, n_out=3) == INVALID
    assert _call(L, n_ranges=9) == INVALID  # more than 8 ranges
    assert _call(L, n_ranges=-1) == INVALID
    assert _call(L, transform=3) == INVALID
    assert _call(L, flags=1) == INVALID  # the forward chain's background flags have no meaning here
    assert _call(L, state=None) == INVALID and _call(L, mparts=None) == INVALID  # records and state go together
    assert _call(L, use_logvar=1, n_out=1) == INVALID and _call(L, logvar=16, n_out=1) == INVALID  # no channel 1 to read
    assert _call(L, preds=8) == MISALIGNED  # the 4 children of a token leave as one 16-byte store
    assert _call(L, logvar=24, n_out=2) == MISALIGNED
    assert _call(L, state=12) == MISALIGNED
    assert _call(L, xn=6) == MISALIGNED
    assert _call(L, width=160) == UNSUPPORTED  # as the other tail entry points


def _misaligned_code():
    src = open(os.path.join(ROOT, "include", "healswin.h")).read()
    return int(re.search(r"HS_ERR_MISALIGNED\s*=?\s*(\d+)", src).group(1))


def test_both_models_have_forward_depth_step():
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerSys
    from heal_swin_amd.models_torch.swin_transformer import SwinTransformerSys
    for cls in (SwinHPTransformerSys, SwinTransformerSys):
        assert callable(getattr(cls, "forward_depth_step", None)), cls
    from heal_swin_amd import losses, ops
    assert callable(ops.expand_ln_head_depth_step) and callable(losses.depth_step_from_rows)


def _tiny_models(f_out):
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys
    from heal_swin_amd.models_torch.swin_transformer import SwinTransformerConfig, SwinTransformerSys
    hp = SwinHPTransformerSys(SwinHPTransformerConfig(patch_size=4, window_size=4, shift_size=2, embed_dim=16, depths=[2, 2], num_heads=[2, 4]),
                              DataSpec(dim_in=8 * 8 * 8, f_in=3, f_out=f_out, base_pix=8, class_names=[]))
    flat = SwinTransformerSys(SwinTransformerConfig(patch_size=2, window_size=4, shift_size=2, embed_dim=16, depths=[2, 2], num_heads=[2, 4]),
                              DataSpec(dim_in=(32, 32), f_in=3, f_out=f_out, base_pix=None, class_names=[]))
    return (hp, torch.zeros(1, 3, 8 * 8 * 8), torch.zeros(1, 8 * 8 * 8)), (flat, torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 32))


def test_argument_errors_are_raised_before_any_device_work():
    from heal_swin_amd.depth_data import DepthTargetTransform
    from heal_swin_amd.depth_evaluation import DepthMetrics
    tr = DepthTargetTransform("log", "standardize")
    assert tr.inverse_op()[0] == 8 | 4 and DepthTargetTransform().inverse_op() == (8, 0, 0.0, 1.0)
    for model, x, target in _tiny_models(1):
        with pytest.raises(ValueError, match="use_logvar needs a two-channel head"):
            model.forward_depth_step(x, target, metrics=DepthMetrics(use_logvar=True, device="cpu"))
        with pytest.raises(AssertionError, match="two channels"):  # the log-variance loss, as forward_depth_loss refuses it
            model.forward_depth_step(x, target, use_logvar=True)
        with pytest.raises(ValueError, match="metrics live on meta"):
            model.forward_depth_step(x, target, metrics=DepthMetrics(device="meta"))
        with pytest.raises(TypeError, match="DepthTargetTransform"):
            model.forward_depth_step(x, target, transform="log")
        with pytest.raises(TypeError, match="DepthMetrics"):
            model.forward_depth_step(x, target, metrics=object())
        with pytest.raises(ValueError, match="depth loss must be"):
            model.forward_depth_step(x, target, loss="l3")
        with pytest.raises(RuntimeError, match="no CPU path"):  # good arguments pass the checks; the model itself needs the GPU
            model.forward_depth_step(x, target, "l1", transform=tr, metrics=DepthMetrics(device="cpu"))
    for model, x, target in _tiny_models(2):
        with pytest.raises(AssertionError, match="one-channel"):  # Huber on two channels
            model.forward_depth_step(x, target, "huber")
        with pytest.raises(RuntimeError, match="no CPU path"):
            model.forward_depth_step(x, target, use_logvar=True, metrics=DepthMetrics(use_logvar=True, device="cpu"))
