"""Host-side checks of the fused depth losses (no GPU needed): the kind selection of losses.depth_loss_spec follows
get_depth_loss, argument errors are raised before any device work, there is no CPU fallback, and the C ABI exports the
depth-loss entry points."""
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch


def test_depth_loss_spec_selects_as_get_depth_loss():
    from heal_swin_amd.losses import DEPTH_KINDS, depth_loss_spec
    assert depth_loss_spec() == (DEPTH_KINDS["l2"], 1.0)
    assert depth_loss_spec("l1") == (DEPTH_KINDS["l1"], 1.0)
    assert depth_loss_spec("huber", huber_delta=0.3) == (DEPTH_KINDS["huber"], 0.3)
    assert depth_loss_spec("huber", use_logvar=True)[0] == DEPTH_KINDS["logvar"]  # use_logvar wins, as in get_depth_loss
    assert depth_loss_spec(NS(use_logvar=False, loss="huber", huber_delta=2.0)) == (DEPTH_KINDS["huber"], 2.0)
    assert depth_loss_spec(NS(use_logvar=True, loss="l1", huber_delta=1.0))[0] == DEPTH_KINDS["logvar"]
    with pytest.raises(ValueError, match="'l1', 'l2' or 'huber'"):
        depth_loss_spec("mse")
    with pytest.raises(ValueError, match="positive"):
        depth_loss_spec("huber", huber_delta=0.0)


def test_depth_loss_kinds_match_the_c_header():
    import os
    import re
    from heal_swin_amd.losses import DEPTH_KINDS
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "healswin.h")).read()
    found = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define HS_DEPTH_(L1|L2|HUBER|LOGVAR) (\d+)", src)}
    assert found == DEPTH_KINDS


def test_depth_loss_argument_errors_and_no_cpu_path():
    from heal_swin_amd.losses import depth_loss
    p1, p2, t = torch.zeros(1, 1, 8), torch.zeros(1, 2, 8), torch.zeros(1, 8)
    with pytest.raises(AssertionError, match="one-channel"):
        depth_loss(p2, t, loss="huber")
    with pytest.raises(AssertionError, match="two channels"):
        depth_loss(p1, t, use_logvar=True)
    with pytest.raises(AssertionError, match=r"target \[B, Npix\]"):
        depth_loss(p1, torch.zeros(1, 9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        depth_loss(p1, t, loss="l1")


def test_depth_loss_symbols_are_exported():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("hs_depth_loss_partials", "hs_depth_loss_fwd", "hs_depth_loss_bwd", "hs_expand_ln_head_depth_fwd", "hs_ln_head_depth_bwd"):
        assert hasattr(lib, s) and s in _lib.EXPORTED_SYMBOLS, s
    assert _lib.lib.hs_depth_loss_partials(2, 1000) == 8
    assert _lib.lib.hs_depth_loss_partials(0, 1000) == 0
    # invalid arguments are refused on the host (no launch): an unknown kind, Huber on two channels, null pointers
    assert _lib.lib.hs_depth_loss_fwd(None, None, None, 1, 8, 1, 8, 8, 1, 0, 1.0, _lib.HS_F32, None) != 0
    assert _lib.lib.hs_depth_loss_fwd(8, 8, 8, 1, 8, 1, 8, 8, 1, 9, 1.0, _lib.HS_F32, None) != 0
    assert _lib.lib.hs_depth_loss_fwd(8, 8, 8, 1, 8, 2, 16, 8, 1, 2, 1.0, _lib.HS_F32, None) != 0
    assert _lib.lib.hs_expand_ln_head_depth_fwd(8, None, 8, 8, 8, 8, 3, 1.0, 1, None, None, None, None, 8, 4, 64, 4, _lib.HS_BF16, None) != 0
    assert _lib.lib.hs_ln_head_depth_bwd(8, 8, 8, 8, 2, 1.0, 8, 2, 8, 8, 8, 8, 8, 8, 16, 64, _lib.HS_BF16, None) != 0
