"""The host side of weight averaging (csrc/weight_avg.hip, optim.FlatWeightAverage): the three entry points are bound and refuse bad
arguments with HS_ERR_INVALID_ARG (1) before anything is launched, as the Adam entry points do, and the constructor refuses what it
cannot average.  No GPU needed; that the header and the binding agree is test_cabi's."""
import ctypes

import pytest

N = 1024


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def scratch():
    """(keep-alive, a 16-byte aligned host address): a refusal reads none of it"""
    buf = ctypes.create_string_buffer(8 * N + 32)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _refused(L, st, what):
    msg = L.lib.hs_last_error().decode()
    assert st == 1, (what, st, msg)
    assert msg.startswith("hs_weight_avg_"), (what, msg)
    return msg


def test_entry_points_are_bound(L):
    for name in ("hs_weight_avg_update", "hs_weight_avg_advance", "hs_weight_avg_swap"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.lib, name), name


def test_update_refuses_bad_arguments(L, scratch):
    _, base = scratch
    P, Q, C = ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * N), ctypes.c_void_p(base + 8 * N)
    up = L.lib.hs_weight_avg_update
    good = dict(avg=P, p=Q, n=N, kind=0, decay=0.5, count=C, guard=None, skip=0)

    def call(**kw):
        a = dict(good, **kw)
        return up(a["avg"], a["p"], a["n"], a["kind"], a["decay"], a["count"], a["guard"], a["skip"], None)
    for name in ("avg", "p", "count"):
        assert "null pointer" in _refused(L, call(**{name: None}), f"null {name}")
    for n in (0, -1, 1 << 40):
        assert "length" in _refused(L, call(n=n), f"n = {n}")
    for kind in (2, -1):
        assert "kind" in _refused(L, call(kind=kind), f"kind = {kind}")
    for decay in (1.5, -0.1, float("nan")):
        assert "decay" in _refused(L, call(decay=decay), f"decay = {decay}")
    for off in (4, 8, 12, 1):
        assert "aligned" in _refused(L, call(avg=ctypes.c_void_p(base + off)), f"avg + {off}")
        assert "aligned" in _refused(L, call(p=ctypes.c_void_p(base + 4 * N + off)), f"p + {off}")
    assert "alignment" in _refused(L, call(count=ctypes.c_void_p(base + 8 * N + 4)), "n_averaged + 4")


def test_advance_refuses_bad_arguments(L, scratch):
    _, base = scratch
    adv = L.lib.hs_weight_avg_advance
    assert "null pointer" in _refused(L, adv(None, None, 0, None), "null n_averaged")
    assert "null pointer" in _refused(L, adv(None, ctypes.c_void_p(base), 1, None), "null n_averaged with a guard")
    assert "alignment" in _refused(L, adv(ctypes.c_void_p(base + 4), None, 0, None), "n_averaged + 4")
    assert "alignment" in _refused(L, adv(ctypes.c_void_p(base), ctypes.c_void_p(base + 18), 1, None), "guard + 2")


def test_swap_refuses_bad_arguments(L, scratch):
    _, base = scratch
    P, Q = ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * N)
    swap = L.lib.hs_weight_avg_swap
    assert "null pointer" in _refused(L, swap(None, Q, None, N, None), "null p")
    assert "null pointer" in _refused(L, swap(P, None, None, N, None), "null avg")
    for n in (0, -5, 1 << 40):
        assert "length" in _refused(L, swap(P, Q, None, n, None), f"n = {n}")
    for off in (4, 8, 1):
        assert "aligned" in _refused(L, swap(P, ctypes.c_void_p(base + 4 * N + off), None, N, None), f"avg + {off}")
        assert "aligned" in _refused(L, swap(ctypes.c_void_p(base + off), Q, None, N, None), f"p + {off}")
    assert "aligned" in _refused(L, swap(P, Q, ctypes.c_void_p(base + 8 * N + 4), N, None), "p_bf16 + 4")
    assert "same buffer" in _refused(L, swap(P, P, None, N, None), "p is avg")


def test_constructor_refusals_that_need_no_device(L):
    import torch
    from heal_swin_amd import optim
    params = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="FlatAdam"):
        optim.FlatWeightAverage(torch.optim.Adam(params, lr=1e-3), "swa")
    # kind and decay are looked at once the optimizer is known to be a FlatAdam: one that was never initialised is enough for that
    fake = optim.FlatAdam.__new__(optim.FlatAdam)
    with pytest.raises(ValueError, match="kind"):
        optim.FlatWeightAverage(fake, "polyak")
    for decay in (-0.01, 1.5):
        with pytest.raises(ValueError, match="decay"):
            optim.FlatWeightAverage(fake, "ema", decay=decay)
