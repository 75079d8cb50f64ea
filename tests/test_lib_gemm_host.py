"""hs_lib_gemm_* on a host without a HIP device: the library loads, hs_lib_gemm_supported() answers 0 without touching hipBLASLt,
every call is refused with a status (nothing aborts), and the op layer's policy keeps the deferred add."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import _lib
    return _lib


def _host_block(nbytes=1 << 16):
    buf = ctypes.create_string_buffer(nbytes + 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_argument_refusals_need_no_device(L):
    keep, p = _host_block()
    P = ctypes.c_void_p
    a, w, c, d = P(p), P(p + 8192), P(p + 16384), P(p + 24576)
    call = L.lib.hs_lib_gemm_nt
    assert call(None, w, None, L.HS_BF16, c, d, 8, 16, 64, None) == 1 and b"NULL" in L.lib.hs_last_error()
    assert call(a, w, None, L.HS_BF16, c, None, 8, 16, 64, None) == 1
    assert call(a, w, None, L.HS_BF16, c, d, 8, 12, 64, None) == 1 and b"multiples of 8" in L.lib.hs_last_error()
    assert call(a, w, None, L.HS_BF16, c, d, 8, 16, 60, None) == 1
    assert call(a, w, None, L.HS_BF16, c, d, 0, 16, 64, None) == 1
    assert call(a, w, a, 9, c, d, 8, 16, 64, None) == 1
    assert call(a, w, None, L.HS_BF16, d, d, 8, 16, 64, None) == 1 and b"alias" in L.lib.hs_last_error()
    assert call(a, w, None, L.HS_BF16, c, a, 8, 16, 64, None) == 1
    assert call(a, w, None, L.HS_BF16, c, P(p + 8192 + 64), 8, 16, 64, None) == 1  # d inside w
    assert call(P(p + 2), w, None, L.HS_BF16, c, d, 8, 16, 64, None) == 5
    assert L.lib.hs_lib_gemm_set_pick(8, 12, 64, 1, 0) == 1 and L.lib.hs_lib_gemm_set_pick(8, 16, 64, 1, 8) == 1
    del keep


def test_without_a_device_the_path_is_off(L):
    import torch  # (first: with a device, hs_lib_gemm_supported() looks for the hipBLASLt copy PyTorch brought)
    from heal_swin_amd import ops
    if L.device_count() > 0:  # tests/test_gpu_lib_gemm.py covers the path itself
        assert L.lib.hs_lib_gemm_supported() == 1
        return
    assert L.lib.hs_lib_gemm_supported() == 0
    keep, p = _host_block()
    P = ctypes.c_void_p
    assert L.lib.hs_lib_gemm_nt(P(p), P(p + 8192), None, L.HS_BF16, P(p + 16384), P(p + 24576), 8, 16, 64, None) == 2
    assert b"not available" in L.lib.hs_last_error()
    assert L.lib.hs_lib_gemm_set_supported(1) == 0 and L.lib.hs_lib_gemm_supported() == 0  # the switch cannot conjure a device
    idx, sol, name = ctypes.c_int(7), ctypes.c_int(7), ctypes.create_string_buffer(64)
    assert L.lib.hs_lib_gemm_pick(8, 16, 64, 1, ctypes.byref(idx), ctypes.byref(sol), name, 64) == 0
    assert (idx.value, sol.value, name.value) == (-1, -1, b"none")
    assert not ops.lib_resid_ok(512, 2048, torch.bfloat16)
    del keep
