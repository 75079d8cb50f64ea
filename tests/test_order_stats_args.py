"""Host-side checks of the order statistics and the depth histogram (no GPU needed): the Python layer raises on bad arguments
before any device work, there is no CPU path, and the C entry points refuse null and invalid arguments with a message."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import _lib
    return _lib


def test_row_kth_value_argument_errors_and_no_cpu_path(L):
    from heal_swin_amd.order_stats import row_kth_value, row_median
    x = torch.zeros(3, 8)
    with pytest.raises(TypeError, match="float32"):
        row_kth_value(x.double(), 0)
    with pytest.raises(TypeError, match="float32"):
        row_median(x.bfloat16())
    with pytest.raises(TypeError, match="float32"):
        row_kth_value([[1.0, 2.0]], 0)
    for k in (-1, 8, 2 ** 31):
        with pytest.raises(ValueError, match="k must be in"):
            row_kth_value(x, k)
    with pytest.raises(ValueError, match="unit inner stride"):
        row_kth_value(torch.zeros(8, 3).t(), 0)
    with pytest.raises(ValueError, match="unit inner stride"):
        row_median(torch.zeros(3, 16)[:, ::2])
    with pytest.raises(ValueError, match=r"\[rows, n\]"):
        row_kth_value(torch.zeros(8), 0)
    with pytest.raises(ValueError, match="overlap"):
        row_kth_value(torch.zeros(8).expand(3, 8), 0)
    with pytest.raises(ValueError, match="between 1 and"):
        row_median(torch.zeros(3, 0))
    with pytest.raises(ValueError, match="splits"):
        row_kth_value(x, 0, splits=-1)
    with pytest.raises(TypeError, match="out"):
        row_kth_value(x, 0, out=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="out"):
        row_kth_value(x, 0, out=torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        row_kth_value(x, 3)


def test_depth_histogram_argument_errors(L):
    from heal_swin_amd.depth_data import DepthHistogram
    for bins in (0, -3, L.HS_HISTOGRAM_MAX_BINS + 1):
        with pytest.raises(ValueError, match="bins must be in"):
            DepthHistogram(bins, (0.0, 1.0))
    with pytest.raises(TypeError, match="integer"):
        DepthHistogram([0.0, 0.5, 1.0], (0.0, 1.0))
    with pytest.raises(ValueError, match="range"):
        DepthHistogram(10)
    with pytest.raises(ValueError):
        DepthHistogram(10, (1.0, 0.0))  # numpy's own refusal
    with pytest.raises(ValueError, match="data_transform"):
        DepthHistogram(10, (0.0, 1.0), data_transform="sqrt")
    with pytest.raises(RuntimeError, match="GPU only"):
        DepthHistogram(10, (0.0, 1.0), device="cpu")


def test_select_and_histogram_entry_points_refuse_on_the_host(L):
    lib = ctypes.CDLL(L.LIB_PATH)
    for s in ("hs_select_rows", "hs_select_rows_workspace", "hs_histogram_update"):
        assert hasattr(lib, s) and s in L.EXPORTED_SYMBOLS, s
    assert L.HS_HISTOGRAM_MAX_BINS == 4096
    ws = L.lib.hs_select_rows_workspace
    assert ws(0) == 0 and ws(-1) == 0 and ws(1) == (4 * 256 + 1) * 4 and ws(8) == 8 * ws(1)

    def refused(status, word):
        msg = L.lib.hs_last_error().decode()
        assert status == 1 and word in msg, (status, msg, word)

    P = 64  # any non-null address: a refusal reads nothing
    sel = L.lib.hs_select_rows
    refused(sel(None, 1, 8, 8, 0, 0, 0, P, P, None), "null")
    refused(sel(P, 1, 8, 8, 0, 0, 0, None, P, None), "null")
    refused(sel(P, 1, 8, 8, 0, 0, 0, P, None, None), "null")
    refused(sel(P, 0, 8, 8, 0, 0, 0, P, P, None), "rows")
    refused(sel(P, 65536, 8, 8, 0, 0, 0, P, P, None), "rows")
    refused(sel(P, 1, 0, 8, 0, 0, 0, P, P, None), "n ")
    refused(sel(P, 1, 2 ** 31, 2 ** 31, 0, 0, 0, P, P, None), "n ")
    refused(sel(P, 1, 8, 8, 8, 0, 0, P, P, None), "k ")
    refused(sel(P, 1, 8, 8, -1, 0, 0, P, P, None), "k ")
    refused(sel(P, 2, 8, 7, 0, 0, 0, P, P, None), "row_stride")
    refused(sel(P, 1, 8, 8, 0, 0, -1, P, P, None), "splits")
    refused(sel(P + 2, 1, 8, 8, 0, 0, 0, P, P, None), "aligned")
    hist = L.lib.hs_histogram_update
    refused(hist(None, 8, L.HS_DT_NONE, 0, P, 10, P, None), "null")
    refused(hist(P, 8, L.HS_DT_NONE, 0, None, 10, P, None), "null")
    refused(hist(P, 8, L.HS_DT_NONE, 0, P, 10, None, None), "null")
    refused(hist(P, 8, L.HS_DT_NONE, 0, P, 0, P, None), "bins")
    refused(hist(P, 8, L.HS_DT_NONE, 0, P, 4097, P, None), "bins")
    refused(hist(P, 8, 7, 0, P, 10, P, None), "transform")
    refused(hist(P, -1, L.HS_DT_NONE, 0, P, 10, P, None), "size")
    assert hist(None, 0, L.HS_DT_NONE, 0, None, 10, None, None) == 0  # nothing to add
