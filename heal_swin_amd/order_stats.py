"""Order statistics of the rows of a matrix on the GPU, exact, without a sort and with every row split over the chip
(`hs_select_rows`, csrc/select.hip).

  row_kth_value(x, k)     the k-th smallest (0-based) element of every row, in torch.sort's order: -inf < finite < +inf < NaN,
                          -0.0 == +0.0 (either may come back).  nan_propagates=False is torch.kthvalue's rule (NaNs take the top
                          ranks), nan_propagates=True torch.median's (a row with a NaN gives NaN).
  row_median(x)           the lower median, k = (n - 1) // 2, with NaN propagation: x.median(1).values, bit for bit.

x: float32 [rows, n] on the GPU with stride(1) == 1 and any row stride >= n (rows and the base pointer may sit at any element
offset).  The result is float32 [rows].  A radix select over four 8-bit digits of the order-preserving key: five launches and
a memset on the current stream, no wait for the device, the same bits for every `splits` (workgroups per row; 0 chooses).
"""
import torch

from ._lib import check, lib, ptr, stream_ptr

MAX_ROWS = 65535
MAX_SPLITS = 65535


def _check_rows(x):
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise TypeError(f"x must be a float32 tensor, got {x.dtype if torch.is_tensor(x) else type(x).__name__}")
    if x.dim() != 2:
        raise ValueError(f"x must be [rows, n], got {tuple(x.shape)}")
    rows, n = x.shape
    if not 1 <= rows <= MAX_ROWS:
        raise ValueError(f"x must have between 1 and {MAX_ROWS} rows, got {rows}")
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"rows must have between 1 and 2^31 - 1 elements, got {n}")
    if n > 1 and x.stride(1) != 1:
        raise ValueError(f"x must have unit inner stride, got stride {x.stride(1)}")
    if rows > 1 and x.stride(0) < n:
        raise ValueError(f"rows must not overlap: row stride {x.stride(0)} < n {n}")
    return rows, n, (x.stride(0) if rows > 1 else n)


def row_kth_value(x, k, *, nan_propagates=False, splits=0, out=None):
    rows, n, row_stride = _check_rows(x)
    k, splits = int(k), int(splits)
    if not 0 <= k < n:
        raise ValueError(f"k must be in [0, {n}), got {k}")
    if not 0 <= splits <= MAX_SPLITS:
        raise ValueError(f"splits must be in [0, {MAX_SPLITS}], got {splits}")
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.float32:
            raise TypeError("out must be a float32 tensor")
        if tuple(out.shape) != (rows,) or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"out must be a contiguous [{rows}] tensor on {x.device}")
    if not x.is_cuda:
        raise RuntimeError("x must be a GPU tensor: the selection runs in the HIP kernel only (no CPU path)")
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=x.device)
    workspace = torch.empty(int(lib.hs_select_rows_workspace(rows)), dtype=torch.uint8, device=x.device)
    check(lib.hs_select_rows(ptr(x), rows, n, row_stride, k, int(bool(nan_propagates)), splits, ptr(workspace), ptr(out),
                             stream_ptr(x.device)), "hs_select_rows")
    return out


def row_median(x, out=None):
    _check_rows(x)
    return row_kth_value(x, (x.shape[1] - 1) // 2, nan_propagates=True, out=out)
