"""heal_swin_amd.order_stats on the GPU (csrc/select.hip): the k-th smallest element of every row against a CPU sort, bit for
bit (zeros by value, NaN as NaN), at every path through the row (scalar-only, one vector, vector + tail, one workgroup's chunk
+- 1, several workgroups per row), at any element offset and row stride, identical for every split; the NaN rules of
torch.kthvalue and torch.median; graph capture; and DepthMetrics' median_std without torch.median."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 2, 3, 4, 5, 255, 1023, 1024, 1025, 4097, 300001]
ROWS = [1, 3, 37]
SPLITS = [0, 1, 2, 7]


@pytest.fixture(scope="module")
def OS():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import order_stats
    return order_stats


def _bits(a):
    return torch.from_numpy(np.asarray(a, np.uint32).view(np.float32).copy())


def _place(x, pad, offset):
    """x [rows, n] (CPU) on the device as a view with row stride n + pad whose first element sits `offset` elements into an
    allocation: rows and base pointer at any 4-byte offset."""
    rows, n = x.shape
    buf = torch.full((offset + rows * (n + pad),), float("nan"), device=DEV)  # a NaN read from outside a row would show
    view = buf[offset:].view(rows, n + pad)[:, :n]
    view.copy_(x)
    return view


def _assert_same(got, want, tag):
    """fp32 CPU tensors equal as bit patterns, zeros by value, NaN as NaN"""
    ok = (got.view(torch.int32) == want.view(torch.int32)) | ((got == 0) & (want == 0)) | (got.isnan() & want.isnan())
    assert bool(ok.all()), (tag, got[~ok][:4], want[~ok][:4])


def _ks(n, seed):
    return sorted({0, (n - 1) // 2, n - 1, int(np.random.default_rng(seed).integers(n))})


def _check(OS, x, ks, tag, pads=(0,), offsets=(0,), splits=SPLITS, nan_propagates=False, want_of=None):
    """row_kth_value(x, k) for every k, placement and split against the CPU sort of x, one device read at the end"""
    srt = x.sort(1).values
    got, want, tags = [], [], []
    for pad in pads:
        for offset in offsets:
            v = _place(x, pad, offset)
            for k in ks:
                for s in splits:
                    got.append(OS.row_kth_value(v, k, nan_propagates=nan_propagates, splits=s))
                    want.append(srt[:, k] if want_of is None else want_of(srt[:, k]))
                    tags.append((pad, offset, k, s))
    got = torch.stack(got).cpu()
    for g, w, t in zip(got, want, tags):
        _assert_same(g, w, (tag,) + t)


@pytest.mark.parametrize("n", SIZES)
def test_kth_value_at_every_shape_offset_and_split(OS, n):
    for rows in ROWS:
        x = torch.randn((rows, n), generator=torch.Generator().manual_seed(1000 * rows + n % 997))
        _check(OS, x, _ks(n, n + rows), (n, rows), pads=(0, 3), offsets=(0, 1))


def _data(kind, rows, n, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(rows * n, dtype=np.int64).reshape(rows, n)
    if kind == "equal":
        return torch.from_numpy(np.repeat(rng.standard_normal(rows).astype(np.float32)[:, None], n, 1).copy())
    if kind == "runs":  # three values in long runs, in an order that is not the sorted one
        third = np.array([0.5, -2.0, 3.0], np.float32)[np.minimum(3 * np.arange(n) // max(n, 1), 2)]
        return torch.from_numpy(np.stack([np.roll(third, r * 7) for r in range(rows)]))
    if kind == "low_byte":
        return _bits(0x3F800000 + (i * 7919 % 251))
    if kind == "high_byte":  # 0x7F400000 and 0xFF400000 are finite: no NaN among them
        return _bits((((i * 37 + 11) % 256) << 24) | 0x00400000)
    if kind == "specials":
        pool = np.array([np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.0, -1.0, 3.4e38, -3.4e38], np.float32)
        return torch.from_numpy(pool[rng.integers(pool.size, size=(rows, n))])
    if kind == "nans":  # NaNs of both signs and several payloads in every row but row 1
        x = rng.standard_normal((rows, n)).astype(np.float32)
        x[rng.random((rows, n)) < 0.01] = np.inf
        nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)
        hit = rng.random((rows, n)) < 0.2
        hit[:, 0] = True
        hit[1] = False
        x[hit] = nan[rng.integers(4, size=int(hit.sum()))]
        return torch.from_numpy(x)
    raise KeyError(kind)


@pytest.mark.parametrize("n", [5, 1025, 4097])
@pytest.mark.parametrize("kind", ["equal", "runs", "low_byte", "high_byte", "specials", "nans"])
def test_kth_value_on_hard_keys(OS, kind, n):
    x = _data(kind, 3, n, seed=n)
    ks = _ks(n, n)
    if kind == "runs":  # the last element of a run and the first of the next
        srt = x[0].sort().values
        edges = (srt[1:] != srt[:-1]).nonzero().flatten().tolist()
        ks = sorted(set(ks) | set(edges) | {e + 1 for e in edges})
    _check(OS, x, ks, kind, pads=(3,), offsets=(1,))
    if kind == "nans":
        nan_rows = x.isnan().any(1)
        assert nan_rows.tolist() == [True, False, True]
        assert bool(x.sort(1).values[0, -1].isnan())  # without propagation the NaNs take the top ranks (checked above at k = n - 1)
        _check(OS, x, ks, "nans propagate", pads=(3,), offsets=(1,), nan_propagates=True,
               want_of=lambda w: torch.where(nan_rows, torch.full_like(w, float("nan")), w))


def test_row_median_is_torch_median(OS):
    for kind, rows, n in (("nans", 3, 4097), ("specials", 5, 1000), ("runs", 2, 6), ("equal", 4, 1)):
        x = _data(kind, rows, n, seed=3)
        got = OS.row_median(_place(x, 5, 3)).cpu()
        assert torch.equal(got.isnan(), x.median(1).values.isnan())
        assert torch.allclose(got, x.median(1).values, rtol=0, atol=0, equal_nan=True), kind
    out = torch.empty(3, device=DEV)
    x = torch.randn(3, 77)
    assert OS.row_median(x.to(DEV), out=out) is out and torch.equal(out.cpu(), x.median(1).values)


def test_select_replays_in_a_graph(OS):
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((8, 20001), generator=gen).to(DEV)
    out = torch.empty(8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        OS.row_median(x, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        OS.row_median(x, out=out)
    for _ in range(2):
        new = torch.randn((8, 20001), generator=gen)
        x.copy_(new)
        out.fill_(-1.0)
        graph.replay()
        assert torch.equal(out.cpu(), new.median(1).values)


# ------------------------------------------------------------------ DepthMetrics.median without torch.median
def _lower_median(stds):
    """torch.median's rule from a CPU sort: the lower median, NaN if the row holds one"""
    s = stds.cpu()
    med = s.sort(1).values[:, (s.shape[1] - 1) // 2]
    return torch.where(s.isnan().any(1), torch.full_like(med, float("nan")), med)


def _assert_median(m, stds_list, tag):
    want = torch.zeros(2, dtype=torch.float64)
    for stds in stds_list:
        want[0] += _lower_median(stds).double().sum()
        want[1] += stds.shape[0]
    got = m.median.cpu()
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)) or (got[0].isnan() and want[0].isnan() and got[1] == want[1]), \
        (tag, got, want)
    got_c, want_c = m.compute()["median_std"], float(want[0] / want[1])
    assert got_c == want_c or (np.isnan(got_c) and np.isnan(want_c)), (tag, got_c, want_c)


def test_depth_metrics_median_does_not_sort(OS, monkeypatch):
    from heal_swin_amd import flat_evaluation as FE
    from heal_swin_amd.depth_evaluation import DepthMetrics
    from _golden import load
    from test_flat_evaluation import projector

    B, npix = 3, 8 * 16 ** 2
    gen = torch.Generator().manual_seed(11)
    pred = torch.randn((B, 2, npix), generator=gen).to(DEV)
    target = (torch.rand((B, npix), generator=gen) * 50 + 0.5).to(DEV)
    name = "resize_pad_plain"
    g = load("flat_eval")
    nchw = torch.from_numpy(g[name + "/depth/pred"])
    nchw = torch.cat([nchw, nchw[:1] * 1.25 + 0.125]).to(DEV)  # B = 3
    flat_target = torch.from_numpy(g[name + "/depth/target"])
    flat_target = torch.cat([flat_target, flat_target[:1]]).to(DEV)
    assert flat_target.shape == (B, npix)
    p = projector(FE, name, layout="image", interpolation="nearest", device=DEV)

    def refuse(*a, **k):
        raise AssertionError("torch.median was reached")

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "median", refuse)
        mp.setattr(torch, "median", refuse)
        for dtype in (torch.float32, torch.bfloat16):
            m = DepthMetrics(use_logvar=True, device=DEV)
            pd = pred.to(dtype)
            m.update(pd, target)
            stds = torch.sqrt(torch.exp(pd[:, 1].float()))
            _assert_median(m, [stds], dtype)
            m.add_median(pd[:, 1])
            _assert_median(m, [stds, stds], (dtype, "add_median"))
        m = DepthMetrics(use_logvar=True, device=DEV)
        m.update(nchw, flat_target, p)
        stds = torch.sqrt(torch.exp(p.depth(nchw, channel=1)))
        assert stds.dtype == torch.float32 and stds.shape == (B, npix)
        _assert_median(m, [stds], "projected")
    # float64 predictions keep torch.median
    m = DepthMetrics(use_logvar=True, device=DEV)
    pd = pred.double()
    m.update(pd, target)
    want = torch.sqrt(torch.exp(pd[:, 1])).median(1).values.sum()
    assert torch.equal(m.median.cpu(), torch.stack([want.cpu(), torch.tensor(float(B), dtype=torch.float64)]))
