"""heal_swin_amd.depth_data.DepthHistogram on the GPU (hs_histogram_update, csrc/depth_data.hip) against np.histogram on the
same float64 values: counts and edges exactly equal -- values on the edges, at and just outside the range's ends, NaN and
+-inf, one crowded bin, the transforms with and without masking, split updates, from_stats and the saved file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LO, HI = -2.5, 3.0  # both are float32 values


@pytest.fixture(scope="module")
def DD():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import depth_data
    return depth_data


def _extras(bins):
    """the values a bin rule can get wrong: float32 roundings of edges, the closed upper end, the floats just outside, non-finite"""
    edges = np.histogram_bin_edges(np.empty(0), bins, (LO, HI))
    pick = edges[np.unique(np.linspace(0, bins, 12).astype(int))].astype(np.float32)
    lo, hi = np.float32(LO), np.float32(HI)
    ends = np.array([hi, lo, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))], np.float32)
    return np.concatenate([pick, ends, np.array([np.nan, np.inf, -np.inf], np.float32)])


def _assert_hist(h, values32, bins, rng_, tag):
    counts, edges = h.compute()
    want, want_edges = np.histogram(np.asarray(values32, np.float32).astype(np.float64), bins, rng_)
    assert counts.dtype == np.int64 and edges.dtype == np.float64 and counts.shape == (bins,)
    assert np.array_equal(edges, want_edges), tag
    assert np.array_equal(counts, want), (tag, np.flatnonzero(counts != want)[:8])


@pytest.mark.parametrize("bins", [1, 7, 1000, 4096])
@pytest.mark.parametrize("n", [1, 1023, 100003])
def test_counts_and_edges_are_numpys(DD, n, bins):
    extras = _extras(bins)
    if n == 1:  # every special value alone
        for v in extras:
            h = DD.DepthHistogram(bins, (LO, HI))
            h.update(torch.tensor([v], device=DEV))
            _assert_hist(h, [v], bins, (LO, HI), (bins, float(v)))
        return
    a = (np.random.default_rng(n + bins).standard_normal(n) * 1.5).astype(np.float32)
    a[:extras.size] = extras
    h = DD.DepthHistogram(bins, (LO, HI))
    h.update(torch.from_numpy(a).to(DEV))
    _assert_hist(h, a, bins, (LO, HI), (n, bins))
    assert int(h.compute()[0].sum()) < n  # values outside the range and non-finite ones were dropped
    # a base pointer off the 16-byte grid (the scalar path), and reset
    h.reset()
    h.update(torch.from_numpy(a).to(DEV)[1:])
    _assert_hist(h, a[1:], bins, (LO, HI), (n, bins, "offset 1"))
    # everything in one bin
    h.reset()
    h.update(torch.full((n,), 0.7, device=DEV))
    _assert_hist(h, np.full(n, 0.7, np.float32), bins, (LO, HI), (n, bins, "one bin"))


def _depths(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.1, 80.0, n).astype(np.float32)
    a[rng.random(n) < 0.1] = 1000.0
    a[rng.random(n) < 0.01] = 0.0  # log: -inf, inv: +inf -- dropped
    return a


def _transformed(a, transform, masking):
    """the accumulator's values as tests/test_gpu_depth_data.py forms them"""
    keep = a[a != 1000] if masking else a
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"None": keep, "log": np.log(keep.astype(np.float64)).astype(np.float32), "inv": 1 / keep}[transform]


@pytest.mark.parametrize("masking", [False, True])
@pytest.mark.parametrize("transform,rng_", [("log", (-3.0, 7.0)), ("inv", (0.0, 10.0)), ("None", (0.0, 1000.0))])
def test_transforms_and_masking(DD, transform, rng_, masking):
    a = _depths(50001, 7)
    h = DD.DepthHistogram(1000, rng_, data_transform=transform, use_masking=masking)
    h.update(torch.from_numpy(a).to(DEV))
    _assert_hist(h, _transformed(a, transform, masking), 1000, rng_, (transform, masking))
    bkg_bin = np.histogram(_transformed(np.array([1000.0], np.float32), transform, False).astype(np.float64), 1000, rng_)[0].argmax()
    assert (h.compute()[0][bkg_bin] > 1000) == (not masking)  # the background value is there to be masked


def test_updates_accumulate(DD):
    a, b = _depths(30012, 1), _depths(4099, 2)
    h2, h1 = DD.DepthHistogram(500, (0.0, 90.0)), DD.DepthHistogram(500, (0.0, 90.0))
    h2.update(torch.from_numpy(a).to(DEV).view(3, -1)[:, :10000])
    h2.update(torch.from_numpy(a).to(DEV).view(3, -1)[:, 10000:])  # non-contiguous views: any shape, as the accumulator
    h2.update(torch.from_numpy(b).to(DEV))
    h1.update(torch.from_numpy(np.concatenate([a, b])).to(DEV))
    assert np.array_equal(h2.compute()[0], h1.compute()[0])
    _assert_hist(h1, np.concatenate([a, b]), 500, (0.0, 90.0), "concatenation")
    h2.update(torch.empty(0, device=DEV))
    assert np.array_equal(h2.compute()[0], h1.compute()[0])


@pytest.mark.parametrize("transform,masking", [("None", False), ("log", True)])
def test_from_stats_is_histogram_without_a_range(DD, transform, masking, tmp_path):
    a = _depths(40009, 3)
    a = a[a != 0]
    dev = torch.from_numpy(a).to(DEV)
    acc = DD.DepthStatsAccumulator(transform, use_masking=masking)
    acc.update(dev)
    h = DD.DepthHistogram.from_stats(acc.compute(), data_transform=transform, use_masking=masking)
    h.update(dev)
    values = _transformed(a, transform, masking).astype(np.float64)
    want, want_edges = np.histogram(values, bins=1000)
    counts, edges = h.compute()
    assert np.array_equal(edges, want_edges) and np.array_equal(counts, want)
    assert counts.sum() == values.size and counts[0] > 0 and counts[-1] > 0
    path = str(tmp_path / "hist.npz")
    h.save(path)
    z = np.load(path)
    assert sorted(z.files) == ["bin_counts", "bin_edges"]
    assert np.array_equal(z["bin_counts"], want) and z["bin_counts"].dtype == np.int64
    assert np.array_equal(z["bin_edges"], want_edges) and z["bin_edges"].dtype == np.float64


def test_degenerate_and_invalid_ranges_are_numpys(DD):
    h = DD.DepthHistogram(10, (2.0, 2.0))  # numpy widens an empty range by 0.5 each way
    h.update(torch.tensor([2.0, 1.4, 2.5, 2.6], device=DEV))
    _assert_hist(h, [2.0, 1.4, 2.5, 2.6], 10, (2.0, 2.0), "degenerate")
    with pytest.raises(ValueError):
        DD.DepthHistogram(10, (3.0, 2.0))
    with pytest.raises(ValueError):
        DD.DepthHistogram(10, (0.0, float("inf")))
    with pytest.raises(TypeError):
        DD.DepthHistogram(10, (0.0, 1.0)).update(torch.zeros(4, dtype=torch.float64, device=DEV))
