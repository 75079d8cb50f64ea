"""heal_swin_amd.depth_data on the host: the depth projection's coordinates against the reference's, the six normalization
tables, argument validation, the error without a GPU and the npz sample format.  (The kernels: test_gpu_depth_data.py.)"""
import numpy as np
import pytest
import torch

from _golden import load
from test_depth_evaluation import _cal

@pytest.fixture(scope="module")
def DD():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import depth_data
    return depth_data


def coord_cases(g):
    """(tag, cal key, rotate_pole, used_size) of every coordinate case in the golden file."""
    out = []
    for k in sorted(k for k in g.files if k.startswith("coords/") and k.endswith("/u")):
        _, key, case, _ = k.split("/")
        _, _, rot, used = case.split("_")
        out.append((f"coords/{key}/{case}", key, rot == "rot", None if used == "cal" else tuple(int(a) for a in used.split("x"))))
    return out


def test_coordinates_match_the_reference(DD):
    """Bit-equal without rotate_pole; within 1e-10 px with it."""
    g = load("depth_data")
    cases = coord_cases(g)
    assert len(cases) == 4 and any(c[3] for c in cases) and any(c[2] for c in cases) and any(c[3] is None for c in cases)
    for tag, key, rot, used in cases:
        u, v = DD.project_depth_s2_points_to_img(g[tag + "/theta"], g[tag + "/phi"], _cal(key), rot, used)
        if rot:  # the rotation goes through scipy in the reference: same mathematics, last-bit differences (test_projection.py)
            np.testing.assert_allclose(u, g[tag + "/u"], atol=1e-10, rtol=0)
            np.testing.assert_allclose(v, g[tag + "/v"], atol=1e-10, rtol=0)
        else:
            assert np.array_equal(u, g[tag + "/u"]) and np.array_equal(v, g[tag + "/v"]), tag


def test_used_size_only_moves_the_centre(DD):
    g = load("depth_data")
    tag = "coords/fv_966x1280/n8_bp8_plain_483x640"
    u0, v0 = DD.project_depth_s2_points_to_img(g[tag + "/theta"], g[tag + "/phi"], _cal("fv_966x1280"))
    u1, v1 = DD.project_depth_s2_points_to_img(g[tag + "/theta"], g[tag + "/phi"], _cal("fv_966x1280"), used_size=(483, 640))
    np.testing.assert_allclose(u0 - u1, 320.0, atol=1e-9)
    np.testing.assert_allclose(v0 - v1, 241.5, atol=1e-9)


REF_TABLES = {  # normalize_depth_data.py:31-109, (mask_background, transform): (max, min, mean, std)
    (False, "log"): (6.907755374908447, -1.8142070770263672, 1.4544509182015166, 2.0786484162088192),
    (False, "inv"): (6.136208534240723, 0.001, 0.9910007833745446, 1.449026079271616),
    (False, "None"): (999.94287109375, 0.16296708583831787, 53.27547067117465, 195.83201099547819),
    (True, "log"): (6.907698154449463, -1.8142070770263672, 1.226225759977343, 1.7902344298584563),
    (True, "inv"): (6.136208534240723, 0.0010000570910051465, 1.0324331088958505, 1.4645187100900352),
    (True, "None"): (999.94287109375, 0.16296708583831787, 13.654291032986958, 29.58008801108711),
}


def test_the_six_tables(DD):
    for (mask, tr), vals in REF_TABLES.items():
        s = DD.get_depth_data_stats(tr, mask)
        assert (s.max, s.min, s.mean, s.std) == vals, (mask, tr)
    assert DD.get_depth_data_stats(None, True).mean == DD.get_depth_data_stats("None", True).mean
    assert DD.get_depth_data_stats("None", False).total_background == 120398457
    assert DD.get_depth_data_stats("None", True).total_pixels == 2876849543


def test_loss_constants_are_the_masked_table(DD):
    from heal_swin_amd import losses
    s = DD.get_depth_data_stats(None, mask_background=True)
    assert (losses.DEPTH_MEAN, losses.DEPTH_STD) == (s.mean, s.std)


def test_argument_validation(DD):
    with pytest.raises(ValueError):
        DD.DepthTargetTransform(data_transform="sqrt")
    with pytest.raises(ValueError):
        DD.DepthTargetTransform(normalize_data="z-score")
    with pytest.raises(ValueError):
        DD.get_depth_data_stats("exp")
    with pytest.raises(ValueError):
        DD.DepthStatsAccumulator(data_transform="exp", device="cuda")
    t = DD.DepthTargetTransform("log", "standardize", mask_background=True)
    assert t._affine == (float(np.float32(1.226225759977343)), float(np.float32(1.7902344298584563)))
    t = DD.DepthTargetTransform("inv", "min-max", data_stats=DD.DataStats("mine", max=4.0, min=1.0, mean=2.0, std=1.0))
    assert t._affine == (1.0, 3.0)
    assert DD.DepthTargetTransform("None", "None")._affine is None
    with pytest.raises(TypeError):
        t.prepare(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError):
        DD.write_depth_sample("unused.npz", np.zeros((3, 4), np.uint8), np.zeros(4, np.float32))


def test_clear_error_without_a_gpu(DD):
    t = DD.DepthTargetTransform("log", "standardize")
    with pytest.raises(RuntimeError, match="GPU"):
        t.prepare(torch.ones(2, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        DD.sample_bilinear_f32(np.zeros((3, 4, 4), np.uint8), np.zeros(3), np.zeros(3))
    with pytest.raises(RuntimeError, match="GPU"):
        DD.sample_depth(np.zeros((4, 4), np.float32), np.zeros(3), np.zeros(3))
    with pytest.raises(RuntimeError, match="GPU"):
        DD.DepthStatsAccumulator(device="cpu")


def test_npz_round_trip(DD, tmp_path):
    rng = np.random.default_rng(3)
    imgs = rng.uniform(0, 255, (2, 3, 96)).astype(np.float32)
    masks = rng.uniform(0, 1000, (2, 96)).astype(np.float32)
    masks[0, :5] = [np.nan, np.inf, 0.0, 1000.0, -0.0]
    for i, name in enumerate(("b_frame", "a_frame")):
        DD.write_depth_sample(str(tmp_path / (name + ".npz")), imgs[i], masks[i])
    ds = DD.HPDepthNpzDataset(str(tmp_path))
    assert len(ds) == 2 and ds.names == ["a_frame", "b_frame"]
    for i, name in enumerate(("b_frame", "a_frame")):
        img, mask = ds.get_item_by_name(name)
        assert img.dtype == np.float32 and mask.dtype == np.float32
        assert np.array_equal(img, imgs[i]) and np.array_equal(mask, masks[i], equal_nan=True)
        raw = np.load(str(tmp_path / (name + ".npz")))
        assert sorted(raw.files) == ["hp_img", "hp_mask"]
