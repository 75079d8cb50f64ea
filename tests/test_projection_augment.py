"""Per-sample rotation augmentation of the projection, the parts that need no GPU: the random matrices, the camera record, the
refusals of the new C entry points (decided before any launch) and the shape checks of the Python surface.  The kernels are
checked in test_gpu_projection_augment.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.test_projection import calibrations


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import projection
    return projection


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_random_rotations_are_orthogonal_with_the_stated_determinant(P):
    eye = np.eye(3)
    for kw, dets in ((dict(max_tilt_deg=7.0), {1}), (dict(max_tilt_deg=7.0, flip=1.0), {-1}), (dict(max_tilt_deg=30.0, flip=0.5), {1, -1}),
                     (dict(roll=False, max_tilt_deg=90.0), {1})):
        a = P.random_rotations(64, generator=_gen(3), **kw)
        assert a.dtype == torch.float64 and a.shape == (64, 3, 3) and a.device.type == "cpu"
        a = a.numpy()
        assert np.abs(np.swapaxes(a, 1, 2) @ a - eye).max() <= 1e-14
        d = np.linalg.det(a)
        assert np.abs(np.abs(d) - 1).max() <= 1e-14
        assert {int(round(x)) for x in d} == dets, kw


@pytest.mark.parametrize("tilt", [0.0, 0.5, 5.0, 60.0])
def test_tilt_is_bounded_and_roll_keeps_the_axis(P, tilt):
    a = P.random_rotations(256, max_tilt_deg=tilt, flip=0.5, generator=_gen(11)).numpy()
    ez = a[:, :, 2]  # A e_z
    ang = np.arctan2(np.hypot(ez[:, 0], ez[:, 1]), ez[:, 2])
    assert ang.max() <= math.radians(tilt) + 1e-14
    if tilt > 0:
        assert ang.max() > 0.8 * math.radians(tilt)  # the range is used


def test_no_augmentation_is_the_identity_exactly(P):
    a = P.random_rotations(5, max_tilt_deg=0, roll=False, flip=0, generator=_gen(1)).numpy()
    assert np.array_equal(a, np.broadcast_to(np.eye(3), (5, 3, 3)))
    assert not np.signbit(a).any()
    # roll alone is a rotation about z; a flip alone is diag(-1, 1, 1)
    r = P.random_rotations(5, generator=_gen(1)).numpy()
    assert np.array_equal(r[:, 2], np.broadcast_to([0.0, 0.0, 1.0], (5, 3))) and np.abs(r[:, 0, 1]).min() > 0
    f = P.random_rotations(5, roll=False, flip=1.0, generator=_gen(1)).numpy()
    assert np.array_equal(f, np.broadcast_to(np.diag([-1.0, 1.0, 1.0]), (5, 3, 3)))


def test_random_rotations_follow_the_generator(P):
    kw = dict(max_tilt_deg=5.0, flip=0.5)
    a, b, c = (P.random_rotations(8, generator=_gen(s), **kw) for s in (7, 7, 8))
    assert torch.equal(a, b) and not torch.equal(a, c)
    with pytest.raises(ValueError):
        P.random_rotations(2, flip=1.5)


def test_camera_record(P):
    from heal_swin_amd._lib import FisheyeCamera

    for name, cal in calibrations().items():
        intr = cal["intrinsic"]
        cam = P.camera_record(cal)
        assert isinstance(cam, FisheyeCamera) and ctypes.sizeof(cam) == 104
        order = int(intr["poly_order"])
        assert cam.poly_order == order and (cam.height, cam.width) == (int(intr["height"]), int(intr["width"]))
        assert list(cam.k) == [float(intr[f"k{i + 1}"]) for i in range(order)] + [0.0] * (8 - order)
        assert (cam.cx_offset, cam.cy_offset, cam.aspect_ratio) == (intr["cx_offset"], intr["cy_offset"], intr["aspect_ratio"])
        small = P.camera_record(cal, used_size=(48, 64))
        assert (small.height, small.width) == (48, 64) and list(small.k) == list(cam.k) and small.cx_offset == cam.cx_offset
    with pytest.raises(ValueError):
        P.camera_record(dict(cal, intrinsic=dict(intr, poly_order=9)))


def test_the_coordinate_entry_point_refuses_before_launch(P):
    """Every refusal is HS_ERR_INVALID_ARG (1) and is decided on the host: the pointers name host memory no kernel could read."""
    from heal_swin_amd._lib import lib

    cam = P.camera_record(calibrations()["mvl_96x128"])
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(nside=4, first=0, count=16, cam=cam, rot=p, batch=2, u=p, v=p):
        return lib.hs_hp_rotated_coords(nside, first, count, None if cam is None else ctypes.byref(cam), rot, batch, u, v, None)

    def with_order(order, **kw):
        c = P.camera_record(calibrations()["mvl_96x128"])
        c.poly_order = order
        for k, val in kw.items():
            setattr(c, k, val)
        return c

    for kw in (dict(nside=3), dict(nside=0), dict(nside=-4), dict(first=12 * 16 - 8), dict(first=-1), dict(count=-1), dict(count=12 * 16 + 1),
               dict(first=12 * 16 + 1, count=0), dict(batch=0), dict(batch=-3), dict(cam=with_order(0)), dict(cam=with_order(9)),
               dict(cam=with_order(4, width=0)), dict(cam=with_order(4, height=-1)), dict(cam=None), dict(rot=None), dict(u=None),
               dict(v=None)):
        assert call(**kw) == 1, kw
        assert lib.hs_last_error()
    assert call(count=0) == 0 and call(first=12 * 16, count=0) == 0 and call(count=0, rot=None, u=None, v=None) == 0


def test_the_per_sample_entry_points_refuse_before_launch(P):
    from heal_swin_amd._lib import lib

    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    stream = None
    calls = {
        "hs_sample_bilinear_u8_per_sample": lambda img=p, b=2, c=3, h=8, w=8, rx=p, ry=p, n=4, out=p: lib.hs_sample_bilinear_u8_per_sample(
            img, b, c, h, w, rx, ry, n, out, stream),
        "hs_sample_bilinear_u8_f32_per_sample": lambda img=p, b=2, c=3, h=8, w=8, rx=p, ry=p, n=4, out=p: lib.hs_sample_bilinear_u8_f32_per_sample(
            img, b, c, h, w, rx, ry, n, out, stream),
        "hs_sample_mask_u8_per_sample": lambda img=p, b=2, c=1, h=8, w=8, rx=p, ry=p, n=4, out=p: lib.hs_sample_mask_u8_per_sample(
            img, b, h, w, rx, ry, n, 0, out, stream),
        "hs_sample_nearest_f32_per_sample": lambda img=p, b=2, c=1, h=8, w=8, rx=p, ry=p, n=4, out=p: lib.hs_sample_nearest_f32_per_sample(
            img, b, h, w, rx, ry, n, 0.0, out, stream),
    }
    for name, call in calls.items():
        for kw in (dict(b=0), dict(b=65536), dict(h=0), dict(w=-1), dict(n=-1), dict(img=None), dict(rx=None), dict(ry=None), dict(out=None)):
            assert call(**kw) == 1, (name, kw)
        assert call(n=0) == 0 and call(n=0, img=None, rx=None, ry=None, out=None) == 0, name
    assert lib.hs_sample_mask_u8_per_sample(p, 2, 8, 8, p, p, 4, 256, p, None) == 1  # the background class must fit uint8


def test_python_argument_checks(P):
    """Shapes are checked before anything touches the device, so the refusals need none."""
    from heal_swin_amd import depth_data as DD

    cal = calibrations()["mvl_96x128"]
    for bad in (np.eye(3), np.zeros((2, 9)), np.zeros((2, 3, 4)), np.zeros((0, 3, 3)), torch.zeros(2, 4, 3, 3)):
        with pytest.raises(ValueError, match="rotations"):
            P.rotated_coords(4, 12, cal, bad)
    img, mask = torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.uint8)
    depth = torch.zeros(2, 8, 8)
    ok, three, flat = np.zeros((2, 5)), np.zeros((3, 5)), np.zeros(10)
    for rx, ry in ((three, three), (flat, flat), (ok, np.zeros((2, 6))), (np.zeros((1, 2, 5)), np.zeros((1, 2, 5)))):
        with pytest.raises(ValueError, match="per_sample"):
            P.sample_bilinear_u8(img, rx, ry, per_sample=True)
        with pytest.raises(ValueError, match="per_sample"):
            P.sample_mask(mask, rx, ry, 0, per_sample=True)
        with pytest.raises(ValueError, match="per_sample"):
            DD.sample_bilinear_f32(img, rx, ry, per_sample=True)
        with pytest.raises(ValueError, match="per_sample"):
            DD.sample_depth(depth, rx, ry, 0.0, per_sample=True)
    with pytest.raises(ValueError, match="per_sample"):  # an unbatched image is a batch of one
        P.sample_bilinear_u8(img[0], ok, ok, per_sample=True)
    with pytest.raises(RuntimeError, match="GPU tensor"):  # well-formed calls still need the device: there is no CPU path
        P.sample_bilinear_u8(img, ok, ok, per_sample=True)
