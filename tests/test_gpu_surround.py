"""Surround view on the GPU: `hs_surround_to_hp` against the host entry point (the same inline function in a host loop, itself
checked against a numpy model in test_surround.py) BIT FOR BIT in every output, `camera` included -- frames u8 and f32, both
blends, with and without the edge feather, 1, 3 and 8 cameras, a dropped camera, a camera-less sample, a non-finite matrix, a
symmetric rig whose exact weight ties the lowest-index rule decides, 8 and 12 base pixels, less than one and several workgroups --
the guard bytes behind every output, `SurroundProjector` under graph capture with the rotations and the present bytes changed
between replays, and the path end to end at a tiny size: rig -> sphere -> model step -> back onto one camera -> confusion matrix."""
import numpy as np
import pytest
import torch

from tests.test_erp import bits, generic_matrices
from tests.test_surround import BKGD, FILL, planes, rig_cals, symmetric_rig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import surround
    return surround


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    """equal as bytes: float planes by their words, so NaNs count"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)


def raw_launch(S, rig, nside, npix, mats, present, frame, labels, depth, outs, background=0, fill=0.0):
    """`hs_surround_to_hp` through the raw C ABI: every argument a device tensor or None, outs = (frame, labels, depth, camera)"""
    from heal_swin_amd._lib import HS_F32, HS_U8, lib, ptr, stream_ptr
    given = next(t for t in (frame, labels, depth) if t is not None)
    kind = HS_F32 if frame is not None and frame.dtype == torch.float32 else HS_U8
    return lib.hs_surround_to_hp(nside, npix, rig, ptr(mats), ptr(present), mats.shape[0], given.shape[-2], given.shape[-1], ptr(frame), kind,
                                 0 if frame is None else frame.shape[2], ptr(outs[0]), ptr(labels), ptr(outs[1]), background, ptr(depth), ptr(outs[2]),
                                 fill, ptr(outs[3]), stream_ptr(mats.device))


# ------------------------------------------------------------------ 1. the kernel against the host entry point, bit for bit
# nside 4: 192 pixels, less than one workgroup of 256; nside 16: 8 and 12 workgroups.  Five channels: a full group of four and a part of one.
@pytest.mark.parametrize("nside,base_pix,n_cam,hw,channels", [(4, 12, 1, (12, 25), 3), (4, 12, 3, (60, 80), 5), (16, 8, 8, (12, 25), 5),
                                                              (16, 12, 3, (12, 25), 3), (16, 12, 8, (60, 80), 5), (16, 8, 1, (60, 80), 16)])
def test_device_equals_the_host_entry_bit_for_bit(S, nside, base_pix, n_cam, hw, channels):
    batch, npix = 5, base_pix * nside * nside
    cals = rig_cals(hw, n_cam, 10 * nside + n_cam)
    rot = generic_matrices(nside + n_cam, 3)[:batch]
    img, fimg, lab, dep = planes(3 * nside + n_cam, batch, n_cam, *hw, channels=channels)
    present = np.ones((batch, n_cam), dtype=bool)
    everyone = S.surround_to_hp_host(cals, nside, S.SurroundProjector(cals, nside, device="cpu").matrices(rot).numpy(), masks=lab, base_pix=base_pix,
                                     return_camera=True)[1]
    drop = int(np.bincount(everyone[1], minlength=256)[:n_cam].argmax())  # the camera that wins most of sample 1 ...
    present[1, drop] = False  # ... is dropped there (with one camera: an empty sample)
    present[2] = False  # a sample without any camera
    for blend in ("winner", "feather"):
        for feather in (0.0, 6.0):
            proj = S.SurroundProjector(cals, nside, base_pix, blend=blend, edge_feather=feather, s2_bkgd_class=BKGD, depth_fill=FILL)
            kw = dict(base_pix=base_pix, blend=blend, edge_feather=feather, s2_bkgd_class=BKGD, depth_fill=FILL, return_camera=True)
            mats = proj.matrices(rot).cpu().numpy()
            mats[3, n_cam - 1, 1, 2] = np.nan  # sample 3: a NaN in its last camera's matrix
            # the projector forms its own matrices, so the NaN travels as a rotation with a NaN: every camera of sample 4 is removed
            bad = rot.copy()
            bad[4, 0, 0] = np.nan
            want = S.surround_to_hp_host(cals, nside, proj.matrices(bad).cpu().numpy(), img, lab, dep, present=present, **kw)
            got = [t.cpu().numpy() for t in proj(dev(img), dev(lab), dev(dep), rotations=bad, present=present, return_camera=True)]  # host arrays
            assert [g.shape for g in got] == [(batch, channels, npix), (batch, npix), (batch, npix), (batch, npix)]
            for name, g, w in zip(("frame u8", "labels", "depth", "camera"), got, want):
                diff = (bits(g) != bits(w)) if g.dtype == np.float32 else (g != w)
                print(f"nside {nside}, {base_pix} base pixels, K = {n_cam}, {hw}, {blend}, feather {feather}, {name}: {diff.sum()} of {diff.size} differ")
            fgot = proj(dev(fimg), rotations=dev(bad), present=dev(present)).cpu().numpy()  # device tensors
            fwant = S.surround_to_hp_host(cals, nside, proj.matrices(bad).cpu().numpy(), fimg, present=present, **dict(kw, return_camera=False))
            print(f"nside {nside}, K = {n_cam}, {hw}, {blend}, feather {feather}, frame f32: {(bits(fgot) != bits(fwant)).sum()} of {fgot.size} differ")
            assert all(same(g, w) for g, w in zip(got, want)) and same(fgot, fwant)
            for b in (2, 4):  # the camera-less sample and the one whose matrices are all NaN are fill values
                assert (got[0][b] == 0).all() and (got[1][b] == BKGD).all() and (bits(got[2][b]) == bits(np.float32(FILL))).all()
                assert (got[3][b] == 255).all() and np.isnan(fgot[b]).all()
            assert (got[3][0] != 255).mean() >= 0.1 and not np.isnan(fgot[0][:, got[3][0] != 255]).any()
            if n_cam > 1:
                assert (everyone[1] == drop).any() and (got[3][1] != drop).all()  # the dropped camera wins nowhere in its sample
    # the raw matrices with one camera's NaN: that camera alone is removed (the last settings: feather, 6 px)
    outs = (torch.empty(batch, channels, npix, dtype=torch.uint8, device="cuda"), torch.empty(batch, npix, dtype=torch.uint8, device="cuda"),
            torch.empty(batch, npix, dtype=torch.float32, device="cuda"), torch.empty(batch, npix, dtype=torch.uint8, device="cuda"))
    assert raw_launch(S, proj._rig, nside, npix, dev(mats), dev(present.view(np.uint8)), dev(img), dev(lab), dev(dep), outs, BKGD, FILL) == 0
    want = S.surround_to_hp_host(cals, nside, mats, img, lab, dep, present=present, **kw)
    assert all(same(o.cpu().numpy(), w) for o, w in zip(outs, want))
    assert (want[3][3] != n_cam - 1).all() and ((want[3][3] != 255).any() or n_cam == 1)
    # one plane at a time, rotations=None, no present mask, and a sample without a batch dimension
    kw = dict(kw, return_camera=False)
    ident = proj.matrices(None, batch).cpu().numpy()
    assert same(proj(masks=dev(lab)).cpu().numpy(), S.surround_to_hp_host(cals, nside, ident, masks=lab, **kw))
    assert same(proj(depth=dev(dep), rotations=rot).cpu().numpy(), S.surround_to_hp_host(cals, nside, proj.matrices(rot).cpu().numpy(), depth=dep, **kw))
    cam_only = proj(masks=dev(lab), return_camera=True)
    assert len(cam_only) == 2 and cam_only[1].dtype == torch.uint8
    one = proj(dev(img[3]), dev(lab[3]), dev(dep[3]), rotations=rot[3:4], present=present[3], return_camera=True)
    full = S.surround_to_hp_host(cals, nside, proj.matrices(rot).cpu().numpy(), img, lab, dep, present=present, **dict(kw, return_camera=True))
    assert one[0].shape == (channels, npix) and all(same(o.cpu().numpy(), w[3]) for o, w in zip(one, full))


def test_a_symmetric_rig_breaks_exact_weight_ties_by_the_lowest_index(S):
    """test_surround.symmetric_rig: pixels halfway between two optical axes have equal weights to the last bit, and the lowest index
    wins, on the device as on the host"""
    cals, mats = symmetric_rig()
    img, fimg, lab, dep = planes(5, 1, 4, 60, 80)
    perm = [3, 2, 1, 0]
    lut = np.full(256, 255, dtype=np.uint8)
    lut[:4] = perm
    for nside in (4, 16):
        npix = 12 * nside * nside
        for blend, feather in (("winner", 0.0), ("feather", 6.0)):
            kw = dict(blend=blend, edge_feather=feather, return_camera=True)
            want = S.surround_to_hp_host(cals, nside, mats, img, lab, dep, **kw)
            turned = S.surround_to_hp_host(cals, nside, mats[:, perm], img[:, perm], lab[:, perm], dep[:, perm], **kw)
            ties = lut[turned[3]] != want[3]  # with the cameras in the other order the other camera of a tie wins
            print(f"nside {nside}, {blend}: {ties.sum()} exact ties, won by cameras {np.bincount(want[3][ties], minlength=4)[:4]}")
            assert ties.sum() >= 4 and (want[3][ties] < lut[turned[3]][ties]).all()
            outs = (torch.empty(1, 3, npix, dtype=torch.uint8, device="cuda"), torch.empty(1, npix, dtype=torch.uint8, device="cuda"),
                    torch.empty(1, npix, dtype=torch.float32, device="cuda"), torch.empty(1, npix, dtype=torch.uint8, device="cuda"))
            assert raw_launch(S, S._rig(cals, blend, 95.0, feather), nside, npix, dev(mats), None, dev(img), dev(lab), dev(dep), outs) == 0
            assert all(same(o.cpu().numpy(), w) for o, w in zip(outs, want))
            fout = (torch.empty(1, 3, npix, dtype=torch.float32, device="cuda"), None, None, None)
            assert raw_launch(S, S._rig(cals, blend, 95.0, feather), nside, npix, dev(mats), None, dev(fimg), None, None, fout) == 0
            assert same(fout[0].cpu().numpy(), S.surround_to_hp_host(cals, nside, mats, fimg, blend=blend, edge_feather=feather))


# ------------------------------------------------------------------ 2. nothing is written behind an output
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_guard_bytes_behind_every_output_survive(S, kind):
    nside, npix, batch, n_cam, (h, w) = 4, 192, 3, 3, (12, 25)
    cals = rig_cals((h, w), n_cam, 8)
    proj = S.SurroundProjector(cals, nside, blend="feather", edge_feather=3.0, device="cpu")
    mats = proj.matrices(generic_matrices(31, 2)[:batch]).numpy()
    img, fimg, lab, dep = planes(32, batch, n_cam, h, w)
    frame = fimg if kind == "f32" else img
    present = np.ones((batch, n_cam), dtype=np.uint8)
    present[1, 2] = 0
    want = S.surround_to_hp_host(cals, nside, mats, frame, lab, dep, present=present, blend="feather", edge_feather=3.0, return_camera=True)
    rot, here, d_frame, d_lab, d_dep = dev(mats), dev(present), dev(frame), dev(lab), dev(dep)
    guard = 8
    o_frame = torch.full((batch * 3 * npix + guard,), 77, dtype=d_frame.dtype, device="cuda")
    o_lab = torch.full((batch * npix + guard,), 77, dtype=torch.uint8, device="cuda")
    o_dep = torch.full((batch * npix + guard,), 77.0, dtype=torch.float32, device="cuda")
    o_cam = torch.full((batch * npix + guard,), 77, dtype=torch.uint8, device="cuda")
    for given in ((True, True, True, True), (True, False, False, False), (False, True, False, True), (False, False, True, False)):
        for o in (o_frame, o_lab, o_dep, o_cam):
            o.fill_(77)
        ins = [t if g else None for t, g in zip((d_frame, d_lab, d_dep), given)]
        outs = [o if g else None for o, g in zip((o_frame, o_lab, o_dep, o_cam), given)]
        assert raw_launch(S, proj._rig, nside, npix, rot, here, *ins, outs) == 0
        for o, g, wnt in zip((o_frame, o_lab, o_dep, o_cam), given, want):
            flat = o.cpu().numpy()
            if g:  # the plane, and the guard behind it
                assert same(flat[:-guard].reshape(wnt.shape), wnt) and (flat[-guard:] == 77).all()
            else:  # a plane that was not given is not written
                assert (flat == 77).all()


# ------------------------------------------------------------------ 3. graph capture
def test_rotations_and_present_change_between_graph_replays(S):
    from heal_swin_amd import projection as P

    nside, (h, w), n_cam = 16, (12, 25), 4
    cals = rig_cals((h, w), n_cam, 6)
    img, _, lab, dep = (dev(t) for t in planes(6, 4, n_cam, h, w))
    first = P.random_rotations(4, 30.0, generator=torch.Generator().manual_seed(1))
    second = P.random_rotations(4, 30.0, generator=torch.Generator().manual_seed(2)).cuda()
    a, here = first.cuda(), torch.ones(4, n_cam, dtype=torch.bool, device="cuda")
    dropped = here.clone()
    dropped[0, 1] = dropped[2, 3] = False
    proj = S.SurroundProjector(cals, nside, frame=generic_matrices(9, 1)[0], s2_bkgd_class=BKGD)

    def step():
        return proj(img, lab, dep, rotations=a, present=here, return_camera=True)

    def equal(x, y):
        return all(torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p, q.view(torch.int32) if q.dtype == torch.float32 else q)
                   for p, q in zip(x, y))

    eager_first = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    replay_first = [t.clone() for t in out]
    a.copy_(second)
    here.copy_(dropped)
    graph.replay()
    torch.cuda.synchronize()
    replay_second = [t.clone() for t in out]
    eager_second = step()
    assert equal(replay_first, eager_first)
    assert equal(replay_second, eager_second)
    assert not torch.equal(replay_second[0], replay_first[0]) and not torch.equal(replay_second[3], replay_first[3])
    assert not (replay_second[3][0] == 1).any() and (replay_first[3][0] == 1).any()
    for rots, mask, replay in ((first, None, replay_first), (second, dropped.cpu().numpy(), replay_second)):
        host = S.surround_to_hp_host(cals, nside, proj.matrices(rots).cpu().numpy(), img.cpu().numpy(), lab.cpu().numpy(), dep.cpu().numpy(),
                                     present=mask, s2_bkgd_class=BKGD, depth_fill=float(BKGD), return_camera=True)
        assert all(same(r.cpu().numpy(), hst) for r, hst in zip(replay, host))


# ------------------------------------------------------------------ 4. end to end at a tiny size
def test_rig_to_model_step_and_back_onto_one_camera(S):
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.evaluation import SegConfusion
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys

    nside, (h, w), batch, K, n_cam = 16, (60, 80), 2, 5, 4  # nside 8 after the patch embedding, 12 base pixels
    cfg = dict(patch_size=4, window_size=16, shift_size=8, shift_strategy="nest_roll", rel_pos_bias="flat", embed_dim=16, depths=[2, 2],
               num_heads=[2, 4], mlp_ratio=4.0, qkv_bias=True, qk_scale=None, use_cos_attn=False, drop_rate=0.0, attn_drop_rate=0.0,
               drop_path_rate=0.0, use_v2_norm_placement=False, ape=False)
    spec = dict(dim_in=12 * nside * nside, f_in=3, f_out=K, base_pix=12, class_names=[])
    torch.manual_seed(0)
    model = SwinHPTransformerSys(SwinHPTransformerConfig(**cfg), DataSpec(**spec)).cuda()
    cals = rig_cals((h, w), n_cam, 44)
    rng = np.random.default_rng(4)
    imgs = dev(rng.integers(0, 256, (batch, n_cam, 3, h, w), dtype=np.uint8))
    target = dev(rng.integers(0, K, (batch, n_cam, h, w), dtype=np.uint8))
    hp_img, hp_mask, cam = S.SurroundProjector(cals, nside)(imgs, target, return_camera=True)
    assert hp_img.shape == (batch, 3, spec["dim_in"]) and hp_mask.shape == cam.shape == (batch, spec["dim_in"]) and int(hp_mask.max()) < K
    assert (cam != 255).float().mean() > 0.9
    loss, preds = model.forward_seg_step(hp_img.float(), hp_mask)
    loss.backward()
    assert torch.isfinite(loss) and preds.shape == hp_mask.shape and preds.dtype == torch.uint8
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    with torch.no_grad():
        logits = model(hp_img.float())
    ids = torch.max(logits, 1).indices.to(torch.uint8)
    c = 2
    back = S.SurroundBackProjector(cals[c], nside)
    assert back.shape == (h, w) and bool(back.valid.all())  # 12 base pixels: every image pixel is covered
    shown = back.masks(logits)
    assert shown.shape == (batch, h, w) and shown.dtype == torch.uint8 and torch.equal(shown, ids[:, back.nearest.long()])
    conf = SegConfusion(K)
    own = target[:, c].contiguous()
    conf.update(logits, own, projector=back)
    want = torch.bincount(own.long().reshape(-1) * K + shown.long().reshape(-1), minlength=K * K).view(K, K)
    assert torch.equal(conf.confmat, want) and int(want.sum()) == batch * int(back.valid.sum())
