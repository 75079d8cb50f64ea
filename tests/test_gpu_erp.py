"""Equirectangular panoramas to HEALPix on the GPU: `hs_erp_to_hp` against the host entry point (the same inline function in a
host loop, itself checked against a numpy model in test_erp.py) BIT FOR BIT -- frames u8 and f32, labels, depth, every
supersampling level, the identity and the exact symmetries (where the HEALPix centres sit on column-rounding boundaries, so
the last bit of every coordinate decides), generic matrices, a non-finite one, 8 and 12 base pixels, one and several blocks --
the guard bytes behind every output, `ERPProjector` under graph capture with the rotations changed between replays, and the
path end to end at a tiny size: panorama -> sphere -> model step -> back onto the panorama -> confusion matrix."""
import numpy as np
import pytest
import torch

from tests.test_erp import BKGD, FILL, bits, generic_matrices, planes
from tests.test_hp_rotate import SYMMETRIES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import erp
    return erp


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    """equal as bytes: float planes by their words, so NaNs count"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)


def case_matrices(seed):
    """the identity, Rz90, Rz180, the mirror, four generic matrices and one with a NaN: nine samples, each under its own"""
    bad = generic_matrices(seed + 1, 1)[:1].copy()
    bad[0, 1, 2] = np.nan
    return np.concatenate((np.stack([SYMMETRIES[n] for n in SYMMETRIES]), generic_matrices(seed, 2), bad))


# ------------------------------------------------------------------ 1. the kernel against the host entry point, bit for bit
# nside 4: 192 pixels, no multiple of the workgroup's 256; nside 16: 8 and 12 blocks
@pytest.mark.parametrize("nside,base_pix,hw,s", [(4, 12, (5, 7), 0), (4, 12, (16, 32), 1), (4, 8, (12, 25), 2), (16, 8, (12, 25), 0),
                                                 (16, 12, (16, 32), 1), (16, 12, (5, 7), 2)])
def test_device_equals_the_host_entry_bit_for_bit(E, nside, base_pix, hw, s):
    mats = case_matrices(nside + s)
    batch = len(mats)
    img, fimg, lab, dep = planes(3 * nside + s, batch, *hw, channels=5)  # five channels: a full group of four and a part of one
    proj = E.ERPProjector(nside, base_pix, s2_bkgd_class=BKGD, supersample=s, depth_fill=FILL)
    kw = dict(base_pix=base_pix, supersample=s, s2_bkgd_class=BKGD, depth_fill=FILL)
    got = [t.cpu().numpy() for t in proj(dev(img[:, :3]), dev(lab), dev(dep), rotations=mats)]
    want = E.erp_to_hp_host(nside, mats, img[:, :3], lab, dep, **kw)
    npix = base_pix * nside * nside
    assert [g.shape for g in got] == [(batch, 3, npix), (batch, npix), (batch, npix)]
    for name, g, w in zip(("frame u8", "labels", "depth"), got, want):
        diff = (bits(g) != bits(w)) if g.dtype == np.float32 else (g != w)
        print(f"nside {nside}, {base_pix} base pixels, {hw}, s = {s}, {name}: {diff.sum()} of {diff.size} differ")
    fgot = proj(dev(fimg), rotations=dev(mats)).cpu().numpy()  # a device tensor
    fwant = E.erp_to_hp_host(nside, mats, fimg, **kw)
    print(f"nside {nside}, {base_pix} base pixels, {hw}, s = {s}, frame f32: {(bits(fgot) != bits(fwant)).sum()} of {fgot.size} differ")
    for g, w in zip(got, want):
        assert same(g, w)
    assert same(fgot, fwant)
    assert np.isnan(fgot[-1]).all() and (got[0][-1] == 0).all() and (got[1][-1] == BKGD).all() and (bits(got[2][-1]) == bits(np.float32(FILL))).all()
    assert not np.isnan(fgot[:-1]).any() and len({got[0][b].tobytes() for b in range(batch - 1)}) == batch - 1  # each under its own matrix
    # one plane at a time, sixteen channels, and a sample without a batch dimension
    assert same(proj(masks=dev(lab), rotations=mats).cpu().numpy(), want[1])
    assert same(proj(depth=dev(dep), rotations=mats).cpu().numpy(), want[2])
    wide = np.concatenate((img, img[:, ::-1], img, img[:, :1]), 1)
    assert wide.shape[1] == 16 and same(proj(dev(wide), rotations=mats).cpu().numpy(), E.erp_to_hp_host(nside, mats, wide, **kw))
    one = proj(dev(img[4, :3]), dev(lab[4]), dev(dep[4]), rotations=mats[4:5])
    assert one[0].shape == (3, npix) and all(same(o.cpu().numpy(), w[4]) for o, w in zip(one, want))
    # rotations=None is the identity
    ident = [t.cpu().numpy() for t in proj(dev(img[:1, :3]), dev(lab[:1]), dev(dep[:1]))]
    assert all(same(i, w[:1]) for i, w in zip(ident, want))


# ------------------------------------------------------------------ 2. nothing is written behind an output
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_guard_bytes_behind_every_output_survive(E, kind):
    from heal_swin_amd._lib import HS_F32, HS_U8, lib, ptr, stream_ptr

    nside, npix, batch, (h, w), s = 4, 192, 3, (5, 7), 1
    mats = generic_matrices(31, 2)[:batch]
    img, fimg, lab, dep = planes(32, batch, h, w)
    frame = fimg if kind == "f32" else img
    want = E.erp_to_hp_host(nside, mats, frame, lab, dep, supersample=s)
    rot, d_frame, d_lab, d_dep = dev(mats), dev(frame), dev(lab), dev(dep)
    guard = 8
    o_frame = torch.full((batch * 3 * npix + guard,), 77, dtype=d_frame.dtype, device="cuda")
    o_lab = torch.full((batch * npix + guard,), 77, dtype=torch.uint8, device="cuda")
    o_dep = torch.full((batch * npix + guard,), 77.0, dtype=torch.float32, device="cuda")
    for given in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        for o in (o_frame, o_lab, o_dep):
            o.fill_(77)
        args = [ptr(t) if g else None for t, g in zip((d_frame, o_frame, d_lab, o_lab, d_dep, o_dep), np.repeat(given, 2))]
        st = lib.hs_erp_to_hp(nside, npix, ptr(rot), batch, h, w, s, args[0], HS_F32 if kind == "f32" else HS_U8, 3, args[1], args[2], args[3], 0,
                              args[4], args[5], 0.0, stream_ptr(rot.device))
        assert st == 0
        for o, g, wnt in zip((o_frame, o_lab, o_dep), given, want):
            flat = o.cpu().numpy()
            if g:  # the plane, and the guard behind it
                assert same(flat[:-guard].reshape(wnt.shape), wnt) and (flat[-guard:] == 77).all()
            else:  # a plane that was not given is not written
                assert (flat == 77).all()


# ------------------------------------------------------------------ 3. graph capture
def test_rotations_change_between_graph_replays(E):
    from heal_swin_amd import projection as P

    nside, (h, w) = 16, (12, 25)
    img, _, lab, dep = (dev(t) for t in planes(6, 4, h, w))
    first = P.random_rotations(4, 30.0, flip=0.5, generator=torch.Generator().manual_seed(1))
    second = P.random_rotations(4, 30.0, flip=0.5, generator=torch.Generator().manual_seed(2)).cuda()
    a = first.cuda()
    proj = E.ERPProjector(nside, layout=E.erp_layout(0.4, False), s2_bkgd_class=BKGD, supersample=1)

    def step():
        return proj(img, lab, dep, rotations=a)

    def equal(x, y):
        return torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2].view(torch.int32), y[2].view(torch.int32))

    eager_first = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    replay_first = [t.clone() for t in out]
    a.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    replay_second = [t.clone() for t in out]
    eager_second = step()
    assert equal(replay_first, eager_first)
    assert equal(replay_second, eager_second)
    assert not torch.equal(replay_second[0], replay_first[0]) and not torch.equal(replay_second[1], replay_first[1])
    host = E.erp_to_hp_host(nside, proj.matrices(second).cpu().numpy(), img.cpu().numpy(), lab.cpu().numpy(), dep.cpu().numpy(), supersample=1,
                            s2_bkgd_class=BKGD, depth_fill=float(BKGD))
    assert all(same(r.cpu().numpy(), hst) for r, hst in zip(replay_second, host))


# ------------------------------------------------------------------ 4. end to end at a tiny size
def test_panorama_to_model_step_and_back(E):
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.evaluation import SegConfusion
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys

    nside, (h, w), batch, K = 16, (16, 32), 2, 5  # nside 8 after the patch embedding, 12 base pixels
    cfg = dict(patch_size=4, window_size=16, shift_size=8, shift_strategy="nest_roll", rel_pos_bias="flat", embed_dim=16, depths=[2, 2],
               num_heads=[2, 4], mlp_ratio=4.0, qkv_bias=True, qk_scale=None, use_cos_attn=False, drop_rate=0.0, attn_drop_rate=0.0,
               drop_path_rate=0.0, use_v2_norm_placement=False, ape=False)
    spec = dict(dim_in=12 * nside * nside, f_in=3, f_out=K, base_pix=12, class_names=[])
    torch.manual_seed(0)
    model = SwinHPTransformerSys(SwinHPTransformerConfig(**cfg), DataSpec(**spec)).cuda()
    rng = np.random.default_rng(4)
    imgs = dev(rng.integers(0, 256, (batch, 3, h, w), dtype=np.uint8))
    target = dev(rng.integers(0, K, (batch, h, w), dtype=np.uint8))
    hp_img, hp_mask = E.ERPProjector(nside, supersample=1)(imgs, target)
    assert hp_img.shape == (batch, 3, spec["dim_in"]) and hp_mask.shape == (batch, spec["dim_in"]) and int(hp_mask.max()) < K
    loss, preds = model.forward_seg_step(hp_img.float(), hp_mask)
    loss.backward()
    assert torch.isfinite(loss) and preds.shape == hp_mask.shape and preds.dtype == torch.uint8
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    with torch.no_grad():
        logits = model(hp_img.float())
    ids = torch.max(logits, 1).indices.to(torch.uint8)
    back = E.ERPBackProjector(h, w, nside)
    shown = back.masks(logits)
    nearest = back.nearest.long()
    assert shown.shape == (batch, h, w) and shown.dtype == torch.uint8 and torch.equal(shown, ids[:, nearest])
    conf = SegConfusion(K)
    conf.update(logits, target, projector=back)
    want = torch.bincount(target.long().reshape(-1) * K + shown.long().reshape(-1), minlength=K * K).view(K, K)
    assert torch.equal(conf.confmat, want) and int(want.sum()) == batch * h * w
    depth = back.depth(logits, channel=1)  # the depth back-projection runs on the same tables
    assert depth.shape == (batch, h, w) and torch.isfinite(depth).all()
