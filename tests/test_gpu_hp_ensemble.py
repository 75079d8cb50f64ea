"""Rotation ensembles on the GPU: `HPRotationEnsemble` (hs_hp_ensemble_add_seg / _add_depth / _finish_seg / _finish_depth) against
the numpy oracle of test_hp_ensemble.py (host tables at directions M^T g_p, float64 softmax, the same covered / valid / finite
rules) and against the host entry points, exact symmetries, the unrotated member, coverage, guards, a non-finite matrix, graph
capture, and `run` on a small model.  Cases, tolerances, exemptions and comparisons are those of test_hp_ensemble.py."""
import numpy as np
import pytest
import torch

from tests.test_hp_ensemble import (BKGD, DEPTH_CASES, MIN_W, SEG_CASES, TOL, TOL_D, TOL_P, bf16_bits, case_id, compare_depth, compare_seg,
                                    depth_case, finish_seg_numpy, one_hot_logits, run_seg_host, seg_case)
from tests.test_hp_rotate import SYMMETRIES, generic_rotations, symmetry_permutation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import __graft_entry__ as g
    g.build()
    from heal_swin_amd import hp_ensemble
    return hp_ensemble


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_pred(values, dtype, layout):
    """float32 numpy [B, K, n] (exactly representable in dtype) -> the device tensor: dense, or the padded [B, n, 16] rows viewed
    as [B, K, n] with NaNs and large numbers in the padding"""
    t = dev(values).to(torch.float32 if dtype == "f32" else torch.bfloat16)
    if layout == "dense":
        return t.contiguous()
    b, k, n = t.shape
    rows = torch.tensor([float("nan"), 1e30, -7.0], device="cuda")[torch.randint(0, 3, (b, n, 16), device="cuda")].to(t.dtype)
    rows[:, :, :k] = t.transpose(1, 2)
    return rows.transpose(1, 2)[:, :k]


def run_seg_device(E, case):
    """(ensemble after its members, probs, preds) of a case through HPRotationEnsemble"""
    from heal_swin_amd._lib import HS_PRED_ROWS16
    from heal_swin_amd.evaluation import _pred_args

    nside, base_pix, _, _, dtype, layout, _, mode, _ = case
    c = seg_case(case)
    ens = E.HPRotationEnsemble(nside, base_pix, s2_bkgd_class=BKGD, mode=mode, min_weight=MIN_W)
    for v, (a, _, valid) in zip(c["values"], c["members"]):
        pred = device_pred(v, dtype, layout)
        assert bool(_pred_args(pred, ens.npix, pred.device)[0] & HS_PRED_ROWS16) == (layout == "rows")  # both load paths are taken
        ens.add(pred, a, dev(valid))
    preds, probs = ens.finish(return_probs=True)
    return ens, probs, preds


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("case", SEG_CASES, ids=case_id)
def test_seg_ensemble_matches_the_oracle(E, case):
    _, _, batch, k, _, _, _, _, _ = case
    ens, probs, preds = run_seg_device(E, case)
    assert preds.dtype == torch.uint8 and preds.shape == (batch, ens.npix) and probs.dtype == torch.float32 and probs.shape == (batch, k, ens.npix)
    compare_seg(case, probs.cpu().numpy(), preds.cpu().numpy(), "device")
    assert torch.equal(ens.finish(), preds)  # the state stays until reset()
    again = run_seg_device(E, case)
    assert torch.equal(again[1], probs) and torch.equal(again[2], preds)  # one writer per accumulator: bit-reproducible


@pytest.mark.parametrize("case", DEPTH_CASES, ids=case_id)
def test_depth_ensemble_matches_the_oracle(E, case):
    nside, base_pix, batch, dtype, _, _ = case
    c = depth_case(case)
    ens = E.HPRotationEnsemble(nside, base_pix, min_weight=MIN_W)
    for i, (v, (a, _, valid)) in enumerate(zip(c["values"], c["members"])):
        t = dev(v).to(torch.float32 if dtype == "f32" else torch.bfloat16)
        if i % 2:  # [B, C, Npix] with channel=: read in place through the strides
            wide = torch.full((batch, 2, ens.npix), float("nan"), dtype=t.dtype, device="cuda")
            wide[:, 1] = t
            ens.add(wide, a, dev(valid), channel=1)
        else:
            ens.add(t, a, dev(valid))
    out = ens.finish()
    assert out.dtype == torch.float32 and out.shape == (batch, ens.npix)
    compare_depth(case, out.cpu().numpy(), "device")


# ------------------------------------------------------------------ 2. against the host entry points
@pytest.mark.parametrize("case", [SEG_CASES[2], SEG_CASES[5], SEG_CASES[6], SEG_CASES[9]], ids=case_id)
def test_device_matches_the_host_entry(E, case):
    """the same statements on both sides but for the exponential (v_exp_f32 on the device, expf on the host), so values are
    compared within the tolerance and class ids outside the oracle's exemptions"""
    k, mode = case[3], case[7]
    ens, probs, preds = run_seg_device(E, case)
    acc, wsum = run_seg_host(E, case)
    h_probs, h_preds = finish_seg_numpy(acc, wsum, k)
    c = seg_case(case)
    d_acc, d_wsum = ens._acc.cpu().numpy(), ens._wsum.cpu().numpy()
    print(f"{case_id(case)}: {np.count_nonzero(d_acc != acc)} of {acc.size} accumulators and {np.count_nonzero(d_wsum != wsum)} of {wsum.size} "
          f"weights differ in their bits, by at most {np.abs(d_acc - acc).max():.3e} / {np.abs(d_wsum - wsum).max():.3e}")
    assert np.abs(d_wsum - wsum).max() <= 1e-6  # the float64 weights agree to about 1e-12 (test_gpu_hp_rotate.py), rounded to fp32 once
    assert np.abs(probs.cpu().numpy() - h_probs).max() <= TOL[mode]
    assert np.array_equal(preds.cpu().numpy()[~c["exempt"]], h_preds[~c["exempt"]])


def test_depth_device_matches_the_host_entry(E):
    case = DEPTH_CASES[1]
    nside, base_pix, _, _, _, _ = case
    c = depth_case(case)
    ens = E.HPRotationEnsemble(nside, base_pix)
    acc = wsum = None
    for v, (a, rot, valid) in zip(c["values"], c["members"]):
        ens.add(dev(v), a, dev(valid))
        acc, wsum = E.add_depth_host(nside, base_pix, v, rot, valid, acc, wsum)
    d_acc, d_wsum = ens._acc.cpu().numpy(), ens._wsum.cpu().numpy()
    print(f"{np.count_nonzero(d_acc != acc)} sums and {np.count_nonzero(d_wsum != wsum)} weights of {acc.size} differ in their bits")
    assert np.abs(d_wsum - wsum).max() <= 1e-6 and (np.abs(d_acc - acc) <= TOL_D * np.abs(acc)).all()


# ------------------------------------------------------------------ 3. exact symmetries
@pytest.mark.parametrize("dtype,layout", [("f32", "dense"), ("bf16", "rows")])
@pytest.mark.parametrize("mode", ["prob", "logit"])
def test_symmetries_bring_one_hot_predictions_back_exactly(E, mode, dtype, layout):
    nside, names, k = 16, list(SYMMETRIES), 10
    npix = 12 * nside * nside
    labels = np.random.default_rng(5).integers(0, k, (len(names), npix))
    mats = np.stack([SYMMETRIES[n] for n in names])
    rotated = np.stack([labels[b][symmetry_permutation(nside, 12, mats[b])] for b in range(len(names))])  # what hs_hp_rotate shows
    ens = E.HPRotationEnsemble(nside, 12, s2_bkgd_class=BKGD, mode=mode)
    ens.add(device_pred(one_hot_logits(rotated, k), dtype, layout), mats)
    preds = ens.finish()
    assert np.array_equal(preds.cpu().numpy(), labels)
    # and the rotator's own output, brought back
    from heal_swin_amd.hp_rotate import HPRotator
    shown = HPRotator(nside, 12)(hp_mask=dev(labels.astype(np.uint8)), rotations=mats)
    assert np.array_equal(shown.cpu().numpy(), rotated)
    assert (ens.valid_plane(mats) == 1).all()


# ------------------------------------------------------------------ 4. the unrotated member alone
@pytest.mark.parametrize("k", [1, 3, 7, 10, 16])
@pytest.mark.parametrize("dtype,layout", [("f32", "dense"), ("f32", "rows"), ("bf16", "dense"), ("bf16", "rows")])
def test_identity_only_is_the_plain_argmax_and_softmax(E, k, dtype, layout):
    nside, base_pix, batch = 8, 5, 3
    v = np.random.default_rng(k).normal(0, 2, (batch, k, base_pix * 64)).astype(np.float32)
    pred = device_pred(v if dtype == "f32" else (bf16_bits(v).astype(np.uint32) << 16).view(np.float32), dtype, layout)
    ens = E.HPRotationEnsemble(nside, base_pix, s2_bkgd_class=BKGD)
    ens.add(pred)
    preds, probs = ens.finish(return_probs=True)
    assert torch.equal(preds, torch.max(pred, 1)[1].to(torch.uint8))
    err = (probs - torch.softmax(pred.float(), 1)).abs().max().item()
    print(f"K {k} {dtype} {layout}: worst |prob - softmax| {err:.3e}")
    assert err <= TOL_P
    assert (ens._wsum == 1).all()
    # torch.max's rule on the rows a random draw does not hold, in the logit mode (the sums of one unrotated member are its
    # logits): a NaN outside class 0 (where there is one), NaNs in two classes, two and all classes tied at the maximum, all -inf
    hi = k - 1
    v[:, hi, 0] = np.nan
    v[:, [k // 2, hi], 1] = np.nan
    v[:, :, 2] = -1.0
    v[:, [k // 2, hi], 2] = 5.0
    v[:, :, 3] = 0.5
    v[:, :, 4] = -np.inf
    pred = device_pred(v if dtype == "f32" else (bf16_bits(v).astype(np.uint32) << 16).view(np.float32), dtype, layout)
    ens = E.HPRotationEnsemble(nside, base_pix, s2_bkgd_class=BKGD, mode="logit")
    ens.add(pred)
    preds = ens.finish()
    want = torch.max(pred.float().cpu(), 1)[1]
    assert want[0, :5].tolist() == [hi, k // 2, k // 2, 0, 0] == np.argmax(v[0, :, :5], 0).tolist()
    assert torch.equal(preds.cpu(), want.to(torch.uint8))


# ------------------------------------------------------------------ 5. coverage, guards, non-finite matrices
def test_untaken_neighbours_carry_no_weight_and_guards_stay(E):
    from heal_swin_amd._lib import lib, ptr, stream_ptr

    case = SEG_CASES[6]  # nside 16, 8 base pixels, batch 3, 12 classes, valid planes, two rotated members
    nside, base_pix, batch, k, _, _, _, _, _ = case
    c, npix, kp = seg_case(case), 8 * 256, 12
    big = dict(acc=torch.full((batch * npix * kp + 8,), -7.0, device="cuda"), wsum=torch.full((batch * npix + 8,), -7.0, device="cuda"),
               preds=torch.full((batch * npix + 8,), 77, dtype=torch.uint8, device="cuda"),
               probs=torch.full((batch * k * npix + 8,), -7.0, device="cuda"), depth=torch.full((batch * npix + 8,), -7.0, device="cuda"))
    s = stream_ptr(big["acc"].device)
    for i, (v, (_, rot, valid)) in enumerate(zip(c["values"], c["members"])):
        pred, m, ok = dev(v), dev(rot), dev(valid)
        assert lib.hs_hp_ensemble_add_seg(nside, npix, ptr(m), batch, ptr(pred), 0, k, k * npix, npix, 1, ptr(ok), 0, int(i > 0), ptr(big["acc"]),
                                          ptr(big["wsum"]), s) == 0
    assert lib.hs_hp_ensemble_finish_seg(npix, batch, k, ptr(big["acc"]), ptr(big["wsum"]), MIN_W, BKGD, ptr(big["preds"]), ptr(big["probs"]),
                                         k * npix, npix, 1, s) == 0
    assert lib.hs_hp_ensemble_finish_depth(npix, batch, ptr(big["acc"]), ptr(big["wsum"]), MIN_W, ptr(big["depth"]), s) == 0
    host = {n: t.cpu().numpy() for n, t in big.items()}
    for n, fill in (("acc", -7.0), ("wsum", -7.0), ("preds", 77), ("probs", -7.0), ("depth", -7.0)):
        assert (host[n][-8:] == fill).all(), n
    acc, wsum = host["acc"][:-8].reshape(batch, npix, kp), host["wsum"][:-8].reshape(batch, npix)
    preds, probs = host["preds"][:-8].reshape(batch, npix), host["probs"][:-8].reshape(batch, k, npix)
    assert np.abs(wsum - c["wsum"]).max() <= 1e-6
    none = (c["wsum"] == 0) & ~c["shaky"]  # the oracle takes no neighbour there, and its brackets are not a rounding matter
    assert none.any() and (wsum[none] == 0).all() and (acc[none] == 0).all()
    assert (preds[none] == BKGD).all() and (probs.transpose(0, 2, 1)[none] == 0).all()
    assert np.isnan(host["depth"][:-8].reshape(batch, npix)[none]).all()
    compare_seg(case, probs, preds, "guarded buffers")


def test_a_non_finite_matrix_leaves_its_sample_alone(E):
    case = SEG_CASES[6]
    nside, base_pix, _, _, dtype, layout, _, mode, _ = case
    c = seg_case(case)
    (v0, v1), ((a0, _, valid0), (a1, _, valid1)) = c["values"], c["members"]
    ens = E.HPRotationEnsemble(nside, base_pix, s2_bkgd_class=BKGD, mode=mode)
    ens.add(dev(v0), a0, dev(valid0))
    first = ens._acc.clone(), ens._wsum.clone()
    bad = dev(a1)  # a device tensor: not looked at on the host
    bad[1, 2, 0] = float("nan")
    ens.add(dev(v1), bad, dev(valid1))
    assert torch.equal(ens._acc[1], first[0][1]) and torch.equal(ens._wsum[1], first[1][1])  # unchanged, bit for bit
    after = ens._acc.clone(), ens._wsum.clone()
    ens.reset()
    ens.add(dev(v0), a0, dev(valid0))
    ens.add(dev(v1), a1, dev(valid1))
    for b in (0, 2):  # the other samples as with the good matrices
        assert torch.equal(ens._acc[b], after[0][b]) and torch.equal(ens._wsum[b], after[1][b]) and not torch.equal(ens._acc[b], first[0][b])
    assert not torch.equal(ens._acc[1], first[0][1])
    ens.reset()
    ens.add(dev(v1), bad)  # as the only member: no weight anywhere in its sample
    preds, probs = ens.finish(return_probs=True)
    assert (preds[1] == BKGD).all() and (probs[1] == 0).all() and (preds[0] != BKGD).any()
    assert (ens.valid_plane(bad)[1] == 0).all()
    with pytest.raises(ValueError, match="orthogonal"):  # the same matrices from the host are refused
        ens.add(dev(v1), bad.cpu().numpy())


def test_valid_plane_marks_what_the_rotated_frame_showed(E):
    from heal_swin_amd.hp_rotate import HPRotator

    nside, a = 16, generic_rotations(12, 3)
    ens8, ens12 = E.HPRotationEnsemble(nside, 8), E.HPRotationEnsemble(nside, 12)
    v8 = ens8.valid_plane(a)
    assert v8.dtype == torch.uint8 and v8.shape == (3, 8 * 256) and set(v8.unique().tolist()) == {0, 1}
    assert (ens12.valid_plane(dev(a)) == 1).all()
    labels = torch.randint(1, 10, (3, 8 * 256), dtype=torch.uint8, device="cuda")
    shown = HPRotator(nside, 8, s2_bkgd_class=0)(hp_mask=labels, rotations=a)
    assert torch.equal(shown != 0, v8 == 1)  # exactly where the rotator filled


# ------------------------------------------------------------------ 6. graph capture
def test_rotations_change_between_graph_replays(E):
    from heal_swin_amd import projection as P
    from tests.test_projection import calibrations

    nside, base_pix, batch, k = 16, 8, 4, 12
    npix = base_pix * nside * nside
    ens = E.HPRotationEnsemble(nside, base_pix, cal_info=calibrations()["mvl_96x128"], rotate_pole=True, s2_bkgd_class=BKGD)
    rows = torch.randn((batch, npix, 16), device="cuda").mul_(4).bfloat16()
    plain, turned = rows.transpose(1, 2)[:, :k], rows.flip(1).transpose(1, 2)[:, :k].contiguous()
    depth = torch.rand((batch, npix), device="cuda") * 100
    first = P.random_rotations(batch, 5.0, flip=0.5, generator=torch.Generator().manual_seed(1))
    second = P.random_rotations(batch, 5.0, flip=0.5, generator=torch.Generator().manual_seed(2)).cuda()
    a = first.cuda()
    dens = E.HPRotationEnsemble(nside, base_pix)

    def step():
        ens.reset()
        ens.add(plain)
        ens.add(turned, a, ens.valid_plane(a))
        preds, probs = ens.finish(return_probs=True)
        dens.reset()
        dens.add(depth, a)
        return preds, probs, dens.finish()

    def same(x, y):
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
    assert same(replay_first, eager_first)
    assert same(replay_second, eager_second)
    assert not torch.equal(replay_second[1], replay_first[1]) and not torch.equal(replay_second[2].view(torch.int32), replay_first[2].view(torch.int32))


# ------------------------------------------------------------------ 7. run
def test_run_equals_the_hand_written_loop(E):
    from heal_swin_amd import projection as P
    from heal_swin_amd.data_spec import DataSpec
    from heal_swin_amd.hp_rotate import HPRotator
    from heal_swin_amd.models_torch.swin_hp_transformer import SwinHPTransformerConfig, SwinHPTransformerSys

    nside, base_pix, batch = 16, 8, 2
    cfg = dict(patch_size=4, window_size=64, shift_size=4, shift_strategy="ring_shift", rel_pos_bias="flat", embed_dim=96, depths=[2, 2],
               num_heads=[3, 6], mlp_ratio=4.0, qkv_bias=True, qk_scale=None, use_cos_attn=True, drop_rate=0.0, attn_drop_rate=0.0,
               drop_path_rate=0.0, use_v2_norm_placement=True, ape=False)
    torch.manual_seed(0)
    model = SwinHPTransformerSys(SwinHPTransformerConfig(**cfg), DataSpec(dim_in=base_pix * nside * nside, f_in=3, f_out=12, base_pix=base_pix,
                                                                          class_names=[])).to("cuda").eval()
    img = torch.randint(0, 256, (batch, 3, base_pix * nside * nside), dtype=torch.uint8, device="cuda")
    gen = torch.Generator().manual_seed(3)
    rots = [P.random_rotations(batch, 7.0, flip=0.5, generator=gen), P.random_rotations(batch, 7.0, flip=0.5, generator=gen).cuda()]
    for dtype in (torch.bfloat16, torch.float32):
        model.compute_dtype = dtype
        ens = E.HPRotationEnsemble(nside, base_pix, s2_bkgd_class=BKGD)
        preds, probs = ens.run(model, img, rots, return_probs=True)
        assert ens._members == 0  # run leaves the ensemble reset
        rot = HPRotator(nside, base_pix)
        hand = E.HPRotationEnsemble(nside, base_pix, s2_bkgd_class=BKGD)
        with torch.no_grad():
            hand.add(model(img))
            for a in rots:
                hand.add(model(rot(img, rotations=a)), a, hand.valid_plane(a))
        want_preds, want_probs = hand.finish(return_probs=True)
        assert torch.equal(preds, want_preds) and torch.equal(probs, want_probs)
        assert preds.shape == (batch, base_pix * nside * nside) and (probs.sum(1) - 1).abs().max() <= 1e-5
        without = ens.run(model, img, rots, include_identity=False)
        assert without.shape == preds.shape and not torch.equal(without, preds)
        # a depth head: channel 0 of the same outputs through the depth state
        mean = ens.run(model, img, rots[:1], channel=0)
        hand.reset()
        with torch.no_grad():
            hand.add(model(img), channel=0)
            hand.add(model(rot(img, rotations=rots[0])), rots[0], hand.valid_plane(rots[0]), channel=0)
        assert mean.dtype == torch.float32 and torch.equal(mean.view(torch.int32), hand.finish().view(torch.int32))
        # the results go straight into the metrics
        from heal_swin_amd.evaluation import SegConfusion
        conf = SegConfusion(12)
        target = torch.randint(0, 12, preds.shape, dtype=torch.uint8, device="cuda")
        conf.update(torch.where(preds == BKGD, torch.zeros_like(preds), preds), target)
        assert int(conf.confmat.sum()) == preds.numel()
