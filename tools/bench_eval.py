#!/usr/bin/env python3
"""Evaluation kernels (csrc/evaluation.hip) at HEAL-SWIN-B's output size against the torch composition a user would write
otherwise (torch.max -> index_select -> bincount): per batch of 8, nside 256, 8 base pixels, 10 classes in the model's padded
fp32 logits (rows of 16 floats, viewed as [B, 10, Npix]), WoodScape 966 x 1280 frames.  Also the host table build time of
one calibration.  Every kernel output is compared with the torch composition's before timing.
python tools/bench_eval.py [--batch 8] [--iters 20] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heal_swin_amd import evaluation as E  # noqa: E402

CAL = dict(name="FV", intrinsic=dict(aspect_ratio=1.0, cx_offset=3.942, cy_offset=-0.472, width=1280.0, height=966.0, poly_order=4,
                                     k1=339.749, k2=-31.988, k3=48.275, k4=-7.201),
           extrinsic=dict(quaternion=[0.5946970238045494, -0.5837953694518585, 0.39063952590941586, -0.39195666481783994]))


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nside", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures the HIP kernels: no GPU visible")
    dev = torch.device("cuda", 0)
    b, k, kpad = a.batch, a.classes, a.classes + (-a.classes) % 8

    tables = {}
    for rot in (False, True):
        t0 = time.perf_counter()
        proj = E.HPBackProjector(CAL, a.nside, 8, rotate_pole=rot, device=dev)
        torch.cuda.synchronize()
        tables["rot" if rot else "plain"] = time.perf_counter() - t0
    npix, n_out = proj.npix, proj.n_out
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.randn((b, npix, kpad), generator=g, device=dev)
    logits = rows[:, :, :k].transpose(1, 2)  # the model's output view
    skew = lambda shape: torch.where(torch.rand(shape, generator=g, device=dev) < 0.7, 0,  # noqa: E731
                                     torch.randint(0, k, shape, generator=g, device=dev)).to(torch.uint8)
    tgt_hp, tgt_img = skew((b, npix)), skew((b,) + proj.shape)
    hp_img = torch.randint(0, 256, (b, 3, npix), generator=g, device=dev).to(torch.uint8)
    near = proj.nearest.reshape(-1).long()
    idx, wgt = proj.idx.reshape(4, -1).long(), proj.wgt.reshape(4, -1)
    bkgd = torch.full((b, 4 * a.nside * a.nside), proj.s2_bkgd_class, dtype=torch.long, device=dev)
    fill = torch.full((b, 3, 4 * a.nside * a.nside), 255.0, dtype=torch.float64, device=dev)
    m = E.SegConfusion(k, device=dev)

    def ours_hp():
        m.update(logits, tgt_hp, check=False)

    def torch_hp():
        return torch.bincount(tgt_hp.long().reshape(-1) * k + torch.max(logits, 1)[1].reshape(-1), minlength=k * k).reshape(k, k)

    def torch_masks():
        return torch.cat([torch.max(logits, 1)[1], bkgd], 1).index_select(1, near).reshape((b,) + proj.shape)

    def ours_img():
        m.update(logits, tgt_img, projector=proj, check=False)

    def torch_img():
        return torch.bincount(tgt_img.long().reshape(-1) * k + torch_masks().reshape(-1), minlength=k * k).reshape(k, k)

    def torch_images():
        full = torch.cat([hp_img.double(), fill], 2)
        gth = [full.index_select(2, idx[j]) * wgt[j] for j in range(4)]
        return (((gth[0] + gth[1]) + gth[2]) + gth[3]).reshape((b, 3) + proj.shape)

    # outputs first: the kernels against the torch composition at the timed sizes
    m.reset()
    ours_hp()
    assert torch.equal(m.confmat, torch_hp()), "HEALPix-domain confusion differs from torch"
    assert torch.equal(proj.masks(logits).long(), torch_masks()), "back-projected labels differ from torch"
    m.reset()
    ours_img()
    assert torch.equal(m.confmat, torch_img()), "image-plane confusion differs from torch"
    img_ours, img_torch = proj.images(hp_img), torch_images()
    img_err = (img_ours - img_torch).abs().max().item()  # torch's gather-multiply-add may fuse; ours is np.sum's order
    assert img_err <= 1e-9, img_err

    covered = int(torch.unique(near[proj.valid.reshape(-1)]).numel())
    row_bytes = kpad * 4
    bytes_hp = b * npix * (row_bytes + 1)  # every logits row once + the targets
    bytes_masks = 4 * n_out + b * (covered * row_bytes + n_out)  # table, the covered rows once, the uint8 output
    bytes_img_conf = 4 * n_out + b * (covered * row_bytes + n_out)  # table, covered rows, the uint8 targets
    bytes_images = 48 * n_out + b * 3 * (npix + 8 * n_out)  # 4 x (i32 + f64) table, the planes once, f64 out
    lab_rand = torch.randint(0, k, (b, npix), generator=g, device=dev).to(torch.uint8)
    lab_one = torch.zeros((b, npix), dtype=torch.uint8, device=dev)
    res = dict(batch=b, nside=a.nside, base_pix=8, npix=npix, classes=k, logits_row_floats=kpad, frame=list(proj.shape),
               covered_hp_pixels=covered, host_table_build_s=tables)
    rows_out = {}
    for name, ours, ref, nbytes in (("hp_confusion", ours_hp, torch_hp, bytes_hp),
                                    ("backprojected_labels", lambda: proj.masks(logits), torch_masks, bytes_masks),
                                    ("image_plane_confusion", ours_img, torch_img, bytes_img_conf),
                                    ("bilinear_image", lambda: proj.images(hp_img), torch_images, bytes_images)):
        t_ours, t_torch = timed(ours, a.iters), timed(ref, a.iters)
        rows_out[name] = dict(kernel_us=round(t_ours, 1), torch_us=round(t_torch, 1), speedup=round(t_torch / t_ours, 2),
                              algorithmic_MB=round(nbytes / 1e6, 1), kernel_TBps=round(nbytes / t_ours / 1e6, 2))
    res["kernels"] = rows_out
    # LDS-histogram contention: labels of one class everywhere against uniformly random labels
    res["hp_confusion_labels_us"] = dict(random=round(timed(lambda: m.update(lab_rand, lab_rand, check=False), a.iters), 1),
                                         one_class=round(timed(lambda: m.update(lab_one, lab_one, check=False), a.iters), 1))
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
