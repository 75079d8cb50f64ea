#!/usr/bin/env python3
"""Generate tests/golden/depth_step.npz from the REFERENCE's own depth `shared_step` body (read-only reference tree).

Run in the build container only:   python tests/golden/make_golden_depth_step.py
Uses make_golden_depth_eval's module stubs, plus the reference's real normalize_depth_data (it needs torch only) and
training/loss_depth_regression.py loaded by path.  For each (transform, normalisation) pair, the four losses taken in turn, the body of
models_lightning/depth_estimation/model_lightning_depth_swin_hp.py:132-159 runs on random outputs [2, f_out, 3072]:

    outputs[:, 0] = transform_and_normalize(outputs[:, 0]); loss = get_depth_loss(cfg)(outputs, masks)
    outputs[:, 0] = unnormalize_and_retransform(outputs[:, 0]); masks = unnormalize_and_retransform(masks)
    DepthMSE / MeanSTD / MeanSTDMedian .update(outputs, masks)

The reference's model emits metres and normalises them for the loss; this project's head emits the normalised value.  So a case
draws the NORMALISED head outputs n, gives the reference h = unnormalize_and_retransform(n) as its model output and stores n as
`outputs`: the reference's loss is then taken on transform_and_normalize(unnormalize_and_retransform(n)), this project's on n (the
documented deviation), which agree to rounding because every h is checked to be finite and >= 1e-3.  Arrays only:
  cases                         "<transform>|<normalisation>|<loss>" names
  <case>/outputs  f32 [2, f_out, 3072]   normalised head outputs (channel 1: log variance)
  <case>/target   f32 [2, 3072]          the dataset's normalised target (background = +inf)
  <case>/huber_delta, <case>/loss, <case>/returned (the step's returned outputs, channel 0 in metres), <case>/mse and, with the
  log variance, <case>/mean_std, <case>/median_std
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_depth_eval import _import_depth  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _import():
    DU, CM = _import_depth()
    root = os.path.dirname(os.path.dirname(os.path.abspath(DU.__file__)))  # .../heal_swin
    ND = _load("_ref_normalize_depth_data", os.path.join(root, "data", "depth_estimation", "normalize_depth_data.py"))
    DU.normalize_depth_data = ND  # the real module in place of the annotation stub
    cfg_name = "heal_swin.models_lightning.depth_estimation.depth_common_config"
    if cfg_name not in sys.modules:  # (the loss module reads the config class for an annotation only)
        for k in range(2, 5):
            parent = ".".join(cfg_name.split(".")[:k])
            sys.modules.setdefault(parent, types.ModuleType(parent))
        sys.modules[cfg_name].CommonDepthConfig = object
    LD = _load("_ref_loss_depth_regression", os.path.join(root, "training", "loss_depth_regression.py"))
    return DU, CM, ND, LD


def main():
    DU, CM, ND, LD = _import()
    rng = np.random.default_rng(20261017)
    B, N = 2, 3072
    out, cases = {}, []
    for transform in ("None", "log", "inv"):
        for norm in ("None", "standardize", "min-max"):
            stats = ND.get_depth_data_stats(data_transform=transform, mask_background=False)
            kw = dict(normalization=norm, data_stats=stats, data_transform=transform)
            # every (transform, normalisation) pair, the four losses in turn (each at least twice): the file stays under 1 MiB
            for loss_name in (("l1", "l2", "huber", "logvar")[len(cases) % 4],):
                use_logvar = loss_name == "logvar"
                f_out = 2 if use_logvar else 1
                # depths of 0.5 .. 20 m (inside every transform's domain), 4 % background (0 -> +inf as the dataset does)
                depth = torch.from_numpy(rng.uniform(0.5, 20.0, (B, N)).astype(np.float32))
                masks = depth.clone()
                masks[torch.from_numpy(rng.random((B, N)) < 0.04)] = float("inf")
                masks = DU.transform_and_normalize(data=masks, **kw)
                pred_m = depth * torch.from_numpy(rng.uniform(0.8, 1.25, (B, N)).astype(np.float32))
                n0 = DU.transform_and_normalize(data=pred_m.clone(), **kw)  # the normalised head output, channel 0
                chans = [n0] + ([torch.from_numpy(rng.normal(0.3, 0.8, (B, N)).astype(np.float32))] if use_logvar else [])
                stored = torch.stack(chans, 1).contiguous()
                outputs = stored.clone()
                outputs[:, 0] = DU.unnormalize_and_retransform(data=outputs[:, 0].clone(), **kw)  # the reference model's output: metres
                h = outputs[:, 0].clone()
                assert bool(torch.isfinite(h).all()) and float(h.min()) >= 1e-3, (transform, norm, float(h.min()))
                cfg = types.SimpleNamespace(use_logvar=use_logvar, loss="l2" if use_logvar else loss_name, huber_delta=0.7)
                loss_fn = LD.get_depth_loss(cfg)
                # ---- the body of shared_step
                outputs[:, 0, ...] = DU.transform_and_normalize(data=outputs[:, 0, ...], **kw)
                loss = loss_fn(outputs, masks.clone(), mask_background=False)
                outputs[:, 0, ...] = DU.unnormalize_and_retransform(data=outputs[:, 0, ...], **kw)
                metres = DU.unnormalize_and_retransform(data=masks.clone(), **kw)
                ms = {"mse": CM.DepthMSE()}
                if use_logvar:
                    ms["mean_std"], ms["median_std"] = CM.MeanSTD(), CM.MeanSTDMedian()
                for m in ms.values():
                    m.update(outputs.clone(), metres.clone())
                # ----
                assert bool(torch.isfinite(outputs[:, 0]).all()) and float(outputs[:, 0].min()) >= 1e-3
                c = f"{transform}|{norm}|{loss_name}"
                cases.append(c)
                out[c + "/outputs"], out[c + "/target"] = stored.numpy(), masks.numpy()
                out[c + "/huber_delta"] = np.asarray(0.7)
                out[c + "/loss"] = np.asarray(float(loss), dtype=np.float64)
                out[c + "/returned"] = outputs.numpy().copy()
                for k, m in ms.items():
                    out[c + "/" + k] = np.asarray(float(m.compute()), dtype=np.float64)
                print(c, "loss", float(loss), {k: float(out[c + "/" + k]) for k in ms},
                      "round trip", float(((outputs[:, 0] - h).abs() / h).max()))
    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "depth_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
