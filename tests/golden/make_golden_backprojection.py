#!/usr/bin/env python3
"""Generate tests/golden/backprojection.npz from the REFERENCE's own back-projection geometry (read-only, /root/reference).

Run in the build container only:   python tests/golden/make_golden_backprojection.py
Imports the reference's data/segmentation/project_on_s2.py exactly as make_golden.py does (same import stubs, same
calibrations) and records, as plain arrays:
  uv/<case>/{u, v}                get_uv_from_hw (:266-287) for a float, an int and a tuple output_resolution
  s2/<cal>/<res>_<rot>/{theta, phi}   project_img_points_to_s2 (:188-248) for the three calibrations x rotate_pole, at a
                                  small output resolution
  s2/fv_966x1280/full_<rot>/{theta, phi}  the same on the full 966 x 1280 FV frame, every STEP-th row and column (the
                                  100-radius table of the reference depends on the largest radius of the FULL grid)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import PROJ_CALS, _import_projection  # noqa: E402

STEP = 16
UV_CASES = {"float": 0.05, "int": 40, "tuple": (30, 41)}
S2_RES = {"fv_966x1280": (36, 48), "mvl_96x128": (24, 32), "rv_60x80": (30, 40)}


def _kind(res):
    return type(res).__name__


def main():
    P = _import_projection()
    out = {}
    fv = PROJ_CALS["fv_966x1280"]["intrinsic"]
    for name, res in UV_CASES.items():
        u, v = P.get_uv_from_hw(fv["height"], fv["width"], res)
        out[f"uv/{name}/res"], out[f"uv/{name}/kind"] = np.atleast_1d(np.array(res)), np.array(_kind(res))
        out[f"uv/{name}/u"], out[f"uv/{name}/v"] = u, v
    for key, cal in PROJ_CALS.items():
        intr = cal["intrinsic"]
        for rotate in (False, True):
            rot = "rot" if rotate else "plain"
            u, v = P.get_uv_from_hw(intr["height"], intr["width"], S2_RES[key])
            theta, phi = P.project_img_points_to_s2(u, v, cal, rotate)
            tag = f"s2/{key}/small_{rot}"
            out[tag + "/res"] = np.array(S2_RES[key])
            out[tag + "/theta"], out[tag + "/phi"] = theta, phi
            if key == "fv_966x1280":
                u, v = P.get_uv_from_hw(intr["height"], intr["width"], 1.0)
                theta, phi = P.project_img_points_to_s2(u, v, cal, rotate)
                tag = f"s2/{key}/full_{rot}"
                out[tag + "/step"] = np.array(STEP)
                out[tag + "/theta"], out[tag + "/phi"] = theta[::STEP, ::STEP], phi[::STEP, ::STEP]
    path = os.path.join(HERE, "backprojection.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
