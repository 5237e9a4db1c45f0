#!/usr/bin/env python3
"""The sphere carry's effect on a dragged sphere, evaluated on the CPU: the numpy
restatements of the feature kernel, the warp, rt_reproject and rt_temporal_merge over the oracle's frames
of exactly the inputs of tests/test_gpu_sphere_motion.py::test_sphere_motion_quality — the main scene with
sphere 2 given sphere 0's diffuse material, 128 x 96, the camera static, 12 steps of sphere 2 moving 0.05
along x, 1 spp per step — against a 16-spp frame of the last step from other seeds.

    python profiles/sphere_motion/evaluate.py [--out FILE]

Prints one JSON line: mean squared errors over the whole frame and over sphere 2's pixels of the 1-spp
frame, of the merged frame with the warp at the carry's caps 2 / 4 / 8 / 16, and without the warp at cap 8.
Needs no GPU."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "oracle"))

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ptload
    import sphere_motion_ref as sm
    import temporal_ref as tr
    from oracle import Oracle, build

    build()
    orc = Oracle()
    pt = ptload.load()
    sc, ab = pt.scenes, pt._abi
    W, H, depth = 128, 96, 6
    Wp, Hp = sc.padded_dims(W, H)
    cam = sc.camera_spherical(W, **sc.MAIN_CAMERA)
    rays = np.zeros(W * H, ab.RAY_DTYPE)
    assert pt.load_library().rt_primary_rays(ab.ptr(cam), W, H, ab.ptr(rays)) == ab.RT_OK
    steps = sm.QUALITY_STEPS
    scenes = [sm.quality_spheres(sc, ab.SPHERE_DTYPE, k) for k in range(steps)]
    seeds = sc.default_seeds(Wp, Hp)
    frames, feats = [], []
    for S in scenes:
        f = np.zeros(W * H * 4, F)
        orc.render_spheres(f, cam, S, W, H, Wp, Hp, 1, depth, 0, seeds)
        frames.append(f)
        feats.append(sm.features_spheres(rays, S).reshape(-1))
    ref = np.zeros(W * H * 4, F)
    orc.render_spheres(ref, cam, scenes[-1], W, H, Wp, Hp, 16, depth, 0, sc.default_seeds(Wp, Hp, skip=12345))
    on2 = sm.sphere_pixels(feats[-1], 6, 6)
    px2 = np.zeros(W * H, bool)
    px2[on2[1][on2[2] == 2]] = True

    def mse(a, sel=slice(None)):
        d = a.reshape(-1, 4)[sel, :3].astype(np.float64) - ref.reshape(-1, 4)[sel, :3].astype(np.float64)
        return float((d * d).mean())

    def chain(cap, warp):
        hist = hl = None
        for k in range(steps):
            car, cl = np.zeros(W * H * 4, F), np.zeros(W * H, F)
            if hist is not None:
                cf = sm.warp_spheres(feats[k], scenes[k], scenes[k - 1]) if warp else feats[k]
                car, cl = tr.reproject(hist, hl, feats[k - 1], cam, cf, W, H, max_history=min(32.0, cap))
            hist, hl = tr.merge(car, cl, frames[k], 1.0, max_history=32.0)
        return hist

    res = {"workload": f"main scene, sphere 2 diffuse, {W}x{H}, {steps} steps of 0.05 along x, 1 spp, depth {depth}",
           "sphere2_pixels": int(px2.sum()), "sphere2_pixel_share": float(px2.mean()),
           "mse_1spp": mse(frames[-1]), "mse_1spp_sphere2": mse(frames[-1], px2)}
    for cap in (2, 4, 8, 16):
        m = chain(float(cap), True)
        res[f"mse_merged_cap{cap}"], res[f"mse_merged_cap{cap}_sphere2"] = mse(m), mse(m, px2)
    m = chain(8.0, False)
    res["mse_merged_nowarp_cap8"], res["mse_merged_nowarp_cap8_sphere2"] = mse(m), mse(m, px2)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
