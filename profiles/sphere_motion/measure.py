#!/usr/bin/env python3
"""Time of the sphere feature warp kernel on the main scene (clrt/main.cpp's spheres and camera) at
1920x1080 after one move of sphere 2 by (0.25, 0, 0.1).

    python profiles/sphere_motion/measure.py [--reps 20] [--warmup 3] [--out FILE]

Prints one JSON line: the median of `rt_last_sphere_warp_ms` (HIP events of its own) over `--reps` calls
after `--warmup`, beside the kernel's compulsory-traffic figure (64 B per pixel for the two feature planes
in and out; the two sphere lists are 480 B each — a figure derived from sizes, not measured — at the 8 TB/s
HBM peak), and the share of sphere 2's pixels that find history through the warped and the unwarped
features.

Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

PIXEL_BYTES = 64  # (P, t) and (N, id) read, the same two float4 written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("measure.py: no GPU visible")
    import ptload

    pt = ptload.load()
    sc, ab = pt.scenes, pt._abi
    W, H = args.width, args.height
    npx = W * H
    prev = np.asarray(sc.main_scene(), ab.SPHERE_DTYPE).reshape(-1).copy()
    cur = prev.copy()
    cur["center"][2] = cur["center"][2] + np.array((0.25, 0.0, 0.1), np.float32)
    rt = pt.RayTracer(0)
    rt.setSpheres(prev)
    c = sc.MAIN_CAMERA
    rt.setFoVAngle(sc.DEFAULT_FOV)
    rt.setSampleRate(1)
    rt.setMaxPathDepth(6)
    rt.setCameraSpherical(c["target"], c["elevation"], c["azimuth"], c["distance"])

    def dev(n):
        return torch.zeros(n, dtype=torch.float32, device="cuda:0")

    frame, prev_feat, cur_feat, warped = dev(npx * 4), dev(npx * 8), dev(npx * 8), dev(npx * 8)
    hist, hist_len, car, car_len = dev(npx * 4), torch.ones(npx, dtype=torch.float32, device="cuda:0"), dev(npx * 4), dev(npx)
    cam = rt.getCamera(W)
    rt.renderFeatures(prev_feat, W, H, kernel=pt.RayTracer.KERNEL_SPHERES)
    rt.setSpheres(cur)
    rt.renderFeatures(cur_feat, W, H, kernel=pt.RayTracer.KERNEL_SPHERES)
    frame_ms = []
    for p in range(args.warmup + 5):
        rt.rayTrace(frame, W, H, 0, kernel=pt.RayTracer.KERNEL_SPHERES)
        frame_ms.append(rt.lastKernelMs())
    dprev = torch.from_numpy(prev.view(np.uint8).copy()).cuda()
    warp_ms = []
    for i in range(args.warmup + args.reps):
        rt.warpFeaturesSpheres(cur_feat, dprev, warped, W, H)
        if i >= args.warmup:
            warp_ms.append(rt.lastSphereWarpMs())
    ids = cur_feat.view(2, npx, 4)[1, :, 3].contiguous().view(torch.int32)
    on2 = ids == -16 - 2
    share = {}
    for label, cf in (("warped", warped), ("unwarped", cur_feat)):
        rt.reproject(hist, hist_len, prev_feat, cam, cf, car, car_len, W, H, max_history=8.0)
        share[label] = float((car_len > 0)[on2].float().mean().item())
    nbytes = PIXEL_BYTES * npx
    res = {
        "workload": f"main scene, {W}x{H}, main.cpp camera, sphere 2 moved by (0.25, 0, 0.1), 1 spp",
        "reps": args.reps, "warmup": args.warmup,
        "sphere_warp_ms_median": statistics.median(warp_ms), "sphere_warp_ms_min": min(warp_ms), "sphere_warp_ms_max": max(warp_ms),
        "sphere_pixel_share": float((ids <= -16).float().mean().item()),
        "sphere2_pixels": int(on2.sum().item()),
        "warp_compulsory_bytes": nbytes,
        "warp_compulsory_us_at_8TBps": nbytes / 8e12 * 1e6,
        "sphere2_pixels_with_history_share_warped": share["warped"],
        "sphere2_pixels_with_history_share_unwarped": share["unwarped"],
        "frame_1spp_kernel_ms_median": statistics.median(frame_ms[args.warmup:]),
        "device": torch.cuda.get_device_name(0),
    }
    res["warp_over_compulsory"] = res["sphere_warp_ms_median"] * 1e3 / res["warp_compulsory_us_at_8TBps"]
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    rt.close()


if __name__ == "__main__":
    main()
