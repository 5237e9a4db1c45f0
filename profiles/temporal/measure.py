#!/usr/bin/env python3
"""Times of the temporal reprojection and merge kernels on the dragon-class view (871,414
triangles, 1920x1080, plymain.cpp camera and lights) after one 3-degree key press.

    python profiles/temporal/measure.py [--reps 20] [--warmup 3] [--out FILE]

Prints one JSON line: the medians of `rt_last_reproject_ms` for each kernel (HIP events of their
own) over `--reps` calls after `--warmup`, beside the compulsory-traffic figures (reprojection 104 B
per pixel, merge 56 B per pixel, at the 8 TB/s HBM peak), the share of pixels that found history
and the 1-spp frame's kernel time.  Per-kernel times from the profiler come from a run of their own:

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python profiles/temporal/measure.py --reps 3

Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

REPROJECT_BYTES = 104  # cur features 32, four-tap footprint once: colour 16 + P 16 + N 16 + len 4, out 16 + 4
MERGE_BYTES = 56       # history 16 + 4, accumulation buffer 16, out 16 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--degrees", type=float, default=3.0, help="the key press: azimuth step")
    ap.add_argument("--tris", type=int, default=None, help="triangles of the synthetic mesh (default: dragon class)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("measure.py: no GPU visible")
    import ptload

    pt = ptload.load()
    sc = pt.scenes
    W, H = args.width, args.height
    npx = W * H
    n_tris = args.tris or sc.MESH_CONFIGS["dragon"]
    rt = pt.RayTracer(0)
    rt.setSpheres(sc.ply_scene())
    c = sc.PLY_CAMERA
    rt.setFoVAngle(sc.DEFAULT_FOV)
    rt.setSampleRate(1)
    rt.setMaxPathDepth(6)
    verts, idx = sc.make_mesh(n_tris)
    rt.setMesh(verts, idx)

    def dev(n):
        return torch.zeros(n, dtype=torch.float32, device="cuda:0")

    frame, prev_feat, cur_feat = dev(npx * 4), dev(npx * 8), dev(npx * 8)
    hist, hist_len, car, car_len = dev(npx * 4), dev(npx), dev(npx * 4), dev(npx)
    # the view before the key press: 8 progressive frames, displayed (merged with no history)
    rt.setCameraSpherical(c["target"], c["elevation"], c["azimuth"], c["distance"])
    prev_cam = rt.getCamera(W)
    rt.renderFeatures(prev_feat, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
    for p in range(8):
        rt.rayTrace(frame, W, H, p, kernel=pt.RayTracer.KERNEL_TRIS)
    rt.temporalMerge(car, car_len, frame, 7.0, hist, hist_len, W, H)
    # the key press, and the new view's first frame
    rt.setCameraSpherical(c["target"], c["elevation"], c["azimuth"] + args.degrees, c["distance"])
    rt.renderFeatures(cur_feat, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
    frame_ms = []
    for p in range(args.warmup + 5):
        rt.rayTrace(frame, W, H, 0, kernel=pt.RayTracer.KERNEL_TRIS)
        frame_ms.append(rt.lastKernelMs())
    shown, shown_len = dev(npx * 4), dev(npx)
    rep_ms, mrg_ms = [], []
    for i in range(args.warmup + args.reps):
        rt.reproject(hist, hist_len, prev_feat, prev_cam, cur_feat, car, car_len, W, H)
        rt.temporalMerge(car, car_len, frame, 1.0, shown, shown_len, W, H)
        if i >= args.warmup:
            rep_ms.append(rt.lastReprojectMs())
            mrg_ms.append(rt.lastReprojectMs(merge=True))
    res = {
        "workload": f"{n_tris} triangles, {W}x{H}, plymain.cpp camera, +{args.degrees:g} degrees azimuth, 1 spp",
        "reps": args.reps, "warmup": args.warmup,
        "reproject_ms_median": statistics.median(rep_ms), "reproject_ms_min": min(rep_ms), "reproject_ms_max": max(rep_ms),
        "merge_ms_median": statistics.median(mrg_ms), "merge_ms_min": min(mrg_ms), "merge_ms_max": max(mrg_ms),
        "reproject_compulsory_bytes": REPROJECT_BYTES * npx,
        "reproject_compulsory_us_at_8TBps": REPROJECT_BYTES * npx / 8e12 * 1e6,
        "merge_compulsory_bytes": MERGE_BYTES * npx,
        "merge_compulsory_us_at_8TBps": MERGE_BYTES * npx / 8e12 * 1e6,
        "valid_share": float((car_len > 0).float().mean().item()),
        "frame_1spp_kernel_ms_median": statistics.median(frame_ms[args.warmup:]),
        "device": torch.cuda.get_device_name(0),
    }
    res["reproject_over_compulsory"] = res["reproject_ms_median"] * 1e3 / res["reproject_compulsory_us_at_8TBps"]
    res["merge_over_compulsory"] = res["merge_ms_median"] * 1e3 / res["merge_compulsory_us_at_8TBps"]
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    rt.close()


if __name__ == "__main__":
    main()
