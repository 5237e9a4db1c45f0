#!/usr/bin/env python3
"""Times of the first-hit feature kernel and the a-trous display filter on the dragon-class view
(871,414 triangles, 1920x1080, plymain.cpp camera and lights).

    python profiles/denoise/measure.py [--reps 20] [--warmup 3] [--passes 5] [--out FILE]

Prints one JSON line: the medians of `rt_last_features_ms` and `rt_last_denoise_ms` (HIP events of
their own) over `--reps` calls after `--warmup`, beside the 1-spp frame's kernel time they accompany
and the compulsory-traffic figure of a pass (64 B per pixel at the 8 TB/s HBM peak).  Per-pass
kernel times come from a run of their own under the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python profiles/denoise/measure.py --reps 3

Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
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
    n_tris = args.tris or sc.MESH_CONFIGS["dragon"]
    rt = pt.RayTracer(0)
    rt.setSpheres(sc.ply_scene())
    c = sc.PLY_CAMERA
    rt.setCameraSpherical(c["target"], c["elevation"], c["azimuth"], c["distance"])
    rt.setFoVAngle(sc.DEFAULT_FOV)
    rt.setSampleRate(1)
    rt.setMaxPathDepth(6)
    verts, idx = sc.make_mesh(n_tris)
    rt.setMesh(verts, idx)

    frame = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    feat = torch.zeros(2 * W * H * 4, dtype=torch.float32, device="cuda:0")
    shown = torch.zeros_like(frame)
    frame_ms = []
    for p in range(args.warmup + 5):  # the 1-spp progressive frames the filter accompanies
        rt.rayTrace(frame, W, H, p, kernel=pt.RayTracer.KERNEL_TRIS)
        frame_ms.append(rt.lastKernelMs())
    feat_ms, den_ms = [], []
    for i in range(args.warmup + args.reps):
        rt.renderFeatures(feat, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
        rt.denoise(frame, feat, shown, W, H, iterations=args.passes)
        if i >= args.warmup:
            feat_ms.append(rt.lastFeaturesMs())
            den_ms.append(rt.lastDenoiseMs())
    ids = feat.view(2, W * H, 4)[1, :, 3].contiguous().view(torch.int32)
    npx = W * H
    res = {
        "workload": f"{n_tris} triangles, {W}x{H}, plymain.cpp camera, 1 spp, {args.passes} passes",
        "reps": args.reps, "warmup": args.warmup,
        "features_ms_median": statistics.median(feat_ms), "features_ms_min": min(feat_ms), "features_ms_max": max(feat_ms),
        "denoise_ms_median": statistics.median(den_ms), "denoise_ms_min": min(den_ms), "denoise_ms_max": max(den_ms),
        "denoise_ms_per_pass": statistics.median(den_ms) / args.passes,
        "frame_1spp_kernel_ms_median": statistics.median(frame_ms[args.warmup:]),
        "compulsory_bytes_per_pass": 64 * npx,
        "compulsory_us_per_pass_at_8TBps": 64 * npx / 8e12 * 1e6,
        "mesh_pixels": int((ids >= 0).sum().item()), "box_pixels": int((ids == -1).sum().item()),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    rt.close()


if __name__ == "__main__":
    main()
