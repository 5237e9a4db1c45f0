#!/usr/bin/env python3
"""Times of the variance-guided display filter's kernels on the dragon-class view (871,414
triangles, 1920x1080, plymain.cpp camera and lights), beside rt_denoise's on the
same build.

    python profiles/variance/measure.py [--reps 20] [--warmup 3] [--passes 5] [--out FILE]

Prints one JSON line: the medians over `--reps` calls after `--warmup` of `rt_last_variance_ms`
(moments; variance with every history at least min_len long, and with none — the 7x7 spatial
estimate everywhere; all passes of rt_denoise_var), of `rt_last_denoise_ms`, and of
`rt_last_reproject_ms` for a moments frame carried across a 3 degree move and merged, with the
compulsory-traffic figure of a filter pass (72 B per pixel at the 8 TB/s HBM peak).  Per-pass kernel
times come from a run of their own under the profiler, summarised by per_pass.py:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python profiles/variance/measure.py --reps 3

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
    npx = W * H
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

    def dev(n):
        return torch.zeros(n, dtype=torch.float32, device="cuda:0")

    frame, prev, mom, shown = dev(npx * 4), dev(npx * 4), dev(npx * 4), dev(npx * 4)
    feat, feat2 = dev(npx * 8), dev(npx * 8)
    var, var_out, carried, carried_len = dev(npx), dev(npx), dev(npx * 4), dev(npx)
    frames = 8  # the progressive 1-spp frames whose moments the filter reads
    long_len = torch.full((npx,), float(frames), dtype=torch.float32, device="cuda:0")
    short_len = torch.ones(npx, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    cam = rt.getCamera(W)
    rt.renderFeatures(feat, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
    for n in range(1, frames + 1):
        prev.copy_(frame)
        torch.cuda.synchronize()
        rt.rayTrace(frame, W, H, n, kernel=pt.RayTracer.KERNEL_TRIS)
        rt.momentsAccumulate(prev, frame, n, mom, mom, W, H)
    rt.setCameraSpherical(c["target"], c["elevation"], c["azimuth"] + 3.0, c["distance"])
    rt.renderFeatures(feat2, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
    t = {k: [] for k in ("moments", "variance_temporal", "variance_spatial", "denoise_var", "denoise", "reproject_moments",
                         "merge_moments")}
    scratch = dev(npx * 4)
    for i in range(args.warmup + args.reps):
        rt.momentsAccumulate(prev, frame, frames, mom, scratch, W, H)
        a = rt.lastVarianceMs("moments")
        rt.variance(frame, mom, short_len, feat, var, W, H)
        b = rt.lastVarianceMs("variance")
        rt.variance(frame, mom, long_len, feat, var, W, H)
        v = rt.lastVarianceMs("variance")
        rt.denoiseVar(frame, var, feat, shown, var_out, W, H, iterations=args.passes)
        d = rt.lastVarianceMs("denoise_var")
        rt.denoise(frame, feat, shown, W, H, iterations=args.passes)
        e = rt.lastDenoiseMs()
        rt.reproject(mom, long_len, feat, cam, feat2, carried, carried_len, W, H)
        r = rt.lastReprojectMs()
        rt.temporalMerge(carried, carried_len, mom, 1.0, scratch, carried_len, W, H)
        m = rt.lastReprojectMs(merge=True)
        if i >= args.warmup:
            for k, x in zip(t, (a, v, b, d, e, r, m)):
                t[k].append(x)
    res = {
        "workload": f"{n_tris} triangles, {W}x{H}, plymain.cpp camera, 1 spp, {frames} frames, {args.passes} passes",
        "reps": args.reps, "warmup": args.warmup,
        "compulsory_bytes_per_pass": 72 * npx,
        "compulsory_us_per_pass_at_8TBps": 72 * npx / 8e12 * 1e6,
        "device": torch.cuda.get_device_name(0),
    }
    for k, xs in t.items():
        res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = statistics.median(xs), min(xs), max(xs)
    res["denoise_var_ms_per_pass"] = res["denoise_var_ms_median"] / args.passes
    res["denoise_var_over_denoise"] = res["denoise_var_ms_median"] / res["denoise_ms_median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    rt.close()


if __name__ == "__main__":
    main()
