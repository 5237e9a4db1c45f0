#!/usr/bin/env python3
"""Time of the history trust kernel on the dragon-class view (871,414 triangles, 1920x1080,
plymain.cpp camera and lights), beside k_variance in its all-7x7 case in the same
process: the same window over three gathered streams.

    python profiles/trust/measure.py [--reps 20] [--warmup 3] [--out FILE]

Prints one JSON line: the median of `rt_last_trust_ms` (HIP events of its own) over `--reps` calls
after `--warmup`; the kernel's compulsory-traffic figure (16 + 16 + 4 + 32 B read and 4 B written
per pixel — a figure derived from sizes, not measured — at the 8 TB/s HBM peak); the median of
`rt_last_variance_ms`' variance kernel over the same number of calls with every history length 0, so
that every pixel takes its 7x7 window (80 B read and 4 B written per pixel by the same derivation);
and the share of pixels the test shortens.  The history is a 1-spp frame of length 8, the accumulation
buffer the next 1-spp frame of the same view.

Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

TRUST_PIXEL_BYTES = 16 + 16 + 4 + 32 + 4     # history, accumulation, length, two feature planes; the length out
VARIANCE_PIXEL_BYTES = 16 + 16 + 4 + 32 + 4  # displayed frame, moments (not read in this case), length, features; out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    rt.setFoVAngle(sc.DEFAULT_FOV)
    rt.setSampleRate(1)
    rt.setMaxPathDepth(6)
    rt.setCameraSpherical(c["target"], c["elevation"], c["azimuth"], c["distance"])
    verts, idx = sc.make_mesh(n_tris)
    rt.setMesh(verts, idx)

    def dev(n):
        return torch.zeros(n, dtype=torch.float32, device="cuda:0")

    hist, cur, feat, out, var = dev(npx * 4), dev(npx * 4), dev(npx * 8), dev(npx), dev(npx)
    rt.renderFeatures(feat, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
    rt.rayTrace(hist, W, H, 0, kernel=pt.RayTracer.KERNEL_TRIS)
    rt.rayTrace(cur, W, H, 0, kernel=pt.RayTracer.KERNEL_TRIS)  # the seeds continue: another 1-spp frame
    hist_len = torch.full((npx,), 8.0, dtype=torch.float32, device="cuda:0")
    trust_ms, var_ms = [], []
    for i in range(args.warmup + args.reps):
        rt.historyTrust(hist, hist_len, cur, 1.0, feat, out, W, H)
        if i >= args.warmup:
            trust_ms.append(rt.lastTrustMs())
    zeros = dev(npx)  # every history length below min_len: every pixel takes the 7x7 window
    for i in range(args.warmup + args.reps):
        rt.variance(cur, hist, zeros, feat, var, W, H)
        if i >= args.warmup:
            var_ms.append(rt.lastVarianceMs("variance"))
    tb, vb = TRUST_PIXEL_BYTES * npx, (VARIANCE_PIXEL_BYTES - 16) * npx  # (the moments are not read in this case)
    res = {
        "workload": f"{n_tris} triangles, {W}x{H}, plymain.cpp camera, 1-spp history of length 8 against the next 1-spp frame",
        "reps": args.reps, "warmup": args.warmup,
        "trust_ms_median": statistics.median(trust_ms), "trust_ms_min": min(trust_ms), "trust_ms_max": max(trust_ms),
        "trust_compulsory_bytes": tb, "trust_compulsory_us_at_8TBps": tb / 8e12 * 1e6,
        "variance_7x7_ms_median": statistics.median(var_ms), "variance_7x7_ms_min": min(var_ms),
        "variance_7x7_ms_max": max(var_ms),
        "variance_7x7_compulsory_bytes": vb, "variance_7x7_compulsory_us_at_8TBps": vb / 8e12 * 1e6,
        "shortened_share": float((out < hist_len).float().mean().item()),
        "device": torch.cuda.get_device_name(0),
    }
    res["trust_over_compulsory"] = res["trust_ms_median"] * 1e3 / res["trust_compulsory_us_at_8TBps"]
    res["variance_7x7_over_compulsory"] = res["variance_7x7_ms_median"] * 1e3 / res["variance_7x7_compulsory_us_at_8TBps"]
    res["trust_over_variance_7x7"] = res["trust_ms_median"] / res["variance_7x7_ms_median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    rt.close()


if __name__ == "__main__":
    main()
