#!/usr/bin/env python3
"""Times of the noise meter on the dragon-class view (871,414 triangles, 1920x1080,
plymain.cpp camera and lights, eight 1-spp progressive frames with their moments and variance through
the library), beside the exposure meter's on the same frame in the same run, and the host wall time of
a display with and without setConverge.

    python profiles/noise/measure.py [--reps 20] [--warmup 3] [--out FILE]

Prints one JSON line.  Kernel times: the medians of `rt_last_noise_ms` (HIP events of their own; the
time covers the 1.5 KB reset of the counts, the histogram / tile kernel and the one-wave statistic) over
`--reps` calls after `--warmup`, beside the compulsory traffic at the 8 TB/s HBM peak (20 B a pixel read)
— with and without the tile plane, on the rendered frame and on an all-equal frame (one bin: the leader
path) — and `rt_last_tonemap_ms`' meter time on the same frame.  Display times: profiles/noise/display_time
(built from display_time.cpp by the command at its top), when it is there, run as a child process; its
JSON is merged in.

Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def stats(ms, floor_us):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "times_compulsory": med * 1e3 / floor_us}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--tris", type=int, default=None, help="triangles of the synthetic mesh (default: dragon class)")
    ap.add_argument("--no-display", action="store_true", help="kernel times only")
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
    n_tiles = ((W + 7) // 8) * ((H + 7) // 8)
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

    def dev(n, dtype=torch.float32):
        return torch.zeros(n, dtype=dtype, device="cuda:0")

    acc, prev, mom, feat, var = dev(npx * 4), dev(npx * 4), dev(npx * 4), dev(npx * 8), dev(npx)
    rt.renderFeatures(feat, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
    for n in range(1, args.frames + 1):
        prev.copy_(acc)
        torch.cuda.synchronize()
        rt.rayTrace(acc, W, H, n, kernel=pt.RayTracer.KERNEL_TRIS)
        rt.momentsAccumulate(prev, acc, n, mom, mom, W, H)
    rt.variance(acc, mom, torch.full((npx,), float(args.frames), dtype=torch.float32, device="cuda:0"), feat, var, W, H)
    equal = torch.tensor([0.25, 0.5, 0.125, 1.0], dtype=torch.float32, device="cuda:0").repeat(npx)
    equal_var = torch.full((npx,), 1e-4, dtype=torch.float32, device="cuda:0")
    tiles, hist, st = dev(2 * n_tiles), dev(pt._abi.RT_METER_BINS, torch.int32), dev(4, torch.int32)
    e = dev(1)
    noise_floor = 20 * npx / 8e12 * 1e6
    lum_floor = 16 * npx / 8e12 * 1e6
    res = {"workload": f"{n_tris} triangles, {W}x{H}, plymain.cpp camera, {args.frames} frames of 1 spp", "reps": args.reps,
           "warmup": args.warmup, "noise_compulsory_us_at_8TBps": noise_floor, "exposure_meter_compulsory_us_at_8TBps": lum_floor,
           "device": torch.cuda.get_device_name(0)}
    for name, src, v in (("rendered", acc, var), ("all_equal", equal, equal_var)):
        for with_tiles in (True, False):
            ms = []
            for i in range(args.warmup + args.reps):
                got = rt.noiseMeter(src, v, W, H, tiles=tiles if with_tiles else None, hist=hist, stats=st)
                if i >= args.warmup:
                    ms.append(rt.lastNoiseMs())
            key = f"noise_{name}_{'tiles' if with_tiles else 'no_tiles'}"
            res[key] = stats(ms, noise_floor)
            res[key]["occupied_bins"] = int((hist != 0).sum().item())
            res[key]["stats"] = {k: float(x) for k, x in got.items()}
        ms = []
        for i in range(args.warmup + args.reps):
            rt.meterExposure(src, e, W, H, rate=0.25)
            if i >= args.warmup:
                ms.append(rt.lastToneMapMs(meter=True))
        res[f"exposure_meter_{name}"] = stats(ms, lum_floor)
    rt.close()
    exe = Path(__file__).resolve().parent / "display_time"
    if exe.exists() and not args.no_display:
        r = subprocess.run([str(exe), "--tris", str(n_tris), "--width", str(W), "--height", str(H), "--reps", str(args.reps),
                            "--warmup", str(args.warmup)], check=True, capture_output=True, text=True, timeout=500)
        res["display"] = json.loads(r.stdout.splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
