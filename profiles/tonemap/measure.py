#!/usr/bin/env python3
"""Times of the meter and of the tone map on the dragon-class view (871,414 triangles,
1920x1080, plymain.cpp camera and lights, a 1-spp progressive frame), and the host wall time of a
display with and without the 8-bit path.

    python profiles/tonemap/measure.py [--reps 20] [--warmup 3] [--out FILE]

Prints one JSON line.  Kernel times: the medians of `rt_last_tonemap_ms` (HIP events of their own) over
`--reps` calls after `--warmup`, beside their compulsory traffic at the 8 TB/s HBM peak (the meter reads
16 B per pixel; the tone map reads 16 B and writes 4 B) — the meter (its time covers the 1.5 KB reset of
the counts, the histogram kernel and the one-lane exposure kernel) on the rendered frame and on an
all-equal frame, the tone map per curve with the sRGB encoding on and off (the difference is the cost
of rt_powf).  Display times: profiles/tonemap/display_time (built from display_time.cpp by the command
at its top), when it is there, run as a child process; its JSON is merged in.

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

    frame = torch.zeros(npx * 4, dtype=torch.float32, device="cuda:0")
    for p in range(2):  # a 1-spp progressive frame
        rt.rayTrace(frame, W, H, p, kernel=pt.RayTracer.KERNEL_TRIS)
    equal = torch.tensor([0.25, 0.5, 0.125, 1.0], dtype=torch.float32, device="cuda:0").repeat(npx)
    e = torch.zeros(1, dtype=torch.float32, device="cuda:0")
    out = torch.zeros(npx, dtype=torch.int32, device="cuda:0")
    hist = torch.zeros(pt._abi.RT_METER_BINS, dtype=torch.int32, device="cuda:0")
    meter_floor = 16 * npx / 8e12 * 1e6
    tone_floor = 20 * npx / 8e12 * 1e6
    res = {"workload": f"{n_tris} triangles, {W}x{H}, plymain.cpp camera, 1 spp", "reps": args.reps, "warmup": args.warmup,
           "meter_compulsory_us_at_8TBps": meter_floor, "tonemap_compulsory_us_at_8TBps": tone_floor,
           "device": torch.cuda.get_device_name(0)}
    for name, src in (("rendered", frame), ("all_equal", equal)):
        ms = []
        for i in range(args.warmup + args.reps):
            rt.meterExposure(src, e, W, H, hist=hist, rate=0.25)
            if i >= args.warmup:
                ms.append(rt.lastToneMapMs(meter=True))
        res[f"meter_{name}"] = stats(ms, meter_floor)
        res[f"meter_{name}"]["occupied_bins"] = int((hist != 0).sum().item())
    rt.meterExposure(frame, e, W, H)
    res["exposure"] = float(e.item())
    for curve, cname in enumerate(("clamp", "reinhard", "aces")):
        for srgb in (1, 0):
            ms = []
            for i in range(args.warmup + args.reps):
                rt.toneMap(frame, out, W, H, exposure=e, curve=curve, srgb=srgb)
                if i >= args.warmup:
                    ms.append(rt.lastToneMapMs())
            res[f"tonemap_{cname}_{'srgb' if srgb else 'linear'}"] = stats(ms, tone_floor)
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
