#!/usr/bin/env python3
"""Times of adaptive sampling on the dragon-class view (871,414 triangles, 1920x1080,
plymain.cpp camera and lights, 1-spp progressive frames).

    python profiles/adaptive/measure.py [--reps 20] [--warmup 3] [--parent-lib FILE] [--no-view] [--out FILE]

Prints one JSON line:
  (a) the render's kernel times against the live share: planes with 100 %, 50 %, 10 % and 1 % of the tiles
      live (a seeded random choice), and no plane; one frame of each in turn, `--reps` rounds after
      `--warmup` — alternating, so that drift falls on all alike; medians and quartiles of
      rt_last_kernel_split_ms' main part (k_tris alone), of rt_last_kernel_ms (with the order kernel) and
      of rt_last_adaptive_ms' order kernel;
  (b) from the same rounds: all tiles live against no plane, the masked path's overhead, beside four times
      the larger interquartile range;
  (c) with --parent-lib (librtmi.so of the parent commit): the unmasked frame of this build against the
      parent's, two contexts in one process, alternating;
  (d) the stop rule's and the order kernel's times beside their compulsory traffic at the 8 TB/s HBM peak
      (the rule: 8 B of tile pair, 4 B of plane and 4 B of scratch read, 4 B of scratch written a tile, the
      stopped words; the order: 4 B of order and 4 B of plane read, 4 B written a tile);
  (e) unless --no-view: `rt_render --events d,d,...` on the same view with --converge at the defaults, with
      and without --adaptive at the defaults: traced displays and process wall time until converged (or
      --view-displays, whichever comes first), beside a one-display run's wall time (the setup both pay).

Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def spread(x):
    q = statistics.quantiles(x, n=4)
    return {"median_ms": statistics.median(x), "q1_ms": q[0], "q3_ms": q[2], "min_ms": min(x), "max_ms": max(x)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=None, help="triangles of the synthetic mesh (default: dragon class)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-view", action="store_true")
    ap.add_argument("--view-displays", type=int, default=1500)
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
    verts, idx = sc.make_mesh(n_tris)
    TRIS = pt.RayTracer.KERNEL_TRIS

    def tracer(lib=None):
        rt = pt.RayTracer(0, lib_path=lib)
        rt.setSpheres(sc.ply_scene())
        c = sc.PLY_CAMERA
        rt.setCameraSpherical(c["target"], c["elevation"], c["azimuth"], c["distance"])
        rt.setFoVAngle(sc.DEFAULT_FOV)
        rt.setSampleRate(1)
        rt.setMaxPathDepth(6)
        rt.setMesh(verts, idx)
        return rt

    def dev(n, dtype=torch.float32):
        return torch.zeros(n, dtype=dtype, device="cuda:0")

    rt = tracer()
    acc = dev(npx * 4)
    for p in range(3):  # the view's lists and schedule exist from here on
        rt.rayTrace(acc, W, H, p, kernel=TRIS)
    res = {"workload": f"{n_tris} triangles, {W}x{H}, plymain.cpp camera, 1 spp a frame", "tiles": n_tiles, "reps": args.reps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}

    # (a), (b): one frame of each configuration in turn
    rng = np.random.default_rng(1)
    rank = rng.permutation(n_tiles)
    shares = (1.0, 0.5, 0.1, 0.01)
    planes = {s: torch.from_numpy((rank >= int(round(s * n_tiles))).astype(np.int32)).cuda() for s in shares}
    plane = dev(n_tiles, torch.int32)
    got = {k: {"k_tris": [], "render": [], "order": []} for k in ("none",) + shares}
    p = 3
    for i in range(args.warmup + args.reps):
        for k in got:
            if k == "none":
                rt.setTileStop(None)
            else:
                plane.copy_(planes[k])
                torch.cuda.synchronize()
                rt.setTileStop(plane, W, H)
            rt.rayTrace(acc, W, H, p, kernel=TRIS)
            p += 1
            if i >= args.warmup:
                got[k]["k_tris"].append(rt.lastKernelSplitMs()[1])
                got[k]["render"].append(rt.lastKernelMs())
                if k != "none":
                    got[k]["order"].append(rt.lastAdaptiveMs(order=True))
    rt.setTileStop(None)
    res["live_share"] = {str(k): {m: spread(v) for m, v in d.items() if v} for k, d in got.items()}
    for k in shares:
        res["live_share"][str(k)]["live_tiles"] = int((planes[k] == 0).sum().item())
    a, b = res["live_share"]["1.0"]["render"], res["live_share"]["none"]["render"]
    iqr = max(a["q3_ms"] - a["q1_ms"], b["q3_ms"] - b["q1_ms"])
    res["all_live_against_no_plane"] = {"difference_ms": a["median_ms"] - b["median_ms"], "four_iqr_ms": 4 * iqr}

    # (c): this build's unmasked frame against the parent's
    if args.parent_lib:
        old = tracer(args.parent_lib)
        acc_old = dev(npx * 4)
        for q in range(3):
            old.rayTrace(acc_old, W, H, q, kernel=TRIS)
        ms = {"this": [], "parent": []}
        for i in range(args.warmup + args.reps):
            for name, t, buf in (("this", rt, acc), ("parent", old, acc_old)):
                t.rayTrace(buf, W, H, p, kernel=TRIS)
                if i >= args.warmup:
                    ms[name].append(t.lastKernelMs())
            p += 1
        res["unmasked_against_parent"] = {k: spread(v) for k, v in ms.items()}
        old.close()

    # (d): the stop rule and the order kernel
    tiles = torch.from_numpy(np.exp(rng.normal(np.log(0.05), 0.7, (n_tiles, 2))).astype(np.float32)).cuda()
    st, order, live = dev(4, torch.int32), dev(n_tiles, torch.int32), dev(1, torch.int32)
    base = torch.from_numpy(rng.permutation(n_tiles).astype(np.int32)).cuda()
    sel, orde = [], []
    for i in range(args.warmup + args.reps):
        plane.zero_()
        torch.cuda.synchronize()
        rt.tileStopSelect(tiles, plane, 20, W, H, stats=st)
        rt.tileStopOrder(base, plane, order, live)
        if i >= args.warmup:
            sel.append(rt.lastAdaptiveMs())
            orde.append(rt.lastAdaptiveMs(order=True))
    stopped = int((plane != 0).sum().item())
    sel_floor = (20 * n_tiles + 4 * stopped + 16) / 8e12 * 1e6
    ord_floor = (12 * n_tiles + 4) / 8e12 * 1e6
    res["stop_select"] = {**spread(sel), "compulsory_us_at_8TBps": sel_floor, "stopped": stopped}
    res["order_stop"] = {**spread(orde), "compulsory_us_at_8TBps": ord_floor, "live": int(live.item())}
    rt.close()

    # (e): the view until converged
    if not args.no_view:
        exe = ROOT / "pathtracer.cl_amd" / "rt_render"
        base_cmd = [str(exe), "--mesh", str(n_tris), "--width", str(W), "--height", str(H), "--converge"]

        def view(extra, displays):
            t0 = time.perf_counter()
            r = subprocess.run(base_cmd + extra + ["--events", ",".join(["d"] * displays)], check=True, capture_output=True,
                               text=True, timeout=900)
            wall = time.perf_counter() - t0
            lines = [json.loads(l) for l in r.stdout.splitlines()][:-1]
            traced = sum(1 for l in lines if l["rendered"])
            out = {"wall_s": wall, "traced_displays": traced, "converged": bool(lines[-1]["converged"])}
            if "tiles_active" in lines[-1]:
                out["tiles_active_last"] = lines[-1]["tiles_active"]
                out["tiles_active_by_display"] = {str(k): lines[k]["tiles_active"] for k in (15, 16, 17, 32, 64, 128, 256, 512, 1024)
                                                   if k < len(lines)}
            return out

        res["view"] = {"one_display": view([], 1), "converge": view([], args.view_displays),
                       "converge_adaptive": view(["--adaptive"], args.view_displays), "displays_cap": args.view_displays}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
