#!/usr/bin/env python3
"""Times and figures of adaptive sampling under the temporal stage on the dragon-class
view (871,414 triangles, 1920x1080, plymain.cpp camera and lights).

    python profiles/adaptive_history/measure.py [--reps 20] [--warmup 3] [--no-view] [--out FILE]

Prints one JSON line:
  (a) from the entries' own event timers, one call of each in turn within every round, medians and quartiles:
      rt_temporal_merge against rt_temporal_merge_len (56 B a pixel against 60), rt_history_trust against
      rt_history_trust_len on the view's real features (a history of 8 frames everywhere, the accumulation
      buffer a noisier copy of it), and rt_tile_len_min with the features;
  (b) unless --no-view: `rt_render --events d x REST, l, d x AFTER` at each of --thresholds, for --temporal
      alone, --adaptive --budget alone, and --temporal --adaptive --adaptive-history without and with --budget:
      whether and after how many traced displays the view is converged() before and after the key, and the tile
      passes traced after the key (a display traces what the display before it left: the live tiles, or with a
      budget its tile_passes; the first display after the key, and every display of --temporal alone, all tiles).

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
    ap.add_argument("--no-view", action="store_true")
    ap.add_argument("--rest", type=int, default=40, help="displays before the key")
    ap.add_argument("--after", type=int, default=60, help="displays after the key")
    ap.add_argument("--thresholds", default="0.02,0.01")
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
    res = {"workload": f"{n_tris} triangles, {W}x{H}, plymain.cpp camera", "tiles": n_tiles, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(1)

    # (a): the kernels (the merges' and the minimum's times do not depend on the values; the trust test's
    # depend on which taps count, so it runs on the view's features)
    rt = pt.RayTracer(0)
    rt.setSpheres(sc.ply_scene())
    c = sc.PLY_CAMERA
    rt.setCameraSpherical(c["target"], c["elevation"], c["azimuth"], c["distance"])
    rt.setFoVAngle(sc.DEFAULT_FOV)
    verts, idx = sc.make_mesh(n_tris)
    rt.setMesh(verts, idx)
    feat = torch.zeros(8 * npx, dtype=torch.float32, device="cuda:0")
    rt.renderFeatures(feat, W, H, kernel=2)
    hist_np = rng.random(4 * npx).astype(np.float32)
    hist = torch.from_numpy(hist_np).cuda()
    cur = torch.from_numpy((hist_np + rng.normal(0.0, 0.1, 4 * npx)).astype(np.float32)).cuda()
    hist_len = torch.full((npx,), 8.0, dtype=torch.float32, device="cuda:0")
    counts = rng.integers(1, 16, n_tiles).astype(np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    cur_len = torch.from_numpy(counts[((ys >> 3) * ((W + 7) // 8) + (xs >> 3)).reshape(-1)]).cuda()
    out, out_len = torch.zeros(4 * npx, dtype=torch.float32, device="cuda:0"), torch.zeros(npx, dtype=torch.float32, device="cuda:0")
    tile_out = torch.zeros(n_tiles, dtype=torch.float32, device="cuda:0")
    got = {k: [] for k in ("merge", "merge_len", "trust", "trust_len", "tile_len_min")}
    for i in range(args.warmup + args.reps):
        keep = i >= args.warmup
        rt.temporalMerge(hist, hist_len, cur, 4.0, out, out_len, W, H)
        if keep:
            got["merge"].append(rt.lastReprojectMs(merge=True))
        rt.temporalMergeLen(hist, hist_len, cur, cur_len, out, out_len, W, H)
        if keep:
            got["merge_len"].append(rt.lastReprojectMs(merge=True))
        rt.historyTrust(hist, hist_len, cur, 4.0, feat, out_len, W, H)
        if keep:
            got["trust"].append(rt.lastTrustMs())
        rt.historyTrustLen(hist, hist_len, cur, cur_len, feat, out_len, W, H)
        if keep:
            got["trust_len"].append(rt.lastTrustMs())
        rt.tileLenMin(hist_len, feat, tile_out, W, H)
        if keep:
            got["tile_len_min"].append(rt.lastTileLenMs())
    rt.close()
    floors = {"merge": 56 * npx, "merge_len": 60 * npx, "tile_len_min": 20 * npx + 4 * n_tiles}
    res["kernels"] = {k: {**spread(v), **({"compulsory_us_at_8TBps": floors[k] / 8e12 * 1e6} if k in floors else {})} for k, v in got.items()}
    for a in ("merge", "trust"):
        res["kernels"][a + "_len"]["over_twin"] = res["kernels"][a + "_len"]["median_ms"] / res["kernels"][a]["median_ms"] - 1.0

    # (b): a resting view, one key press, until converged again
    if not args.no_view:
        cli = ROOT / "pathtracer.cl_amd" / "rt_render"
        events = ",".join(["d"] * args.rest + ["l"] + ["d"] * args.after)
        res["view"] = {"rest": args.rest, "after": args.after, "thresholds": {}}
        for th in (float(t) for t in args.thresholds.split(",")):
            base = [str(cli), "--mesh", str(n_tris), "--width", str(W), "--height", str(H), "--events", events, "--converge", str(th),
                    "--converge-min-frames", "4"]
            adaptive = ["--adaptive", str(th), "--adaptive-min-frames", "4", "--adaptive-dilate", "0"]
            budget = ["--budget", "4", "--budget-limits", ",".join(str(th * k) for k in (2, 4, 8))]

            def view(extra):
                t0 = time.perf_counter()
                r = subprocess.run(base + extra, check=True, capture_output=True, text=True, timeout=900)
                wall = time.perf_counter() - t0
                lines = [json.loads(l) for l in r.stdout.splitlines()][:-1]
                key = next(i for i, l in enumerate(lines) if l["event"] == "l")
                fig = {"wall_s": wall}
                for name, part in (("rest", lines[:key]), ("after_key", lines[key + 1:])):
                    traced = [l for l in part if l["rendered"]]
                    passes, left = 0, n_tiles  # (the planes are zeroed where the count starts afresh)
                    for l in traced:
                        passes += left
                        if "tiles_active" not in l:
                            left = n_tiles
                        else:  # (before a budget has run: one pass a live tile)
                            left = l["tile_passes"] if l.get("rounds", 0) > 0 else l["tiles_active"]
                    fig[name] = {"traced_displays": len(traced), "converged": bool(traced and traced[-1]["converged"]),
                                 "tile_passes_traced": passes, "tiles_active_last": traced[-1].get("tiles_active") if traced else None}
                return fig

            res["view"]["thresholds"][str(th)] = {
                "temporal": view(["--temporal"]), "adaptive_budget": view(adaptive + budget),
                "temporal_adaptive_history": view(["--temporal"] + adaptive + ["--adaptive-history"]),
                "temporal_adaptive_history_budget": view(["--temporal"] + adaptive + budget + ["--adaptive-history"])}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
