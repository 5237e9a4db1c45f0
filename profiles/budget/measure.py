#!/usr/bin/env python3
"""Times of the per-tile sample counts on the dragon-class view (871,414 triangles,
1920x1080, plymain.cpp camera and lights, 1-spp passes).

    python profiles/budget/measure.py [--reps 20] [--warmup 3] [--no-view] [--out FILE]

Prints one JSON line:
  (a) k_fold_tiles with every tile, 50 % and 1 % of the tiles folded (a seeded random choice), moments and
      lengths on, one call of each in turn within every round; medians and quartiles of rt_last_budget_ms'
      fold, beside the compulsory traffic at the 8 TB/s HBM peak: 84 B a folded pixel (sample 16, acc 16 + 16,
      moments 16 + 16, lengths 4), 4 B a pixel that is not (its length), 8 B a tile (count, passes);
  (b) k_tile_budget (with its stats' reset) and k_pass_mask, likewise (12 + 4 B and 8 + 4 B a tile);
  (c) profiles/budget/display_time (built beside this script): the host wall time of a display() of a
      resting view with setAdaptive alone and with setSampleBudget at 1, 2 and 4 rounds, alternated in one
      process, the differences beside four times the larger interquartile range;
  (d) unless --no-view: `rt_render --events d,d,...` on the same view with --converge and --adaptive at
      --threshold (a configuration where the stop rule acts), with and without --budget: traced displays and
      process wall time until converged (or --view-displays), beside a one-display run's wall time.

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
    ap.add_argument("--view-displays", type=int, default=300)
    ap.add_argument("--threshold", type=float, default=0.02, help="--converge and --adaptive threshold of (d)")
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
    res = {"workload": f"{n_tris} triangles, {W}x{H}, plymain.cpp camera, 1 spp a pass", "tiles": n_tiles, "reps": args.reps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(1)

    def dev(a):
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()

    # (a), (b): the kernels on made-up planes (their times do not depend on the values)
    rt = pt.RayTracer(0)
    sample, acc, mom = (dev(rng.random(4 * npx).astype(np.float32)) for _ in range(3))
    length = torch.zeros(npx, dtype=torch.float32, device="cuda:0")
    count = dev(rng.integers(1, 64, n_tiles).astype(np.uint32))
    rank = rng.permutation(n_tiles)
    shares = (1.0, 0.5, 0.01)
    passes = {s: dev((rank < int(round(s * n_tiles))).astype(np.uint32)) for s in shares}
    tiles = dev(np.exp(rng.normal(np.log(0.1), 0.7, (n_tiles, 2))).astype(np.float32))
    stop = dev(((rng.random(n_tiles) < 0.3) * 9).astype(np.uint32))
    out_passes, mask = (torch.zeros(n_tiles, dtype=torch.int32, device="cuda:0") for _ in range(2))
    stats = torch.zeros(13, dtype=torch.int32, device="cuda:0")
    got = {**{f"fold_{s}": [] for s in shares}, "budget": [], "mask": []}
    for i in range(args.warmup + args.reps):
        for s in shares:
            rt.foldTiles(sample, acc, count, passes[s], 0, W, H, mom_in=mom, mom_out=mom, len_out=length)
            if i >= args.warmup:
                got[f"fold_{s}"].append(rt.lastBudgetMs("fold"))
        rt.tileBudget(tiles, stop, out_passes, W, H, stats=stats)
        rt.tilePassMask(stop, out_passes, 1, mask, W, H)
        if i >= args.warmup:
            got["budget"].append(rt.lastBudgetMs("budget"))
            got["mask"].append(rt.lastBudgetMs("mask"))
    rt.close()
    res["kernels"] = {}
    for s in shares:
        folded_px = float(s) * npx  # (a tile's pixels inside the frame: on average)
        floor_us = (84 * folded_px + 4 * (npx - folded_px) + 8 * n_tiles) / 8e12 * 1e6
        res["kernels"][f"fold_{s}"] = {**spread(got[f"fold_{s}"]), "folded_tiles": int(passes[s].sum().item()),
                                       "compulsory_us_at_8TBps": floor_us}
    res["kernels"]["tile_budget"] = {**spread(got["budget"]), "compulsory_us_at_8TBps": (16 * n_tiles + 52) / 8e12 * 1e6}
    res["kernels"]["pass_mask"] = {**spread(got["mask"]), "compulsory_us_at_8TBps": 12 * n_tiles / 8e12 * 1e6}

    # (c): a display() at 1, 2 and 4 rounds against setAdaptive alone
    exe = Path(__file__).resolve().parent / "display_time"
    r = subprocess.run([str(exe), "--tris", str(n_tris), "--width", str(W), "--height", str(H), "--reps", str(args.reps), "--warmup",
                        str(args.warmup)], check=True, capture_output=True, text=True, timeout=600)
    disp = json.loads(r.stdout.splitlines()[-1])
    base = disp["display_adaptive_ms"]
    for k in ("rounds_1", "rounds_2", "rounds_4"):
        d = disp[f"display_{k}_ms"]
        d["difference_ms"] = d["median"] - base["median"]
        d["four_iqr_ms"] = 4 * max(d["q3"] - d["q1"], base["q3"] - base["q1"])
    res["display"] = disp

    # (d): the view until converged
    if not args.no_view:
        cli = ROOT / "pathtracer.cl_amd" / "rt_render"
        th = args.threshold
        base_cmd = [str(cli), "--mesh", str(n_tris), "--width", str(W), "--height", str(H), "--converge", str(th),
                    "--converge-min-frames", "4", "--adaptive", str(th), "--adaptive-min-frames", "4", "--adaptive-dilate", "0"]
        limits = ",".join(str(th * k) for k in (2, 4, 8))

        def view(extra, displays):
            t0 = time.perf_counter()
            r = subprocess.run(base_cmd + extra + ["--events", ",".join(["d"] * displays)], check=True, capture_output=True,
                               text=True, timeout=900)
            wall = time.perf_counter() - t0
            lines = [json.loads(l) for l in r.stdout.splitlines()][:-1]
            traced = [l for l in lines if l["rendered"]]
            out = {"wall_s": wall, "traced_displays": len(traced), "converged": bool(lines[-1]["converged"]),
                   "tiles_active_last": lines[-1]["tiles_active"]}
            if "tile_passes" in lines[-1]:
                out["tile_passes_budgeted"] = sum(l["tile_passes"] for l in traced)
                out["rounds_by_display"] = [l["rounds"] for l in traced][:64]
            return out

        res["view"] = {"threshold": th, "budget_limits": limits, "one_display": view([], 1),
                       "adaptive": view([], args.view_displays),
                       "adaptive_budget": view(["--budget", "4", "--budget-limits", limits], args.view_displays),
                       "displays_cap": args.view_displays}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
