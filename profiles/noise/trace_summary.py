#!/usr/bin/env python3
"""Per-kernel durations out of a `rocprofv3 --kernel-trace` run of `profiles/noise/measure.py --reps R
--no-display`: from the run's *kernel_trace.csv, the calls of every kernel of the two meters in dispatch
order, split into measure.py's variants (each `warmup + reps` calls), the warm-ups dropped; per variant
the median, minimum and maximum, ns.

    python profiles/noise/trace_summary.py DIR [--reps 5] [--warmup 3] [--out FILE]"""
from __future__ import annotations

import csv
import json
import statistics
import sys
from pathlib import Path

# measure.py's order: per frame (rendered, all-equal) the noise meter with and without the tile plane,
# then the exposure meter
VARIANTS = {"k_noise_hist": ("rendered_tiles", "rendered_no_tiles", "all_equal_tiles", "all_equal_no_tiles"),
            "k_noise_stat": ("rendered_tiles", "rendered_no_tiles", "all_equal_tiles", "all_equal_no_tiles"),
            "k_lum_hist": ("rendered", "all_equal"), "k_exposure": ("rendered", "all_equal")}


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    root = Path(sys.argv[1])
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    reps, warmup = arg("--reps", 5), arg("--warmup", 3)
    calls = {k: [] for k in VARIANTS}
    for f in sorted(root.rglob("*kernel_trace.csv")):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                for k in VARIANTS:
                    if k in row.get("Kernel_Name", ""):
                        calls[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    res = {"source": f"rocprofv3 --kernel-trace --stats -- python profiles/noise/measure.py --reps {reps} --no-display "
                     f"(kernel durations, ns; per variant the {reps} calls after {warmup} warm-ups)"}
    for k, names in VARIANTS.items():
        ns = [d for _, d in sorted(calls[k])]
        per = warmup + reps
        if len(ns) != per * len(names):
            raise SystemExit(f"{k}: {len(ns)} calls, {per * len(names)} expected")
        for i, name in enumerate(names):
            v = ns[per * i + warmup:per * (i + 1)]
            res[f"{k}_{name}"] = {"median_ns": statistics.median(v), "min_ns": min(v), "max_ns": max(v)}
    line = json.dumps(res)
    print(line)
    if out:
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
