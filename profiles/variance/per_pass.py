#!/usr/bin/env python3
"""Per-pass kernel times of rt_denoise_var and rt_denoise from a rocprofv3 kernel trace of
profiles/variance/measure.py (csv output):

    python profiles/variance/per_pass.py TRACE_DIR [--out per_pass.json]

A 5-pass call dispatches the staged form at steps 1 and 2, then the gather form at steps 4, 8 and
16: the gather dispatches are told apart by their order in time."""
from __future__ import annotations

import argparse
import csv
import json
import re
import statistics
from pathlib import Path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    files = sorted(Path(args.trace_dir).rglob("*kernel_trace.csv"))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {args.trace_dir}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    us = {}

    def add(key, a, b):
        us.setdefault(key, []).append((b - a) / 1e3)

    labels = {"k_atrous_var_lds<1>": "denoise_var step 1 (lds)", "k_atrous_var_lds<2>": "denoise_var step 2 (lds)",
              "k_atrous_lds<1>": "denoise step 1 (lds)", "k_atrous_lds<2>": "denoise step 2 (lds)", "k_moments": "k_moments",
              "k_variance": "k_variance", "k_reproject": "k_reproject", "k_temporal_merge": "k_temporal_merge"}
    gather = {"k_atrous_var": ["denoise_var", 0], "k_atrous": ["denoise", 0]}
    for a, b, name in rows:
        found = re.search(r"\bk_[a-z_]+(?:<\d+>)?", name)  # no arguments, namespace or return type
        base = found.group(0) if found else ""
        if base in labels:
            add(labels[base], a, b)
        elif base in gather:
            g = gather[base]
            add(f"{g[0]} step {4 << (g[1] % 3)} (gather)", a, b)
            g[1] += 1
    res = {k: {"dispatches": len(v), "median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
           for k, v in sorted(us.items())}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
