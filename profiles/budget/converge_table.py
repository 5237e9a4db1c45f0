#!/usr/bin/env python3
"""At which display the golden view converges with and without per-tile sample counts, on
the CPU: the restatements (tests/budget_ref.py and what it builds on) over the oracle's frames of the golden
triangle view at 64x48, 1 spp a pass, default seeds — the view `rt_render --mesh 2000 --events d,d,...
--converge T --converge-min-frames 4 --adaptive A --adaptive-max-ratio 4 --adaptive-min-frames 4
--adaptive-dilate 0 [--budget M --budget-limits ...]` shows.  Per run: the display at which the view is
converged (1-based; null: not within --displays), the tile passes traced until then, and per display the
level, the live tiles and the rounds.

    python profiles/budget/converge_table.py [--converge T] [--adaptive A] [--displays N] [--max-passes M]
                                             [--limits a,b,...] [--out FILE]

Prints one JSON line.  Needs no GPU."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

import budget_ref as br  # noqa: E402
import features_ref as fr  # noqa: E402
import noise_ref as nr  # noqa: E402
import ptload  # noqa: E402
import variance_ref as vr  # noqa: E402
from oracle import MeshBVH, Oracle  # noqa: E402

F = np.float32
CASE = "tris_64x48_sr1"
MIN_FRAMES = 4


def arg(name, default, kind=float):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def golden_view(pt, orc):
    """(W, H, Wpad, Hpad, seeds, render, variance) of the golden triangle view: the oracle's render in place,
    and rt_variance's restatement with the view's features."""
    with np.load(ROOT / "tests" / "golden" / f"{CASE}.npz", allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    m = json.loads((ROOT / "tests" / "golden" / "meta.json").read_text())["cases"][CASE]
    sc, ab = pt.scenes, pt._abi
    W, H = m["W"], m["H"]
    Wp, Hp = sc.padded_dims(W, H)
    spheres = g["spheres"].view(ab.SPHERE_DTYPE)
    bvh = MeshBVH(orc, g["verts"], g["idx"])
    cam = np.ascontiguousarray(g["camera"], F)
    rays = np.zeros(W * H, ab.RAY_DTYPE)
    assert pt.load_library().rt_primary_rays(ab.ptr(cam), W, H, ab.ptr(rays)) == ab.RT_OK
    feat = fr.features_tris(orc, rays, g["verts"], g["idx"]).reshape(-1)

    def render(acc, progression, seeds):
        orc.render_tris(acc, cam, spheres, W, H, Wp, Hp, 1, m["max_depth"], progression, seeds, g["verts"], g["idx"], bvh=bvh)

    def variance(shown, mom, length):
        return vr.variance(orc, shown, mom, length, feat, W, H)

    return W, H, Wp, Hp, sc.default_seeds(Wp, Hp), render, variance


def run(view, converge, adaptive, displays, budget_prm):
    W, H, Wp, Hp, seeds, render, variance = view
    rule = dict(threshold=adaptive, max_ratio=4.0, min_frames=MIN_FRAMES, dilate=0)
    seq = br.refine(render, variance, lambda shown, var: nr.meter(shown, var, W, H, threshold=converge), W, H, Wp, Hp, seeds,
                    displays, converge, MIN_FRAMES, rule, budget_prm)
    return {"converged_at": len(seq) if seq[-1]["converged"] else None, "tile_passes_traced": sum(d["traced"] for d in seq),
            "displays": [{"n": d["n"], "level": d["level"], "active": d["active"], "rounds": d["rounds"],
                          "by_passes": d["by_passes"]} for d in seq]}


def main():
    converge, adaptive = arg("--converge", 0.3), arg("--adaptive", 0.2)
    displays, max_passes = arg("--displays", 40, int), arg("--max-passes", 4, int)
    limits = [float(v) for v in arg("--limits", "0.1,0.2,0.4", str).split(",")]
    out = arg("--out", None, str)
    pt = ptload.load()
    view = golden_view(pt, Oracle())
    budget_prm = dict(max_passes=max_passes, limits=limits)
    line = json.dumps({"workload": "golden triangle view, 64x48, 1 spp a pass, default seeds", "converge": converge,
                       "converge_min_frames": MIN_FRAMES,
                       "adaptive": dict(threshold=adaptive, max_ratio=4.0, min_frames=MIN_FRAMES, dilate=0), "budget": budget_prm,
                       "plain": run(view, converge, adaptive, displays, None),
                       "budgeted": run(view, converge, adaptive, displays, budget_prm)})
    print(line)
    if out:
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
