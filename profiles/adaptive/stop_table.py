#!/usr/bin/env python3
"""What the stop rule stops, and how good it is when it does, on the CPU: the
restatements (tests/adaptive_ref.py, tests/noise_ref.py, tests/variance_ref.py) over the oracle's frames of
the golden triangle view at 128x96 (camera[0:4] *= 2), progressive 1-spp frames from the default seeds
(progression 1..64) — profiles/noise/level_table.py's view — rendered the way the view renders them with
setAdaptive: under the stop plane, stopped tiles keeping accumulation, moments and length.  The rule runs
at rt_adaptive_defaults' parameters (--min-frames N for another min_frames).  Per n at which the live
share changes, and at the table's fixed n: the live tiles, and for the pixels of the tiles stopped so far
the 0.95 quantile of the actual relative luminance error |L - L_ref| / (max(L_ref, 0) + 1e-3) against a
sampleRate-32 (1,024-spp) frame from other seeds, beside the threshold, with that error's maximum and the
share of those pixels whose error is not exactly 0; the same quantile for the pixels of the tiles each n
stopped and for the live tiles' pixels; and the meter's level of the whole frame.

    python profiles/adaptive/stop_table.py [--min-frames N] [--out FILE]

Prints one JSON line.  Needs no GPU."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

import adaptive_ref as ar  # noqa: E402
import noise_ref as nr  # noqa: E402
import ptload  # noqa: E402
from oracle import MeshBVH, Oracle  # noqa: E402

F = np.float32
U = np.uint32
CASE = "tris_64x48_sr1"
FIXED = (16, 17, 20, 24, 32, 48, 64)


def q95(x):
    x = np.sort(x)
    return float(x[nr.rank(0.95, x.size)]) if x.size else None


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    rule = dict(ar.DEFAULTS)
    if "--min-frames" in sys.argv:
        rule["min_frames"] = int(sys.argv[sys.argv.index("--min-frames") + 1])
    pt = ptload.load()
    sc, orc = pt.scenes, Oracle()
    with np.load(ROOT / "tests" / "golden" / f"{CASE}.npz", allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    depth = json.loads((ROOT / "tests" / "golden" / "meta.json").read_text())["cases"][CASE]["max_depth"]
    W, H = 128, 96
    Wp, Hp = sc.padded_dims(W, H)
    cam = g["camera"].copy()
    cam[0:4] *= 2
    spheres = g["spheres"].view(pt._abi.SPHERE_DTYPE)
    bvh = MeshBVH(orc, g["verts"], g["idx"])
    ref = np.zeros(W * H * 4, F)
    orc.render_tris(ref, cam, spheres, W, H, Wp, Hp, 32, depth, 0, sc.default_seeds(Wp, Hp, skip=12345).copy(), g["verts"],
                    g["idx"], bvh=bvh)
    L_ref = np.asarray(nr.lum(ref.reshape(-1, 4)), np.float64)
    seeds = sc.default_seeds(Wp, Hp).copy()
    acc, mom, rows = np.zeros(W * H * 4, F), None, []
    stop = np.zeros(ar.n_tiles(W, H), U)
    for n in range(1, 65):
        prev, seeds_prev, full = acc.copy(), seeds.copy(), acc.copy()
        orc.render_tris(full, cam, spheres, W, H, Wp, Hp, 1, depth, n, seeds, g["verts"], g["idx"], bvh=bvh)
        acc, seeds = ar.masked(stop, W, H, Wp, Hp, prev, full, seeds_prev, seeds)
        mom, length = ar.moments_tiles(prev, acc, n, mom, stop, W, H)
        if n < 4:
            continue
        st, _, tiles = nr.meter(acc, ar.variance_temporal(mom, length), W, H)
        stop, sel = ar.select(tiles, stop, n, W, H, **rule)
        if not (sel["stopped_now"] or n in FIXED):
            continue
        L = np.asarray(nr.lum(acc.reshape(-1, 4)), np.float64)
        actual = np.abs(L - L_ref) / (np.maximum(L_ref, 0.0) + 1e-3)
        px_stop = stop[ar.pixel_tiles(W, H)]
        rows.append({"n": n, "live": sel["active"], "live_share": sel["active"] / sel["tiles"], "stopped_now": sel["stopped_now"],
                     "stopped_actual_q95": q95(actual[px_stop != 0]),
                     "stopped_actual_max": float(actual[px_stop != 0].max()) if (px_stop != 0).any() else None,
                     "stopped_nonzero_share": float((actual[px_stop != 0] > 0).mean()) if (px_stop != 0).any() else None, "stopped_now_actual_q95": q95(actual[px_stop == n]),
                     "live_actual_q95": q95(actual[px_stop == 0]), "level": float(st["level"])})
    line = json.dumps({"workload": "golden triangle view, 128x96, 1 spp a frame, default seeds, rendered under the stop plane; "
                                   "reference: 1,024 spp, other seeds", "rule": rule, "tiles": int(stop.size), "rows": rows})
    print(line)
    if out:
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
