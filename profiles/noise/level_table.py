#!/usr/bin/env python3
"""How honest the noise meter is, on the CPU: the restatements (tests/noise_ref.py,
tests/variance_ref.py) over the oracle's frames of the golden triangle view at 128x96 (camera[0:4] *= 2),
progressive 1-spp frames from the default seeds (progression 1..64, lengths n everywhere).  Per n from
min_len = 4 on, where the variance is the temporal estimate: the meter's level at percentile 0.95 (lum_floor
1e-3), the 0.95 quantile of the estimated relative error itself, and the 0.95 quantile of the actual
relative luminance error |L - L_ref| / (max(L_ref, 0) + 1e-3) against a sampleRate-32 (1,024-spp) frame
from other seeds (§4.11's reference frame).

    python profiles/noise/level_table.py [--out FILE]

Prints one JSON line.  Needs no GPU."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

import noise_ref as nr  # noqa: E402
import ptload  # noqa: E402
import variance_ref as vr  # noqa: E402
from oracle import MeshBVH, Oracle  # noqa: E402

F = np.float32
CASE = "tris_64x48_sr1"


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
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
    for n in range(1, 65):
        prev = acc.copy()
        orc.render_tris(acc, cam, spheres, W, H, Wp, Hp, 1, depth, n, seeds, g["verts"], g["idx"], bvh=bvh)
        mom = vr.moments(prev, acc, n, mom)
        if n < 4:
            continue
        m = mom.reshape(-1, 4)
        d = m[:, 1] - m[:, 0] * m[:, 0]
        var = (np.where(d > 0, d, F(0.0)).astype(F) / (F(n) - F(1.0))).astype(F)  # rt_variance where len >= min_len
        st = nr.meter(acc, var, W, H)[0]
        valid, e = nr.errors(acc, var)
        L = np.asarray(nr.lum(acc.reshape(-1, 4)), np.float64)
        actual = np.sort(np.abs(L - L_ref) / (np.maximum(L_ref, 0.0) + 1e-3))
        rows.append({"n": n, "level": float(st["level"]), "estimated_q95": float(np.sort(e[valid])[nr.rank(0.95, int(valid.sum()))]),
                     "actual_q95": float(actual[nr.rank(0.95, actual.size)]), "below_0.05": st["below"], "counted": st["counted"]})
    line = json.dumps({"workload": "golden triangle view, 128x96, 1 spp a frame, default seeds; reference: 1,024 spp, other seeds",
                       "rows": rows})
    print(line)
    if out:
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
