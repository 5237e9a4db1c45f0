#!/usr/bin/env python3
"""A/B of librtmi builds on the display stages whose kernels call rt_display_util.h and whose device
code differs from the parent's (the exposure meter, the noise meter, the history trust), after
profiles/frame_ab.py: one process per build per round, builds alternating round by round.

    python profiles/display_shared/ab.py P1=parent.so P2=parent.so new= [--rounds 3] [--reps 40] [--out FILE]
    (LABEL= with an empty path: the in-tree build)

The view is profiles/noise/measure.py's: the dragon-class mesh (871,414 triangles) at 1920x1080 under
the plymain.cpp camera, eight 1-spp progressive frames with their moments and variance.  Per build the
median of `--reps` calls (after `--warmup`) of each stage's own timer — `rt_last_tonemap_ms`' meter time,
`rt_last_noise_ms`, `rt_last_trust_ms` — the two meters on the rendered frame and on an all-equal frame
(one bin: the leader path), and the sha1 of every output, compared across builds.  A stage passes when
the branch's median is not above the larger parent median by more than the two parent labels' medians
differ in the same call.  Prints one JSON line (also to --out).

Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
STAGES = ("meter_rendered", "meter_all_equal", "noise_rendered", "noise_all_equal", "trust")


def child(args):
    sys.path.insert(0, str(ROOT))
    import torch
    import ptload

    pt = ptload.load()
    sc = pt.scenes
    W, H, frames = 1920, 1080, 8
    npx = W * H
    n_tiles = ((W + 7) // 8) * ((H + 7) // 8)
    rt = pt.RayTracer(0, lib_path=args.lib or None)
    rt.setSpheres(sc.ply_scene())
    c = sc.PLY_CAMERA
    rt.setCameraSpherical(c["target"], c["elevation"], c["azimuth"], c["distance"])
    rt.setFoVAngle(sc.DEFAULT_FOV)
    rt.setSampleRate(1)
    rt.setMaxPathDepth(6)
    rt.setMesh(*sc.make_mesh(sc.MESH_CONFIGS["dragon"]))

    def dev(n, dtype=torch.float32):
        return torch.zeros(n, dtype=dtype, device="cuda:0")

    acc, prev, mom, feat, var = dev(npx * 4), dev(npx * 4), dev(npx * 4), dev(npx * 8), dev(npx)
    rt.renderFeatures(feat, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
    for n in range(1, frames + 1):
        prev.copy_(acc)
        torch.cuda.synchronize()
        rt.rayTrace(acc, W, H, n, kernel=pt.RayTracer.KERNEL_TRIS)
        rt.momentsAccumulate(prev, acc, n, mom, mom, W, H)
    hist_len = torch.full((npx,), float(frames - 1), dtype=torch.float32, device="cuda:0")
    rt.variance(acc, mom, torch.full((npx,), float(frames), dtype=torch.float32, device="cuda:0"), feat, var, W, H)
    equal = torch.tensor([0.25, 0.5, 0.125, 1.0], dtype=torch.float32, device="cuda:0").repeat(npx)
    equal_var = torch.full((npx,), 1e-4, dtype=torch.float32, device="cuda:0")
    tiles, hist, st = dev(2 * n_tiles), dev(pt._abi.RT_METER_BINS, torch.int32), dev(4, torch.int32)
    e, out_len = dev(1), dev(npx)
    sha = hashlib.sha1()

    def timed(call, last, outs):
        ms = []
        for i in range(args.warmup + args.reps):
            call()
            if i >= args.warmup:
                ms.append(last())
        for o in outs:
            sha.update(o.cpu().numpy().tobytes())
        return {"median_ms": statistics.median(ms), "min_ms": min(ms)}

    res = {}
    for name, src, v in (("rendered", acc, var), ("all_equal", equal, equal_var)):
        def meter():
            e.zero_()
            rt.meterExposure(src, e, W, H, hist=hist)

        res[f"meter_{name}"] = timed(meter, lambda: rt.lastToneMapMs(meter=True), (hist, e))
        res[f"noise_{name}"] = timed(lambda: rt.noiseMeter(src, v, W, H, tiles=tiles, hist=hist, stats=st), rt.lastNoiseMs,
                                     (hist, st, tiles))
    # the history: the accumulation buffer one frame earlier, seven frames long everywhere
    res["trust"] = timed(lambda: rt.historyTrust(prev, hist_len, acc, float(frames), feat, out_len, W, H), rt.lastTrustMs,
                         (out_len,))
    res["shortened"] = int((out_len < hist_len).sum().item())
    res["sha1"] = sha.hexdigest()
    rt.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = {}
    for rnd in range(args.rounds):
        for spec in (args.libs if rnd % 2 == 0 else list(reversed(args.libs))):
            label, _, path = spec.partition("=")
            r = subprocess.run([sys.executable, "-u", __file__, "--child", "--lib", path, "--reps", str(args.reps),
                                "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=240, env=dict(os.environ))
            if r.returncode != 0:  # nothing more is started on the device after a failed child
                print(r.stderr[-2000:], file=sys.stderr)
                sys.exit(r.returncode)
            line = json.loads(r.stdout.strip().split("\n")[-1])
            runs.setdefault(label, []).append(line)
            print(f"round {rnd + 1} {label}: " + " ".join(f"{s} {line[s]['median_ms']:.4f}" for s in STAGES), flush=True)
    out = {"rounds": args.rounds, "reps": args.reps, "warmup": args.warmup,
           "bit_identical": len({x["sha1"] for v in runs.values() for x in v}) == 1,
           "trust_pixels_shortened": sorted({x["shortened"] for v in runs.values() for x in v})}
    parents = [lab for lab in runs if lab != "new"]
    for s in STAGES:
        row = {lab: {"median_ms": statistics.median(x[s]["median_ms"] for x in v), "min_ms": min(x[s]["min_ms"] for x in v),
                     "round_medians_ms": [x[s]["median_ms"] for x in v]} for lab, v in runs.items()}
        if len(parents) == 2 and "new" in runs:
            p = [row[lab]["median_ms"] for lab in parents]
            row["spread_ms"] = abs(p[0] - p[1])
            row["branch_minus_parent_ms"] = row["new"]["median_ms"] - max(p)
            row["passes"] = row["branch_minus_parent_ms"] <= row["spread_ms"]
        out[s] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
