"""Measurement of the PLOC builder against the LBVH builder on the dragon-class mesh (871,414
triangles, the bench's own), in one process on one GPU (the record is
profiles/ploc/measure.json):

  builds   rt_set_mesh under "gpu" and "ploc", alternating: after warm-up, `--reps` builds each:
           rt_mesh_stats.build_seconds and the host clock around the synchronous call.  Then, in
           builds of their own (the events wait after every launch, so these are slower as a whole),
           the builder's own HIP events: RT_BUILD_PROFILE names a file and every build appends its
           round count and the time of each stage and of each of the round's kernels.
  frames   the bench frame (1920 x 1080, sampleRate 16, depth 6, the same seeds every frame) on the
           host build's, the LBVH's and the PLOC tree: contexts alternating in one process, median
           and quartiles of `--frames` kernel times each; `--parent-lib` adds the LBVH tree of
           another build of the library (the parent commit's) as a fourth context.  Afterwards one
           counting frame per context: the traversal's step counts.

  python profiles/ploc/measure.py [--mode builds|frames|all] [--tris N] [--parent-lib FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ptload  # noqa: E402


def stats(x, digits=3):
    q = statistics.quantiles(x, n=4) if len(x) >= 2 else [x[0]] * 3
    return dict(median=round(statistics.median(x), digits), q1=round(q[0], digits), q3=round(q[2], digits),
                min=round(min(x), digits), max=round(max(x), digits), n=len(x))


def context(pt, builder, W=1920, sr=16, lib=None):
    sc = pt.scenes
    rt = pt.RayTracer(0, lib_path=lib) if lib else pt.RayTracer(0)
    rt.setSpheres(sc.ply_scene())
    rt.setCamera(sc.camera_spherical(W, **sc.PLY_CAMERA))
    rt.setSampleRate(sr)
    rt.setMaxPathDepth(6)
    rt.setBuilder(builder)
    return rt


def builds(pt, verts, idx, reps, warm=2):
    ctxs = {b: context(pt, b) for b in ("gpu", "ploc")}
    dev, host = {b: [] for b in ctxs}, {b: [] for b in ctxs}
    for i in range(warm + reps):
        for b, rt in ctxs.items():
            t0 = time.perf_counter()
            rt.setMesh(verts, idx)
            t1 = time.perf_counter()
            if i >= warm:
                dev[b].append(rt.meshInfo()["build_seconds"] * 1e3)
                host[b].append((t1 - t0) * 1e3)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "build_profile.jsonl"
        os.environ["RT_BUILD_PROFILE"] = str(path)
        try:
            for _ in range(5):
                for rt in ctxs.values():
                    rt.setMesh(verts, idx)
        finally:
            del os.environ["RT_BUILD_PROFILE"]
        lines = [json.loads(x) for x in path.read_text().splitlines()]
    for b, rt in ctxs.items():
        info = rt.meshInfo()
        mine = [x for x in lines if x["builder"] == b]
        stages = {k: round(statistics.median([x["ms"][k] for x in mine]), 3) for k in mine[0]["ms"]}
        out[b] = dict(build_ms=stats(dev[b]), set_mesh_host_ms=stats(host[b]), rounds=mine[0]["rounds"],
                      stage_ms_by_events=stages, stage_ms_sum=round(sum(stages.values()), 3),
                      n_nodes4=info["n_nodes4"], depth4=info["depth4"], stack4=info["stack4"])
        rt.close()
        print(b, json.dumps(out[b]), flush=True)
    return out


def frames(pt, verts, idx, n_frames, parent_lib, W=1920, H=1080, sr=16, warm=2):
    sc = pt.scenes
    Wp, Hp = sc.padded_dims(W, H)
    seeds = sc.default_seeds(Wp, Hp)
    plan = [("host", "host", None), ("gpu", "gpu", None), ("ploc", "ploc", None)]
    if parent_lib:
        plan.insert(2, ("gpu_parent", "gpu", parent_lib))
    ctxs, out = {}, {}
    for name, builder, lib in plan:
        rt = context(pt, builder, W, sr, lib)
        rt.setMesh(verts, idx)
        info = rt.meshInfo()
        out[name] = dict(build_ms=round(info["build_seconds"] * 1e3, 2), n_nodes4=info["n_nodes4"], depth4=info["depth4"])
        ctxs[name] = rt
    buf = np.zeros(W * H * 4, np.float32)
    times = {name: [] for name in ctxs}
    first = None
    for i in range(warm + n_frames):  # warm-up rounds: lists, schedule, the measured-cost order
        for name, rt in ctxs.items():
            rt.setSeeds(Wp, Hp, seeds)
            rt.rayTrace(buf, W, H, 0, kernel=2)
            if i >= warm:
                times[name].append(rt.lastKernelMs())
            if first is None:
                first = buf.copy()
            assert np.array_equal(buf.view(np.uint32), first.view(np.uint32)), f"{name}: the frame differs"
    for name, rt in ctxs.items():
        rt.setCounting(True)
        rt.setSeeds(Wp, Hp, seeds)
        rt.rayTrace(buf, W, H, 0, kernel=2)
        c = rt.counters()
        out[name].update(frame_ms=stats(times[name]),
                         steps={k: int(c[k]) for k in ("nodes_visited", "leaves_visited", "tris_tested", "rays_closest",
                                                       "rays_shadow")})
        rt.close()
        print(name, json.dumps(out[name]), flush=True)
    spread = max(v["frame_ms"]["q3"] - v["frame_ms"]["q1"] for v in out.values())
    gain = out["gpu"]["frame_ms"]["median"] - out["ploc"]["frame_ms"]["median"]
    out["verdict"] = dict(spread_ms=round(spread, 3), lbvh_minus_ploc_ms=round(gain, 3),
                          ploc_faster_by_more_than_4_spreads=bool(gain > 4 * spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["builds", "frames", "all"])
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pt = ptload.load()
    sc = pt.scenes
    n = args.tris or sc.MESH_CONFIGS["dragon"]
    verts, idx = sc.make_mesh(n)
    res = dict(n_tris=n, n_verts=len(verts))
    if args.mode in ("builds", "all"):
        res["builds"] = builds(pt, verts, idx, args.reps)
    if args.mode in ("frames", "all"):
        res["frames"] = frames(pt, verts, idx, args.frames, args.parent_lib)
    text = json.dumps(res, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
