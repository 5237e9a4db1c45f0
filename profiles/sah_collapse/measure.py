"""Measurement of RT_COLLAPSE_SAH (the device builders' collapse by dynamic programming, DESIGN.md
§4.6c) on the dragon-class mesh (871,414 triangles, the bench's own), in one process on one GPU; the
record is profiles/sah_collapse/measure.json.

  builds   rt_set_mesh under "gpu" and "ploc", build options off and on, collapse greedy and sah
           (and, with --parent-lib, under the parent commit's library: the greedy baseline),
           alternating in a rotating order: after warm-up `--reps` builds each,
           rt_mesh_stats.build_seconds.  Then, in builds of their own, the builder's HIP events
           per stage (RT_BUILD_PROFILE; "collapse_cost" is k_collapse_cost and its parent links).
  frames   the bench frame (1920 x 1080, sampleRate 16, depth 6, the same seeds every frame) on
           every tree and the host-built one: contexts alternating in a rotating order, median and
           quartiles of `--frames` kernel times each, then one counting frame per context (the
           traversal's step counts).

A gain of sah over greedy counts as shown only beyond four times the largest interquartile range
among the device contexts.

  python profiles/sah_collapse/measure.py [--tris N] [--parent-lib FILE] [--reps R] [--frames F] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

import ptload  # noqa: E402


def stats(x, digits=3):
    q = statistics.quantiles(x, n=4) if len(x) >= 2 else [x[0]] * 3
    return dict(median=round(statistics.median(x), digits), q1=round(q[0], digits), q3=round(q[2], digits),
                min=round(min(x), digits), max=round(max(x), digits), n=len(x))


def iqr(s):
    return s["q3"] - s["q1"]


def context(pt, builder, lights, mode, lib=None, W=1920, sr=16):
    sc = pt.scenes
    rt = pt.RayTracer(0, lib_path=lib) if lib else pt.RayTracer(0)
    rt.setSpheres(sc.ply_scene())
    rt.setCamera(sc.camera_spherical(W, **sc.PLY_CAMERA))
    rt.setSampleRate(sr)
    rt.setMaxPathDepth(6)
    rt.setBuilder(builder)
    if lights:
        rt.setBuildOptions(True)
    if mode == "sah":
        rt.setCollapse("sah")
    return rt


def plan(parent_lib):
    """(name, builder, lights, mode, library)"""
    p = [("host", "host", False, "greedy", None)]
    for b in ("gpu", "ploc"):
        for lights in (False, True):
            tag = f"{b}_{'on' if lights else 'off'}"
            if parent_lib:
                p.append((f"{tag}_parent", b, lights, "greedy", parent_lib))
            p.append((f"{tag}_greedy", b, lights, "greedy", None))
            p.append((f"{tag}_sah", b, lights, "sah", None))
    return p


def rotated(names, i):
    return names[i % len(names):] + names[:i % len(names)]


def run(pt, verts, idx, reps, n_frames, parent_lib, W=1920, H=1080, sr=16, warm=2):
    sc = pt.scenes
    ctxs = {name: context(pt, b, lights, mode, lib, W, sr) for name, b, lights, mode, lib in plan(parent_lib)}
    out = {name: {} for name in ctxs}
    # ---- builds
    dev = {name: [] for name in ctxs if name != "host"}
    names = list(dev)
    for i in range(warm + reps):
        for name in rotated(names, i):
            ctxs[name].setMesh(verts, idx)
            if i >= warm:
                dev[name].append(ctxs[name].meshInfo()["build_seconds"] * 1e3)
    ctxs["host"].setMesh(verts, idx)
    out["host"]["build_ms"] = round(ctxs["host"].meshInfo()["build_seconds"] * 1e3, 2)
    with tempfile.TemporaryDirectory() as tmp:  # the stage split, by the builder's own events
        for name in names:
            if name.endswith("_parent"):
                continue
            path = Path(tmp) / f"{name}.jsonl"
            os.environ["RT_BUILD_PROFILE"] = str(path)
            try:
                for _ in range(5):
                    ctxs[name].setMesh(verts, idx)
            finally:
                del os.environ["RT_BUILD_PROFILE"]
            lines = [json.loads(x) for x in path.read_text().splitlines()]
            out[name]["stage_ms_by_events"] = {k: round(statistics.median([x["ms"][k] for x in lines]), 3)
                                               for k in lines[0]["ms"]}
    for name in ctxs:
        if name in dev:
            out[name]["build_ms"] = stats(dev[name])
        info = ctxs[name].meshInfo()
        out[name].update({k: info[k] for k in ("n_tris_tree", "n_tris_cone", "n_nodes4", "n_nodes4_shadow", "depth4",
                                               "stack4", "collapse")})
        print(name, json.dumps(out[name]), flush=True)
    # ---- frames
    Wp, Hp = sc.padded_dims(W, H)
    seeds = sc.default_seeds(Wp, Hp)
    buf = np.zeros(W * H * 4, np.float32)
    times = {name: [] for name in ctxs}
    first = None
    every = list(ctxs)
    for i in range(warm + n_frames):  # warm-up rounds: lists, schedule, the measured-cost order
        for name in rotated(every, i):
            rt = ctxs[name]
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
        rt.setCounting(False)
        out[name].update(frame_ms=stats(times[name]),
                         steps={k: int(c[k]) for k in ("nodes_visited", "leaves_visited", "tris_tested", "rays_closest",
                                                       "rays_shadow")})
        print(name, json.dumps(out[name]["frame_ms"]), json.dumps(out[name]["steps"]), flush=True)
    for rt in ctxs.values():
        rt.close()
    # ---- the verdict
    v = {}
    spread = max(iqr(out[name]["frame_ms"]) for name in dev)
    v["spread_ms"] = round(spread, 3)
    host = out["host"]["frame_ms"]["median"]
    for b in ("gpu", "ploc"):
        for lights in ("off", "on"):
            tag = f"{b}_{lights}"
            g, s = out[f"{tag}_greedy"], out[f"{tag}_sah"]
            work = lambda x: x["steps"]["nodes_visited"] + x["steps"]["tris_tested"]
            r = dict(greedy_ms=g["frame_ms"]["median"], sah_ms=s["frame_ms"]["median"],
                     gain_ms=round(g["frame_ms"]["median"] - s["frame_ms"]["median"], 3),
                     gap_to_host_greedy_ms=round(g["frame_ms"]["median"] - host, 3),
                     gap_to_host_sah_ms=round(s["frame_ms"]["median"] - host, 3),
                     steps_ratio=round(work(s) / work(g), 4),
                     build_ms_greedy=g["build_ms"]["median"], build_ms_sah=s["build_ms"]["median"])
            r["gain_beyond_4_spreads"] = bool(r["gain_ms"] > 4 * spread)
            if parent_lib:
                par = out[f"{tag}_parent"]
                r["greedy_steps_equal_parent"] = g["steps"] == par["steps"]
                r["greedy_minus_parent_frame_ms"] = round(g["frame_ms"]["median"] - par["frame_ms"]["median"], 3)
                r["greedy_minus_parent_build_ms"] = round(g["build_ms"]["median"] - par["build_ms"]["median"], 3)
                r["frame_iqr_ms"] = round(max(iqr(par["frame_ms"]), iqr(g["frame_ms"])), 3)
                r["build_iqr_ms"] = round(max(iqr(par["build_ms"]), iqr(g["build_ms"])), 3)
                r["greedy_within_iqr_of_parent"] = bool(abs(r["greedy_minus_parent_frame_ms"]) <= r["frame_iqr_ms"] and
                                                        abs(r["greedy_minus_parent_build_ms"]) <= r["build_iqr_ms"])
            v[tag] = r
    out["verdict"] = v
    return out


def main():
    ap = argparse.ArgumentParser()
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
    res.update(run(pt, verts, idx, args.reps, args.frames, args.parent_lib))
    text = json.dumps(res, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
