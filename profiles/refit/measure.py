"""Measurement of rt_update_mesh on the dragon-class mesh (871,414 triangles, the bench's own), in
one process on one GPU (the record is profiles/refit/measure.json):

  updates  per builder (gpu; host in dynamic mode; host default, whose updates may rebuild): after
           warm-up, 20 updates to the rigid and 20 to the wobble positions (each from the built
           positions, so every update moves the mesh): rt_mesh_update_info.ms (HIP events around the
           refit kernels) and the host clock around the whole synchronous call; beside them the
           rt_set_mesh the refit replaces, measured here the same way.
  frames   the bench frame (1920 x 1080, sampleRate 16, depth 6, the same seeds every frame) on a
           refitted tree against a fresh build of the same vertices, and dynamic mode against the
           default build on the unmoved mesh: contexts alternating in one process, median of
           `--frames` kernel times each.

  python profiles/refit/measure.py [--mode updates|frames|all] [--tris N] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/refit/measure.py --mode updates --reps 5 --builders gpu
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ptload  # noqa: E402
import refit_ref as rr  # noqa: E402  (the deformations the tests use)

ACTION = {1: "refit", 2: "rebuilt"}


def med(x):
    return round(statistics.median(x), 4) if x else None


def context(pt, builder, dynamic, verts, idx, W=1920, sr=16):
    sc = pt.scenes
    rt = pt.RayTracer(0)
    rt.setSpheres(sc.ply_scene())
    rt.setCamera(sc.camera_spherical(W, **sc.PLY_CAMERA))
    rt.setSampleRate(sr)
    rt.setMaxPathDepth(6)
    rt.setBuilder(builder)
    rt.setMeshDynamic(dynamic)
    t0 = time.perf_counter()
    rt.setMesh(verts, idx)
    return rt, (time.perf_counter() - t0) * 1e3


def updates(pt, verts, idx, moved, builders, reps, warm=3):
    out = {}
    for name in builders:
        builder, dynamic = {"gpu": ("gpu", False), "host_dynamic": ("host", True), "host_default": ("host", False)}[name]
        rt, _ = context(pt, builder, dynamic, verts, idx)
        set_ms = []
        for _ in range(5 if builder == "gpu" else 1):  # the call the refit replaces, on this machine, this run
            t0 = time.perf_counter()
            rt.setMesh(verts, idx)
            set_ms.append((time.perf_counter() - t0) * 1e3)
        rec = dict(set_mesh_host_ms=med(set_ms), n_tris_tree=rt.meshInfo()["n_tris_tree"])
        for what, nv in moved.items():
            dev, host, actions, ratio, unhit = [], [], [], None, None
            for i in range(warm + reps):
                rt.updateMesh(verts)  # back to the built positions (not timed)
                t0 = time.perf_counter()
                up = rt.updateMesh(nv)
                t1 = time.perf_counter()
                if i >= warm:
                    dev.append(up["ms"])
                    host.append((t1 - t0) * 1e3)
                    actions.append(ACTION[up["action"]])
                    ratio, unhit = up["area_ratio"], up["now_unhittable"]
            rec[what] = dict(device_ms=med(dev), device_ms_min=round(min(dev), 4), device_ms_max=round(max(dev), 4),
                             host_ms=med(host), actions=sorted(set(actions)), area_ratio=ratio, now_unhittable=unhit,
                             newly_hittable=up["newly_hittable"], reps=reps)
        out[name] = rec
        rt.close()
        print(name, json.dumps(rec), flush=True)
    return out


def frames(pt, verts, idx, wobble, n_frames, W=1920, H=1080, sr=16):
    sc = pt.scenes
    Wp, Hp = sc.padded_dims(W, H)
    seeds = sc.default_seeds(Wp, Hp)
    plan = [  # name, builder, dynamic, built from, moved to
        ("host_default_unmoved", "host", False, verts, None),
        ("host_dynamic_unmoved", "host", True, verts, None),
        ("host_dynamic_wobble_refit", "host", True, verts, wobble),
        ("host_dynamic_wobble_fresh", "host", True, wobble, None),
        ("host_default_wobble_fresh", "host", False, wobble, None),
        ("gpu_wobble_refit", "gpu", False, verts, wobble),
        ("gpu_wobble_fresh", "gpu", False, wobble, None),
    ]
    ctxs, out = {}, {}
    for name, builder, dynamic, v, to in plan:
        rt, set_ms = context(pt, builder, dynamic, v, idx, W, sr)
        out[name] = dict(set_mesh_host_ms=round(set_ms, 2), n_tris_tree=rt.meshInfo()["n_tris_tree"])
        if to is not None:
            up = rt.updateMesh(to)
            out[name].update(action=ACTION[up["action"]], area_ratio=up["area_ratio"], update_device_ms=up["ms"])
        ctxs[name] = rt
    buf = np.zeros(W * H * 4, np.float32)
    times = {name: [] for name in ctxs}
    for i in range(2 + n_frames):  # two warm-up rounds: lists, schedule, the measured-cost order
        for name, rt in ctxs.items():
            rt.setSeeds(Wp, Hp, seeds)
            rt.rayTrace(buf, W, H, 0, kernel=2)
            if i >= 2:
                times[name].append(rt.lastKernelMs())
    for name, rt in ctxs.items():
        out[name].update(frame_ms=med(times[name]), frame_ms_min=round(min(times[name]), 3),
                         frame_ms_max=round(max(times[name]), 3), frames=n_frames)
        rt.close()
        print(name, json.dumps(out[name]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["updates", "frames", "all"])
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--builders", default="gpu,host_dynamic,host_default")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pt = ptload.load()
    sc = pt.scenes
    n = args.tris or sc.MESH_CONFIGS["dragon"]
    verts, idx = sc.make_mesh(n)
    moved = {"rigid": rr.rigid(verts), "wobble": rr.wobble(verts)}
    res = dict(n_tris=n, n_verts=len(verts))
    if args.mode in ("updates", "all"):
        res["updates"] = updates(pt, verts, idx, moved, args.builders.split(","), args.reps)
    if args.mode in ("frames", "all"):
        res["frames"] = frames(pt, verts, idx, moved["wobble"], args.frames)
    text = json.dumps(res, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
