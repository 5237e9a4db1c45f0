"""Measurement of RT_BUILD_OPT_LIGHTS (the device builders with the never-hit culling and the
lights' cone split) on the dragon-class mesh (871,414 triangles, the bench's own),
in one process on one GPU; the record is profiles/build_lights/measure.json.

  builds   rt_set_mesh under "gpu" and "ploc" with the option off and on (and, with --parent-lib,
           under the parent commit's library: the option-off baseline), alternating: after
           warm-up `--reps` builds each, rt_mesh_stats.build_seconds.  Then, in builds of their own,
           the builder's HIP events per stage (RT_BUILD_PROFILE).
  frames   the bench frame (1920 x 1080, sampleRate 16, depth 6, the same seeds every frame) on
           every tree: contexts alternating, median and quartiles of `--frames` kernel times each,
           then one counting frame per context (the traversal's step counts).
  update   rt_update_mesh on the option-on meshes and on the host-built one: refit_ref's wobble
           (a rebuild where it makes a left-out triangle hittable) and the exact quarter turn
           (always a refit): rt_mesh_update_info.ms, which includes k_refit_cone on the option-on
           meshes and not on the host-built one, and where the shadow queries start afterwards.

  python profiles/build_lights/measure.py [--tris N] [--parent-lib FILE] [--reps R] [--frames F] [--builds-only] [--out FILE]
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
sys.path.insert(0, str(ROOT / "tests"))

import ptload  # noqa: E402
import refit_ref as rr  # noqa: E402


def stats(x, digits=3):
    q = statistics.quantiles(x, n=4) if len(x) >= 2 else [x[0]] * 3
    return dict(median=round(statistics.median(x), digits), q1=round(q[0], digits), q3=round(q[2], digits),
                min=round(min(x), digits), max=round(max(x), digits), n=len(x))


def context(pt, builder, on, lib=None, W=1920, sr=16):
    sc = pt.scenes
    rt = pt.RayTracer(0, lib_path=lib) if lib else pt.RayTracer(0)
    rt.setSpheres(sc.ply_scene())
    rt.setCamera(sc.camera_spherical(W, **sc.PLY_CAMERA))
    rt.setSampleRate(sr)
    rt.setMaxPathDepth(6)
    rt.setBuilder(builder)
    if on:
        rt.setBuildOptions(True)
    return rt


def plan(parent_lib):
    p = [("host", "host", False, None)]
    for b in ("gpu", "ploc"):
        if parent_lib:
            p.append((f"{b}_parent", b, False, parent_lib))
        p.append((f"{b}_off", b, False, None))
        p.append((f"{b}_on", b, True, None))
    return p


def mesh_figures(info):
    return {k: info[k] for k in ("n_tris_tree", "n_tris_cone", "n_nodes4", "n_nodes4_shadow", "cone_root", "depth4", "stack4")}


def run(pt, verts, idx, reps, n_frames, parent_lib, builds_only=False, W=1920, H=1080, sr=16, warm=2):
    sc = pt.scenes
    ctxs = {name: context(pt, b, on, lib, W, sr) for name, b, on, lib in plan(parent_lib)}
    out = {name: {} for name in ctxs}
    # ---- builds
    dev = {name: [] for name in ctxs if name != "host"}
    names = list(dev)
    for i in range(warm + reps):
        # every repetition starts one context further on: a build's time depends a little on which
        # build came before it (what that one freed), and a fixed order would give each context
        # the same predecessor every time
        for name in names[i % len(names):] + names[:i % len(names)]:
            ctxs[name].setMesh(verts, idx)
            if i >= warm:
                dev[name].append(ctxs[name].meshInfo()["build_seconds"] * 1e3)
    ctxs["host"].setMesh(verts, idx)
    out["host"]["build_ms"] = round(ctxs["host"].meshInfo()["build_seconds"] * 1e3, 2)
    with tempfile.TemporaryDirectory() as tmp:  # the stage split, by the builder's own events
        for name in ("gpu_off", "gpu_on", "ploc_off", "ploc_on"):
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
        out[name].update(mesh_figures(ctxs[name].meshInfo()))
        print(name, json.dumps(out[name]), flush=True)
    if builds_only:
        for rt in ctxs.values():
            rt.close()
        return out
    # ---- frames
    Wp, Hp = sc.padded_dims(W, H)
    seeds = sc.default_seeds(Wp, Hp)
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
        rt.setCounting(False)
        out[name].update(frame_ms=stats(times[name]), shadow_start=rt.renderInfo().get("shadow_start"),
                         steps={k: int(c[k]) for k in ("nodes_visited", "leaves_visited", "tris_tested", "rays_closest",
                                                       "rays_shadow")})
        print(name, json.dumps(out[name]["frame_ms"]), json.dumps(out[name]["steps"]), flush=True)
    # ---- updates
    turned = np.ascontiguousarray(np.stack([verts[:, 2], verts[:, 1], -verts[:, 0]], axis=1), np.float32)
    poses = (("wobble", rr.wobble(verts)), ("quarter_turn", turned))
    for name in ("host", "gpu_on", "ploc_on"):
        rt = ctxs[name]
        out[name]["update"] = {}
        for pose, nv in poses:
            ms, action = [], None
            for _ in range(max(3, reps // 2)):
                rt.setMesh(verts, idx)
                up = rt.updateMesh(nv)
                action = {pt._abi.RT_MESH_UPDATE_REFIT: "refit", pt._abi.RT_MESH_UPDATE_REBUILT: "rebuilt"}[up["action"]]
                ms.append(up["ms"])
            rt.setSeeds(Wp, Hp, seeds)
            rt.rayTrace(buf, W, H, 0, kernel=2)
            out[name]["update"][pose] = dict(action=action, newly_hittable=up["newly_hittable"],
                                             ms=stats(ms) if action == "refit" else None,
                                             cone_root=rt.meshInfo()["cone_root"],
                                             shadow_start_after=rt.renderInfo().get("shadow_start"))
        print(name, "update", json.dumps(out[name]["update"]), flush=True)
    for rt in ctxs.values():
        rt.close()
    # ---- the verdict
    v = {}
    spread = max(x["frame_ms"]["q3"] - x["frame_ms"]["q1"] for x in out.values())
    v["spread_ms"] = round(spread, 3)
    for b in ("gpu", "ploc"):
        off, on, host = (out[f"{b}_off"]["frame_ms"]["median"], out[f"{b}_on"]["frame_ms"]["median"],
                         out["host"]["frame_ms"]["median"])
        v[b] = dict(gap_to_host_off_ms=round(off - host, 3), gap_to_host_on_ms=round(on - host, 3),
                    taken_back_ms=round(off - on, 3), beyond_4_spreads=bool(off - on > 4 * spread))
        if parent_lib:
            par = out[f"{b}_parent"]
            iqr_f = max(par["frame_ms"]["q3"] - par["frame_ms"]["q1"],
                        out[f"{b}_off"]["frame_ms"]["q3"] - out[f"{b}_off"]["frame_ms"]["q1"])
            iqr_b = max(par["build_ms"]["q3"] - par["build_ms"]["q1"],
                        out[f"{b}_off"]["build_ms"]["q3"] - out[f"{b}_off"]["build_ms"]["q1"])
            v[b]["off_minus_parent_frame_ms"] = round(off - par["frame_ms"]["median"], 3)
            v[b]["off_minus_parent_build_ms"] = round(out[f"{b}_off"]["build_ms"]["median"] - par["build_ms"]["median"], 3)
            v[b]["off_within_iqr_of_parent"] = bool(abs(v[b]["off_minus_parent_frame_ms"]) <= iqr_f and
                                                    abs(v[b]["off_minus_parent_build_ms"]) <= iqr_b)
    out["verdict"] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--builds-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pt = ptload.load()
    sc = pt.scenes
    n = args.tris or sc.MESH_CONFIGS["dragon"]
    verts, idx = sc.make_mesh(n)
    res = dict(n_tris=n, n_verts=len(verts))
    res.update(run(pt, verts, idx, args.reps, args.frames, args.parent_lib, args.builds_only))
    text = json.dumps(res, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
