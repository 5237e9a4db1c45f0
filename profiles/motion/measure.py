#!/usr/bin/env python3
"""Time of the feature warp kernel on the dragon-class view (871,414 triangles, 1920x1080,
plymain.cpp camera and lights) after one `wobble` update of the mesh.

    python profiles/motion/measure.py [--reps 20] [--warmup 3] [--out FILE]

Prints one JSON line: the median of `rt_last_warp_ms` (HIP events of its own) over `--reps` calls
after `--warmup`, beside the kernel's compulsory-traffic figure (64 B per pixel for the two feature
planes in and out, 84 B per mesh pixel of gathered indices and vertices before any cache reuse — a
figure derived from sizes, not measured — at the 8 TB/s HBM peak), the refit's device time and the
1-spp frame's kernel time of the same run, and the share of mesh pixels that find history through
the warped features.

Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

PIXEL_BYTES = 64       # (P, t) and (N, id) read, the same two float4 written
MESH_PIXEL_BYTES = 84  # 3 indices, 2 x 3 vertices of 12 B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=None, help="triangles of the synthetic mesh (default: dragon class)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("measure.py: no GPU visible")
    import ptload
    from refit_ref import wobble

    pt = ptload.load()
    sc = pt.scenes
    W, H = args.width, args.height
    npx = W * H
    n_tris = args.tris or sc.MESH_CONFIGS["dragon"]
    rt = pt.RayTracer(0)
    rt.setSpheres(sc.ply_scene())
    c = sc.PLY_CAMERA
    rt.setFoVAngle(sc.DEFAULT_FOV)
    rt.setSampleRate(1)
    rt.setMaxPathDepth(6)
    rt.setCameraSpherical(c["target"], c["elevation"], c["azimuth"], c["distance"])
    verts, idx = sc.make_mesh(n_tris)
    rt.setMesh(verts, idx)

    def dev(n):
        return torch.zeros(n, dtype=torch.float32, device="cuda:0")

    frame, prev_feat, cur_feat, warped = dev(npx * 4), dev(npx * 8), dev(npx * 8), dev(npx * 8)
    hist, hist_len, car, car_len = dev(npx * 4), torch.ones(npx, dtype=torch.float32, device="cuda:0"), dev(npx * 4), dev(npx)
    cam = rt.getCamera(W)
    rt.renderFeatures(prev_feat, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
    rest = rt.meshPose(device=True)  # the pose the kept frame was displayed in
    moved = torch.from_numpy(wobble(verts)).cuda()
    refit_ms, actions = [], []
    for i in range(args.warmup + 5):  # the same update again: the refit's time does not depend on the pose before it
        up = rt.updateMesh(moved, device=True)
        refit_ms.append(up["ms"])
        actions.append(up["action"])
    rt.renderFeatures(cur_feat, W, H, kernel=pt.RayTracer.KERNEL_TRIS)
    frame_ms = []
    for p in range(args.warmup + 5):
        rt.rayTrace(frame, W, H, 0, kernel=pt.RayTracer.KERNEL_TRIS)
        frame_ms.append(rt.lastKernelMs())
    warp_ms = []
    for i in range(args.warmup + args.reps):
        rt.warpFeatures(cur_feat, rest, warped, W, H)
        if i >= args.warmup:
            warp_ms.append(rt.lastWarpMs())
    rt.reproject(hist, hist_len, prev_feat, cam, warped, car, car_len, W, H, max_history=8.0)
    ids = cur_feat.view(2, npx, 4)[1, :, 3].contiguous().view(torch.int32)
    mesh = ids >= 0
    n_mesh = int(mesh.sum().item())
    nbytes = PIXEL_BYTES * npx + MESH_PIXEL_BYTES * n_mesh
    res = {
        "workload": f"{n_tris} triangles, {W}x{H}, plymain.cpp camera, one wobble update, 1 spp",
        "reps": args.reps, "warmup": args.warmup,
        "warp_ms_median": statistics.median(warp_ms), "warp_ms_min": min(warp_ms), "warp_ms_max": max(warp_ms),
        "mesh_pixels": n_mesh, "mesh_pixel_share": n_mesh / npx,
        "warp_compulsory_bytes": nbytes,
        "warp_compulsory_us_at_8TBps": nbytes / 8e12 * 1e6,
        "mesh_pixels_with_history_share": float((car_len > 0)[mesh].float().mean().item()) if n_mesh else 0.0,
        "refit_ms_median": statistics.median(refit_ms[args.warmup:]),
        "update_actions": sorted(set(actions)),
        "frame_1spp_kernel_ms_median": statistics.median(frame_ms[args.warmup:]),
        "device": torch.cuda.get_device_name(0),
    }
    res["warp_over_compulsory"] = res["warp_ms_median"] * 1e3 / res["warp_compulsory_us_at_8TBps"]
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    rt.close()


if __name__ == "__main__":
    main()
