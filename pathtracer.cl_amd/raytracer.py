"""`RayTracer` — the reference's host API over the MI355X C-ABI.

Mirrors clrt/RayTracer.h:51-70 (camera, settings, scene) and RayTracerCL::rayTrace
(clrt/RayTracerCL.h:111-112): same method names, same argument meaning, the same RGBA32F
framebuffer layout (W*H float4, row-major, alpha 0) and the same progression semantics
(0 overwrites, p > 0 mixes with weight 1/p — GlutCLWindow.cpp:144-158).  Errors raise
`RtError`, as the reference throws cl::Error.

The framebuffer may be a numpy array (host) or a torch CUDA tensor on the tracer's device
(rendered in place, no copy).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _abi


class RayTracer:
    KERNEL_SPHERES = _abi.RT_KERNEL_SPHERES
    KERNEL_SPHERES_SS = _abi.RT_KERNEL_SPHERES_SS
    KERNEL_TRIS = _abi.RT_KERNEL_TRIS

    def __init__(self, device: int = 0, lib_path=None):
        # lib_path: another build of librtmi.so (in-process A/B of kernel variants)
        self._lib = _abi.load(lib_path)
        h = ctypes.c_void_p()
        st = self._lib.rt_create(int(device), ctypes.byref(h))
        if st != _abi.RT_OK:
            raise _abi.RtError(st, f"rt_create(device={device}): {self._lib.rt_status_string(st).decode()}")
        self._h = h
        self.device = device
        self._spheres: list[np.ndarray] = []
        self._scene_dirty = True
        self._fov = 53.0
        self._sample_rate = 8
        self._max_depth = 4
        self._mesh = None

    # ---- lifetime --------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st: int, what: str):
        if st != _abi.RT_OK:
            detail = self._lib.rt_last_error(self._h).decode(errors="replace")
            raise _abi.RtError(st, f"{what}: {self._lib.rt_status_string(st).decode()} ({detail})")

    # ---- camera (RayTracer.h:56-60) ------------------------------------------------------
    def setCameraMatrix(self, m) -> None:
        """4x4 view matrix (rows = gmtl matrix rows); stored column-major across the ABI."""
        m = np.asarray(m, np.float32).reshape(4, 4)
        colmajor = np.ascontiguousarray(m.T).reshape(-1)
        self._check(self._lib.rt_set_view_matrix(self._h, _abi.ptr(colmajor)), "rt_set_view_matrix")

    def setCameraSpherical(self, target, elevationDeg: float, azimuthDeg: float, distance: float) -> None:
        t = [float(v) for v in target]
        self._check(self._lib.rt_set_camera_spherical(self._h, *t, float(elevationDeg), float(azimuthDeg),
                                                      float(distance)), "rt_set_camera_spherical")

    def setFoVAngle(self, fovDeg: float) -> None:
        self._fov = float(fovDeg)
        self._check(self._lib.rt_set_fov(self._h, self._fov), "rt_set_fov")

    def getFoVAngle(self) -> float:
        return self._fov

    def setCamera(self, cam16) -> None:
        """Explicit Camera struct (view, up, right, position float4s) — fixture replay."""
        cam = np.ascontiguousarray(cam16, np.float32).reshape(16)
        self._check(self._lib.rt_set_camera(self._h, _abi.ptr(cam)), "rt_set_camera")

    # ---- settings (RayTracer.h:62-66) ----------------------------------------------------
    def setSampleRate(self, sampleRate: int) -> None:
        self._sample_rate = int(sampleRate)
        self._check(self._lib.rt_set_params(self._h, self._sample_rate, self._max_depth), "rt_set_params")

    def getSampleRate(self) -> int:
        return self._sample_rate

    def setMaxPathDepth(self, depth: int) -> None:
        self._max_depth = int(depth)
        self._check(self._lib.rt_set_params(self._h, self._sample_rate, self._max_depth), "rt_set_params")

    def getMaxPathDepth(self) -> int:
        return self._max_depth

    def setTraversal(self, linear) -> None:
        """False/"bvh": 4-wide BVH, compressed nodes (default); "bvh4f": the same tree with full-precision
        nodes; True/"linear": the reference loop."""
        t = {False: _abi.RT_TRAVERSAL_BVH, True: _abi.RT_TRAVERSAL_LINEAR, "bvh": _abi.RT_TRAVERSAL_BVH,
             "linear": _abi.RT_TRAVERSAL_LINEAR, "bvh4f": _abi.RT_TRAVERSAL_BVH4F}[linear]
        self._check(self._lib.rt_set_traversal(self._h, t), "rt_set_traversal")

    def setBuilder(self, builder: str) -> None:
        """BVH builder for the next setMesh: "host" (binned SAH, default), "gpu" (LBVH on the device) or
        "ploc" (PLOC on the device: slower to build than "gpu", trees that trace nearer the host build's)."""
        b = {"host": _abi.RT_BUILD_HOST, "gpu": _abi.RT_BUILD_GPU, "ploc": _abi.RT_BUILD_GPU_PLOC}[builder]
        self._check(self._lib.rt_set_builder(self._h, b), "rt_set_builder")

    def setBuildOptions(self, lights: bool) -> None:
        """Options of the device builders ("gpu", "ploc") for the next setMesh. lights: leave the never-hit
        triangles out and give the shadow queries a second tree, split by what can occlude the lights of the
        last setSpheres (as the host build does). Off by default; the host builder ignores it."""
        o = _abi.RT_BUILD_OPT_LIGHTS if lights else 0
        self._check(self._lib.rt_set_build_options(self._h, o), "rt_set_build_options")

    def getBuildOptions(self) -> int:
        o = ctypes.c_uint32(0)
        self._check(self._lib.rt_get_build_options(self._h, ctypes.byref(o)), "rt_get_build_options")
        return int(o.value)

    def setCollapse(self, mode: str) -> None:
        """How the device builders ("gpu", "ploc") collapse their binary tree to the 4-wide one, for the
        next setMesh: "greedy" (default) or "sah" (the host build's rule, by dynamic programming over the
        binary tree). The host builder ignores it; results never depend on it."""
        m = {"greedy": _abi.RT_COLLAPSE_GREEDY, "sah": _abi.RT_COLLAPSE_SAH}[mode]
        self._check(self._lib.rt_set_collapse(self._h, m), "rt_set_collapse")

    def getCollapse(self) -> str:
        m = ctypes.c_int32(0)
        self._check(self._lib.rt_get_collapse(self._h, ctypes.byref(m)), "rt_get_collapse")
        return {_abi.RT_COLLAPSE_GREEDY: "greedy", _abi.RT_COLLAPSE_SAH: "sah"}[int(m.value)]

    def setNDRange(self, nd_y: int) -> None:
        """Work-group height of the reference launch (fixes the padded seed height)."""
        self._check(self._lib.rt_set_ndrange(self._h, int(nd_y)), "rt_set_ndrange")

    # ---- scene (RayTracer.h:68-70) --------------------------------------------------------
    def addSphere(self, sphere) -> None:
        s = np.asarray(sphere, _abi.SPHERE_DTYPE).reshape(-1)
        for rec in s:
            self._spheres.append(rec.copy())
        self._scene_dirty = True

    def removeSphere(self, sphere) -> None:
        """Removes the first sphere equal to `sphere` (a stub in the reference, RayTracer.cpp:55-58)."""
        s = np.asarray(sphere, _abi.SPHERE_DTYPE).reshape(-1)[0]
        for i, rec in enumerate(self._spheres):
            if rec.tobytes() == s.tobytes():
                del self._spheres[i]
                self._scene_dirty = True
                return

    def clearSpheres(self) -> None:
        self._spheres.clear()
        self._scene_dirty = True

    def setSpheres(self, spheres) -> None:
        self.clearSpheres()
        self.addSphere(spheres)

    def setMesh(self, verts, idx) -> None:
        """Triangle mesh for the raytrace_tris kernel; the BVH is built on the host, its cost area
        leaning toward the lights of the spheres added so far (uploaded first; culling only)."""
        self._sync_scene()
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
        self._check(self._lib.rt_set_mesh(self._h, _abi.ptr(v), v.shape[0], _abi.ptr(i), i.shape[0]), "rt_set_mesh")
        self._mesh = (v.shape[0], i.shape[0])

    def setMeshDynamic(self, on: bool) -> None:
        """The next host-built setMesh keeps every triangle in the tree (also those no ray can hit),
        so that every later updateMesh refits and none has to rebuild."""
        self._check(self._lib.rt_set_mesh_dynamic(self._h, int(bool(on))), "rt_set_mesh_dynamic")

    def updateMesh(self, verts, device: bool = False) -> dict:
        """New positions for the vertices of the last setMesh (same count, same indices): both trees
        are refitted on the device, or rebuilt where a refit cannot stand for a build (the returned
        rt_mesh_update_info says which, and why).  device=True: `verts` is device memory (a torch
        tensor, or an address with the mesh's vertex count)."""
        if device:
            v, n = verts, (verts.numel() // 3 if hasattr(verts, "numel") else (self._mesh or (0, 0))[0])
        else:
            v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
            n = v.shape[0]
        self._check(self._lib.rt_update_mesh(self._h, _abi.ptr(v), n, _abi.RT_MESH_VERTS_DEVICE if device else 0),
                    "rt_update_mesh")
        return self.lastMeshUpdate()

    def lastMeshUpdate(self) -> dict:
        i = _abi.RtMeshUpdateInfo()
        self._check(self._lib.rt_last_mesh_update(self._h, ctypes.byref(i)), "rt_last_mesh_update")
        return {f: getattr(i, f) for f, _ in _abi.RtMeshUpdateInfo._fields_}

    def meshInfo(self) -> dict:
        st = _abi.RtMeshStats()
        self._check(self._lib.rt_mesh_info(self._h, ctypes.byref(st)), "rt_mesh_info")
        return {f: getattr(st, f) for f, _ in _abi.RtMeshStats._fields_}

    def _sync_scene(self):
        if self._scene_dirty:
            arr = np.array(self._spheres, dtype=_abi.SPHERE_DTYPE) if self._spheres else np.zeros(0, _abi.SPHERE_DTYPE)
            self._check(self._lib.rt_set_spheres(self._h, _abi.ptr(arr) if len(arr) else None, len(arr)),
                        "rt_set_spheres")
            self._scene_dirty = False

    # ---- seeds (RayTracerCL.cpp:147-171) --------------------------------------------------
    def setSeeds(self, wpad: int, hpad: int, seeds=None) -> None:
        self._check(self._lib.rt_set_seed_layout(self._h, int(wpad), int(hpad)), "rt_set_seed_layout")
        if seeds is not None:
            s = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
            self._check(self._lib.rt_set_seeds(self._h, _abi.ptr(s), s.size), "rt_set_seeds")

    def packSeedRows(self, rows, buf) -> None:
        """Copy seed rows (both planes) into `buf` ([2, n, Wpad] uint32; numpy or torch CUDA)."""
        r = np.ascontiguousarray(rows, np.uint32)
        flags = _abi.RT_OUT_DEVICE if getattr(buf, "is_cuda", False) else 0
        self._check(self._lib.rt_pack_seed_rows(self._h, _abi.ptr(r), r.size, _abi.ptr(buf), flags),
                    "rt_pack_seed_rows")

    def unpackSeedRows(self, rows, buf) -> None:
        """Write seed rows (both planes) from `buf` ([2, n, Wpad] uint32; numpy or torch CUDA)."""
        r = np.ascontiguousarray(rows, np.uint32)
        flags = _abi.RT_OUT_DEVICE if getattr(buf, "is_cuda", False) else 0
        self._check(self._lib.rt_unpack_seed_rows(self._h, _abi.ptr(r), r.size, _abi.ptr(buf), flags),
                    "rt_unpack_seed_rows")

    def getSeeds(self) -> np.ndarray:
        w, h = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.rt_seed_layout(self._h, ctypes.byref(w), ctypes.byref(h)), "rt_seed_layout")
        out = np.empty(2 * w.value * h.value, np.uint32)
        self._check(self._lib.rt_get_seeds(self._h, _abi.ptr(out), out.size), "rt_get_seeds")
        return out

    # ---- render (RayTracerCL::rayTrace) ---------------------------------------------------
    def rayTrace(self, out, width: int, height: int, progression: int, kernel: int = _abi.RT_KERNEL_SPHERES,
                 tile: tuple | None = None, stream=None, sync: bool = True, halo: bool = False) -> None:
        """Render into `out` (W*H*4 float32 — or tile rows*W*4 — numpy or torch CUDA tensor).
        tile = (stripe_rows, n_ranks, rank) for interleaved stripes, or (stripe_rows, n_ranks,
        rank, owner) with a per-stripe owner map (partitionStripes).
        halo=True: the caller keeps this tile's seed rows current (dist.SeedHalo), which
        permits progressive sphere frames on a tile."""
        self._sync_scene()
        t, _keep = _abi.tile_struct(tile)  # (_keep: the owner map the struct points into)
        tp = ctypes.byref(t) if t else None
        rows = self._lib.rt_tile_rows(height, tp)
        flags = self._buffer(out, int(width) * int(rows) * 4, "framebuffer") | (_abi.RT_SEEDS_HALO if halo else 0)
        args = (self._h, _abi.ptr(out), int(width), int(height), int(progression), int(kernel), tp, flags)
        self._aux_call("rt_render", args, stream, sync)

    # ---- first-hit features and the display denoiser (pathtracer_rt.h) --------------------
    _WORDS = ("uint32", "int32")

    @staticmethod
    def _buffer(buf, need: int, what: str, dtypes: tuple = ("float32",)) -> int:
        """The checks of a buffer that crosses the ABI (one of `dtypes`, contiguous, `need` elements);
        returns the RT_OUT_DEVICE flag of a torch CUDA tensor, 0 for host memory."""
        if isinstance(buf, np.ndarray):
            if buf.dtype not in [np.dtype(d) for d in dtypes] or not buf.flags["C_CONTIGUOUS"]:
                raise ValueError(f"{what} must be a contiguous {dtypes[0]} array")
            n, dev = buf.size, 0
        else:
            if str(buf.dtype) not in ["torch." + d for d in dtypes]:
                raise TypeError(f"{what} must be {' or '.join(dtypes)}")
            if not buf.is_contiguous():
                raise ValueError(f"{what} must be contiguous")
            n, dev = buf.numel(), _abi.RT_OUT_DEVICE if getattr(buf, "is_cuda", False) else 0
        if n < need:
            raise ValueError(f"{what} holds {n} {'floats' if dtypes == ('float32',) else 'words'}, {need} needed")
        return dev

    def _same_kind(self, method: str, bufs: list, who: str = "the buffers", also: tuple = ()) -> int:
        """_buffer for every (buf, need, what[, dtypes]) of `bufs` whose buf is not None; all of them (and
        the flags `also`) host arrays, or all device tensors: returns their common flag."""
        flags = {self._buffer(*b) for b in bufs if b[0] is not None} | set(also)
        if len(flags) != 1:
            raise ValueError(f"{method}: {who} must all be host arrays or all device tensors")
        return flags.pop()

    def _aux_call(self, name: str, args: tuple, stream, sync: bool) -> None:
        """`name` on the context's stream and waited for, or `name`_async on `stream` (sync: then waited for)."""
        if sync and stream is None:
            self._check(getattr(self._lib, name)(*args), name)
        else:
            sp = ctypes.c_void_p(stream) if isinstance(stream, int) else stream
            self._check(getattr(self._lib, name + "_async")(*args, sp), name + "_async")
            if sync:
                self.synchronize()

    def _last_ms(self, name: str, n_slots: int = 1, slot: int = 0) -> float:
        """`name`(handle, n_slots float pointers): the one at `slot`, the others null."""
        ms = ctypes.c_float()
        a = [None] * n_slots
        a[slot] = ctypes.byref(ms)
        self._check(getattr(self._lib, name)(self._h, *a), name)
        return ms.value

    def _defaults(self, prm_type, name: str) -> dict:
        prm = prm_type()
        self._check(getattr(self._lib, name)(ctypes.byref(prm)), name)
        return {f: getattr(prm, f) for f, _ in prm_type._fields_}

    def getCamera(self, width: int) -> np.ndarray:
        """The Camera (16 floats) a render of this width would use."""
        cam = np.empty(_abi.CAMERA_FLOATS, np.float32)
        self._check(self._lib.rt_get_camera(self._h, int(width), _abi.ptr(cam)), "rt_get_camera")
        return cam

    def primaryRays(self, width: int, height: int) -> np.ndarray:
        """The pixel-centre camera rays of a W x H frame under the current camera (RAY_DTYPE, row-major)."""
        cam = self.getCamera(width)
        rays = np.empty(int(width) * int(height), _abi.RAY_DTYPE)
        st = self._lib.rt_primary_rays(_abi.ptr(cam), int(width), int(height), _abi.ptr(rays))
        self._check(st, "rt_primary_rays")
        return rays

    def renderFeatures(self, feat, width: int, height: int, kernel: int = _abi.RT_KERNEL_TRIS, stream=None,
                       sync: bool = True) -> None:
        """First-hit features of every pixel-centre ray into `feat` (2 planes of W*H float4: (P, t),
        then (N, surface id as int32 bits); numpy or torch CUDA tensor)."""
        self._sync_scene()
        flags = self._buffer(feat, 2 * int(width) * int(height) * 4, "feature buffer")
        self._aux_call("rt_render_features", (self._h, _abi.ptr(feat), int(width), int(height), int(kernel), flags), stream, sync)

    def denoise(self, src, feat, dst, width: int, height: int, iterations: int = 5, sigma_color: float = 2.0,
                sigma_normal: float = 0.3, sigma_plane: float = 0.1, stream=None, sync: bool = True) -> None:
        """Edge-avoiding a-trous filter of the RGBA32F frame `src` guided by `feat` (renderFeatures)
        into `dst` (may be `src`); all three numpy arrays, or all three torch CUDA tensors.  The
        accumulation buffer of a progressive render is `src`: it is only read."""
        px = int(width) * int(height)
        flags = self._same_kind("denoise", [(src, px * 4, "source frame"), (feat, px * 8, "feature buffer"),
                                            (dst, px * 4, "destination frame")], who="source, features and destination")
        prm = _abi.RtDenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_plane))
        args = (self._h, _abi.ptr(src), _abi.ptr(feat), _abi.ptr(dst), int(width), int(height), ctypes.byref(prm), flags)
        self._aux_call("rt_denoise", args, stream, sync)

    def lastFeaturesMs(self) -> float:
        return self._last_ms("rt_last_features_ms")

    def lastDenoiseMs(self) -> float:
        """Device time of all passes of the last denoise, ms."""
        return self._last_ms("rt_last_denoise_ms")

    # ---- temporal reprojection of the displayed frame (pathtracer_rt.h) ----
    def reprojectDefaults(self) -> dict:
        return self._defaults(_abi.RtReprojectParams, "rt_reproject_defaults")

    def reproject(self, prev_rgba, prev_len, prev_feat, prev_cam, cur_feat, out_rgba, out_len, width: int, height: int,
                  plane_tol: float = 0.01, normal_min: float = 0.9, max_history: float = 32.0, stream=None,
                  sync: bool = True) -> None:
        """Carry the previous view's displayed frame `prev_rgba` with its per-pixel history lengths
        `prev_len` (W*H floats), features `prev_feat` and Camera `prev_cam` (16 floats, getCamera)
        over to the view whose features are `cur_feat`: `out_rgba`, `out_len`.  The six buffers are
        all numpy arrays or all torch CUDA tensors; the inputs are only read."""
        px = int(width) * int(height)
        flags = self._same_kind("reproject", [
            (prev_rgba, px * 4, "previous frame"), (prev_len, px, "previous history lengths"),
            (prev_feat, px * 8, "previous feature buffer"), (cur_feat, px * 8, "feature buffer"),
            (out_rgba, px * 4, "destination frame"), (out_len, px, "destination history lengths")])
        cam = np.ascontiguousarray(prev_cam, np.float32)
        if cam.size != _abi.CAMERA_FLOATS:
            raise ValueError(f"prev_cam holds {cam.size} floats, {_abi.CAMERA_FLOATS} needed")
        prm = _abi.RtReprojectParams(float(plane_tol), float(normal_min), float(max_history))
        args = (self._h, _abi.ptr(prev_rgba), _abi.ptr(prev_len), _abi.ptr(prev_feat), _abi.ptr(cam), _abi.ptr(cur_feat),
                _abi.ptr(out_rgba), _abi.ptr(out_len), int(width), int(height), ctypes.byref(prm), flags)
        self._aux_call("rt_reproject", args, stream, sync)

    def temporalMerge(self, hist_rgba, hist_len, cur_rgba, n_cur: float, out_rgba, out_len, width: int, height: int,
                      max_history: float = 32.0, stream=None, sync: bool = True) -> None:
        """Blend the carried history (`hist_rgba`, `hist_len`) with the accumulation buffer `cur_rgba`
        of `n_cur` = max(progression, 1) frames into `out_rgba`, `out_len` (may be the history's
        buffers); all numpy arrays or all torch CUDA tensors.  `cur_rgba` is only read."""
        px = int(width) * int(height)
        flags = self._same_kind("temporalMerge", [
            (hist_rgba, px * 4, "history frame"), (hist_len, px, "history lengths"), (cur_rgba, px * 4, "current frame"),
            (out_rgba, px * 4, "destination frame"), (out_len, px, "destination history lengths")])
        args = (self._h, _abi.ptr(hist_rgba), _abi.ptr(hist_len), _abi.ptr(cur_rgba), float(n_cur), float(max_history),
                _abi.ptr(out_rgba), _abi.ptr(out_len), int(width), int(height), flags)
        self._aux_call("rt_temporal_merge", args, stream, sync)

    def lastReprojectMs(self, merge: bool = False) -> float:
        """Device time of the last reprojection kernel, or (merge=True) of the last merge kernel, ms."""
        return self._last_ms("rt_last_reproject_ms", 2, 1 if merge else 0)

    # ---- lag-adaptive trust of the carried history (pathtracer_rt.h) ----
    def trustDefaults(self) -> dict:
        return self._defaults(_abi.RtTrustParams, "rt_trust_defaults")

    def historyTrust(self, hist_rgba, hist_len, cur_rgba, n_cur: float, feat, out_len, width: int, height: int,
                     tolerance: float | None = None, sigma_normal: float = 0.3, sigma_plane: float = 0.1, stream=None,
                     sync: bool = True) -> None:
        """The history length each pixel of the carried history (`hist_rgba`, `hist_len`, as reproject
        wrote them for the current view) still deserves against the accumulation buffer `cur_rgba` of
        `n_cur` = max(progression, 1) frames, judged over a 7x7 window guided by `feat`: `out_len` (W*H
        floats; may be `hist_len`), to be passed to temporalMerge as its `hist_len`.  `tolerance` in
        standard deviations (None: the library's default; inf: everything is trusted).  All numpy arrays
        or all torch CUDA tensors; the inputs are only read."""
        px = int(width) * int(height)
        flags = self._same_kind("historyTrust", [
            (hist_rgba, px * 4, "history frame"), (hist_len, px, "history lengths"), (cur_rgba, px * 4, "current frame"),
            (feat, px * 8, "feature buffer"), (out_len, px, "destination history lengths")])
        if tolerance is None:
            tolerance = self.trustDefaults()["tolerance"]
        prm = _abi.RtTrustParams(float(tolerance), float(sigma_normal), float(sigma_plane))
        args = (self._h, _abi.ptr(hist_rgba), _abi.ptr(hist_len), _abi.ptr(cur_rgba), float(n_cur), _abi.ptr(feat),
                _abi.ptr(out_len), int(width), int(height), ctypes.byref(prm), flags)
        self._aux_call("rt_history_trust", args, stream, sync)

    def lastTrustMs(self) -> float:
        """Device time of the last historyTrust kernel, ms."""
        return self._last_ms("rt_last_trust_ms")

    # ---- carrying the displayed frame across updateMesh (pathtracer_rt.h) ----
    def meshPose(self, out=None, device: bool = False):
        """The vertices of the current mesh as the trees hold them (the last successful setMesh /
        updateMesh), [n_verts, 3] float32: into `out` (a numpy array, or a torch CUDA tensor), else
        into a new numpy array — or, device=True, a new torch tensor on the tracer's device."""
        if not self._mesh:
            raise _abi.RtError(_abi.RT_ERR_NO_MESH, "rt_mesh_pose: no mesh set")
        n = self._mesh[0]
        if out is None:
            if device:
                import torch

                out = torch.empty((n, 3), dtype=torch.float32, device=f"cuda:{self.device}")
            else:
                out = np.empty((n, 3), np.float32)
        flags = self._buffer(out, 3 * n, "pose buffer")
        self._check(self._lib.rt_mesh_pose(self._h, _abi.ptr(out), n, flags), "rt_mesh_pose")
        return out

    def warpFeatures(self, cur_feat, prev_verts, out_feat, width: int, height: int, stream=None, sync: bool = True) -> None:
        """Rewrite the current pose's features `cur_feat` (renderFeatures) into the earlier pose
        `prev_verts` of the same mesh ([n_verts, 3]): `out_feat` (may be `cur_feat`) holds, for every
        mesh pixel, position and normal of the same material point in that pose — reproject's
        `cur_feat` across an updateMesh.  All numpy arrays or all torch CUDA tensors."""
        px = int(width) * int(height)
        n = (self._mesh or (0, 0))[0]
        if isinstance(prev_verts, np.ndarray):
            prev_verts = np.ascontiguousarray(prev_verts, np.float32)
        nv = (prev_verts.size if isinstance(prev_verts, np.ndarray) else prev_verts.numel()) // 3
        flags = self._same_kind("warpFeatures", [(cur_feat, px * 8, "feature buffer"), (prev_verts, 3 * n, "earlier pose"),
                                                 (out_feat, px * 8, "destination feature buffer")])
        args = (self._h, _abi.ptr(cur_feat), _abi.ptr(prev_verts), nv, _abi.ptr(out_feat), int(width), int(height), flags)
        self._aux_call("rt_warp_features", args, stream, sync)

    def lastWarpMs(self) -> float:
        """Device time of the last warpFeatures kernel, ms."""
        return self._last_ms("rt_last_warp_ms")

    # ---- carrying the displayed frame across sphere moves (pathtracer_rt.h) ----
    def warpFeaturesSpheres(self, cur_feat, prev_spheres, out_feat, width: int, height: int, stream=None,
                            sync: bool = True) -> None:
        """Put every sphere pixel of `cur_feat` (renderFeatures with a sphere kernel under the current
        spheres) back where its sphere stood in `prev_spheres` (a SPHERE_DTYPE array, or a CUDA byte
        tensor of one; sphere i of both lists is the same object; it may be empty): `out_feat` (may be
        `cur_feat`) is reproject's `cur_feat` across a change of the spheres.  All numpy arrays or all
        torch CUDA tensors."""
        self._sync_scene()
        px = int(width) * int(height)
        size = _abi.SPHERE_DTYPE.itemsize
        if isinstance(prev_spheres, np.ndarray):
            prev_spheres = np.ascontiguousarray(prev_spheres, _abi.SPHERE_DTYPE).reshape(-1)
            n_prev, f_prev = prev_spheres.size, 0
        else:
            if prev_spheres.dtype.__str__() != "torch.uint8" or not prev_spheres.is_contiguous():
                raise TypeError("earlier spheres must be a SPHERE_DTYPE array or a contiguous uint8 tensor of one")
            if prev_spheres.numel() % size:
                raise ValueError(f"earlier spheres hold {prev_spheres.numel()} bytes, no multiple of {size}")
            n_prev, f_prev = prev_spheres.numel() // size, _abi.RT_OUT_DEVICE if prev_spheres.is_cuda else 0
        flags = self._same_kind("warpFeaturesSpheres", [(cur_feat, px * 8, "feature buffer"),
                                                        (out_feat, px * 8, "destination feature buffer")], also=(f_prev,))
        args = (self._h, _abi.ptr(cur_feat), _abi.ptr(prev_spheres) if n_prev else None, n_prev, _abi.ptr(out_feat),
                int(width), int(height), flags)
        self._aux_call("rt_warp_features_spheres", args, stream, sync)

    def lastSphereWarpMs(self) -> float:
        """Device time of the last warpFeaturesSpheres kernel, ms."""
        return self._last_ms("rt_last_sphere_warp_ms")

    # ---- variance-guided display filter (pathtracer_rt.h) ----
    def denoiseVarDefaults(self) -> dict:
        return self._defaults(_abi.RtDenoiseVarParams, "rt_denoise_var_defaults")

    def momentsAccumulate(self, prev_rgba, cur_rgba, n_cur: float, mom_in, mom_out, width: int, height: int,
                          stream=None, sync: bool = True) -> None:
        """After a progressive frame: fold the frame's own luminance (recovered from the accumulation
        buffer after it, `cur_rgba`, and a copy taken before it, `prev_rgba`; `n_cur` =
        max(progression, 1)) into the view's moments frame `mom_in` -> `mom_out` (may be the same
        buffer).  With n_cur == 1 `prev_rgba` and `mom_in` are not read and may be None.  All numpy
        arrays or all torch CUDA tensors; the accumulation buffers are only read."""
        px = int(width) * int(height)
        flags = self._same_kind("momentsAccumulate", [
            (prev_rgba, px * 4, "previous accumulation"), (cur_rgba, px * 4, "current accumulation"),
            (mom_in, px * 4, "moments"), (mom_out, px * 4, "destination moments")])
        args = (self._h, _abi.ptr(prev_rgba), _abi.ptr(cur_rgba), float(n_cur), _abi.ptr(mom_in), _abi.ptr(mom_out),
                int(width), int(height), flags)
        self._aux_call("rt_moments_accumulate", args, stream, sync)

    def variance(self, disp_rgba, mom_rgba, length, feat, out_var, width: int, height: int, sigma_normal: float = 0.3,
                 sigma_plane: float = 0.1, min_len: float = 4.0, stream=None, sync: bool = True) -> None:
        """The variance of the displayed luminance into `out_var` (W*H floats): from the moments frame
        `mom_rgba` where the history length `length` (W*H floats) reaches `min_len`, else from a 7x7
        feature-weighted window of `disp_rgba`, the frame about to be displayed.  All numpy arrays or
        all torch CUDA tensors; the inputs are only read."""
        px = int(width) * int(height)
        flags = self._same_kind("variance", [
            (disp_rgba, px * 4, "displayed frame"), (mom_rgba, px * 4, "moments"), (length, px, "history lengths"),
            (feat, px * 8, "feature buffer"), (out_var, px, "destination variance")])
        prm = _abi.RtDenoiseVarParams(5, 4.0, float(sigma_normal), float(sigma_plane), float(min_len))
        args = (self._h, _abi.ptr(disp_rgba), _abi.ptr(mom_rgba), _abi.ptr(length), _abi.ptr(feat), _abi.ptr(out_var),
                int(width), int(height), ctypes.byref(prm), flags)
        self._aux_call("rt_variance", args, stream, sync)

    def denoiseVar(self, src, var, feat, dst, dst_var, width: int, height: int, iterations: int = 5,
                   sigma_lum: float = 4.0, sigma_normal: float = 0.3, sigma_plane: float = 0.1, stream=None,
                   sync: bool = True) -> None:
        """Variance-guided a-trous filter of the RGBA32F frame `src` with its variance plane `var`
        (W*H floats, `variance`) guided by `feat` into `dst` (may be `src`) and `dst_var` (may be
        `var`, or None); all numpy arrays or all torch CUDA tensors."""
        px = int(width) * int(height)
        flags = self._same_kind("denoiseVar", [
            (src, px * 4, "source frame"), (var, px, "variance"), (feat, px * 8, "feature buffer"),
            (dst, px * 4, "destination frame"), (dst_var, px, "destination variance")])
        prm = _abi.RtDenoiseVarParams(int(iterations), float(sigma_lum), float(sigma_normal), float(sigma_plane), 4.0)
        args = (self._h, _abi.ptr(src), _abi.ptr(var), _abi.ptr(feat), _abi.ptr(dst), _abi.ptr(dst_var), int(width),
                int(height), ctypes.byref(prm), flags)
        self._aux_call("rt_denoise_var", args, stream, sync)

    def lastVarianceMs(self, which: str = "denoise_var") -> float:
        """Device time of the last `moments` kernel, `variance` kernel, or of all passes of the last
        `denoise_var`, ms."""
        return self._last_ms("rt_last_variance_ms", 3, ("moments", "variance", "denoise_var").index(which))

    # ---- tone-mapped 8-bit display output with auto-exposure (pathtracer_rt.h) ----
    def toneMapDefaults(self) -> dict:
        return self._defaults(_abi.RtTonemapParams, "rt_tonemap_defaults")

    def meterDefaults(self) -> dict:
        return self._defaults(_abi.RtMeterParams, "rt_meter_defaults")

    def meterExposure(self, rgba, exposure, width: int, height: int, hist=None, stream=None, sync: bool = True,
                      **params) -> None:
        """Meter the RGBA32F frame `rgba`: `exposure` (one float32) is read as the previous exposure (not
        positive: none) and written as the new one; `hist` (None, or 384 uint32 / int32 words) receives
        the luminance histogram.  `params`: fields of rt_meter_params other than the library's defaults
        (key, lo, hi, e_min, e_max, rate).  All numpy arrays or all torch CUDA tensors; the frame is
        only read."""
        px = int(width) * int(height)
        flags = self._same_kind("meterExposure", [(rgba, px * 4, "frame"), (exposure, 1, "exposure"),
                                                  (hist, _abi.RT_METER_BINS, "histogram", self._WORDS)])
        prm = _abi.RtMeterParams(**{**self.meterDefaults(), **{k: float(v) for k, v in params.items()}})
        args = (self._h, _abi.ptr(rgba), _abi.ptr(exposure), _abi.ptr(hist), int(width), int(height), ctypes.byref(prm),
                flags)
        self._aux_call("rt_meter_exposure", args, stream, sync)

    def toneMap(self, rgba, out_rgba8, width: int, height: int, exposure=None, stream=None, sync: bool = True,
                **params) -> None:
        """Tone-map the RGBA32F frame `rgba` into `out_rgba8` (W*H uint32 / int32 words: r | g << 8 |
        b << 16 | 255 << 24) under `exposure`: a buffer of one float32 as meterExposure wrote it, or a
        number, the fixed factor (None: the library's default, 1).  `params`: fields of rt_tonemap_params
        other than the library's defaults (curve, srgb, dither, white).  All numpy arrays or all torch CUDA
        tensors; the frame is only read."""
        px = int(width) * int(height)
        d = {**self.toneMapDefaults(), **params}
        if isinstance(exposure, (int, float, np.floating)):
            d["exposure"], exposure = float(exposure), None
        flags = self._same_kind("toneMap", [(rgba, px * 4, "frame"), (out_rgba8, px, "destination 8-bit frame", self._WORDS),
                                            (exposure, 1, "exposure")])
        prm = _abi.RtTonemapParams(int(d["curve"]), int(d["srgb"]), int(d["dither"]), float(d["exposure"]), float(d["white"]))
        args = (self._h, _abi.ptr(rgba), _abi.ptr(exposure), _abi.ptr(out_rgba8), int(width), int(height), ctypes.byref(prm),
                flags)
        self._aux_call("rt_tonemap", args, stream, sync)

    def lastToneMapMs(self, meter: bool = False) -> float:
        """Device time of the last tone-map kernel, or (meter=True) of the last meter, ms."""
        return self._last_ms("rt_last_tonemap_ms", 2, 0 if meter else 1)

    # ---- the noise meter (pathtracer_rt.h) ----
    def noiseDefaults(self) -> dict:
        return self._defaults(_abi.RtNoiseParams, "rt_noise_defaults")

    def noiseMeter(self, rgba, var, width: int, height: int, percentile: float | None = None,
                   threshold: float | None = None, lum_floor: float | None = None, tiles=None, hist=None, stats=None,
                   stream=None, sync: bool = True):
        """Meter the RGBA32F frame `rgba` with the variance plane of its luminance `var` (W*H floats,
        `variance`): the relative standard error sqrt(var) / (max(lum, 0) + lum_floor) per pixel, its
        histogram into `hist` (None, or 384 uint32 / int32 words), per 8x8 tile its (mean, max) into
        `tiles` (None, or ceil(W/8) ceil(H/8) pairs of float32).  Returns the stats as a dict: `level`
        (np.float32, an upper bound of the error at `percentile`), `counted`, `skipped`, `below` (the
        pixels in bins at or under `threshold`).  None for a parameter: the library's default.  All
        numpy arrays or all torch CUDA tensors; the inputs are only read.  `stats` (4 uint32 / int32
        words of the buffers' kind) receives the struct's words as well; with sync=False it must be
        given, nothing is read back and None is returned."""
        px = int(width) * int(height)
        n_tiles = ((int(width) + 7) // 8) * ((int(height) + 7) // 8)
        flags = self._same_kind("noiseMeter", [
            (rgba, px * 4, "frame"), (var, px, "variance"), (tiles, 2 * n_tiles, "tile map"),
            (hist, _abi.RT_METER_BINS, "histogram", self._WORDS), (stats, 4, "stats", self._WORDS)])
        if stats is None:
            if not sync:
                raise ValueError("noiseMeter: sync=False needs a stats buffer")
            if flags:
                import torch

                stats = torch.zeros(4, dtype=torch.int32, device=rgba.device)
            else:
                stats = np.zeros(4, np.uint32)
        d = self.noiseDefaults()
        for k, v in (("percentile", percentile), ("threshold", threshold), ("lum_floor", lum_floor)):
            if v is not None:
                d[k] = float(v)
        prm = _abi.RtNoiseParams(d["percentile"], d["threshold"], d["lum_floor"])
        args = (self._h, _abi.ptr(rgba), _abi.ptr(var), _abi.ptr(stats), _abi.ptr(tiles), _abi.ptr(hist), int(width),
                int(height), ctypes.byref(prm), flags)
        self._aux_call("rt_noise_meter", args, stream, sync)
        if not sync:
            return None
        w = stats if isinstance(stats, np.ndarray) else stats.cpu().numpy()
        w = np.ascontiguousarray(w).view(np.uint32)
        return dict(level=w[:1].view(np.float32)[0], counted=int(w[1]), skipped=int(w[2]), below=int(w[3]))

    def lastNoiseMs(self) -> float:
        """Device time of the last noise meter, ms."""
        return self._last_ms("rt_last_noise_ms")

    # ---- adaptive sampling on the tile map (pathtracer_rt.h) ----
    @staticmethod
    def _tiles(width: int, height: int) -> int:
        return ((int(width) + 7) // 8) * ((int(height) + 7) // 8)

    def adaptiveDefaults(self) -> dict:
        return self._defaults(_abi.RtAdaptiveParams, "rt_adaptive_defaults")

    def setTileStop(self, stop, width: int = 0, height: int = 0) -> None:
        """The stop plane that masks the raytrace_tris renders of `width` x `height` from now on: one
        uint32 / int32 word per 8x8 tile, 0 = rendered, anything else = left alone (framebuffer and
        seeds).  A numpy array is copied now; a torch CUDA tensor is borrowed, read at every render, and
        must stay alive until the plane is cleared (`stop` None) or replaced."""
        if stop is None:
            self._keep_stop = None
            self._check(self._lib.rt_set_tile_stop(self._h, None, 0, 0, 0), "rt_set_tile_stop")
            return
        flags = self._buffer(stop, self._tiles(width, height), "stop plane", self._WORDS)
        self._check(self._lib.rt_set_tile_stop(self._h, _abi.ptr(stop), int(width), int(height), flags), "rt_set_tile_stop")
        self._keep_stop = stop if flags else None

    def tileStopSelect(self, tiles, stop, n_frames: int, width: int, height: int, threshold: float | None = None,
                       max_ratio: float | None = None, min_frames: int | None = None, dilate: int | None = None,
                       stats=None, stream=None, sync: bool = True):
        """The stop rule on noiseMeter's tile map `tiles` ((mean, max) pairs): `stop` (a word per tile,
        0 = live, k = stopped after k frames) is updated in place — a live tile stops, with `n_frames`,
        when every tile within `dilate` tiles of it is stopped already or quiet (n_frames >= min_frames,
        mean <= threshold, max <= threshold max_ratio).  None for a parameter: the library's default.
        Returns the stats as a dict (`tiles`, `active`, `stopped_now`, `frames`).  All numpy arrays or all
        torch CUDA tensors; `stats` (4 words of the buffers' kind) receives the struct's words as well;
        with sync=False it must be given, nothing is read back and None is returned."""
        return self._stop_select("tileStopSelect", tiles, None, stop, n_frames, width, height, threshold, max_ratio, min_frames,
                                 dilate, stats, stream, sync)

    def _stop_select(self, who, tiles, tile_frames, stop, n_frames, width, height, threshold, max_ratio, min_frames, dilate,
                     stats, stream, sync):
        """tileStopSelect (`tile_frames` None) and tileStopSelectFrames."""
        n = self._tiles(width, height)
        flags = self._same_kind(who, [(tiles, 2 * n, "tile map"), (tile_frames, n, "tile frames"),
                                      (stop, n, "stop plane", self._WORDS), (stats, 4, "stats", self._WORDS)])
        if stats is None:
            if not sync:
                raise ValueError(f"{who}: sync=False needs a stats buffer")
            if flags:
                import torch

                stats = torch.zeros(4, dtype=torch.int32, device=tiles.device)
            else:
                stats = np.zeros(4, np.uint32)
        d = self.adaptiveDefaults()
        for k, v in (("threshold", threshold), ("max_ratio", max_ratio), ("min_frames", min_frames), ("dilate", dilate)):
            if v is not None:
                d[k] = v
        prm = _abi.RtAdaptiveParams(float(d["threshold"]), float(d["max_ratio"]), int(d["min_frames"]), int(d["dilate"]))
        tail = (_abi.ptr(stop), int(n_frames), _abi.ptr(stats), int(width), int(height), ctypes.byref(prm), flags)
        if tile_frames is None:
            self._aux_call("rt_tile_stop_select", (self._h, _abi.ptr(tiles)) + tail, stream, sync)
        else:
            self._aux_call("rt_tile_stop_select_frames", (self._h, _abi.ptr(tiles), _abi.ptr(tile_frames)) + tail, stream, sync)
        if not sync:
            return None
        w = stats if isinstance(stats, np.ndarray) else stats.cpu().numpy()
        w = np.ascontiguousarray(w).view(np.uint32)
        return dict(tiles=int(w[0]), active=int(w[1]), stopped_now=int(w[2]), frames=int(w[3]))

    def tileStopOrder(self, base, stop, order_out, live_out, stream=None, sync: bool = True) -> None:
        """The pixel queue's order under the plane `stop` (n words), as a masked render computes it:
        `order_out` (n words) = the entries of the tile order `base` (n words; None: 0, 1, ...) whose tile
        is live, in base's order, then n in every remaining position; `live_out` (one word) their number.
        All numpy arrays or all torch CUDA tensors."""
        n = stop.size if isinstance(stop, np.ndarray) else stop.numel()
        flags = self._same_kind("tileStopOrder", [(base, n, "base order", self._WORDS), (stop, n, "stop plane", self._WORDS),
                                                  (order_out, n, "destination order", self._WORDS),
                                                  (live_out, 1, "live count", self._WORDS)])
        args = (self._h, _abi.ptr(base), _abi.ptr(stop), int(n), _abi.ptr(order_out), _abi.ptr(live_out), flags)
        self._aux_call("rt_tile_stop_order", args, stream, sync)

    def momentsAccumulateTiles(self, prev_rgba, cur_rgba, n_cur: float, mom_in, mom_out, stop, len_out, width: int,
                               height: int, stream=None, sync: bool = True) -> None:
        """momentsAccumulate under the plane `stop` (a word per 8x8 tile): the pixels of live tiles as
        momentsAccumulate, with `len_out` (W*H floats) = n_cur; the pixels of stopped tiles keep their
        moments and get the frame count their tile stopped at — `variance`'s `length`.  All numpy arrays
        or all torch CUDA tensors."""
        px = int(width) * int(height)
        flags = self._same_kind("momentsAccumulateTiles", [
            (prev_rgba, px * 4, "previous accumulation"), (cur_rgba, px * 4, "current accumulation"),
            (mom_in, px * 4, "moments"), (mom_out, px * 4, "destination moments"),
            (stop, self._tiles(width, height), "stop plane", self._WORDS), (len_out, px, "destination history lengths")])
        args = (self._h, _abi.ptr(prev_rgba), _abi.ptr(cur_rgba), float(n_cur), _abi.ptr(mom_in), _abi.ptr(mom_out),
                _abi.ptr(stop), _abi.ptr(len_out), int(width), int(height), flags)
        self._aux_call("rt_moments_accumulate_tiles", args, stream, sync)

    def lastAdaptiveMs(self, order: bool = False) -> float:
        """Device time of the last stop rule, or (order=True) of the last masked order kernel, ms."""
        return self._last_ms("rt_last_adaptive_ms", 2, 1 if order else 0)

    # ---- per-tile sample counts (pathtracer_rt.h) ----
    def budgetDefaults(self) -> dict:
        """rt_budget_defaults: `max_passes` and the `limits` it reads (max_passes - 1 floats)."""
        prm = _abi.RtBudgetParams()
        self._check(self._lib.rt_budget_defaults(ctypes.byref(prm)), "rt_budget_defaults")
        return dict(max_passes=int(prm.max_passes), limits=[float(v) for v in prm.limits][:prm.max_passes - 1])

    def foldTiles(self, sample_rgba, acc_rgba, count, passes, pass_: int, width: int, height: int, mom_in=None, mom_out=None,
                  len_out=None, stream=None, sync: bool = True) -> None:
        """The progressive mix of a frame's own sample `sample_rgba` into `acc_rgba` with a weight per 8x8
        tile: tile t is folded when `passes` is None or passes[t] > pass_; its count c = count[t] becomes
        c + 1 = n, its pixels old + (sample - old) (1 / n), its moments (`mom_in` to `mom_out`, both or
        neither, may be one buffer) momentsAccumulate's with n_cur = n, `len_out` n.  Other tiles keep
        frame, count and moments, and get len_out = count[t].  All numpy arrays or all torch CUDA tensors."""
        px, n = int(width) * int(height), self._tiles(width, height)
        flags = self._same_kind("foldTiles", [
            (sample_rgba, px * 4, "sample frame"), (acc_rgba, px * 4, "accumulation buffer"), (count, n, "count plane", self._WORDS),
            (passes, n, "passes plane", self._WORDS), (mom_in, px * 4, "moments"), (mom_out, px * 4, "destination moments"),
            (len_out, px, "destination history lengths")])
        args = (self._h, _abi.ptr(sample_rgba), _abi.ptr(acc_rgba), _abi.ptr(count), _abi.ptr(passes), int(pass_),
                _abi.ptr(mom_in), _abi.ptr(mom_out), _abi.ptr(len_out), int(width), int(height), flags)
        self._aux_call("rt_fold_tiles", args, stream, sync)

    def tileBudget(self, tiles, stop, passes_out, width: int, height: int, max_passes: int | None = None, limits=None,
                   stats=None, stream=None, sync: bool = True):
        """The budget rule on noiseMeter's tile map `tiles`: passes_out[t] = 0 where stop[t] != 0 (`stop`
        may be None), else 1 + the number of the first max_passes - 1 `limits` the tile's mean lies above.
        None for a parameter: the library's default.  Returns the stats as a dict (`tiles`, `rounds`,
        `tile_passes`, `by_passes`); `stats` (13 words of the buffers' kind) receives the struct's words as
        well; with sync=False it must be given, nothing is read back and None is returned."""
        n = self._tiles(width, height)
        flags = self._same_kind("tileBudget", [(tiles, 2 * n, "tile map"), (stop, n, "stop plane", self._WORDS),
                                               (passes_out, n, "passes plane", self._WORDS), (stats, 13, "stats", self._WORDS)])
        if stats is None:
            if not sync:
                raise ValueError("tileBudget: sync=False needs a stats buffer")
            if flags:
                import torch

                stats = torch.zeros(13, dtype=torch.int32, device=tiles.device)
            else:
                stats = np.zeros(13, np.uint32)
        prm = _abi.RtBudgetParams()
        self._check(self._lib.rt_budget_defaults(ctypes.byref(prm)), "rt_budget_defaults")
        if max_passes is not None:
            prm.max_passes = int(max_passes)
        if limits is not None:
            if len(limits) > _abi.RT_BUDGET_MAX_PASSES - 1:
                raise ValueError("tileBudget: more than 7 limits")
            for k, v in enumerate(limits):
                prm.limits[k] = float(v)
        args = (self._h, _abi.ptr(tiles), _abi.ptr(stop), _abi.ptr(passes_out), _abi.ptr(stats), int(width), int(height),
                ctypes.byref(prm), flags)
        self._aux_call("rt_tile_budget", args, stream, sync)
        if not sync:
            return None
        w = stats if isinstance(stats, np.ndarray) else stats.cpu().numpy()
        w = np.ascontiguousarray(w).view(np.uint32)
        return dict(tiles=int(w[0]), rounds=int(w[1]), tile_passes=int(w[2]), by_passes=[int(v) for v in w[4:13]])

    def tilePassMask(self, stop, passes, pass_: int, mask_out, width: int, height: int, stream=None, sync: bool = True) -> None:
        """The stop plane (setTileStop's sense) of pass `pass_`: mask_out[t] = 0 where stop[t] == 0 (`stop`
        may be None) and passes[t] > pass_, else 1.  All numpy arrays or all torch CUDA tensors."""
        n = self._tiles(width, height)
        flags = self._same_kind("tilePassMask", [(stop, n, "stop plane", self._WORDS), (passes, n, "passes plane", self._WORDS),
                                                 (mask_out, n, "destination mask", self._WORDS)])
        args = (self._h, _abi.ptr(stop), _abi.ptr(passes), int(pass_), _abi.ptr(mask_out), int(width), int(height), flags)
        self._aux_call("rt_tile_pass_mask", args, stream, sync)

    def lastBudgetMs(self, which: str = "fold") -> float:
        """Device time of the last fold ("fold"), budget rule ("budget") or pass mask ("mask"), ms."""
        return self._last_ms("rt_last_budget_ms", 3, ("fold", "budget", "mask").index(which))

    # ---- adaptive sampling under the temporal stage: per-pixel frame counts (pathtracer_rt.h) ----
    def temporalMergeLen(self, hist_rgba, hist_len, cur_rgba, cur_len, out_rgba, out_len, width: int, height: int,
                         max_history: float = 32.0, stream=None, sync: bool = True) -> None:
        """temporalMerge with the accumulation buffer's frame count per pixel: `cur_len` (W*H floats, as
        momentsAccumulateTiles and foldTiles write them; a value under 1 or a NaN reads as 1), apart from
        both outputs.  All numpy arrays or all torch CUDA tensors."""
        px = int(width) * int(height)
        flags = self._same_kind("temporalMergeLen", [
            (hist_rgba, px * 4, "history frame"), (hist_len, px, "history lengths"), (cur_rgba, px * 4, "current frame"),
            (cur_len, px, "current frame counts"), (out_rgba, px * 4, "destination frame"),
            (out_len, px, "destination history lengths")])
        args = (self._h, _abi.ptr(hist_rgba), _abi.ptr(hist_len), _abi.ptr(cur_rgba), _abi.ptr(cur_len), float(max_history),
                _abi.ptr(out_rgba), _abi.ptr(out_len), int(width), int(height), flags)
        self._aux_call("rt_temporal_merge_len", args, stream, sync)

    def historyTrustLen(self, hist_rgba, hist_len, cur_rgba, cur_len, feat, out_len, width: int, height: int,
                        tolerance: float | None = None, sigma_normal: float = 0.3, sigma_plane: float = 0.1, stream=None,
                        sync: bool = True) -> None:
        """historyTrust with the frame count of each pixel's test taken from `cur_len` (temporalMergeLen's) at
        the pixel itself: its window's taps in tiles of other counts are weighed as if they had the centre's.
        All numpy arrays or all torch CUDA tensors."""
        px = int(width) * int(height)
        flags = self._same_kind("historyTrustLen", [
            (hist_rgba, px * 4, "history frame"), (hist_len, px, "history lengths"), (cur_rgba, px * 4, "current frame"),
            (cur_len, px, "current frame counts"), (feat, px * 8, "feature buffer"), (out_len, px, "destination history lengths")])
        if tolerance is None:
            tolerance = self.trustDefaults()["tolerance"]
        prm = _abi.RtTrustParams(float(tolerance), float(sigma_normal), float(sigma_plane))
        args = (self._h, _abi.ptr(hist_rgba), _abi.ptr(hist_len), _abi.ptr(cur_rgba), _abi.ptr(cur_len), _abi.ptr(feat),
                _abi.ptr(out_len), int(width), int(height), ctypes.byref(prm), flags)
        self._aux_call("rt_history_trust_len", args, stream, sync)

    def tileLenMin(self, length, feat, tiles_out, width: int, height: int, stream=None, sync: bool = True) -> None:
        """Per 8x8 tile (noiseMeter's grid) the shortest of the history lengths `length` (W*H floats; negative
        and NaN read as 0) among the tile's pixels that met a surface by `feat` (None: among all its pixels):
        `tiles_out`, a float per tile, +inf where no pixel counts.  All numpy arrays or all torch CUDA tensors."""
        px = int(width) * int(height)
        flags = self._same_kind("tileLenMin", [(length, px, "history lengths"), (feat, px * 8, "feature buffer"),
                                               (tiles_out, self._tiles(width, height), "tile lengths")])
        args = (self._h, _abi.ptr(length), _abi.ptr(feat), _abi.ptr(tiles_out), int(width), int(height), flags)
        self._aux_call("rt_tile_len_min", args, stream, sync)

    def lastTileLenMs(self) -> float:
        """Device time of the last tileLenMin kernel, ms."""
        return self._last_ms("rt_last_tile_len_ms")

    def tileStopSelectFrames(self, tiles, tile_frames, stop, n_frames: int, width: int, height: int,
                             threshold: float | None = None, max_ratio: float | None = None, min_frames: int | None = None,
                             dilate: int | None = None, stats=None, stream=None, sync: bool = True):
        """tileStopSelect with the frame gate per tile: tile t can be quiet only where tile_frames[t] >=
        min_frames (`tile_frames`: a float per tile, tileLenMin's output; a NaN does not pass).  A tile
        stopped now still gets the word `n_frames`."""
        return self._stop_select("tileStopSelectFrames", tiles, tile_frames, stop, n_frames, width, height, threshold, max_ratio,
                                 min_frames, dilate, stats, stream, sync)

    def read(self, host: np.ndarray) -> None:
        """Blocking readback of the last frame into `host` (GlutCLWindow.cpp:214-225)."""
        if host.dtype != np.float32 or not host.flags["C_CONTIGUOUS"]:
            raise ValueError("host buffer must be a contiguous float32 array")
        self._check(self._lib.rt_read(self._h, _abi.ptr(host), host.size), "rt_read")

    def synchronize(self) -> None:
        self._check(self._lib.rt_synchronize(self._h), "rt_synchronize")

    def partitionStripes(self, width: int, height: int, stripe: int, n_ranks: int) -> np.ndarray:
        """rt_partition_stripes: the cost-balanced owner of each of the frame's row stripes for the
        current camera, mesh and lights (a whole-frame probe, LPT over the stripes; cached per view)."""
        self._sync_scene()
        ns = (int(height) + int(stripe) - 1) // int(stripe)
        owner = np.empty(max(ns, 1), np.uint32)
        made = ctypes.c_int(0)
        self._check(self._lib.rt_partition_stripes(self._h, int(width), int(height), int(stripe), int(n_ranks),
                                                   _abi.ptr(owner), ctypes.byref(made)), "rt_partition_stripes")
        return owner[:ns]

    # ---- instrumentation ------------------------------------------------------------------
    def setCounting(self, enable: bool) -> None:
        self._check(self._lib.rt_set_counting(self._h, int(bool(enable))), "rt_set_counting")

    def counters(self) -> dict:
        c = _abi.RtCounters()
        self._check(self._lib.rt_get_counters(self._h, ctypes.byref(c)), "rt_get_counters")
        return {f: getattr(c, f) for f, _ in _abi.RtCounters._fields_}

    def counterTotals(self, reset: bool = True) -> dict:
        """rt_counter_totals: the counters summed over every render since the last reset (waits for
        the renders; frames enqueued back to back each add their own counts), with `renders` = how
        many renders they cover.  Raises if a defect guard fired in any of them."""
        c = _abi.RtCounters()
        n = ctypes.c_uint64(0)
        self._check(self._lib.rt_counter_totals(self._h, ctypes.byref(c), ctypes.byref(n), int(bool(reset))),
                    "rt_counter_totals")
        d = {f: getattr(c, f) for f, _ in _abi.RtCounters._fields_}
        d["renders"] = n.value
        return d

    def lastKernelMs(self) -> float:
        return self._last_ms("rt_last_kernel_ms")

    def lastKernelSplitMs(self) -> tuple[float, float]:
        """(candidate-list pre-pass, main kernel) device times of the last render, ms."""
        pre, main = ctypes.c_float(), ctypes.c_float()
        self._check(self._lib.rt_last_kernel_split_ms(self._h, ctypes.byref(pre), ctypes.byref(main)),
                    "rt_last_kernel_split_ms")
        return pre.value, main.value

    def renderInfo(self) -> dict:
        """rt_last_render_info: the last render's lists, sample split and schedule (no result depends
        on any of it)."""
        fn = getattr(self._lib, "rt_last_render_info", None)
        if fn is None:  # an older library loaded for an A/B run
            return {}
        i = _abi.RtRenderInfo()
        self._check(fn(self._h, ctypes.byref(i)), "rt_last_render_info")
        return {f: getattr(i, f) for f, _ in _abi.RtRenderInfo._fields_}

    def longChains(self) -> np.ndarray:
        """rt_last_long_chains: the last sample-split render's long chains (tile-local y * W + x),
        the pixels whose seed pass ran on the second stream (cooperative queries)."""
        n = ctypes.c_uint32(0)
        self._check(self._lib.rt_last_long_chains(self._h, None, 0, ctypes.byref(n)), "rt_last_long_chains")
        out = np.empty(n.value, np.uint32)
        if n.value:
            self._check(self._lib.rt_last_long_chains(self._h, _abi.ptr(out), n.value, ctypes.byref(n)),
                        "rt_last_long_chains")
        return out

    def listCounts(self) -> np.ndarray:
        """rt_last_list_counts: per pixel of the last triangle render (tile-local y * W + x) the records
        of its camera-ray candidate list; 0: no candidate, 0xffff: no list (the tree).  Empty when the
        render used no lists."""
        n = ctypes.c_uint32(0)
        self._check(self._lib.rt_last_list_counts(self._h, None, 0, ctypes.byref(n)), "rt_last_list_counts")
        out = np.empty(n.value, np.uint16)
        if n.value:
            self._check(self._lib.rt_last_list_counts(self._h, _abi.ptr(out), n.value, ctypes.byref(n)),
                        "rt_last_list_counts")
        return out

    def meshTree(self) -> dict:
        """rt_mesh_tree: the current mesh's trees as the kernels read them.  The layout's fields, and
        `nodes4` (n_nodes4 x 32 float32, the closest-hit tree), `nodes4q` ((n_nodes4 + n_nodes4_shadow)
        x 16 uint32, None without compressed nodes), `tris` (n_records x 12 float32)."""
        lay = _abi.RtTreeLayout()
        self._check(self._lib.rt_mesh_tree(self._h, ctypes.byref(lay), None, None, None), "rt_mesh_tree")
        nodes4 = np.empty((lay.n_nodes4, 32), np.float32)
        nodes4q = np.empty((lay.n_nodes4 + lay.n_nodes4_shadow, 16), np.uint32) if lay.compressed else None
        tris = np.empty((lay.n_records, 12), np.float32)
        self._check(self._lib.rt_mesh_tree(self._h, ctypes.byref(lay), _abi.ptr(nodes4), _abi.ptr(nodes4q),
                                           _abi.ptr(tris)), "rt_mesh_tree")
        out = {f: getattr(lay, f) for f, _ in _abi.RtTreeLayout._fields_}
        out.update(nodes4=nodes4, nodes4q=nodes4q, tris=tris)
        return out

    def traceRays(self, rays: np.ndarray, any_hit: bool = False) -> tuple[np.ndarray, np.ndarray]:
        r = np.ascontiguousarray(rays, _abi.RAY_DTYPE)
        idx = np.empty(r.size, np.int32)
        t = np.empty(r.size, np.float32)
        self._check(self._lib.rt_trace_rays(self._h, _abi.ptr(r), r.size, int(bool(any_hit)), _abi.ptr(idx),
                                            _abi.ptr(t)), "rt_trace_rays")
        return idx, t
