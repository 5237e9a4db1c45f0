"""The three experiments of DESIGN.md §4.14 — A: nothing moves, B: the light moves, C: the mesh turns —
over a backend that supplies frames, features and the display stages: the oracle with the float32
restatements (tests/test_trust_host.py) or the device (tests/test_gpu_trust.py).  Both run exactly
these inputs, so the device reproduces the CPU's figures to the digit.

128 x 96, the golden view with camera[0:4] *= 2, the 2000-triangle mesh, the ply_scene light; 12
frames at 1 spp with continuing seeds, the carried length capped at 8 (the merge's at 32); mean
squared errors of the last frame against a sampleRate-16 frame of the last scene from
default_seeds(skip=12345)."""
from __future__ import annotations

import numpy as np

import features_ref as fr
import motion_ref as mr
import temporal_ref as tr
import trust_ref as tref

F = np.float32
W, H = 128, 96
FRAMES = 12
CARRY_CAP, MERGE_CAP = 8.0, 32.0
TARGET, EL0, AZ0, DIST = (0.0, -4.0, 0.0), 40.0, 105.0, 5.0
SWEEP = (1.0, 1.5, 2.0, 3.0)


def turn(verts, deg, centre):
    """`deg` degrees about the vertical axis through `centre`, binary64, rounded to float32."""
    v, c = np.asarray(verts, F).astype(np.float64), np.array(centre, np.float64)
    a = np.deg2rad(deg)
    d = v - c
    out = np.stack([np.cos(a) * d[:, 0] + np.sin(a) * d[:, 2], d[:, 1], -np.sin(a) * d[:, 0] + np.cos(a) * d[:, 2]], axis=1)
    return np.ascontiguousarray((out + c).astype(F))


def camera(sc):
    cam = sc.camera_spherical(64, target=TARGET, elevation=EL0, azimuth=AZ0, distance=DIST)
    cam[0:4] *= 2
    return cam


def scenes_of(sc, which):
    """Per frame (spheres, vertices) of experiment `which`, and the mesh's indices."""
    verts, idx = sc.make_mesh(2000)
    out = []
    for k in range(FRAMES):
        S, v = sc.ply_scene(), verts
        if which == "B":  # the light's centre x from -2.2 to +2.2, 0.4 per frame (y = 4, z = 2)
            S[-1]["center"] = (F(-2.2) + F(0.4) * F(k), 4.0, 2.0)
        if which == "C":  # DESIGN.md §4.13's turning mesh
            v = turn(verts, 2.0 * k, sc.MESH_CENTER)
        out.append((S, v))
    return out, idx


class CpuBackend:
    """The oracle's BVH-mode frames and linear-loop features, the display stages by the restatements."""

    def __init__(self, pt, orc):
        self.pt, self.orc, self.sc = pt, orc, pt.scenes
        self.cam = camera(self.sc)
        self.Wp, self.Hp = self.sc.padded_dims(W, H)
        rays = np.zeros(W * H, pt._abi.RAY_DTYPE)
        assert pt.load_library().rt_primary_rays(pt._abi.ptr(self.cam), W, H, pt._abi.ptr(rays)) == pt._abi.RT_OK
        self.rays = rays

    def frames(self, scenes, idx):
        """The 1-spp frames and features of the scenes, then the reference frame of the last one."""
        seeds = self.sc.default_seeds(self.Wp, self.Hp)
        out, feats = [], {}
        for S, v in scenes:
            bvh = self.orc.build_bvh(v, idx)
            frame = np.zeros(W * H * 4, F)
            self.orc.render_tris(frame, self.cam, S, W, H, self.Wp, self.Hp, 1, 6, 0, seeds, v, idx, bvh=bvh)
            if id(v) not in feats:  # (the spheres are not in the features of RT_KERNEL_TRIS: one per pose)
                feats[id(v)] = fr.features_tris(self.orc, self.rays, v, idx).reshape(-1)
            out.append((frame, feats[id(v)]))
            bvh.close()
        S, v = scenes[-1]
        bvh = self.orc.build_bvh(v, idx)
        ref = np.zeros(W * H * 4, F)
        self.orc.render_tris(ref, self.cam, S, W, H, self.Wp, self.Hp, 16, 6, 0,
                             self.sc.default_seeds(self.Wp, self.Hp, skip=12345), v, idx, bvh=bvh)
        bvh.close()
        return out, ref

    def warp(self, feat, idx, cur, prev):
        return mr.warp(feat, idx, cur, prev)

    def reproject(self, hist, hl, pfeat, cfeat):
        return tr.reproject(hist, hl, pfeat, self.cam, cfeat, W, H, max_history=CARRY_CAP)

    def trust(self, car, cl, frame, n, feat, tol):
        return tref.trust(self.orc, car, cl, frame, n, feat, W, H, tolerance=tol)

    def merge(self, car, cl, frame, n):
        return tr.merge(car, cl, frame, n, max_history=MERGE_CAP)

    def atrous(self, src, feat, it):
        return fr.atrous(self.orc, src, feat, W, H, iterations=it)


def chain(be, frames, scenes, idx, tol):
    """The carried frame of the last of `frames` (tol None: untrusted): (merged, its lengths, the last
    trusted plane or None, the carried lengths it judged)."""
    hist = hl = pfeat = tl = cl = None
    for k, (frame, feat) in enumerate(frames):
        car, cl = np.zeros(W * H * 4, F), np.zeros(W * H, F)
        tl = None
        if hist is not None:
            cfeat = feat
            if scenes[k][1] is not scenes[k - 1][1]:  # the mesh moved: the taps are sought where the material was
                cfeat = be.warp(feat, idx, scenes[k][1], scenes[k - 1][1])
            car, cl = be.reproject(hist, hl, pfeat, cfeat)
            if tol is not None:
                tl = be.trust(car, cl, frame, 1.0, feat, tol)
        hist, hl = be.merge(car, cl if tl is None else tl, frame, 1.0)
        pfeat = feat
    return hist, hl, tl, cl


def mse(a, ref, sel=slice(None)):
    d = a.reshape(-1, 4)[sel, :3].astype(np.float64) - ref.reshape(-1, 4)[sel, :3].astype(np.float64)
    return float((d * d).mean())


def evaluate(be, which, tols=(1.5,)):
    """The figures of experiment `which`: a dict of mean squared errors — "1spp", "alone3" (a-trous
    alone, 3 passes), "alone" ({passes: mse} at 2, 3, 5), per tolerance (None: untrusted) "merged" and
    "merged3", on the mesh pixels "mesh_*" — and "cut": the share of the frame's pixels whose trusted length
    is below half the carried one in the last frame."""
    scenes, idx = scenes_of(be.sc, which)
    frames, ref = be.frames(scenes, idx)
    frame, feat = frames[-1]
    meshpx = fr.feature_ids(feat) >= 0
    alone = {it: be.atrous(frame, feat, it) for it in (2, 3, 5)}
    res = {"1spp": mse(frame, ref), "mesh_1spp": mse(frame, ref, meshpx), "mesh_share": float(meshpx.mean()),
           "alone": {it: mse(a, ref) for it, a in alone.items()}, "alone3": mse(alone[3], ref),
           "mesh_alone3": mse(alone[3], ref, meshpx), "merged": {}, "merged3": {}, "mesh_merged": {}, "mesh_merged3": {},
           "cut": {}}
    for tol in (None,) + tuple(tols):
        hist, _, tl, cl = chain(be, frames, scenes, idx, tol)
        f3 = be.atrous(hist, feat, 3)
        res["merged"][tol], res["merged3"][tol] = mse(hist, ref), mse(f3, ref)
        res["mesh_merged"][tol], res["mesh_merged3"][tol] = mse(hist, ref, meshpx), mse(f3, ref, meshpx)
        if tol is not None:
            res["cut"][tol] = float((tl < cl / F(2.0)).mean())
    return res


# ---- inputs of the bit-equality tests ---------------------------------------------------------

W0, H0 = 64, 48  # the golden triangle case
# (33, 9): one pixel beyond a block's edge in both directions
WINDOWS = {(1, 1): (20, 20), (5, 3): (8, 30), (37, 29): (3, 9), (64, 48): (0, 0), (33, 9): (12, 20)}


def _crop_frame(frame, x0, y0, w, h):
    return np.ascontiguousarray(np.asarray(frame, F).reshape(H0, W0, 4)[y0:y0 + h, x0:x0 + w]).reshape(-1)


def golden_inputs(g, feat, w, h):
    """(hist, hist_len, cur, feat) from the golden 64 x 48 triangle case: its first progressive frame as
    the history, its last as the accumulation buffer, `feat` (the view's features) cropped like them;
    lengths of 0, 1, 2.5 and 8."""
    x0, y0 = WINDOWS[(w, h)]
    ln = np.array([0.0, 1.0, 2.5, 8.0, 8.0], F)[np.arange(w * h) % 5]
    np.random.default_rng(w + h).shuffle(ln)
    if w * h == 1:
        ln[:] = 2.5
    return (_crop_frame(g["frames"][0], x0, y0, w, h), ln, _crop_frame(g["frames"][-1], x0, y0, w, h),
            fr.crop_features(feat, W0, H0, x0, y0, w, h))


def synthetic_inputs(w, h, seed, huge=True):
    """A frame no scene produces: a gently curved sheet cut into 3 x 2 patches of random surface classes
    (triangles, the box, two spheres, nothing), history lengths with zeros, history colours in [-0.5, 1.5), the accumulation buffer noisier
    and differently shaded, with (huge) some components of 1e20 and -1e20, whose squared luminance overflows."""
    rng = np.random.default_rng(seed)
    n = w * h
    ys, xs = np.mgrid[0:h, 0:w]
    pool = np.array([3, 77, 1999, fr.RT_FEAT_BOX, fr.RT_FEAT_NONE, fr.RT_FEAT_SPHERE0, fr.RT_FEAT_SPHERE0 - 2], np.int32)
    patch = rng.integers(0, len(pool), (h // 2 + 1, w // 3 + 1))
    ids = pool[patch[ys // 2, xs // 3]].reshape(-1).astype(np.int32)
    feat = np.zeros((2, n, 4), F)
    feat[0, :, 0], feat[0, :, 1] = (xs.reshape(-1) * 0.02).astype(F), (ys.reshape(-1) * 0.02).astype(F)
    feat[0, :, 2] = rng.normal(0.0, 0.03, n).astype(F)
    feat[0, :, 3] = 3.0
    nrm = np.array([0.0, 0.0, -1.0]) + rng.normal(0.0, 0.1, (n, 3))
    feat[1, :, :3] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    feat[1, :, 3] = ids.view(F)
    ln = np.array([0.0, 0.0, 1.0, 3.25, 8.0, 32.0], F)[rng.integers(0, 6, n)]
    hist = (rng.random(n * 4, dtype=F) * F(2.0) - F(0.5)).astype(F)
    # the accumulation buffer: the history with noise, and a smooth change of shading on top of it (about
    # half of the windows are shortened)
    shade = (0.4 * np.sin(xs * 0.3) * np.cos(ys * 0.2)).astype(F).reshape(-1)
    cur = (hist + rng.normal(0.0, 0.3, n * 4).astype(F) + np.repeat(shade, 4)).astype(F)
    if huge:
        for buf in (hist, cur):
            k = rng.integers(0, n * 4, max(n // 40, 1))
            buf[k] = np.where(rng.random(len(k)) < 0.5, F(1e20), F(-1e20))
    return hist, ln, cur, feat.reshape(-1)
