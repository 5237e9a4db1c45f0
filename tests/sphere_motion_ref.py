"""float32 numpy restatement of rt_warp_features_spheres and its binary64 twin,
shared by tests/test_sphere_motion_host.py and tests/test_gpu_sphere_motion.py.  Every operation is one
IEEE operation of the working type in the order the definition gives (numpy float32 arrays round each
product and sum separately).  Spheres are records of the package's SPHERE_DTYPE (fields "center" and
"radius" are all that is read)."""
from __future__ import annotations

import numpy as np

F = np.float32
RT_FEAT_NONE, RT_FEAT_SPHERE0 = -2, -16


def _geometry(spheres):
    """(n, 4) float32: centre and radius of every sphere."""
    s = np.asarray(spheres).reshape(-1)
    g = np.zeros((len(s), 4), F)
    if len(s):
        g[:, :3], g[:, 3] = s["center"], s["radius"]
    return g


def sphere_pixels(cur_feat, n_cur, n_prev):
    """(feature planes (2, n, 4), sphere pixels (id <= RT_FEAT_SPHERE0), their sphere index as int64,
    whether that index is below both counts)."""
    cf = np.asarray(cur_feat, F).reshape(2, -1, 4)
    ids = np.ascontiguousarray(cf[1, :, 3]).view(np.int32)
    k = np.flatnonzero(ids <= RT_FEAT_SPHERE0)
    s = RT_FEAT_SPHERE0 - ids[k].astype(np.int64)  # (no overflow for INT32_MIN)
    return cf, k, s, (s < n_cur) & (s < n_prev)


def moved_points(N, prev_geom, T=F):
    """Rules 4 and 5 in the type T for unit normals N (n, 3) and the earlier spheres' (centre, radius)
    rows prev_geom (n, 4): (P', ok)."""
    N, g = np.asarray(N, F).astype(T), np.asarray(prev_geom, F).astype(T)
    with np.errstate(all="ignore"):
        r = g[:, 3]
        P = g[:, :3] + N * r[:, None]
        ok = (r > 0) & np.isfinite(r) & np.isfinite(P).all(axis=1)
    return P, ok


def warp_spheres(cur_feat, cur_spheres, prev_spheres):
    """rt_warp_features_spheres: the warped feature buffer (2 * n * 4 float32)."""
    cur, prev = _geometry(cur_spheres), _geometry(prev_spheres)
    cf, k, s, inside = sphere_pixels(cur_feat, len(cur), len(prev))
    out = cf.copy()
    out[0, k] = (0.0, 0.0, 0.0, np.inf)  # "no surface" until a rule below keeps the pixel
    out[1, k, :3] = 0.0
    out.view(np.int32)[1, k, 3] = RT_FEAT_NONE
    k, s = k[inside], s[inside]
    same = (cur[s].view(np.uint32) == prev[s].view(np.uint32)).all(axis=1)  # rule 3: the input's bits
    out[:, k[same]] = cf[:, k[same]]
    k, s = k[~same], s[~same]
    P, ok = moved_points(cf[1, k, :3], prev[s], F)
    k = k[ok]
    out[0, k, :3], out[0, k, 3] = P[ok], cf[0, k, 3]
    out[1, k] = cf[1, k]
    return out.reshape(-1)


def warp_spheres64(cur_feat, cur_spheres, prev_spheres):
    """The binary64 twin of rule 4 over the pixels of moved spheres whose index is in range:
    (pixels, their sphere index, P', ok)."""
    cur, prev = _geometry(cur_spheres), _geometry(prev_spheres)
    cf, k, s, inside = sphere_pixels(cur_feat, len(cur), len(prev))
    k, s = k[inside], s[inside]
    moved = ~(cur[s].view(np.uint32) == prev[s].view(np.uint32)).all(axis=1)
    k, s = k[moved], s[moved]
    P, ok = moved_points(cf[1, k, :3], prev[s], np.float64)
    return k, s, P, ok


def features_spheres(rays, spheres):
    """The feature buffer (2, n, 4) float32 of the sphere kernels for `rays` (RAY_DTYPE, the pixel-centre
    rays of rt_primary_rays): a restatement of k_features_sph — intersect_sphere over the list (strict
    interval beyond SMALL_F, the lowest index on ties), P = o + d t, N = (P - C) * (1 / r), then the box."""
    import features_ref as fr

    o, d = np.ascontiguousarray(rays["o"], F), np.ascontiguousarray(rays["d"], F)
    g = _geometry(spheres)
    n = len(o)
    hit = np.full(n, -1, np.int64)
    tmax = np.full(n, np.inf, F)
    with np.errstate(all="ignore"):
        for i, (cx, cy, cz, r) in enumerate(g):
            ox, oy, oz = o[:, 0] - cx, o[:, 1] - cy, o[:, 2] - cz
            dist2 = (ox * ox + oy * oy) + oz * oz
            b_neg = -((ox * d[:, 0] + oy * d[:, 1]) + oz * d[:, 2])
            disc = b_neg * b_neg - (dist2 - r * r)
            sq = np.sqrt(np.where(disc > 0, disc, F(0.0)))
            dd = np.where(disc > 0, np.where(b_neg - sq > fr.SMALL_F, b_neg - sq, b_neg + sq), F(0.0)).astype(F)
            take = (dd > fr.SMALL_F) & (dd < tmax)
            hit[take], tmax[take] = i, dd[take]
    feat = np.zeros((2, n, 4), F)
    fid = np.full(n, RT_FEAT_NONE, np.int32)
    feat[0, :, 3] = np.inf
    k = np.flatnonzero(hit >= 0)
    s = g[hit[k]]
    P = fr.hit_points(o[k], d[k], tmax[k])
    feat[0, k, :3], feat[0, k, 3] = P, tmax[k]
    feat[1, k, :3] = (P - s[:, :3]) * (F(1.0) / s[:, 3])[:, None]
    fid[k] = (RT_FEAT_SPHERE0 - hit[k]).astype(np.int32)
    miss = np.flatnonzero(hit < 0)
    bt, ok, Pb, Nb = fr.box_hits(o[miss], d[miss])
    mb = miss[ok]
    feat[0, mb, :3], feat[0, mb, 3], feat[1, mb, :3] = Pb[ok], bt[ok], Nb[ok]
    fid[mb] = fr.RT_FEAT_BOX
    feat[1, :, 3] = fid.view(F)
    return feat


QUALITY_STEPS, QUALITY_STEP_X = 12, 0.05


def quality_spheres(scenes, sphere_dtype, k):
    """The scene of the quality evaluation at step k: main_scene() with sphere 2 given
    sphere 0's diffuse material and moved k * 0.05 along x (the product in binary64, rounded once)."""
    s = np.asarray(scenes.main_scene(), sphere_dtype).reshape(-1).copy()
    centre, radius = s["center"][2].copy(), s["radius"][2]
    s[2] = s[0]
    s["center"][2], s["radius"][2] = centre, radius
    s["center"][2, 0] = F(centre[0] + QUALITY_STEP_X * k)
    return s
