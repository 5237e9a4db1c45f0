"""float32 numpy restatement of rt_warp_features and its binary64 twin, shared by
tests/test_motion_host.py and tests/test_gpu_motion.py.  Every operation is one IEEE operation of the
working type in the order the definition gives (numpy float32 arrays round each product, sum,
difference, quotient and square root separately)."""
from __future__ import annotations

import numpy as np

F = np.float32
RT_FEAT_NONE = -2


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def solve(P, cur, prev, T=F):
    """Steps 3-5 of the definition in the type T for points P (n, 3) with their triangles' current
    and earlier vertices cur, prev (n, 3 vertices, 3): (P', N', ok, u, v)."""
    P, cur, prev = (np.asarray(x, F).astype(T) for x in (P, cur, prev))
    with np.errstate(all="ignore"):
        a = cur[:, 0]
        e1, e2, w = cur[:, 1] - a, cur[:, 2] - a, P - a
        n = _cross(e1, e2)
        nn = _dot(n, n)
        u = _dot(_cross(w, e2), n) / nn
        v = _dot(_cross(e1, w), n) / nn
        pa = prev[:, 0]
        f1, f2 = prev[:, 1] - pa, prev[:, 2] - pa
        Pp = (pa + f1 * u[:, None]) + f2 * v[:, None]
        m = _cross(f2, f1)
        ln = np.sqrt(_dot(m, m))
        N = m / ln[:, None]
        ok = (nn != 0) & (ln > 0) & np.isfinite(Pp).all(axis=1) & np.isfinite(N).all(axis=1)
    return Pp, N, ok, u, v


def _mesh_pixels(cur_feat, idx, n_verts):
    """(feature planes (2, n, 4), ids, the mesh pixels whose id and indices are in range, their triangles)."""
    cf = np.asarray(cur_feat, F).reshape(2, -1, 4)
    tri = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    ids = np.ascontiguousarray(cf[1, :, 3]).view(np.int32)
    k = np.flatnonzero((ids >= 0) & (ids < len(tri)))
    t = tri[ids[k]]
    inside = ((t >= 0) & (t < n_verts)).all(axis=1)
    return cf, ids, k[inside], t[inside]


def warp(cur_feat, idx, pose, prev_verts):
    """rt_warp_features: the warped feature buffer (2 * n * 4 float32).  Pixels with id < 0 keep
    their bits; a mesh pixel that cannot be carried is "no surface"."""
    pose, prev = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (pose, prev_verts))
    cf, ids, k, t = _mesh_pixels(cur_feat, idx, len(pose))
    out = cf.copy()
    mesh = ids >= 0
    out[0, mesh] = (0.0, 0.0, 0.0, np.inf)
    out[1, mesh, :3] = 0.0
    out.view(np.int32)[1, mesh, 3] = RT_FEAT_NONE
    Pp, N, ok, _, _ = solve(cf[0, k, :3], pose[t], prev[t], F)
    k = k[ok]
    out[0, k, :3], out[0, k, 3] = Pp[ok], cf[0, k, 3]
    out[1, k, :3], out[1, k, 3] = N[ok], cf[1, k, 3]
    return out.reshape(-1)


def warp64(cur_feat, idx, pose, prev_verts):
    """The binary64 twin of the same expressions over the mesh pixels: (pixels, P', N', ok, u, v)."""
    pose, prev = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (pose, prev_verts))
    cf, _, k, t = _mesh_pixels(cur_feat, idx, len(pose))
    return (k,) + solve(cf[0, k, :3], pose[t], prev[t], np.float64)
