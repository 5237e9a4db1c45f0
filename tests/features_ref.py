"""float32 numpy restatements of the first-hit features and the a-trous filter,
shared by tests/test_gpu_features.py and tests/test_gpu_denoise.py.  Every operation is one IEEE
float32 operation in the order the definition gives (numpy float32 arrays round each product, sum,
quotient and square root separately); the exponential is the pinned one, through the oracle."""
from __future__ import annotations

import numpy as np

F = np.float32
RT_FEAT_BOX, RT_FEAT_NONE, RT_FEAT_SPHERE0 = -1, -2, -16
SMALL_F = F(1e-4)
BOX = (F(6.0), F(5.0), F(6.0))


def mesh_normals(verts, idx, ids):
    """N = normalize(cross3(e2, e1)) of triangles `ids`, e1 = v1 - v0, e2 = v2 - v0 (get_triangle)."""
    v = np.asarray(verts, F).reshape(-1, 3)
    tri = np.asarray(idx, np.int32).reshape(-1, 3)[ids]
    v0, v1, v2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    a, b = e2, e1
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                  a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    ln = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    return n / ln[:, None]


def hit_points(o, d, t):
    """P = o + d * t per component, multiply then add."""
    return (o + d * t[:, None]).astype(F)


def box_hits(o, d):
    """intersect_box(o, d, SMALL_F, 6, 5, 6) and box_normal (geometryFuncs.h:71-150) for rays whose
    direction has no zero component; returns (t, accepted, P, N)."""
    assert np.all(d != 0)
    with np.errstate(all="ignore"):
        t1 = (F(0.0) - BOX[0] - o[:, 0]) / d[:, 0]
        t2 = (F(0.0) + BOX[0] - o[:, 0]) / d[:, 0]
        nt, ft = np.minimum(t1, t2), np.maximum(t1, t2)
        for k in (1, 2):
            t1 = (F(0.0) - BOX[k] - o[:, k]) / d[:, k]
            t2 = (F(0.0) + BOX[k] - o[:, k]) / d[:, k]
            lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
            nt, ft = np.maximum(lo, nt), np.minimum(hi, ft)
        t = np.where((nt > ft) | (ft < SMALL_F), F(np.inf), np.where(nt < SMALL_F, ft, nt)).astype(F)
        ok = (t > SMALL_F) & (t < F(np.inf))
        P = hit_points(o, d, np.where(ok, t, F(0.0)).astype(F))
        dx = np.abs(np.abs(P[:, 0]) - BOX[0])
        dy = np.abs(np.abs(P[:, 1]) - BOX[1])
        dz = np.abs(np.abs(P[:, 2]) - BOX[2])
        N = np.zeros_like(P)
        ax = np.where((dx < dy) & (dx < dz), 0, np.where(dy < dz, 1, 2))
        r = np.arange(len(P))
        N[r, ax] = -P[r, ax] / np.abs(P[r, ax])
    return t, ok, P, N


def features_tris(orc, rays, verts, idx):
    """The feature buffer (2, n, 4) float32 of RT_KERNEL_TRIS for `rays` (RAY_DTYPE), mesh hits by the
    oracle's linear loop."""
    o, d = np.ascontiguousarray(rays["o"], F), np.ascontiguousarray(rays["d"], F)
    ids, t = orc.closest_hits(rays, np.ascontiguousarray(verts, F), np.ascontiguousarray(idx, np.int32))
    n = len(rays)
    feat = np.zeros((2, n, 4), F)
    fid = np.full(n, RT_FEAT_NONE, np.int32)
    feat[0, :, 3] = np.inf
    hit = ids >= 0
    feat[0, hit, :3] = hit_points(o[hit], d[hit], t[hit])
    feat[0, hit, 3] = t[hit]
    feat[1, hit, :3] = mesh_normals(verts, idx, ids[hit])
    fid[hit] = ids[hit]
    miss = np.flatnonzero(~hit)
    bt, ok, P, N = box_hits(o[miss], d[miss])
    mb = miss[ok]
    feat[0, mb, :3], feat[0, mb, 3], feat[1, mb, :3] = P[ok], bt[ok], N[ok]
    fid[mb] = RT_FEAT_BOX
    feat[1, :, 3] = fid.view(F)
    return feat


def classify_spheres64(o, d, centres, radii):
    """float64 analytic first surface of rays (o, d) in the sphere scene: RT_FEAT_SPHERE0 - s for the
    nearest sphere met beyond SMALL_F, else RT_FEAT_BOX (the far wall of the box) or RT_FEAT_NONE."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = len(d)
    best_t = np.full(n, np.inf)
    ids = np.full(n, RT_FEAT_NONE, np.int32)
    dd = (d * d).sum(axis=1)
    for s, (c, r) in enumerate(zip(np.asarray(centres, np.float64), np.asarray(radii, np.float64))):
        oc = o - c
        b = (oc * d).sum(axis=1)
        disc = b * b - dd * ((oc * oc).sum(axis=1) - r * r)
        ok = disc > 0
        sq = np.sqrt(np.where(ok, disc, 0.0))
        t = np.where((-b - sq) / dd > 1e-4, (-b - sq) / dd, (-b + sq) / dd)
        ok &= (t > 1e-4) & (t < best_t)
        best_t[ok], ids[ok] = t[ok], RT_FEAT_SPHERE0 - s
    with np.errstate(all="ignore"):
        half = np.array(BOX, np.float64)
        ta, tb = (-half - o) / d, (half - o) / d
        near, far = np.minimum(ta, tb).max(axis=1), np.maximum(ta, tb).min(axis=1)
        tbox = np.where(near > 1e-4, near, far)
        box = (near <= far) & (tbox > 1e-4)
    ids[(ids == RT_FEAT_NONE) & box] = RT_FEAT_BOX
    return ids


def stable_spheres64(o, d, centres, radii, eps=1e-5):
    """(ids, stable): the float64 classification of the rays, and where it stays the same when a
    component of d moves by +-eps."""
    ids = classify_spheres64(o, d, centres, radii)
    stable = np.ones(len(ids), bool)
    for k in range(3):
        for sgn in (-1.0, 1.0):
            e = np.zeros(3)
            e[k] = sgn * eps
            stable &= classify_spheres64(o, np.asarray(d, np.float64) + e, centres, radii) == ids
    return ids, stable


def feature_ids(feat):
    return np.ascontiguousarray(feat.reshape(2, -1, 4)[1, :, 3]).view(np.int32)


def crop_features(feat, W, H, x0, y0, w, h):
    """The (w, h) window at (x0, y0) of a W x H feature buffer, as a feature buffer of its own."""
    f = feat.reshape(2, H, W, 4)[:, y0:y0 + h, x0:x0 + w, :]
    return np.ascontiguousarray(f).reshape(-1)


def inverse_variances(iterations, sigma_color, sigma_normal, sigma_plane):
    with np.errstate(all="ignore"):
        isc = []
        for i in range(iterations):
            sc = F(np.ldexp(F(sigma_color), -i))
            isc.append(F(1.0) / F(sc * sc))
        isn = F(1.0) / F(F(sigma_normal) * F(sigma_normal))
        isp = F(1.0) / F(F(sigma_plane) * F(sigma_plane))
    return isc, isn, isp


def atrous(orc, col, feat, W, H, iterations=5, sigma_color=2.0, sigma_normal=0.3, sigma_plane=0.1):
    """The filter of DESIGN.md §4.9: returns the W*H*4 float32 output."""
    c = np.array(col, F).reshape(H, W, 4)
    f = np.asarray(feat, F).reshape(2, H, W, 4)
    P, N = f[0, :, :, :3], f[1, :, :, :3]
    isc, isn, isp = inverse_variances(iterations, sigma_color, sigma_normal, sigma_plane)
    k = [F(0.375), F(0.25), F(0.0625)]
    ys, xs = np.mgrid[0:H, 0:W]
    for i in range(iterations):
        s = 1 << i
        acc = np.zeros((H, W, 3), F)
        wsum = np.zeros((H, W), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + s * dy, xs + s * dx
                ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                if not ok.any():
                    continue
                py, px = ys[ok], xs[ok]
                cq, cp = c[qy[ok], qx[ok], :3], c[py, px, :3]
                h = F(k[abs(dx)] * k[abs(dy)])
                dc = cq - cp
                ec = dc[:, 0] * dc[:, 0] + dc[:, 1] * dc[:, 1] + dc[:, 2] * dc[:, 2]
                dn = N[qy[ok], qx[ok]] - N[py, px]
                en = dn[:, 0] * dn[:, 0] + dn[:, 1] * dn[:, 1] + dn[:, 2] * dn[:, 2]
                dp, n_p = P[qy[ok], qx[ok]] - P[py, px], N[py, px]
                pl = dp[:, 0] * n_p[:, 0] + dp[:, 1] * n_p[:, 1] + dp[:, 2] * n_p[:, 2]
                ep = pl * pl
                arg = -((ec * isc[i] + en * isn) + ep * isp)
                w = h * orc.math("exp", arg.astype(F))
                acc[py, px] = acc[py, px] + cq * w[:, None]
                wsum[py, px] = wsum[py, px] + w
        out = c.copy()
        out[:, :, :3] = acc / wsum[:, :, None]
        c = out
    return c.reshape(-1)
