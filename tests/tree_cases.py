"""Meshes and deterministic ray sets shared by tests/test_tree_host.py and tests/test_gpu_tree.py.

The meshes sit on the edges of the builders (leaf sizes, equal Morton codes, zero extent on an
axis, far from the origin, mixed scales, the 1e-4 determinant bound, not encodable, nothing
hittable); the rays on the edges of the traversal (signed zero direction components, origins on
vertex coordinates and on decoded box planes, shared vertices and edges, rays in a triangle's
plane, tmin / tmax exactly on a hit, empty intervals, non-unit directions).
"""
from __future__ import annotations

import numpy as np

F32 = np.float32

TRUNCATED = (1, 2, 4, 5, 8, 9)  # around the GPU builder's kLeafMax 4 and RT_LEAF_MAX 8
MESHES = [f"sphere200_first{n}" for n in TRUNCATED] + [
    "sphere2000", "one_centre600", "flat_grid", "far_grid", "mixed_scales", "det_bound", "huge8", "unhittable"]
NOT_ENCODABLE = ("huge8",)
NOTHING_HITTABLE = ("unhittable",)


def _soup(tri) -> tuple[np.ndarray, np.ndarray]:
    tri = np.asarray(tri, F32).reshape(-1, 3, 3)
    return np.ascontiguousarray(tri.reshape(-1, 3)), np.arange(3 * len(tri), dtype=np.int32).reshape(-1, 3)


def _grid(origin, cell, n=16):
    """n x n cells, two triangles each, in the plane y = origin[1] (shared vertices and edges)."""
    o = np.asarray(origin, F32)
    c = F32(cell)
    k = np.arange(n + 1, dtype=F32)
    xs, zs = o[0] + c * k, o[2] + c * k
    verts = np.stack([np.repeat(xs, n + 1), np.full((n + 1) ** 2, o[1], F32), np.tile(zs, n + 1)], axis=1).astype(F32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).reshape(-1)
    idx = np.concatenate([np.stack([a, a + 1, a + n + 2], axis=1), np.stack([a, a + n + 2, a + n + 1], axis=1)])
    return verts, np.ascontiguousarray(idx, np.int32)


def det_bound_mesh(nt=4000, seed=23):
    """Triangles whose |e1 x e2| straddles the 1e-4 determinant bound (as
    test_unhittable_triangles_left_out_of_the_tree builds them)."""
    rng = np.random.default_rng(seed)
    cr = np.exp(rng.uniform(np.log(2e-5), np.log(5e-4), nt))
    a = np.sqrt(cr) * np.exp(rng.uniform(-1.5, 1.5, nt))
    b = cr / a
    nrm = rng.normal(size=(nt, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    t1 = np.cross(nrm, rng.normal(size=(nt, 3)))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    c = rng.uniform(-3, 3, (nt, 3))
    return _soup(np.stack([c, c + a[:, None] * t1, c + b[:, None] * t2], axis=1))


def make(name, sc):
    """(verts [V, 3] float32, idx [n, 3] int32) of the mesh `name`; sc: pathtracer.cl_amd.scenes."""
    if name.startswith("sphere200_first"):
        v, i = sc.make_mesh(200)
        return v, np.ascontiguousarray(i[:int(name[len("sphere200_first"):])])
    if name == "sphere2000":
        return sc.make_mesh(2000)
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one_centre600":  # every box is symmetric about the origin: one centroid, one Morton code
        n = 600
        h = rng.uniform(0.05, 2.0, (n, 3))
        r = rng.uniform(-0.9, 0.9, (n, 3)) * h
        tri = np.stack([np.stack([-h[:, 0], -h[:, 1], r[:, 2]], axis=1), np.stack([h[:, 0], r[:, 1], -h[:, 2]], axis=1),
                        np.stack([r[:, 0], h[:, 1], h[:, 2]], axis=1)], axis=1)
        return _soup(tri)
    if name == "flat_grid":
        return _grid((-2.0, 0.25, -2.0), 0.25)
    if name == "far_grid":
        return _grid((1000.0, 1000.0, 1000.0), 0.05)
    if name == "mixed_scales":
        n = 3000
        c = rng.uniform(-4, 4, (2 * n, 1, 3))
        ext = np.concatenate([rng.uniform(0.5, 8.0, n), np.full(n, 0.02)])[:, None, None]
        tri = c + ext * rng.uniform(-0.5, 0.5, (2 * n, 3, 3))
        tri[1] = tri[0]  # duplicates and a rotated copy: the tie rule
        tri[3] = tri[2][[1, 2, 0]]
        tri[n + 1] = tri[n]
        return _soup(tri)
    if name == "det_bound":
        return det_bound_mesh()
    if name == "huge8":  # coordinates within +-20000: a node wider than 255 * 2^7, no compressed nodes
        return _soup(rng.uniform(-20000.0, 20000.0, (8, 3, 3)))
    if name == "unhittable":  # |e1 x e2| about 1e-6: below the bound for every unit direction
        c = rng.uniform(-2, 2, (64, 1, 3))
        return _soup(c + 1e-3 * rng.uniform(-0.5, 0.5, (64, 3, 3)))
    raise KeyError(name)


# Triangles of the spill mesh per builder: a count at which the builder's stack4 is at least
# RT_STACK_DEPTH + 4 and the model walk (tree_ref.live_stack) of the two test rays keeps
# RT_STACK_DEPTH + 3 entries live (DESIGN.md §4.2a has the figures)
SPILL_COUNT = {"host": 32768, "gpu": 131072}


def spill_stack(n, r_lo=1.0, r_hi=1.25):
    """n parallel triangles (-r, -r, z), (2r, -r, z), (-r, 2r, z), z evenly spaced in [-3, 3], r random
    in [1, 1.25]: a ray along z through (0.9, 0.9) is inside every box and outside every triangle,
    one through (0, 0) hits them all."""
    z = np.linspace(-3.0, 3.0, n)
    r = np.random.default_rng(1).uniform(r_lo, r_hi, n)
    tri = np.stack([np.stack([-r, -r, z], axis=1), np.stack([2 * r, -r, z], axis=1), np.stack([-r, 2 * r, z], axis=1)], axis=1)
    return _soup(tri)


# ---- rays ----------------------------------------------------------------------------------------
def _unit32(d):
    d = np.asarray(d, F32)
    return (d / np.sqrt((d * d).sum(axis=1, dtype=F32))[:, None]).astype(F32)


def tree_planes(tree, limit=4096):
    """(axis, value) of box planes of the read-back tree: decoded planes of the compressed nodes, or
    the full-precision ones without them."""
    from tree_ref import RT_EMPTY_CHILD, decoded_boxes

    if tree["nodes4q"] is not None:
        lo, hi = decoded_boxes(tree)
        used = tree["nodes4q"][:, 12:16].view(np.int32) != RT_EMPTY_CHILD
    else:
        f = tree["nodes4"].astype(np.float64)
        lo = np.stack([f[:, 0:4], f[:, 8:12], f[:, 16:20]], axis=2)
        hi = np.stack([f[:, 4:8], f[:, 12:16], f[:, 20:24]], axis=2)
        used = tree["nodes4"][:, 24:28].view(np.int32) != RT_EMPTY_CHILD
    out = []
    for a in range(3):
        vals = np.unique(np.concatenate([lo[:, :, a][used], hi[:, :, a][used]]).astype(F32))
        out += [(a, x) for x in vals[:: max(1, len(vals) * 3 // limit)]]
    return out


def base_rays(verts, idx, planes, ray_dtype, seed=5):
    """About 1200 closest-hit queries on the edges listed in the module's docstring; returns
    (rays, n_derive): the hits of the first n_derive rays get the tmin / tmax queries of `derived`."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, F32).reshape(-1, 3)
    t = np.asarray(idx, np.int32).reshape(-1, 3)
    tri = v[t]
    nt = len(t)
    lo, hi = tri.min(axis=(0, 1)), tri.max(axis=(0, 1))
    diag = F32(max(float(np.linalg.norm(hi.astype(np.float64) - lo)), 1e-2))
    mid = ((tri + np.roll(tri, -1, axis=1)) * F32(0.5)).astype(F32)  # edge midpoints
    cen = (tri.sum(axis=1) / F32(3)).astype(F32)

    def pick(a, n):
        a = a.reshape(-1, 3)
        return a[rng.integers(0, len(a), n)]

    O, D = [], []
    # A: axis directions (two components exactly +0 / -0) through vertices and edge midpoints; the
    # origin shares two coordinates with its target
    tg = np.concatenate([pick(tri, 96), pick(mid, 96)])
    ax = np.arange(len(tg)) % 3
    sg = np.where((np.arange(len(tg)) // 3) % 2 == 0, F32(1), F32(-1))
    d = np.where((np.arange(len(tg)) // 6 % 2 == 0)[:, None], F32(0.0), F32(-0.0)) * np.ones((len(tg), 3), F32)
    d[np.arange(len(tg)), ax] = sg
    o = tg.copy()
    o[np.arange(len(tg)), ax] = tg[np.arange(len(tg)), ax] - sg * (F32(0.37) * diag + F32(0.5))
    O.append(o), D.append(d)
    # B: one component exactly zero, unit length, toward vertices, midpoints and centroids
    tg = np.concatenate([pick(tri, 48), pick(mid, 40), pick(cen, 40)])
    ax = np.arange(len(tg)) % 3
    ang = rng.uniform(0, 2 * np.pi, len(tg))
    d = np.zeros((len(tg), 3), F32)
    d[np.arange(len(tg)), (ax + 1) % 3] = np.cos(ang)
    d[np.arange(len(tg)), (ax + 2) % 3] = np.sin(ang)
    d = _unit32(d)
    d[np.arange(len(tg)), ax] = np.where(np.arange(len(tg)) % 2 == 0, F32(0.0), F32(-0.0))
    O.append((tg - d * (F32(0.6) * diag + F32(0.3))).astype(F32)), D.append(d)
    # C: origins exactly on a box plane of the tree; toward a triangle, or along an axis in the plane
    if planes:
        sel = [planes[i] for i in rng.integers(0, len(planes), 96)]
        o = (lo + (hi - lo) * rng.uniform(-0.2, 1.2, (96, 3))).astype(F32)
        tg = pick(cen, 96)
        d = np.zeros((96, 3), F32)
        for i, (a, x) in enumerate(sel):
            o[i, a] = x
            if i % 2:
                b = (a + 1 + (i // 2) % 2) % 3
                d[i, b] = F32(1) if tg[i, b] >= o[i, b] else F32(-1)
            else:
                d[i] = tg[i] - o[i]
                if not d[i].any():
                    d[i, a] = 1
        O.append(o), D.append(_unit32(d))
    # D: rays lying in a triangle's plane
    k = rng.integers(0, nt, 96)
    e1, e2 = tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0]
    d = e1 + F32(0.2) * e2
    ok = (d * d).sum(axis=1) > 0
    O.append((tri[k, 0] - F32(0.7) * e1 + F32(0.3) * e2)[ok].astype(F32)), D.append(_unit32(d[ok]))
    # E: general directions aimed inside triangles
    k = rng.integers(0, nt, 512)
    ab = rng.uniform(0.1, 0.45, (512, 2)).astype(F32)
    tg = tri[k, 0] + ab[:, :1] * (tri[k, 1] - tri[k, 0]) + ab[:, 1:] * (tri[k, 2] - tri[k, 0])
    dr = rng.normal(size=(512, 3))
    dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    o = (tg + dr * (rng.uniform(0.3, 1.2, (512, 1)) * float(diag))).astype(F32)
    d = _unit32(tg - o)
    O.append(o), D.append(d)
    n_derive = sum(len(x) for x in O)
    # F: non-unit directions (the documented linear fallback when triangles were culled)
    O.append(o[:128]), D.append(np.concatenate([d[:64] * F32(1e-3), d[64:128] * F32(50.0)]).astype(F32))
    # G: empty intervals: tmax = 0, tmax < tmin
    O.append(o[128:192]), D.append(d[128:192])
    rays = np.zeros(sum(len(x) for x in O), ray_dtype)
    rays["o"], rays["d"] = np.concatenate(O), np.concatenate(D)
    rays["tmin"], rays["tmax"] = F32(1e-4), F32(np.inf)
    rays["tmax"][-64:] = F32(0.0)
    rays["tmin"][-32:] = F32(1.0)
    rays["tmax"][-32:] = F32(0.5)
    rays["propagation"] = 1.0
    return rays, n_derive


def derived(rays, hit_idx, hit_t, limit=480):
    """For (at most `limit`, evenly taken) hits: the same ray with tmax on the hit's t and on its two
    float neighbours, and with tmin likewise."""
    h = np.flatnonzero(hit_idx >= 0)
    if len(h) > limit:
        h = h[np.linspace(0, len(h) - 1, limit).astype(np.int64)]
    t = hit_t[h].astype(F32)
    near = [t, np.nextafter(t, F32(-np.inf)), np.nextafter(t, F32(np.inf))]
    out = []
    for field in ("tmax", "tmin"):
        for x in near:
            r = rays[h].copy()
            r[field] = x
            out.append(r)
    return np.concatenate(out) if len(h) else rays[:0].copy()


def queries(orc, verts, idx, tree, ray_dtype):
    """The whole query set of a mesh (about 4096 rays: `base_rays` with the planes of `tree`, then
    `derived` from the oracle's hits) and the oracle's linear-loop answers (closest index, closest t,
    occlusion flag).  Every query is asked both as a closest-hit and as an any-hit query."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    t = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    rays, n_derive = base_rays(v, t, tree_planes(tree), ray_dtype)
    hi, ht = orc.closest_hits(rays[:n_derive], v, t)
    rays = np.concatenate([rays, derived(rays[:n_derive], hi, ht)])
    ci, ct = orc.closest_hits(rays, v, t)
    return rays, (ci, ct, orc.any_hits(rays, v, t))
