"""The refit of rt_update_mesh (csrc/rt_refit.hip) restated in numpy: from a tree's links, its
record order and new vertices, the float32 padded boxes of the triangles, the full-precision
child boxes of either tree level by level, and the records.  float32 min / max and the single
float32 operations of the pad are exact restatements, so the results compare bit for bit.

Also the vertex deformations the refit tests share (binary64, rounded to float32)."""
from __future__ import annotations

import numpy as np

F32 = np.float32
RT_EMPTY_CHILD = 0x7FFFFFFF


# ---- deformations --------------------------------------------------------------------------------
def _frame(verts):
    v = np.asarray(verts, F32).reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    return v, 0.5 * (lo + hi), float((hi - lo).max())


def rigid(verts):
    """20 degrees about y through the box centre, then a translation by (0.3, -0.2, 0.1)."""
    v, c, _ = _frame(verts)
    a = np.deg2rad(20.0)
    d = v - c
    out = np.stack([np.cos(a) * d[:, 0] + np.sin(a) * d[:, 2], d[:, 1], -np.sin(a) * d[:, 0] + np.cos(a) * d[:, 2]], axis=1)
    return np.ascontiguousarray((out + c + np.array([0.3, -0.2, 0.1])).astype(F32))


def wobble(verts):
    """v + 0.03 ext sin(3 pi / ext (v.yzx - c.yzx) + (0.3, 1.1, 2.0))."""
    v, c, ext = _frame(verts)
    ph = 3.0 * np.pi / ext * (v[:, [1, 2, 0]] - c[[1, 2, 0]]) + np.array([0.3, 1.1, 2.0])
    return np.ascontiguousarray((v + 0.03 * ext * np.sin(ph)).astype(F32))


def shrink(verts):
    """c + 0.9 (v - c)."""
    v, c, _ = _frame(verts)
    return np.ascontiguousarray((c + 0.9 * (v - c)).astype(F32))


def scale(verts, s):
    v, c, _ = _frame(verts)
    return np.ascontiguousarray((c + s * (v - c)).astype(F32))


DEFORM = {"rigid": rigid, "wobble": wobble, "shrink": shrink}


# ---- the refit -----------------------------------------------------------------------------------
def padded_boxes(verts, idx):
    """Per input triangle the float32 box padded by ext / 512 + 1e-6 (1 + maxabs), every operation
    in float32 as rt_bvh.cpp and k_prep evaluate it: lo, hi [n, 3] float32."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    p = v[np.ascontiguousarray(idx, np.int32).reshape(-1, 3)]  # [n, 3 vertices, 3]
    lo, hi = p.min(axis=1), p.max(axis=1)
    maxabs = np.abs(p).max(axis=(1, 2))
    ext = (hi - lo).max(axis=1)
    pad = (ext * F32(1.0 / 512.0) + F32(1e-6) * (F32(1.0) + maxabs)).astype(F32)
    return (lo - pad[:, None]).astype(F32), (hi + pad[:, None]).astype(F32)


def records(verts, idx, orig):
    """The 12-float records of the triangles `orig` (a slot order): (v0, orig), (v1 - v0, 0), (v2 - v0, 0)."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    orig = np.asarray(orig, np.int64)
    p = v[np.ascontiguousarray(idx, np.int32).reshape(-1, 3)[orig]]
    out = np.zeros((len(orig), 12), F32)
    out[:, 0:3] = p[:, 0]
    out[:, 3] = orig.astype(np.int32).view(F32)
    out[:, 4:7] = p[:, 1] - p[:, 0]
    out[:, 8:11] = p[:, 2] - p[:, 0]
    return out


def levels(links, n0):
    """Node index ranges [lo, hi) per depth of the breadth-first numbered tree whose node n0 + i has
    the links links[i]; asserts that every level is the index range after the one above it."""
    out, lo, hi = [], n0, n0 + 1
    while True:
        out.append((lo, hi))
        sub = links[lo - n0:hi - n0]
        inner = sub[(sub >= 0) & (sub != RT_EMPTY_CHILD)]
        if not len(inner):
            break
        assert inner.min() == hi and len(np.unique(inner)) == len(inner) == inner.max() - hi + 1, "not breadth-first"
        lo, hi = hi, int(inner.max()) + 1
    assert hi - n0 == len(links), "levels do not cover the tree"
    return out


def full_nodes(links, n0, slot_lo, slot_hi):
    """The full-precision 4-wide nodes (rt_internal.h: lo.x[4], hi.x[4], lo.y[4], hi.y[4], lo.z[4],
    hi.z[4], links[4], 0[4]) of the tree with node n0 + i = links[i] ([m, 4] int32: inner links are
    node indices in the same numbering, leaf links ~(first << 3 | count - 1) over the slots of
    slot_lo / slot_hi, [n_slots, 3] float32 padded boxes).  A leaf child's box is the union of its
    slots' boxes, an inner child's the union of the child node's used boxes; unused slots hold 0."""
    links = np.ascontiguousarray(links, np.int32)
    m = len(links)
    lo = np.zeros((m, 4, 3), F32)
    hi = np.zeros((m, 4, 3), F32)
    nlo = np.full((m, 3), np.inf, F32)  # union of the node's used child boxes
    nhi = np.full((m, 3), -np.inf, F32)
    for a, b in reversed(levels(links, n0)):
        L = links[a - n0:b - n0]
        for k in range(4):
            c = L[:, k]
            used = c != RT_EMPTY_CHILD
            leaf = used & (c < 0)
            inner = used & (c >= 0)
            blo = np.zeros((b - a, 3), F32)
            bhi = np.zeros((b - a, 3), F32)
            if leaf.any():
                enc = ~c[leaf]
                first, count = enc >> 3, (enc & 7) + 1
                l = np.full((len(enc), 3), np.inf, F32)
                h = np.full((len(enc), 3), -np.inf, F32)
                for j in range(8):
                    sel = count > j
                    l[sel] = np.minimum(l[sel], slot_lo[first[sel] + j])
                    h[sel] = np.maximum(h[sel], slot_hi[first[sel] + j])
                blo[leaf], bhi[leaf] = l, h
            if inner.any():
                blo[inner], bhi[inner] = nlo[c[inner] - n0], nhi[c[inner] - n0]
            lo[a - n0:b - n0, k], hi[a - n0:b - n0, k] = blo, bhi
        u = (L != RT_EMPTY_CHILD)[:, :, None]
        nlo[a - n0:b - n0] = np.where(u, lo[a - n0:b - n0], F32(np.inf)).min(axis=1)
        nhi[a - n0:b - n0] = np.where(u, hi[a - n0:b - n0], F32(-np.inf)).max(axis=1)
    out = np.zeros((m, 32), F32)
    for ax in range(3):
        out[:, 8 * ax:8 * ax + 4] = lo[:, :, ax]
        out[:, 8 * ax + 4:8 * ax + 8] = hi[:, :, ax]
    out[:, 24:28] = links.view(F32)
    return out


def refit(tree, verts, idx):
    """The refit of a read-back tree (meshTree() or tree_ref.read_dump) to `verts`: dict with `tris`
    (all record slots), `nodes4` (the closest-hit tree) and `nodes4_shadow` (None without one)."""
    n4, ns = int(tree["n_nodes4"]), int(tree["n_nodes4_shadow"])
    orig = tree["tris"][:, 3].view(np.int32).astype(np.int64)
    tlo, thi = padded_boxes(verts, idx)
    slot_lo, slot_hi = tlo[orig], thi[orig]
    q = tree["nodes4q"]
    la = q[:n4, 12:16].view(np.int32) if q is not None else tree["nodes4"][:, 24:28].view(np.int32)
    out = dict(tris=records(verts, idx, orig), nodes4=full_nodes(la, 0, slot_lo, slot_hi), nodes4_shadow=None)
    if ns:
        out["nodes4_shadow"] = full_nodes(q[n4:, 12:16].view(np.int32), n4, slot_lo, slot_hi)
    return out


def half_area_sum(nodes4):
    """Sum over the used children of dx dy + dy dz + dz dx, binary64 (rt_mesh_update_info.area_ratio)."""
    f = nodes4.astype(np.float64)
    used = nodes4[:, 24:28].view(np.int32) != RT_EMPTY_CHILD
    dx, dy, dz = f[:, 4:8] - f[:, 0:4], f[:, 12:16] - f[:, 8:12], f[:, 20:24] - f[:, 16:20]
    return float(((dx * dy + dy * dz + dz * dx) * used).sum())


def as_closest(tree, ref):
    """The shadow tree of `tree` presented as a closest-hit tree of its own (node and slot numbering
    from 0, no compressed nodes), with the refitted full-precision nodes and records of `ref`:
    tree_ref.check_tree(root 0) then checks its links, records and full-precision boxes."""
    n4, n = int(tree["n_nodes4"]), len(ref["tris"]) // 2
    f = ref["nodes4_shadow"].copy()
    c = f[:, 24:28].view(np.int32)
    inner = (c >= 0) & (c != RT_EMPTY_CHILD)
    leaf = c < 0
    enc = ~c
    c[...] = np.where(inner, c - n4, np.where(leaf, ~((((enc >> 3) - n) << 3) | (enc & 7)), c))
    return dict(n_nodes4=len(f), n_nodes4_shadow=0, shadow_root=0, n_records=n, compressed=0, nodes4=f, nodes4q=None,
                tris=ref["tris"][n:2 * n])


def closest_only(tree, ref):
    """Likewise the closest-hit tree alone, full-precision nodes only."""
    n = len(ref["tris"]) // (2 if int(tree["n_nodes4_shadow"]) else 1)
    return dict(n_nodes4=int(tree["n_nodes4"]), n_nodes4_shadow=0, shadow_root=0, n_records=n, compressed=0,
                nodes4=ref["nodes4"], nodes4q=None, tris=ref["tris"][:n])
