"""Verifier of the built 4-wide trees (numpy: float64, exact comparisons, integers).

`check_tree` takes a mesh and the trees as the kernels read them — `RayTracer.meshTree()` on the
GPU, or tests/cpp/host_tree_dump (`read_dump`) for the host builder without one — and checks
every link, record, box, compressed plane and normal box against the rules of rt_bvh.cpp,
rt_build_gpu.hip and rt_quant.h, restated here from their comments.  A violation raises
`TreeError` naming the node, the child and the axis.  `live_stack` is a plain model of the
traversal's stack use, to prove that a ray set reaches the spill tail (rt_traverse.h Stack).

A float32 is a float64 exactly, and a decoded plane `origin + q * 2^e` is the exact sum of two
float64 values: `_two_sum` keeps its rounding error, so containment is decided exactly.
"""
from __future__ import annotations

import numpy as np

RT_STACK_DEPTH = 20  # rt_internal.h
RT_EMPTY_CHILD = 0x7FFFFFFF
RT_LEAF_MAX = 8
QEXP_MIN, QEXP_MAX = -24, 7  # rt_quant.h
DUMP_MAGIC = 0x44545452
U = 2.0 ** -24  # float32 unit roundoff
F32 = np.float32


class TreeError(AssertionError):
    pass


# ---- input ---------------------------------------------------------------------------------------
def read_dump(path) -> dict:
    """The file tests/cpp/host_tree_dump writes: the arrays of `meshTree()`, plus `nodes4_shadow`
    (the shadow tree's full-precision nodes) and `reported` = per tree root the builder's
    n_hit, depth4, stack4."""
    raw = np.fromfile(path, np.uint32)
    h = raw[:16]
    assert h[0] == DUMP_MAGIC, "not a host_tree_dump file"
    n_tris, n4, ns, sroot, nrec, comp = (int(x) for x in h[1:7])
    pos = 16
    out = dict(n_tris=n_tris, n_nodes4=n4, n_nodes4_shadow=ns, shadow_root=sroot, n_records=nrec, compressed=comp)

    def take(n, dtype, cols):
        nonlocal pos
        a = raw[pos:pos + n * cols].view(dtype).reshape(n, cols).copy()
        pos += n * cols
        return a

    out["nodes4"] = take(n4, np.float32, 32)
    out["nodes4q"] = take(n4 + ns, np.uint32, 16) if comp else None
    out["tris"] = take(nrec, np.float32, 12)
    out["nodes4_shadow"] = take(ns, np.float32, 32) if ns else None
    assert pos == raw.size, "host_tree_dump file length"
    out["reported"] = {0: dict(n_hit=int(h[7]), depth4=int(h[8]), stack4=int(h[9]))}
    if ns:
        out["reported"][sroot] = dict(n_hit=int(h[10]), depth4=int(h[11]), stack4=int(h[12]))
    return out


# ---- exact helpers -------------------------------------------------------------------------------
def _two_sum(a, b):
    """s, e with s + e == a + b exactly (Knuth), s = fl(a + b)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _le(s, e, x):
    """s + e <= x exactly, for the pair of _two_sum."""
    return (s < x) | ((s == x) & (e <= 0))


def _lt(s, e, x):
    return (s < x) | ((s == x) & (e < 0))


def _ge(s, e, x):
    return (s > x) | ((s == x) & (e >= 0))


def _gt(s, e, x):
    return (s > x) | ((s == x) & (e > 0))


AXES = "xyz"


def _fail(tag, nodes, mask, what):
    """Raise for the first True of mask ([m], [m, 4], [m, 3] (axis) or [m, 4, 3]); nodes: [m] indices."""
    mask = np.asarray(mask)
    if not mask.any():
        return
    at = np.argwhere(mask)[0]
    where = f"node {int(nodes[at[0]])}"
    if mask.ndim == 3:
        where += f" child {int(at[1])} axis {AXES[at[2]]}"
    elif mask.ndim == 2 and mask.shape[1] == 4:
        where += f" child {int(at[1])}"
    elif mask.ndim == 2:
        where += f" axis {AXES[at[1]]}"
    raise TreeError(f"{tag}: {where}: {what} ({int(mask.sum())} in all)")


# ---- the mesh ------------------------------------------------------------------------------------
def triangle_terms(verts, idx) -> dict:
    """Per input triangle: the float32 record fields and the float64 terms the builders use."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    t = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    p = v[t]  # [n, 3 vertices, 3]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]  # float32 subtraction (get_triangle)
    lo, hi = p.min(axis=1).astype(np.float64), p.max(axis=1).astype(np.float64)
    a, b = e2.astype(np.float64), e1.astype(np.float64)
    # N = e2 x e1, each component one rounded difference of two exact products (rt_bvh.cpp)
    nrm = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                    a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    l1l2 = np.abs(b).sum(axis=1) * np.abs(a).sum(axis=1)
    # the documented pad of a triangle's box: ext / 512 + 1e-6 (1 + maxabs)
    ext = (hi - lo).max(axis=1)
    maxabs = np.abs(p).max(axis=(1, 2)).astype(np.float64)
    pad = ext / 512.0 + 1e-6 * (1.0 + maxabs)
    # float rounding of that expression as the builders evaluate it in float32: the pad itself
    # (two products, two sums: below 4u relative) and the final lo - pad / hi + pad (half an ulp
    # of the result: at most u (|coordinate| + pad))
    slack = 4.0 * U * pad[:, None] + U * (np.maximum(np.abs(lo), np.abs(hi)) + pad[:, None])
    return dict(v0=p[:, 0], e1=e1, e2=e2, lo=lo, hi=hi, nrm=nrm, l1l2=l1l2, plo=lo - pad[:, None] + slack,
                phi=hi + pad[:, None] - slack)


def never_hit_rule(terms) -> np.ndarray:
    """The value the host builder's never_hit compares (rt_bvh.cpp): a triangle is left out of the
    tree when 1.001 (|e2 x e1| + 16 u |e1|_1 |e2|_1) < 0.999 * 1e-4f.  Returns that left side over
    the right side, in float64 as the builder evaluates it."""
    cr = np.sqrt((terms["nrm"] ** 2).sum(axis=1))
    return 1.001 * (cr + 16.0 * U * terms["l1l2"]) / (0.999 * float(F32(1e-4)))


# binary64 evaluates the rule on both sides with a handful of roundings (below 1e-14 relative);
# a triangle whose ratio is within RULE_MARGIN of 1 may fall either way
RULE_MARGIN = 1e-9
# The rule's own slack: 16 u |e1|_1 |e2|_1 >= 0, so a triangle with |e1 x e2| >= 0.999 / 1.001 x 1e-4
# is kept whatever its edge lengths: "clearly above the bound" is that factor, 0.998002
CLEARLY_ABOVE = 0.999 / 1.001


# ---- the walk ------------------------------------------------------------------------------------
def _links(tree, root):
    n4, ns = int(tree["n_nodes4"]), int(tree["n_nodes4_shadow"])
    q = tree["nodes4q"]
    shadow = root != 0
    if shadow:
        assert q is not None and ns > 0 and root == int(tree["shadow_root"]) == n4, "shadow root"
        return q[:, 12:16].view(np.int32), n4, n4 + ns
    if q is not None:
        return q[:, 12:16].view(np.int32), 0, n4
    return tree["nodes4"][:, 24:28].view(np.int32), 0, n4


def walk(tree, root, n_tris, tag="tree"):
    """Structure checks; returns the breadth-first order with per-node depth (root 1), stack entries
    live after the node's pushes (`stack += children - 1` per level, all ancestors live), and the
    leaf / inner children as arrays."""
    L, n0, n1 = _links(tree, root)
    r0 = n_tris if root != 0 else 0
    links = L.tolist()
    seen = np.zeros(n1 - n0, bool)
    order, depth, stack = [root], {root: 1}, {}
    stack_in = {root: 0}
    leaves, inners = [], []  # (node, child, first, count), (node, child, target)
    if not (n0 <= root < n1):
        raise TreeError(f"{tag}: root {root} outside the node range [{n0}, {n1})")
    seen[root - n0] = True
    h = 0
    while h < len(order):
        n = order[h]
        h += 1
        kids = links[n]
        nk, empty_seen = 0, False
        inner_base, n_inner, tri_next = None, 0, None
        for k, c in enumerate(kids):
            if c == RT_EMPTY_CHILD:
                empty_seen = True
                continue
            if empty_seen:
                raise TreeError(f"{tag}: node {n} child {k}: a used slot after an empty one (empty slots trail)")
            nk += 1
            if c >= 0:
                if not (n0 <= c < n1):
                    raise TreeError(f"{tag}: node {n} child {k}: inner link {c} outside [{n0}, {n1})")
                if seen[c - n0]:
                    raise TreeError(f"{tag}: node {n} child {k}: node {c} is reached twice")
                if inner_base is None:
                    inner_base = c
                elif c != inner_base + n_inner:
                    raise TreeError(f"{tag}: node {n} child {k}: inner children not consecutive "
                                    f"({c} after {inner_base + n_inner - 1})")
                n_inner += 1
                seen[c - n0] = True
                order.append(c)
                depth[c] = depth[n] + 1
                inners.append((n, k, c))
            else:
                enc = ~c
                first, count = enc >> 3, (enc & 7) + 1
                if not (1 <= count <= RT_LEAF_MAX):
                    raise TreeError(f"{tag}: node {n} child {k}: leaf of {count} triangles")
                if first < r0 or first + count > r0 + n_tris:
                    raise TreeError(f"{tag}: node {n} child {k}: leaf slots [{first}, {first + count}) outside "
                                    f"[{r0}, {r0 + n_tris})")
                if tri_next is not None and first != tri_next:
                    raise TreeError(f"{tag}: node {n} child {k}: leaf slots not consecutive in child order "
                                    f"({first}, expected {tri_next})")
                tri_next = first + count
                leaves.append((n, k, first, count))
        if nk == 0:
            raise TreeError(f"{tag}: node {n}: no children")
        stack[n] = stack_in[n] + nk - 1
        for c in kids:
            if c != RT_EMPTY_CHILD and c >= 0:
                stack_in[c] = stack[n]
    if not seen.all():
        raise TreeError(f"{tag}: node {n0 + int(np.flatnonzero(~seen)[0])} is not reached from root {root} "
                        f"({int((~seen).sum())} in all)")
    leaves = np.array(leaves, np.int64).reshape(-1, 4)
    diff = np.zeros(n_tris + 1, np.int64)
    np.add.at(diff, leaves[:, 2] - r0, 1)
    np.add.at(diff, leaves[:, 2] + leaves[:, 3] - r0, -1)
    cover = np.cumsum(diff)[:n_tris]
    if (cover > 1).any():
        s = r0 + int(np.flatnonzero(cover > 1)[0])
        hit = leaves[(leaves[:, 2] <= s) & (s < leaves[:, 2] + leaves[:, 3])]
        raise TreeError(f"{tag}: node {int(hit[-1, 0])} child {int(hit[-1, 1])}: record {s} is reached from two leaves")
    n_rec = int(cover.sum())
    if not cover[:n_rec].all():
        raise TreeError(f"{tag}: record {r0 + int(np.flatnonzero(cover == 0)[0])} is skipped: the leaves do not "
                        f"cover the slots [{r0}, {r0 + n_rec})")
    order = np.array(order, np.int64)
    return dict(order=order, depth=np.array([depth[n] for n in order.tolist()], np.int64),
                stack=np.array([stack[n] for n in order.tolist()], np.int64), leaves=leaves,
                inners=np.array(inners, np.int64).reshape(-1, 3), n0=n0, n1=n1, r0=r0, n_rec=n_rec, links=L)


# ---- the checks ----------------------------------------------------------------------------------
def check_tree(verts, idx, tree, root, *, builder, reported=None, det_cull=True) -> dict:
    """Every invariant of one tree of `tree` (the closest-hit tree: root 0; the shadow tree: root
    tree["shadow_root"]).  builder: "host" or "gpu".  reported: the builder's own n_hit (n_tris_tree),
    depth4 and stack4, compared with the values recomputed here (keys that are absent are not
    compared).  Returns the recomputed figures."""
    assert builder in ("host", "gpu")
    tag = f"{builder} tree, root {root}"
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    t = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    n_tris = len(t)
    n4, ns = int(tree["n_nodes4"]), int(tree["n_nodes4_shadow"])
    q, recs = tree["nodes4q"], tree["tris"]
    if int(tree["n_records"]) != n_tris * (2 if ns else 1) or len(recs) != int(tree["n_records"]):
        raise TreeError(f"{tag}: {tree['n_records']} records for {n_tris} triangles and {ns} shadow nodes")
    if bool(tree["compressed"]) != (q is not None) or (q is not None and len(q) != n4 + ns):
        raise TreeError(f"{tag}: compressed flag / array mismatch")
    if builder == "gpu" and ns:
        raise TreeError(f"{tag}: the GPU builder makes one tree")
    w = walk(tree, root, n_tris, tag)
    n0, r0, n_rec, L = w["n0"], w["r0"], w["n_rec"], w["links"]
    order = w["order"]
    m = len(order)
    loc = order - n0  # local node index
    full = tree["nodes4"] if root == 0 else tree.get("nodes4_shadow")
    if root == 0 and q is not None:  # the two copies of the closest tree's links agree
        _fail(tag, np.arange(n4), tree["nodes4"][:, 24:28].view(np.int32) != L[:n4],
              "full-precision link differs from the compressed node's")
    if root != 0 and full is not None:
        _fail(tag, n0 + np.arange(ns), full[:, 24:28].view(np.int32) != L[n0:], "full-precision link differs")

    # ---- records
    T = triangle_terms(v, t)
    rr = recs[r0:r0 + n_tris]
    orig = rr[:, 3].view(np.int32).astype(np.int64)
    if not np.array_equal(np.sort(orig), np.arange(n_tris)):
        raise TreeError(f"{tag}: the records' original indices are not a permutation of the {n_tris} triangles")
    for name, cols in (("v0", slice(0, 3)), ("e1", slice(4, 7)), ("e2", slice(8, 11))):
        bad = rr[:, cols].view(np.uint32) != np.ascontiguousarray(T[name][orig]).view(np.uint32)
        if bad.any():
            s = int(np.argwhere(bad)[0][0])
            raise TreeError(f"{tag}: record {r0 + s} (triangle {orig[s]}): {name} is not the float32 "
                            f"{'vertex' if name == 'v0' else 'subtraction'} of the input")
    bad = (rr[:, 7].view(np.uint32) != 0) | (rr[:, 11].view(np.uint32) != 0)
    if bad.any():  # rt_traverse.h reads r1.w of a tree leaf's record as 0 (the lists' early end)
        raise TreeError(f"{tag}: record {r0 + int(np.flatnonzero(bad)[0])}: the fourth component of e1 / e2 is not 0")
    kept = orig[:n_rec]

    # ---- culling
    if builder == "gpu":
        if n_rec != n_tris:
            raise TreeError(f"{tag}: the GPU builder keeps every triangle, {n_rec} of {n_tris} are in the tree")
    else:
        ratio = never_hit_rule(T)
        in_tree = np.zeros(n_tris, bool)
        in_tree[kept] = True
        must_keep = ratio >= 1.0 + RULE_MARGIN
        must_drop = ratio < 1.0 - RULE_MARGIN
        if not must_keep.any() and not (~must_drop).any():  # nothing hittable: triangle 0 alone stays
            must_keep[0], must_drop[0] = True, False
        if (must_keep & ~in_tree).any():
            k = int(np.flatnonzero(must_keep & ~in_tree)[0])
            raise TreeError(f"{tag}: triangle {k} is missing from the tree, never_hit ratio {ratio[k]:.6f} >= 1")
        if (must_drop & in_tree).any():
            k = int(np.flatnonzero(must_drop & in_tree)[0])
            raise TreeError(f"{tag}: triangle {k} is in the tree, never_hit ratio {ratio[k]:.6f} < 1")
        cr = np.sqrt((T["nrm"] ** 2).sum(axis=1))
        clearly = cr >= CLEARLY_ABOVE * float(F32(1e-4))
        if (clearly & ~in_tree).any():
            k = int(np.flatnonzero(clearly & ~in_tree)[0])
            raise TreeError(f"{tag}: triangle {k} with |e1 x e2| = {cr[k]:.4e} is missing from the tree")

    # ---- per child: bounds of everything below it (min part, max part), bottom-up by level
    rec_min = np.concatenate([T["lo"], T["plo"], T["nrm"]], axis=1)[kept]  # [n_rec, 9]
    rec_max = np.concatenate([T["hi"], T["phi"], T["nrm"], T["l1l2"][:, None]], axis=1)[kept]  # [n_rec, 10]
    lv = w["leaves"]
    srt = np.argsort(lv[:, 2])
    starts = lv[srt, 2] - r0
    cmin = np.full((w["n1"] - n0, 4, 9), np.inf)
    cmax = np.full((cmin.shape[0], 4, 10), -np.inf)
    cmin[lv[srt, 0] - n0, lv[srt, 1]] = np.minimum.reduceat(rec_min, starts, axis=0)
    cmax[lv[srt, 0] - n0, lv[srt, 1]] = np.maximum.reduceat(rec_max, starts, axis=0)
    inn = w["inners"]
    if len(inn):  # (the walk's order need not be sorted by index: map through it)
        pos = np.empty(cmin.shape[0], np.int64)
        pos[loc] = np.arange(m)
        child_depth = w["depth"][pos[inn[:, 2] - n0]]
        for d in range(int(w["depth"].max()), 1, -1):
            sel = inn[child_depth == d]
            cmin[sel[:, 0] - n0, sel[:, 1]] = cmin[sel[:, 2] - n0].min(axis=1)
            cmax[sel[:, 0] - n0, sel[:, 1]] = cmax[sel[:, 2] - n0].max(axis=1)
    cmin, cmax = cmin[loc], cmax[loc]  # in walk order: row i is node order[i]
    links = L[order]
    used = links != RT_EMPTY_CHILD
    u3 = used[:, :, None]
    vlo, vhi = cmin[:, :, 0:3], cmax[:, :, 0:3]

    # ---- full-precision boxes
    if full is not None:
        f = full[loc].astype(np.float64)
        flo = np.stack([f[:, 0:4], f[:, 8:12], f[:, 16:20]], axis=2)  # [m, 4, 3]
        fhi = np.stack([f[:, 4:8], f[:, 12:16], f[:, 20:24]], axis=2)
        _fail(tag, order, u3 & ((flo > vlo) | (fhi < vhi)), "the full-precision box does not contain a vertex below it")
        _fail(tag, order, u3 & ((flo > cmin[:, :, 3:6]) | (fhi < cmax[:, :, 3:6])),
              "the full-precision box pads a triangle below it by less than ext/512 + 1e-6 (1 + maxabs)")

    # ---- compressed boxes
    if q is not None:
        d = q[order]
        origin = d[:, 0:3].view(F32).astype(np.float64)  # [m, 3]
        field = np.stack([(d[:, 3] >> (5 * a)) & 31 for a in range(3)], axis=1).astype(np.int64)
        e = field - 24
        _fail(tag, order, (e < QEXP_MIN) | (e > QEXP_MAX), "grid exponent outside [-24, 7]")
        _fail(tag, order, (d[:, 3] >> 15) & 1 != 0, "bit 15 of d[3] is set")
        step = np.ldexp(1.0, e)  # [m, 3]
        sh = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
        ql = ((np.stack([d[:, 4], d[:, 6], d[:, 8]], axis=1)[:, None, :] >> sh) & 255).astype(np.float64)  # [m, 4, 3]
        qh = ((np.stack([d[:, 5], d[:, 7], d[:, 9]], axis=1)[:, None, :] >> sh) & 255).astype(np.float64)
        _fail(tag, order, ~u3 & ((ql != 255) | (qh != 0)), "an unused slot is not the inverted box lo 255, hi 0")
        meta = ((d[:, 3:4] >> (16 + 4 * np.arange(4, dtype=np.uint32))[None, :]) & 15).astype(np.int64)  # [m, 4]
        is_inner = used & (links >= 0)
        is_leaf = used & (links < 0)
        rank = np.cumsum(is_inner, axis=1) - 1
        want = np.where(is_leaf, 8 | ((~links) & 7), np.where(is_inner, rank, 0))
        _fail(tag, order, meta != want, "the d[3] meta nibble disagrees with the explicit link")
        o3, s3 = origin[:, None, :], step[:, None, :]
        dl = _two_sum(o3, ql * s3)
        dh = _two_sum(o3, qh * s3)
        _fail(tag, order, u3 & ~(_le(*dl, vlo) & _ge(*dh, vhi)), "the decoded box does not contain a vertex below it")
        if full is not None:
            _fail(tag, order, u3 & ~(_le(*dl, flo) & _ge(*dh, fhi)),
                  "the decoded box does not contain the full-precision child box")
            # tightness (rt_quant.h): origin = the minimum corner of the children's boxes; the exponent
            # the smallest in range for which every child fits in 0..255; planes rounded outward
            omin = np.where(u3, flo, np.inf).min(axis=1)
            _fail(tag, order, origin != omin, "the origin is not the minimum corner of the children's boxes")
            _fail(tag, order, u3 & ~_gt(*_two_sum(o3, (ql + 1) * s3), flo),
                  "a lower plane is a whole grid step or more below its box")
            _fail(tag, order, u3 & ~_lt(*_two_sum(o3, (qh - 1) * s3), fhi),
                  "an upper plane is a whole grid step or more above its box")
            fits_below = (~u3 | _ge(*_two_sum(o3, 255.0 * (s3 / 2)), fhi)).all(axis=1)  # at exponent e - 1
            _fail(tag, order, (e > QEXP_MIN) & fits_below, "the grid exponent is larger than the children need")

        # ---- normal boxes
        E = (d[:, 10] >> 24).astype(np.int64)
        cull = E != 255
        nlo = np.stack([(d[:, 10] >> (8 * a)) & 255 for a in range(3)], axis=1).astype(np.float64) - 128.0
        nhi = np.stack([(d[:, 11] >> (8 * a)) & 255 for a in range(3)], axis=1).astype(np.float64) - 128.0
        _fail(tag, order, ~cull & ((d[:, 10] != 255 << 24) | (d[:, 11] != 0xFFFFFF)), "the no-cull normal box is not the documented word pair")
        below_lo = np.where(u3, cmin[:, :, 6:9], np.inf).min(axis=1)  # [m, 3]: e2 x e1 below the node
        below_hi = np.where(u3, cmax[:, :, 6:9], -np.inf).max(axis=1)
        err = np.where(used, cmax[:, :, 9], -np.inf).max(axis=1)
        allowed = 8.0 * U * err <= 5e-7
        _fail(tag, order, cull & ~allowed, "a cullable node whose det error bound 8u max |e1|_1 |e2|_1 exceeds 5e-7")
        nstep = np.ldexp(1.0, np.where(cull, E - 128, 0))[:, None]
        c3 = cull[:, None]
        _fail(tag, order, c3 & ((nlo * nstep > below_lo) | (nhi * nstep < below_hi)),
              "the normal box does not contain e2 x e1 of a triangle below it")
        if det_cull:
            _fail(tag, order, ~cull & allowed, "a node within the error bound has no normal box")
            _fail(tag, order, c3 & ((nlo != np.floor(below_lo / nstep)) | (nhi != np.ceil(below_hi / nstep))),
                  "a normal-box plane is not the outward rounding of its bound")
            mx = np.maximum(np.abs(below_lo), np.abs(below_hi)).max(axis=1)
            ee = E - 128
            _fail(tag, order, cull & (ee > -120) & (mx <= 127.0 * np.ldexp(1.0, ee - 1)),
                  "the normal box's exponent is larger than its bounds need")
            _fail(tag, order, cull & (ee < -120), "the normal box's exponent is below -120")

    # ---- reported numbers
    got = dict(n_hit=n_rec, depth4=int(w["depth"].max()), stack4=int(w["stack"].max()), n_nodes=m)
    for k, val in (reported or {}).items():
        if k in got and int(val) != got[k]:
            at = int(order[np.argmax(w["stack"])]) if k == "stack4" else int(order[np.argmax(w["depth"])])
            raise TreeError(f"{tag}: node {at}: the builder reports {k} {int(val)}, the links give {got[k]}")
    return got


def check_fallback(tree, tag="tree"):
    """The compressed nodes exist exactly when every node can be encoded (rt_quant.h: an axis needs
    no grid step beyond 2^7, i.e. the children span at most 255 * 128 on it)."""
    f = tree["nodes4"].astype(np.float64)
    used = tree["nodes4"][:, 24:28].view(np.int32) != RT_EMPTY_CHILD
    lo = np.stack([f[:, 0:4], f[:, 8:12], f[:, 16:20]], axis=2)
    hi = np.stack([f[:, 4:8], f[:, 12:16], f[:, 20:24]], axis=2)
    ext = np.where(used[:, :, None], hi, -np.inf).max(axis=1) - np.where(used[:, :, None], lo, np.inf).min(axis=1)
    limit = 255.0 * 2.0 ** QEXP_MAX
    n, a = np.unravel_index(np.argmax(ext), ext.shape)
    if tree["nodes4q"] is None and ext[n, a] <= limit:
        raise TreeError(f"{tag}: node {n} axis {AXES[a]}: the widest node spans {ext[n, a]:.6g} <= {limit:g}, every "
                        "node can be encoded, yet the builder dropped the compressed nodes")
    if tree["nodes4q"] is not None and ext[n, a] > limit:
        raise TreeError(f"{tag}: node {n} axis {AXES[a]}: spans {ext[n, a]:.6g} > {limit:g} and cannot be encoded, "
                        "yet there are compressed nodes")


# ---- the stack model -----------------------------------------------------------------------------
def decoded_boxes(tree):
    """lo, hi [n, 4, 3] float64 of every compressed node's children (unused slots inverted)."""
    q = tree["nodes4q"]
    origin = q[:, 0:3].view(F32).astype(np.float64)[:, None, :]
    step = np.ldexp(1.0, np.stack([(q[:, 3] >> (5 * a)) & 31 for a in range(3)], axis=1).astype(np.int64) - 24)[:, None, :]
    sh = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    ql = ((np.stack([q[:, 4], q[:, 6], q[:, 8]], axis=1)[:, None, :] >> sh) & 255).astype(np.float64)
    qh = ((np.stack([q[:, 5], q[:, 7], q[:, 9]], axis=1)[:, None, :] >> sh) & 255).astype(np.float64)
    return origin + ql * step, origin + qh * step


def live_stack(tree, root, rays) -> np.ndarray:
    """Per ray the largest number of live stack entries of a nearest-first depth-first walk of the
    compressed tree: float64 slab test on the decoded boxes from t = -1e-3 (the traversal's lower
    clamp) with no upper bound and no determinant cull; a node whose k children are met pushes
    k - 1 and descends into the nearest; a leaf pops.  Not bit parity with the kernel: an
    upper-side model, used only to prove that a ray set reaches the spill tail."""
    lo, hi = decoded_boxes(tree)
    L = tree["nodes4q"][:, 12:16].view(np.int32)
    links = L.tolist()
    out = np.zeros(len(rays), np.int64)
    for i, r in enumerate(rays):
        o = np.asarray(r["o"], np.float64)
        with np.errstate(divide="ignore"):
            inv = 1.0 / np.asarray(r["d"], np.float64)
        with np.errstate(invalid="ignore"):  # every node's slab test at once; the walk below only follows it
            ta, tb = (lo - o) * inv, (hi - o) * inv
        near, far = np.fmin(ta, tb), np.fmax(ta, tb)  # NaN (0 x inf): that slab does not bound
        tn = np.maximum(np.where(np.isnan(near), -np.inf, near).max(axis=2), -1e-3)
        tf = np.where(np.isnan(far), np.inf, far).min(axis=2)
        hit = (tn <= tf) & (L != RT_EMPTY_CHILD)
        nearest_first = np.argsort(np.where(hit, tn, np.inf), axis=1, kind="stable").tolist()
        nhit = hit.sum(axis=1).tolist()
        best, node, stack = 0, root, []
        while True:
            if node >= 0 and nhit[node]:
                kids, ordr = links[node], nearest_first[node]
                for j in range(nhit[node] - 1, 0, -1):
                    stack.append(kids[ordr[j]])
                best = max(best, len(stack))
                node = kids[ordr[0]]
                continue
            if not stack:
                break
            node = stack.pop()
        out[i] = best
    return out
