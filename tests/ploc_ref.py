"""A numpy restatement of the device builders of rt_build_gpu.hip: the prep and the sort (steps
1-2, in their float32 arithmetic), the radix tree (LBVH), the PLOC rounds, the collapse to the
4-wide tree, the tree's SAH cost and a canonical walk that compares two 4-wide trees.

Binary trees are dicts: `child` [m, 2] int (>= 0 an inner node, < 0 the leaf ~slot), `box`
[m, 6] float32, `size` [m], `root`, and the leaves' `lbox` [n, 6] = tbox[perm], `perm` [n].
4-wide trees are dicts with `nodes4` [m, 32] float32 in the device layout (rt_internal.h) and
`orig` [n]: the original triangle index of every record slot — `as_tree4` makes one of
RayTracer.meshTree().

The collapse on the device hands out node and slot numbers through atomics, so they differ from
run to run: `same_tree4` never compares numbers.  It walks both trees from the root and compares,
slot by slot, the kind, the bits of the child's box, a leaf's triangles in order, and recurses
into an inner child.
"""
from __future__ import annotations

from bisect import bisect_left

import numpy as np

F32 = np.float32
RT_EMPTY_CHILD = 0x7FFFFFFF
LEAF_MAX = 4  # kLeafMax
PLOC_R = 16  # kPlocR


def ceil_log2(n: int) -> int:
    return int(n - 1).bit_length() if n > 1 else 0


def round_cap(n: int) -> int:
    """The first halving round; at most round_cap(n) + ceil_log2(n) rounds in all."""
    return 6 * ceil_log2(n) + 16


# ---- steps 1-2 -----------------------------------------------------------------------------------
def _spread21(v):
    v = v & np.uint64(0x1FFFFF)
    for sh, m in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3),
                  (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(sh))) & np.uint64(m)
    return v


def prep(verts, idx) -> dict:
    """k_prep, k_morton and the stable sort: `tbox` [n, 6] per input triangle, the sorted `keys`
    and `perm` (slot -> triangle)."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    t = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    p = v[t]
    lo, hi = p.min(axis=1), p.max(axis=1)
    maxabs = np.abs(p).max(axis=(1, 2))
    ext = (hi - lo).max(axis=1)
    pad = ext * F32(1.0 / 512.0) + F32(1e-6) * (F32(1.0) + maxabs)
    cent = F32(0.5) * (lo + hi)
    tbox = np.concatenate([lo - pad[:, None], hi + pad[:, None]], axis=1)
    assert tbox.dtype == F32 and cent.dtype == F32
    blo, bhi = cent.min(axis=0), cent.max(axis=0)
    keys = np.zeros(len(t), np.uint64)
    for a in range(3):
        e = bhi[a] - blo[a]
        u = (cent[:, a] - blo[a]) / e if e > 0 else np.zeros(len(t), F32)
        u = np.minimum(np.maximum(u, F32(0)), F32(1))
        q = np.minimum(u * F32(2097152.0), F32(2097151.0)).astype(np.uint64)
        keys |= _spread21(q) << np.uint64(2 - a)
    perm = np.argsort(keys, kind="stable")
    return dict(tbox=tbox, keys=keys[perm], perm=perm.astype(np.int64))


def box_area(b):
    """The file's box_area, float32, every operation rounded; b [..., 6]."""
    b = np.asarray(b, F32)
    dx, dy, dz = b[..., 3] - b[..., 0], b[..., 4] - b[..., 1], b[..., 5] - b[..., 2]
    a = F32(2.0) * ((dx * dy + dy * dz) + dz * dx)
    return np.where((dx >= 0) & (dy >= 0) & (dz >= 0), a, F32(0.0)).astype(F32)


def union(a, b):
    return np.concatenate([np.minimum(a[..., :3], b[..., :3]), np.maximum(a[..., 3:], b[..., 3:])], axis=-1)


# ---- step 3-4: the radix tree --------------------------------------------------------------------
def radix_tree(pre) -> dict:
    """Karras' tree over the sorted keys (equal keys told apart by the slot), built top-down: the
    same nodes, numbered in another order."""
    keys = [int(k) for k in pre["keys"]]
    n = len(keys)
    lbox = pre["tbox"][pre["perm"]]
    child = np.zeros((max(n - 1, 0), 2), np.int64)
    todo = [(0, n - 1, -1, 0)] if n >= 2 else []
    made = 0
    while todo:
        lo, hi, par, side = todo.pop()
        if lo == hi:
            child[par, side] = ~lo
            continue
        me = made
        made += 1
        if par >= 0:
            child[par, side] = me
        x = keys[lo] ^ keys[hi]
        if x:
            s = x.bit_length() - 1  # the highest differing bit: 0 below the split, 1 above
            g = bisect_left(keys, ((keys[lo] >> s) | 1) << s, lo, hi + 1) - 1
        else:
            s = (lo ^ hi).bit_length() - 1
            g = (((lo >> s) | 1) << s) - 1
        assert lo <= g < hi
        todo.append((g + 1, hi, me, 1))
        todo.append((lo, g, me, 0))
    assert made == max(n - 1, 0)
    box = np.zeros((len(child), 6), F32)
    size = np.zeros(len(child), np.int64)
    for i in range(len(child) - 1, -1, -1):  # children are numbered after their parents
        cb = [box[c] if c >= 0 else lbox[~c] for c in child[i]]
        box[i] = union(cb[0], cb[1])
        size[i] = sum(size[c] if c >= 0 else 1 for c in child[i])
    return dict(child=child, box=box, size=size, root=0 if n >= 2 else ~0, lbox=lbox, perm=pre["perm"])


# ---- step 3'-4': PLOC ----------------------------------------------------------------------------
def nearest(box, radius):
    """nn [C]: per position the candidate j != i within `radius` with the smallest
    (area of the union, 0 for the buddy i ^ 1 else 1, j); chosen among the candidates themselves."""
    C = len(box)
    i = np.arange(C)[:, None]
    k = np.concatenate([np.arange(-radius, 0), np.arange(1, radius + 1)])[None, :]
    j = i + k
    valid = (j >= 0) & (j < C)
    jc = np.clip(j, 0, C - 1)
    d = box_area(union(box[:, None, :], box[jc]))
    order = np.lexsort((j, (j != (i ^ 1)).astype(np.int8), d, ~valid), axis=1)
    return np.take_along_axis(j, order[:, :1], axis=1)[:, 0]


def ploc_clusters(box, radius=PLOC_R, cap=None) -> dict:
    """The rule on an array of boxes [n, 6] in slot order.  Returns child / box / size / root and
    `rounds`, `merges` (per round the (i, nn(i)) leader pairs as positions)."""
    box = np.ascontiguousarray(box, F32)
    n = len(box)
    cap = round_cap(n) if cap is None else cap
    bound = cap + ceil_log2(n)
    child = np.zeros((max(n - 1, 0), 2), np.int64)
    nbox = np.zeros((len(child), 6), F32)
    nsize = np.zeros(len(child), np.int64)
    cid, cbox, csize = ~np.arange(n), box.copy(), np.ones(n, np.int64)
    K, rounds, merges = 0, 0, []
    while len(cid) > 1:
        if rounds >= bound:
            raise RuntimeError("round bound")
        C = len(cid)
        pos = np.arange(C)
        if rounds >= cap:
            nn = np.where((pos ^ 1) < C, pos ^ 1, -1)
        else:
            nn = nearest(cbox, radius)
        mutual = (nn >= 0) & (nn[np.clip(nn, 0, C - 1)] == pos)
        leader = mutual & (pos < nn)
        keep = ~(mutual & (pos > nn))
        li = np.flatnonzero(leader)
        if len(li) == 0:
            raise RuntimeError("no progress")
        lj = nn[li]
        node = K + np.arange(len(li))
        child[node, 0], child[node, 1] = cid[li], cid[lj]
        nbox[node] = union(cbox[li], cbox[lj])
        nsize[node] = csize[li] + csize[lj]
        merges.append(np.stack([li, lj], axis=1))
        cid, cbox, csize = cid.copy(), cbox.copy(), csize.copy()
        cid[li], cbox[li], csize[li] = node, nbox[node], nsize[node]
        cid, cbox, csize = cid[keep], cbox[keep], csize[keep]
        K += len(li)
        rounds += 1
    assert K == max(n - 1, 0)
    return dict(child=child, box=nbox, size=nsize, root=n - 2 if n >= 2 else ~0, rounds=rounds, merges=merges)


def ploc_tree(pre, radius=PLOC_R, cap=None) -> dict:
    lbox = pre["tbox"][pre["perm"]]
    out = ploc_clusters(lbox, radius, cap)
    out.update(lbox=lbox, perm=pre["perm"])
    return out


def check_binary(tree, n):
    """Every slot under exactly one leaf, n - 1 nodes each reached once, sizes add up, root n - 2."""
    child, size = tree["child"], tree["size"]
    assert len(child) == n - 1 and tree["root"] == n - 2
    kids = child.reshape(-1)
    leaves = np.sort(~kids[kids < 0])
    assert np.array_equal(leaves, np.arange(n)), "every slot under exactly one leaf"
    inner = np.sort(kids[kids >= 0])
    assert np.array_equal(inner, np.arange(n - 2)), "every node but the root has one parent"
    assert (child < np.arange(n - 1)[:, None]).all(), "children are made before their parents"
    want = np.where(child >= 0, size[np.clip(child, 0, None)], 1).sum(axis=1)
    assert np.array_equal(size, want) and size[n - 2] == n, "sizes add up"


# ---- step 5: the collapse ------------------------------------------------------------------------
def collapse(tree) -> dict:
    """k_collapse's rule on a binary tree; nodes numbered breadth-first, slots in that order."""
    child, box, size, lbox, perm = tree["child"], tree["box"], tree["size"], tree["lbox"], tree["perm"]
    n = len(lbox)
    area = box_area(box) if len(box) else np.zeros(0, F32)
    size_of = lambda c: int(size[c]) if c >= 0 else 1
    expandable = lambda c: c >= 0 and size_of(c) > LEAF_MAX

    def slots(c):
        if c < 0:
            return [~c]
        return slots(int(child[c, 0])) + slots(int(child[c, 1]))

    nodes, orig = [], []
    front = [(tree["root"], 0)]
    n_nodes = 1
    while front:
        nxt = []
        for b, out in front:
            while len(nodes) <= out:
                nodes.append(None)
            if b < 0 or n < 2 or size_of(b) <= LEAF_MAX:
                kids = [b]
            else:
                kids = [int(child[b, 0]), int(child[b, 1])]
                while len(kids) < 4:
                    best, best_a = -1, F32(-1.0)
                    for i, c in enumerate(kids):
                        if expandable(c) and area[c] > best_a:
                            best, best_a = i, area[c]
                    if best < 0:
                        break
                    c = kids[best]
                    kids[best] = int(child[c, 0])
                    kids.append(int(child[c, 1]))
            nd = np.zeros(32, F32)
            codes = np.full(4, RT_EMPTY_CHILD, np.int32)
            for k, c in enumerate(kids):
                if n >= 2 and expandable(c):
                    bx = box[c]
                    codes[k] = n_nodes
                    nxt.append((c, n_nodes))
                    n_nodes += 1
                else:
                    sl = slots(c) if n >= 2 else list(range(n))
                    bx = (box[c] if c >= 0 else lbox[~c]) if n >= 2 else lbox[0]
                    codes[k] = ~((len(orig) << 3) | (len(sl) - 1))
                    orig += [int(perm[s]) for s in sl]
                nd[0 + k], nd[4 + k], nd[8 + k], nd[12 + k], nd[16 + k], nd[20 + k] = bx[0], bx[3], bx[1], bx[4], bx[2], bx[5]
            nd[24:28] = codes.view(F32)
            nodes[out] = nd
        front = nxt
    assert len(orig) == n
    return dict(nodes4=np.stack(nodes), orig=np.asarray(orig, np.int64))


def as_tree4(mesh_tree) -> dict:
    """RayTracer.meshTree()'s closest-hit tree in this module's form."""
    return dict(nodes4=mesh_tree["nodes4"], orig=mesh_tree["tris"][:, 3].copy().view(np.int32).astype(np.int64))


def _slots(t4, i):
    """Node i's used slots: (code, box [6] float32 as lo xyz, hi xyz)."""
    nd = t4["nodes4"][i]
    codes = nd[24:28].view(np.int32)
    return [(int(codes[k]), nd[[0 + k, 8 + k, 16 + k, 4 + k, 12 + k, 20 + k]]) for k in range(4)]


def _leaf(t4, code):
    enc = ~code
    first, cnt = enc >> 3, (enc & 7) + 1
    return [int(x) for x in t4["orig"][first:first + cnt]]


def same_tree4(a, b, tag=""):
    """The canonical walk; raises AssertionError at the first difference."""
    todo = [(0, 0, "root")]
    seen = 0
    while todo:
        ia, ib, path = todo.pop()
        seen += 1
        for k, ((ca, ba), (cb, bb)) in enumerate(zip(_slots(a, ia), _slots(b, ib))):
            where = f"{tag} {path}.{k}"
            kind = lambda c: "empty" if c == RT_EMPTY_CHILD else ("inner" if c >= 0 else "leaf")
            assert kind(ca) == kind(cb), f"{where}: {kind(ca)} against {kind(cb)}"
            assert np.array_equal(ba.view(np.uint32), bb.view(np.uint32)), f"{where}: box {ba} against {bb}"
            if kind(ca) == "leaf":
                assert _leaf(a, ca) == _leaf(b, cb), f"{where}: triangles {_leaf(a, ca)} against {_leaf(b, cb)}"
            elif kind(ca) == "inner":
                todo.append((ca, cb, f"{path}.{k}"))
    assert seen == len(a["nodes4"]) == len(b["nodes4"]), f"{tag}: {seen} nodes walked of {len(a['nodes4'])} / {len(b['nodes4'])}"


def sah_cost(t4) -> float:
    """(1 + sum of inner-child areas / root area) + sum of leaf-child areas x triangles / root area,
    in float64; the root area is that of the union of the root node's child boxes."""
    nd = t4["nodes4"].astype(np.float64)
    codes = t4["nodes4"][:, 24:28].view(np.int32)
    ext = [nd[:, 4 + 8 * a:8 + 8 * a] - nd[:, 8 * a:4 + 8 * a] for a in range(3)]
    area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0])
    used = codes[0] != RT_EMPTY_CHILD
    lo = [nd[0, 8 * a:4 + 8 * a][used].min() for a in range(3)]
    hi = [nd[0, 4 + 8 * a:8 + 8 * a][used].max() for a in range(3)]
    e = [h - l for h, l in zip(hi, lo)]
    root = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
    inner = (codes >= 0) & (codes != RT_EMPTY_CHILD)
    leaf = codes < 0
    tris = np.where(leaf, ((~codes) & 7) + 1, 0)
    return float(1.0 + area[inner].sum() / root + (area * tris)[leaf].sum() / root)


def build(verts, idx, builder, radius=PLOC_R, cap=None) -> dict:
    """The 4-wide tree of `builder` ("gpu": radix tree, "ploc"), with the binary tree as `binary`."""
    pre = prep(verts, idx)
    binary = radix_tree(pre) if builder == "gpu" else ploc_tree(pre, radius, cap)
    out = collapse(binary)
    out["binary"] = binary
    return out
