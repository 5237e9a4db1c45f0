"""A numpy restatement of RT_COLLAPSE_SAH (rt_build_gpu.hip k_collapse_cost / k_collapse_sah,
DESIGN.md §4.6c): the collapse of a device builder's binary tree to the 4-wide tree by dynamic
programming, as the host build's.  Binary and 4-wide trees are ploc_ref's dicts.

Per binary node c, D[c][j] (j = 1..4) is the cost of presenting c's triangles as at most j children
of a wide node; a step is one wide-node visit or one triangle of a visited leaf, weighted by the
box's float32 area.  Every product and sum is one rounded float32 operation.
"""
from __future__ import annotations

import numpy as np

import ploc_ref as pr

F32 = np.float32
INF = F32(np.inf)
LEAF_MAX = pr.LEAF_MAX


def _post_order(tree):
    """The inner nodes, children before parents."""
    child, root = tree["child"], tree["root"]
    if root < 0:
        return []
    out, todo = [], [int(root)]
    while todo:
        i = todo.pop()
        out.append(i)
        todo += [int(c) for c in child[i] if c >= 0]
    return out[::-1]


def cost_pass(tree, leaf_max=LEAF_MAX) -> dict:
    """The bottom-up pass: `D` [m, 5] float32 (column j), `split` [m, 5] (column j: the left child's
    share of j children, 0: the node stays whole), `as_leaf` [m], `a_star` [m] (the left child's share
    when the node is a wide node itself)."""
    child, box, size, lbox = tree["child"], tree["box"], tree["size"], tree["lbox"]
    m = len(child)
    with np.errstate(over="ignore", invalid="ignore"):
        area = pr.box_area(box) if m else np.zeros(0, F32)
        larea = pr.box_area(lbox)
    D = np.zeros((m, 5), F32)
    split = np.zeros((m, 5), np.int64)
    as_leaf = np.zeros(m, bool)
    a_star = np.ones(m, np.int64)
    dc = lambda c, j: D[c, j] if c >= 0 else larea[~c]
    with np.errstate(over="ignore", invalid="ignore"):
        for i in _post_order(tree):
            l, r = int(child[i, 0]), int(child[i, 1])
            small = int(size[i]) <= leaf_max
            leaf_c = F32(area[i] * F32(size[i])) if small else INF
            best_int = F32(dc(l, 1) + dc(r, 3))
            for a in (2, 3):
                v = F32(dc(l, a) + dc(r, 4 - a))
                if v < best_int:
                    best_int, a_star[i] = v, a
            inner_c = F32(area[i] + best_int)
            as_leaf[i] = small and bool(leaf_c <= inner_c)
            D[i, 1] = leaf_c if as_leaf[i] else inner_c
            for j in (2, 3, 4):
                best, arg = D[i, 1], 0
                for a in range(1, j):
                    v = F32(dc(l, a) + dc(r, j - a))
                    if v < best:
                        best, arg = v, a
                D[i, j], split[i, j] = best, arg
    return dict(D=D, split=split, as_leaf=as_leaf, a_star=a_star)


def collapse_sah(tree, leaf_max=LEAF_MAX) -> dict:
    """The top-down pass on `tree`; nodes numbered breadth-first, record slots in that order; `cost`
    holds the bottom-up pass's arrays."""
    child, box, lbox, perm = tree["child"], tree["box"], tree["lbox"], tree["perm"]
    n = len(lbox)
    cp = cost_pass(tree, leaf_max)
    split, as_leaf, a_star = cp["split"], cp["as_leaf"], cp["a_star"]

    def slots(c):
        return [~c] if c < 0 else slots(int(child[c, 0])) + slots(int(child[c, 1]))

    def expand(c, j):
        s = 0 if c < 0 else int(split[c, j])
        if s == 0:
            return [c]
        return expand(int(child[c, 0]), s) + expand(int(child[c, 1]), j - s)

    nodes, orig = [], []
    front = [(int(tree["root"]), 0)]
    n_nodes = 1
    while front:
        nxt = []
        for b, out in front:
            while len(nodes) <= out:
                nodes.append(None)
            if b < 0 or n < 2:
                kids = [b]  # the single triangle
            else:
                a = int(a_star[b])
                kids = expand(int(child[b, 0]), a) + expand(int(child[b, 1]), 4 - a)
            assert 1 <= len(kids) <= 4
            nd = np.zeros(32, F32)
            codes = np.full(4, pr.RT_EMPTY_CHILD, np.int32)
            for k, c in enumerate(kids):
                if n >= 2 and c >= 0 and not as_leaf[c]:
                    bx = box[c]
                    codes[k] = n_nodes
                    nxt.append((c, n_nodes))
                    n_nodes += 1
                else:
                    sl = slots(c) if n >= 2 else [0]
                    assert len(sl) <= leaf_max
                    bx = (box[c] if c >= 0 else lbox[~c]) if n >= 2 else lbox[0]
                    codes[k] = ~((len(orig) << 3) | (len(sl) - 1))
                    orig += [int(perm[s]) for s in sl]
                nd[0 + k], nd[4 + k], nd[8 + k], nd[12 + k], nd[16 + k], nd[20 + k] = bx[0], bx[3], bx[1], bx[4], bx[2], bx[5]
            nd[24:28] = codes.view(F32)
            nodes[out] = nd
        front = nxt
    assert len(orig) == n
    return dict(nodes4=np.stack(nodes), orig=np.asarray(orig, np.int64), cost=cp)


def binary(verts, idx, builder, sub=None) -> dict:
    """The builder's binary tree over the triangles `sub` lists (None: all), `perm` naming the
    mesh's triangles — a part of the mesh is built as the device builds it: the sort and the tree
    over the list alone."""
    idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    pre = pr.prep(verts, idx if sub is None else idx[np.asarray(sub, np.int64)])
    tree = pr.radix_tree(pre) if builder == "gpu" else pr.ploc_tree(pre)
    if sub is not None:
        tree["perm"] = np.asarray(sub, np.int64)[tree["perm"]]
    return tree


def build(verts, idx, builder, collapse="sah", sub=None) -> dict:
    """The 4-wide tree of `builder` ("gpu", "ploc") under `collapse` ("greedy", "sah")."""
    b = binary(verts, idx, builder, sub)
    out = collapse_sah(b) if collapse == "sah" else pr.collapse(b)
    out["binary"] = b
    return out


def depth_stack(t4):
    """(depth, worst-case traversal stack as the device collapse counts it: a node's children but
    one wait while the traversal descends)."""
    codes = t4["nodes4"][:, 24:28].view(np.int32)
    best_d = best_s = 0
    todo = [(0, 1, 0)]
    while todo:
        i, d, s = todo.pop()
        nk = int((codes[i] != pr.RT_EMPTY_CHILD).sum())
        st = s + max(nk - 1, 0)
        best_d, best_s = max(best_d, d), max(best_s, st)
        todo += [(int(c), d + 1, st) for c in codes[i] if c >= 0 and c != pr.RT_EMPTY_CHILD]
    return best_d, best_s


def leaves(t4):
    """Per leaf child of the whole tree its triangle list."""
    codes = t4["nodes4"][:, 24:28].view(np.int32).reshape(-1)
    return [pr._leaf(t4, int(c)) for c in codes if c < 0]


def check_tree4(t4, n, leaf_max=LEAF_MAX):
    """Every triangle in exactly one leaf, leaves of 1..leaf_max, every node reached by the walk."""
    lv = leaves(t4)
    assert all(1 <= len(l) <= leaf_max for l in lv), "a leaf's size"
    assert sorted(t for l in lv for t in l) == list(range(n)), "every triangle in exactly one leaf"
    pr.same_tree4(t4, t4)


def same_links(tree, root, ref4, n_tris, tag=""):
    """A part of the shadow tree (compressed nodes alone: RayTracer.meshTree()'s nodes4q, records
    offset by n_tris) against the restatement's tree of that part: slot by slot the kind and a
    leaf's triangles in order, inner children followed."""
    q = tree["nodes4q"]
    orig = tree["tris"][:, 3].view(np.int32)
    codes_b = ref4["nodes4"][:, 24:28].view(np.int32)
    todo, seen = [(int(root), 0)], 0
    while todo:
        ia, ib = todo.pop()
        seen += 1
        for k, (ca, cb) in enumerate(zip(q[ia, 12:16].view(np.int32).tolist(), codes_b[ib].tolist())):
            kind = lambda c: "empty" if c == pr.RT_EMPTY_CHILD else ("inner" if c >= 0 else "leaf")
            assert kind(ca) == kind(cb), f"{tag} node {ia} slot {k}: {kind(ca)} against {kind(cb)}"
            if kind(ca) == "leaf":
                enc = ~ca
                got = orig[(enc >> 3):(enc >> 3) + (enc & 7) + 1].tolist()
                assert (enc >> 3) >= n_tris and got == pr._leaf(ref4, cb), f"{tag} node {ia} slot {k}: {got}"
            elif kind(ca) == "inner":
                todo.append((ca, cb))
    assert seen == len(ref4["nodes4"]), f"{tag}: {seen} nodes walked of {len(ref4['nodes4'])}"
