"""RT_COLLAPSE_SAH as tests/collapse_ref.py restates it (rt_build_gpu.hip k_collapse_cost /
k_collapse_sah), without a GPU: the 4-wide trees' invariants on every mesh the GPU
tests use, the cost against the greedy collapse's, and hand-worked trees."""
from __future__ import annotations

import numpy as np
import pytest

import collapse_cases as cc
import collapse_ref as cr
import ploc_cases as pc
import ploc_ref as pr

ALL = pc.MESHES + list(pc.CAP_MESHES)


def cube(x, y=0.0, z=0.0, w=1.0):
    return [x, y, z, x + w, y + w, z + w]


def clusters(boxes):
    """The PLOC tree over hand-made boxes, in the form the collapse reads."""
    lbox = np.array(boxes, np.float32)
    t = pr.ploc_clusters(lbox)
    t.update(lbox=lbox, perm=np.arange(len(lbox)))
    return t


def kinds(t4, i=0):
    """Node i's children: an int (an inner child's node) or a leaf's triangle list."""
    codes = t4["nodes4"][i, 24:28].view(np.int32)
    return [int(c) if c >= 0 else pr._leaf(t4, int(c)) for c in codes if c != pr.RT_EMPTY_CHILD]


# ---- invariants ----------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", cc.BUILDERS)
@pytest.mark.parametrize("name", ALL)
def test_invariants(name, builder, pt):
    verts, idx = pc.make(name, pt.scenes)
    t4 = cc.ref_tree(name, pt.scenes, builder)
    cr.check_tree4(t4, len(idx))  # one leaf per triangle, leaves of 1..4, the walk reaches every node
    if len(idx) >= 2:  # the root is a wide node of the rule's children, whatever its size
        assert len(kinds(t4)) >= 2
    # no child the rule calls a leaf has more than kLeafMax triangles
    b, cp = t4["binary"], t4["cost"]
    assert not (cp["as_leaf"] & (b["size"] > pr.LEAF_MAX)).any()
    assert ((cp["split"] >= 0) & (cp["split"] < np.arange(5)[None, :].clip(1))).all()


# ---- cost ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", cc.BUILDERS)
@pytest.mark.parametrize("name", [n for n in ALL if n != "sphere200_first1"])  # (one triangle: one tree)
def test_cost_not_above_the_greedy_collapse(name, builder, pt):
    sah, greedy = (pr.sah_cost(cc.ref_tree(name, pt.scenes, builder, m)) for m in ("sah", "greedy"))
    (_, s_s), (_, s_g) = (cr.depth_stack(cc.ref_tree(name, pt.scenes, builder, m)) for m in ("sah", "greedy"))
    n_s, n_g = (len(cc.ref_tree(name, pt.scenes, builder, m)["nodes4"]) for m in ("sah", "greedy"))
    print(f"{name} {builder}: sah_cost greedy {greedy:.6g} -> sah {sah:.6g} (ratio {sah / greedy:.4f}), nodes {n_g} -> {n_s}, "
          f"stack {s_g} -> {s_s}")
    # the DP is optimal in float32 sums, sah_cost is float64: an exact tie may land a rounding apart
    assert sah <= greedy * (1 + 1e-5)
    if name in cc.MUCH_BETTER:
        assert sah < 0.95 * greedy


# ---- hand-worked trees ---------------------------------------------------------------------------
def test_two_distant_pairs():
    """Unit cubes at 0, 1.5 and 100, 101.5.  A cube's area is 6; a pair's box is 2.5 x 1 x 1, area 12.
    A pair as a leaf costs 12 * 2 = 24, as a node 12 + (6 + 6) = 24: D[pair][1] = 24 (a leaf, <=), and
    as two children 6 + 6 = 12 < 24: split[pair][2] = 1.  The root: a = 1: 24 + 12 = 36, a = 2:
    12 + 12 = 24, a = 3: 12 + 24 = 36, so a* = 2 and both pairs dissolve: four leaves of one."""
    t = clusters([cube(0), cube(1.5), cube(100), cube(101.5)])
    assert t["child"].tolist() == [[~0, ~1], [~2, ~3], [0, 1]]
    cp = cr.cost_pass(t)
    assert cp["D"][0, 1:].tolist() == [24, 12, 12, 12] and cp["split"][0, 1:].tolist() == [0, 1, 1, 1]
    assert cp["as_leaf"].tolist() == [True, True, False] and cp["a_star"][2] == 2
    t4 = cr.collapse_sah(t)
    assert kinds(t4) == [[0], [1], [2], [3]] and len(t4["nodes4"]) == 1
    assert kinds(pr.collapse(t)) == [[0, 1, 2, 3]]  # the greedy rule: one leaf in a 102.5-long box


def test_four_identical_boxes():
    """Area A = 6 everywhere.  A pair: leaf 2A = 12 against A + 2A = 18, a leaf; as two children
    A + A = 12 is not < 12, so it stays whole.  The four: leaf_c = 4A = 24 against A + 4A = 30: as_leaf.
    Under a parent they are one leaf of four; as the tree's root, which is always a wide node, they
    are the two pairs."""
    t = clusters([cube(0)] * 4)
    cp = cr.cost_pass(t)
    assert cp["D"][2, 1] == 24 and cp["as_leaf"][2] and cp["split"][:, 2:].max() == 0
    assert kinds(cr.collapse_sah(t)) == [[0, 1], [2, 3]]
    both = clusters([cube(0)] * 4 + [cube(100)] * 4)
    assert both["child"][-1].tolist() == [4, 5]
    assert kinds(cr.collapse_sah(both)) == [[0, 1, 2, 3], [4, 5, 6, 7]]


def test_infinite_costs_never_make_a_large_leaf():
    """Six boxes of extent 1e19: every area and every sum is +INF, leaf_c <= inner_c holds
    everywhere.  The size test keeps the subtrees of 5 and 6 triangles from becoming leaves."""
    big = [0.0, 0.0, 0.0, 1e19, 1e19, 1e19]
    lbox = np.array([big] * 6, np.float32)
    with np.errstate(over="ignore"):
        assert np.isinf(pr.box_area(lbox)).all()
    child = np.array([[~0, ~1], [0, ~2], [1, ~3], [2, ~4], [3, ~5]], np.int64)  # a chain: sizes 2 .. 6
    t = dict(child=child, box=np.array([big] * 5, np.float32), size=np.array([2, 3, 4, 5, 6]), root=4, lbox=lbox,
             perm=np.arange(6))
    cp = cr.cost_pass(t)
    assert np.isinf(cp["D"][:, 1:]).all()
    assert cp["as_leaf"].tolist() == [True, True, True, False, False]
    t4 = cr.collapse_sah(t)
    cr.check_tree4(t4, 6)
    assert max(len(l) for l in cr.leaves(t4)) == 4
    assert kinds(t4) == [1, [5]] and kinds(t4, 1) == [[0, 1, 2, 3], [4]]


def test_smallest_counts():
    one = clusters([cube(0)])
    assert kinds(cr.collapse_sah(one)) == [[0]]
    assert kinds(cr.collapse_sah(clusters([cube(0), cube(5)]))) == [[0], [1]]
    cr.check_tree4(cr.collapse_sah(clusters([cube(0), cube(5), cube(6.5)])), 3)
