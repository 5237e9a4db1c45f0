"""The PLOC rule as tests/ploc_ref.py restates it (rt_build_gpu.hip k_ploc_*), without
a GPU: hand-made arrays, the round cap, the binary tree's invariants at every size the GPU tests
use, and the precondition of the GPU quality test — the collapsed PLOC tree costs less than the
collapsed radix tree of the same sorted order."""
from __future__ import annotations

import numpy as np
import pytest

import ploc_cases as pc
import ploc_ref as pr


def cube(x, y=0.0, z=0.0, w=1.0):
    return [x, y, z, x + w, y + w, z + w]


def test_two_distant_pairs():
    t = pr.ploc_clusters(np.array([cube(0), cube(1.5), cube(100), cube(101.5)], np.float32))
    assert t["rounds"] == 2 and t["root"] == 2
    assert t["child"].tolist() == [[~0, ~1], [~2, ~3], [0, 1]]
    assert t["size"].tolist() == [2, 2, 4]
    assert t["box"][2].tolist() == [0, 0, 0, 102.5, 1, 1]


def test_identical_boxes_pair_as_buddies():
    t = pr.ploc_clusters(np.array([cube(0)] * 8, np.float32))
    assert t["rounds"] == 3
    assert t["child"].tolist() == [[~0, ~1], [~2, ~3], [~4, ~5], [~6, ~7], [0, 1], [2, 3], [4, 5]]
    assert [m.tolist() for m in t["merges"]] == [[[0, 1], [2, 3], [4, 5], [6, 7]], [[0, 1], [2, 3]], [[0, 1]]]


def test_odd_count():
    """Five equal boxes: position 4 has no buddy and chooses the lowest position, which has chosen
    its own buddy, so it waits until it is the second of two."""
    t = pr.ploc_clusters(np.array([cube(0)] * 5, np.float32))
    assert t["rounds"] == 3
    assert t["child"].tolist() == [[~0, ~1], [~2, ~3], [0, 1], [2, ~4]]
    pr.check_binary(t, 5)
    # seven boxes in a row, the gaps growing: the pairs form from the left, the last box is left over
    x = np.cumsum([0, 1.1, 1.3, 1.2, 1.6, 1.3, 1.9])
    t = pr.ploc_clusters(np.array([cube(v) for v in x], np.float32))
    pr.check_binary(t, 7)
    assert t["child"][:3].tolist() == [[~0, ~1], [~2, ~3], [~4, ~5]]


def test_smallest_counts():
    one = pr.ploc_clusters(np.array([cube(0)], np.float32))
    assert one["rounds"] == 0 and one["root"] == ~0 and len(one["child"]) == 0
    two = pr.ploc_clusters(np.array([cube(0), cube(5)], np.float32))
    assert two["rounds"] == 1 and two["root"] == 0 and two["child"].tolist() == [[~0, ~1]]
    three = pr.ploc_clusters(np.array([cube(0), cube(5), cube(6.5)], np.float32))
    assert three["child"].tolist() == [[~1, ~2], [~0, 0]] and three["root"] == 1
    pr.check_binary(three, 3)


def test_ties_prefer_the_buddy_then_the_lowest_position():
    # 1 is as near to 0 as to 2: position 1's buddy is 0; position 2's buddy 3 is far, it takes the lower 1
    b = np.array([cube(0), cube(2), cube(4), cube(50)], np.float32)
    assert pr.nearest(b, 16).tolist() == [1, 0, 1, 2]
    # without a buddy among the equal ones: the lowest position
    b = np.array([cube(50), cube(2), cube(0), cube(4)], np.float32)
    assert pr.nearest(b, 16).tolist() == [3, 2, 1, 1]
    # the window: position 0 does not see position 17
    b = np.array([cube(0)] + [cube(100 + 3 * k) for k in range(16)] + [cube(1)], np.float32)
    assert pr.nearest(b, 16)[0] == 1 and pr.nearest(b, 17)[0] == 17


def test_round_cap_on_the_shrinking_strip():
    x, w = pc.strip_boxes()
    box = np.stack([x, -w, -w, x + w, w, w], axis=1).astype(np.float32)
    cap = pr.round_cap(4096)
    assert cap == 88
    t = pr.ploc_clusters(box)
    print(f"shrinking strip: {t['rounds']} rounds, cap {cap}")
    assert cap < t["rounds"] <= cap + 12, "precondition: the strip reaches the halving rounds"
    pr.check_binary(t, 4096)
    free = pr.ploc_clusters(box[:512], cap=10 ** 6)  # the rule alone: about one merge per round
    assert free["rounds"] > pr.round_cap(512) + 9
    halved = pr.ploc_clusters(box, cap=0)  # halving rounds alone: the balanced tree over the order
    assert halved["rounds"] == 12
    pr.check_binary(halved, 4096)


def test_identical_boxes_4096():
    t = pr.ploc_clusters(np.tile(np.array(cube(0), np.float32), (4096, 1)))
    assert t["rounds"] == 12
    pr.check_binary(t, 4096)


@pytest.mark.parametrize("name", pc.MESHES + list(pc.CAP_MESHES))
def test_binary_tree_invariants(name, pt):
    verts, idx = pc.make(name, pt.scenes)
    n = len(idx)
    t4 = pc.ref_tree(name, pt.scenes, "ploc")
    if n >= 2:
        pr.check_binary(t4["binary"], n)
        assert t4["binary"]["rounds"] <= pr.round_cap(n) + pr.ceil_log2(n)
    assert sorted(t4["orig"].tolist()) == list(range(n)), "every triangle in one leaf of the 4-wide tree"
    pr.same_tree4(t4, t4, name)  # the walk reaches every node


@pytest.mark.parametrize("name", pc.BETTER + pc.NOT_WORSE)
def test_ploc_costs_less_than_the_radix_tree(name, pt):
    ploc, lbvh = (pr.sah_cost(pc.ref_tree(name, pt.scenes, b)) for b in ("ploc", "gpu"))
    print(f"{name}: sah_cost ploc {ploc:.6g}, lbvh {lbvh:.6g}, ratio {ploc / lbvh:.4f}")
    if name in pc.BETTER:
        assert ploc < lbvh
    else:
        assert ploc <= lbvh
