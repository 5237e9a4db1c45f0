"""Meshes shared by tests/test_ploc_host.py and tests/test_gpu_ploc.py: tree_cases' meshes, displaced
spheres around the PLOC window (radius 16), one block (256) and its halo, several blocks and several
scan tiles, and the two meshes that reach the round cap."""
from __future__ import annotations

import numpy as np

import ploc_ref as pr
import tree_cases as tc

SPHERES = (17, 33, 255, 256, 257, 1000, 20000)
CAP_MESHES = ("strip4096", "same4096")
# sah_cost(PLOC) < sah_cost(LBVH) on these, <= on regular grids, where the radix tree is already ideal.
# The grids are not tree_cases' flat_grid and far_grid: a triangle's pad grows with its largest
# coordinate (1e-6 (1 + maxabs)) and the rounding of lo - pad with the coordinate's binade, so their
# boxes differ in the last bits from cell to cell, those bits and not the buddy rule decide between
# the equal neighbours, and PLOC costs 1.3 % / 1.1 % more than the radix tree there (with unpadded
# boxes: 8.0 against 8.0, 8.06 against 8.0).  The grids below lie in one binade ([32, 64) on every axis,
# y = 60 the largest coordinate of every triangle): every padded box has the same extent to the bit, as
# on the unpadded grid the rule was designed on.
BETTER = ("sphere2000", "mixed_scales", "det_bound", "sphere200", "sphere20000")
NOT_WORSE = ("binade_grid16", "binade_grid32")
MESHES = list(tc.MESHES) + [f"sphere{n}" for n in SPHERES if n != 2000] + list(NOT_WORSE)


def strip_boxes(n=4096, q=0.999):
    """n boxes in a row along x, each the factor q smaller than the one before and centred on
    y = z = 0: every position's nearest neighbour is the next, smaller one, so a round merges
    little more than the last pair."""
    w = q ** np.arange(n)
    x = np.concatenate([[0.0], np.cumsum(w)[:-1]])
    return x, w


def strip_tris(n=4096, q=0.999):
    """Triangles whose boxes are strip_boxes, in the sorted order as given (the centroids differ
    in x alone)."""
    x, w = strip_boxes(n, q)
    tri = np.stack([np.stack([x, -w, -w], 1), np.stack([x + w, w, w], 1), np.stack([x, w, -w], 1)], 1)
    return tc._soup(tri)


def same_tris(n=4096):
    """n copies of one triangle: every area is equal, the buddy rule decides every round."""
    return tc._soup(np.tile(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, 0.25]]), (n, 1, 1)))


def make(name, sc):
    if name == "strip4096":
        return strip_tris()
    if name == "same4096":
        return same_tris()
    if name.startswith("binade_grid"):
        n = int(name[len("binade_grid"):])
        return tc._grid((33.0, 60.0, 33.0), 16.0 / n, n)
    if name.startswith("sphere") and "_" not in name and name != "sphere2000":
        return sc.make_mesh(int(name[len("sphere"):]))
    return tc.make(name, sc)


_trees = {}


def ref_tree(name, sc, builder):
    """The restatement's 4-wide tree of `name` under "gpu" or "ploc", computed once."""
    key = (name, builder)
    if key not in _trees:
        _trees[key] = pr.build(*make(name, sc), builder)
    return _trees[key]
