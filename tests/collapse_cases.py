"""Meshes and cached restatement trees shared by tests/test_collapse_host.py and
tests/test_gpu_collapse.py (RT_COLLAPSE_SAH)."""
from __future__ import annotations

import collapse_ref as cr
import ploc_cases as pc
import ploc_ref as pr

BUILDERS = ("gpu", "ploc")
# sah_cost(SAH collapse) < 0.95 sah_cost(greedy collapse), both builders
MUCH_BETTER = ("sphere2000", "sphere20000", "mixed_scales", "det_bound", "binade_grid16", "binade_grid32")
# the device trees compared node for node with the restatement
DEVICE_MESHES = ["sphere17", "sphere33", "sphere257", "sphere1000", "sphere2000"] + \
    [f"sphere200_first{n}" for n in (1, 2, 4, 5, 8, 9)] + \
    ["mixed_scales", "det_bound", "one_centre600", "flat_grid", "huge8", "strip4096", "same4096"]

_trees = {}


def ref_tree(name, sc, builder, mode="sah"):
    """The restatement's 4-wide tree of `name` under `builder` and `mode`, computed once; the
    binary tree is ploc_cases' own."""
    if mode == "greedy":
        return pc.ref_tree(name, sc, builder)
    key = (name, builder)
    if key not in _trees:
        b = pc.ref_tree(name, sc, builder)["binary"]
        _trees[key] = cr.collapse_sah(b)
        _trees[key]["binary"] = b
    return _trees[key]
