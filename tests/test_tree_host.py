"""The host builder's trees (rt_bvh.cpp, rt_quant.h), checked node by node without a GPU:
tests/cpp/host_tree_dump builds the closest-hit tree and the light-leaning shadow tree as
rt_set_mesh lays them out, tests/tree_ref.py verifies every link, record, box, compressed plane,
normal box and the reported depth4 / stack4."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import tree_cases as tc
import tree_ref as tr
from conftest import ROOT


@pytest.fixture(scope="module")
def dump_tool():
    subprocess.run(["make", "-s", "-C", str(ROOT / "tests" / "cpp"), "host_tree_dump"], check=True)
    return ROOT / "tests" / "cpp" / "host_tree_dump"


def host_trees(tool, tmp, verts, idx, lights):
    np.ascontiguousarray(verts, np.float32).tofile(tmp / "verts.f32")
    np.ascontiguousarray(idx, np.int32).tofile(tmp / "idx.i32")
    np.ascontiguousarray(lights, np.float32).tofile(tmp / "lights.f32")
    r = subprocess.run([str(tool), str(tmp / "verts.f32"), str(tmp / "idx.i32"), str(tmp / "tree.bin"),
                        str(tmp / "lights.f32")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return tr.read_dump(tmp / "tree.bin")


def scene_lights(sc):
    s = sc.ply_scene()
    return np.ascontiguousarray(s["center"][s["emission_power"] != 0], np.float32)


def check_both(verts, idx, tree):
    """check_tree of the closest-hit tree and, where there is one, of the shadow tree, each against the
    builder's own n_hit, depth4 and stack4."""
    out = {0: tr.check_tree(verts, idx, tree, 0, builder="host", reported=tree["reported"][0])}
    if tree["n_nodes4_shadow"]:
        root = tree["shadow_root"]
        out[root] = tr.check_tree(verts, idx, tree, root, builder="host", reported=tree["reported"][root])
    return out


@pytest.mark.parametrize("name", tc.MESHES)
def test_host_trees(name, pt, dump_tool, tmp_path):
    verts, idx = tc.make(name, pt.scenes)
    tree = host_trees(dump_tool, tmp_path, verts, idx, scene_lights(pt.scenes))
    n = len(idx)
    assert tree["n_tris"] == n
    tr.check_fallback(tree, "host tree")
    if name in tc.NOT_ENCODABLE:
        assert tree["compressed"] == 0 and tree["nodes4q"] is None and tree["n_nodes4_shadow"] == 0
        assert tree["n_records"] == n
    else:
        assert tree["compressed"] == 1 and tree["n_nodes4_shadow"] > 0 and tree["shadow_root"] == tree["n_nodes4"]
        assert tree["n_records"] == 2 * n
    got = check_both(verts, idx, tree)
    if name in tc.NOTHING_HITTABLE:  # the builder keeps a one-leaf tree over triangle 0
        assert tree["n_nodes4"] == 1 and got[0]["n_hit"] == 1
    elif name == "det_bound":
        assert 0 < got[0]["n_hit"] < n
        q = tree["nodes4q"]
        assert ((q[:, 10] >> 24) != 255).mean() > 0.5  # the mesh whose normal boxes cull
    elif name != "mixed_scales":  # (its 0.02-extent triangles are partly below the bound)
        assert got[0]["n_hit"] == n
    for g in got.values():
        assert g["n_hit"] == got[0]["n_hit"]


def test_spill_stack_reaches_past_the_lds_part(pt, dump_tool, tmp_path):
    """The mesh of the GPU spill tests, at the host build's count: the builder reports a stack4 past
    the LDS part, and the model walk of a ray inside every box keeps more than RT_STACK_DEPTH
    entries live.  (Both are preconditions of tests/test_gpu_tree.py; here they pin the dump.)"""
    verts, idx = tc.spill_stack(tc.SPILL_COUNT["host"])
    tree = host_trees(dump_tool, tmp_path, verts, idx, scene_lights(pt.scenes))
    got = check_both(verts, idx, tree)
    assert got[0]["stack4"] >= tr.RT_STACK_DEPTH + 4
    rays = np.zeros(2, pt._abi.RAY_DTYPE)
    rays["o"] = [(0.9, 0.9, -4.0), (0.0, 0.0, -4.0)]
    rays["d"] = (0.0, 0.0, 1.0)
    live = tr.live_stack(tree, 0, rays)
    assert live.min() >= tr.RT_STACK_DEPTH + 3, live


def _corrupt(tree, fn):
    t = dict(tree)
    for k in ("nodes4", "nodes4q", "tris", "nodes4_shadow"):
        t[k] = None if tree[k] is None else tree[k].copy()
    fn(t)
    return t


def test_verifier_rejects_corrupted_trees(pt, dump_tool, tmp_path):
    """The verifier itself: single-field corruptions of a good tree are each named."""
    verts, idx = tc.make("sphere2000", pt.scenes)
    tree = host_trees(dump_tool, tmp_path, verts, idx, scene_lights(pt.scenes))
    check_both(verts, idx, tree)
    q = tree["nodes4q"]
    node = 3
    links = q[node, 12:16].view(np.int32)
    k = int(np.flatnonzero(links != tr.RT_EMPTY_CHILD)[-1])

    def plane_up(t):  # lower x plane of child k one grid step higher: the box no longer contains
        t["nodes4q"][node, 4] += np.uint32(1 << (8 * k))

    def plane_down(t):  # upper x plane one step further out: contains, but not tight
        t["nodes4q"][node, 5] += np.uint32(1 << (8 * k))

    def nbox_shrink(t):
        i = int(np.flatnonzero((t["nodes4q"][:, 10] >> 24) != 255)[0])
        t["nodes4q"][i, 11] -= np.uint32(1)

    def link_twice(t):
        inner = np.argwhere(t["nodes4q"][:t["n_nodes4"], 12:16].view(np.int32) >= 0)
        (a, ka), (b, kb) = inner[0], inner[-1]
        t["nodes4q"][b, 12 + kb] = t["nodes4q"][a, 12 + ka]
        t["nodes4"][b, 24 + kb] = t["nodes4"][a, 24 + ka]

    def record_edge(t):
        t["tris"][5, 4] = np.nextafter(t["tris"][5, 4], np.float32(np.inf))

    def full_box(t):  # the full-precision box of child k loses its pad on x
        t["nodes4"][node, 0 + k] = np.nextafter(verts.reshape(-1, 3)[:, 0].max(), np.float32(np.inf))

    for fn, words in ((plane_up, "decoded box does not contain"), (plane_down, "grid step or more above"),
                      (nbox_shrink, "normal"), (link_twice, "reached twice"), (record_edge, "e1 is not"),
                      (full_box, "full-precision box")):
        with pytest.raises(tr.TreeError, match="node|record") as e:
            check_both(verts, idx, _corrupt(tree, fn))
        assert words in str(e.value), (fn.__name__, str(e.value))
    bad = dict(tree["reported"][0], stack4=tree["reported"][0]["stack4"] - 1)
    with pytest.raises(tr.TreeError, match="stack4"):
        tr.check_tree(verts, idx, tree, 0, builder="host", reported=bad)
