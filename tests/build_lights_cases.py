"""Helpers of tests/test_gpu_build_lights.py: the device builders under RT_BUILD_OPT_LIGHTS
(setBuildOptions(True)).  The meshes and lights are the host test's
(tests/test_light_cone_host.py SPLIT_CASES), the rules its float64 restatements (rule_ratio,
tree_ref.never_hit_rule) with its RULE_MARGIN."""
from __future__ import annotations

import numpy as np

import test_light_cone_host as lh
import tree_ref as tr

BUILDERS = ("gpu", "ploc")
K_LEAF_MAX = 4  # the device collapse's largest leaf (rt_build_gpu.hip kLeafMax): a part must be larger


def builder_id(pt, builder):
    return {"host": pt._abi.RT_BUILD_HOST, "gpu": pt._abi.RT_BUILD_GPU, "ploc": pt._abi.RT_BUILD_GPU_PLOC}[builder]


def spheres_for(sc, lights):
    """The mesh scene's spheres with `lights` [(x, y, z, r)] in place of its own light."""
    base = sc.ply_scene()
    if list(lights) == [lh.PLY_LIGHT]:
        return base
    out = [base[base["emission_power"] == 0]]
    for x, y, z, r in lights:
        out.append(sc.init_sphere(center=(x, y, z), radius=r, emission_power=1.0, emission=(1.1, 1.1, 1.1)))
    return np.concatenate(out)


def context(pt, spheres, builder, lights_opt=True):
    rt = pt.RayTracer(0)
    rt.setSpheres(spheres)
    rt.setBuilder(builder)
    rt.setBuildOptions(lights_opt)
    rt.setTraversal("bvh")
    return rt


def classes(verts, idx, lights):
    """Per triangle, by the restated rules: surely left out, surely kept, and of the kept surely
    parked / surely a possible occluder (outside RULE_MARGIN of either threshold)."""
    hit = tr.never_hit_rule(tr.triangle_terms(np.ascontiguousarray(verts, np.float32).reshape(-1, 3),
                                              np.ascontiguousarray(idx, np.int32).reshape(-1, 3)))
    occ = lh.rule_ratio(verts, idx, lights) if len(lights) else np.full(len(hit), np.inf)
    m = lh.RULE_MARGIN
    out, kept = hit < 1.0 - m, hit >= 1.0 + m
    if not (hit >= 1.0 - m).any():  # nothing hittable: triangle 0 alone stays
        out, kept = out.copy(), kept.copy()
        out[0], kept[0] = False, True
    return dict(out=out, kept=kept, parked=kept & (occ < 1.0 - m), occluder=kept & (occ >= 1.0 + m),
                unsure=int((np.abs(hit - 1.0) <= m).sum() + (np.abs(occ - 1.0) <= m).sum()))


def expect_split(verts, idx, lights):
    """True / False when the restated rules decide whether the build splits, None when a triangle
    within the margin could tip a part over the leaf size."""
    c = classes(verts, idx, lights)
    lo_a, lo_b = int(c["occluder"].sum()), int(c["parked"].sum())
    if lo_a > K_LEAF_MAX and lo_b > K_LEAF_MAX:
        return True
    if lo_a + c["unsure"] <= K_LEAF_MAX or lo_b + c["unsure"] <= K_LEAF_MAX:
        return False
    return None


def check_two_trees(pt, rt, builder, verts, idx, lights, tag):
    """Item 1 of the feature's checks on the mesh `rt` holds: a valid two-tree build in the host
    build's layout whose parts follow the restated rules.  Returns (meshInfo, meshTree)."""
    info, tree = rt.meshInfo(), rt.meshTree()
    n = len(idx)
    assert info["builder"] == builder_id(pt, builder), (tag, info)
    assert info["n_nodes4_shadow"] > 0, (tag, info)
    assert info["cone_root"] == info["n_nodes4"] + 1, (tag, info)
    assert 0 < info["n_tris_cone"] < info["n_tris_tree"] <= info["n_tris"] == n, (tag, info)
    root = tree["shadow_root"]
    assert root == tree["n_nodes4"] == info["n_nodes4"] and tree["n_nodes4_shadow"] == info["n_nodes4_shadow"]
    assert tree["compressed"] == 1 and tree["n_records"] == 2 * n
    tr.check_fallback(tree, tag)
    rep = dict(n_hit=info["n_tris_tree"], depth4=info["depth4"], stack4=info["stack4"])
    got0 = tr.check_tree(verts, idx, tree, 0, builder="host", reported=rep)
    got = tr.check_tree(verts, idx, tree, root, builder="host", reported=dict(n_hit=info["n_tris_tree"]))
    assert got["n_hit"] == got0["n_hit"] == info["n_tris_tree"]
    # the root: exactly two children, A then B
    links = tree["nodes4q"][root, 12:16].view(np.int32)
    assert links.tolist() == [root + 1, root + 2, tr.RT_EMPTY_CHILD, tr.RT_EMPTY_CHILD], (tag, links)
    lv_a, slots_a = lh.subtree(tree, root + 1)
    lv_b, slots_b = lh.subtree(tree, root + 2)
    for d, (la, lb) in enumerate(zip(lv_a, lv_b)):  # A's nodes before B's on every level
        assert la.max() < lb.min(), (tag, d)
    for d, la in enumerate(lv_a):
        la = np.sort(la)  # (within a level part the device collapse numbers the nodes in any order)
        assert np.array_equal(la, np.arange(la[0], la[0] + len(la))), f"{tag}: level {d} of A is not an index range"
    # A's records are the slots [0, n_cone) of the shadow tree's half, B's the slots up to n_hit
    n_cone, n_hit = info["n_tris_cone"], info["n_tris_tree"]
    assert np.array_equal(np.sort(slots_a), n + np.arange(n_cone)), tag
    assert np.array_equal(np.sort(slots_b), n + np.arange(n_cone, n_hit)), tag
    orig = tree["tris"][:, 3].view(np.int32)
    in_a, in_b = orig[slots_a], orig[slots_b]
    kept0 = orig[:n_hit]
    assert np.array_equal(np.sort(np.concatenate([in_a, in_b])), np.sort(kept0)), f"{tag}: A and B are not the kept set"
    # the left-out records follow in triangle order, in both halves
    tail = orig[n_hit:n]
    assert np.array_equal(tail, np.sort(tail)) and np.array_equal(orig[n + n_hit:], tail), tag
    # the rules, restated
    c = classes(verts, idx, lights)
    wrong_b, wrong_a = in_b[c["occluder"][in_b]], in_a[c["parked"][in_a]]
    assert len(wrong_b) == 0 and len(wrong_a) == 0, (tag, wrong_b[:5], wrong_a[:5])
    assert not c["kept"][tail].any() and not c["out"][kept0].any(), tag
    return info, tree


def check_one_tree(pt, rt, builder, verts, idx, tag, culled=True):
    """The build without a split: one tree (culled by the never-hit rule, the verifier's "host"
    mode), no shadow nodes, no cone."""
    info, tree = rt.meshInfo(), rt.meshTree()
    assert info["builder"] == builder_id(pt, builder), (tag, info)
    assert (info["n_nodes4_shadow"], info["cone_root"], info["n_tris_cone"]) == (0, 0, 0), (tag, info)
    assert tree["n_nodes4_shadow"] == 0 and tree["shadow_root"] == 0 and tree["n_records"] == len(idx)
    tr.check_fallback(tree, tag)
    rep = dict(n_hit=info["n_tris_tree"], depth4=info["depth4"], stack4=info["stack4"])
    tr.check_tree(verts, idx, tree, 0, builder="host" if culled else "gpu", reported=rep)
    return info, tree


def _canon(tree, root):
    """The tree at `root` in walk order, free of node numbering: per node its compressed words
    0-11 (boxes, meta, normal box), the kinds of its links, and its leaves' triangles."""
    q = tree["nodes4q"]
    orig = tree["tris"][:, 3].view(np.int32)
    out, todo = [], [root]
    while todo:
        i = todo.pop()
        links = q[i, 12:16].view(np.int32).tolist()
        kinds, leaves = [], []
        for c in links:
            if c == tr.RT_EMPTY_CHILD:
                kinds.append("e")
            elif c >= 0:
                kinds.append("i")
                todo.append(c)
            else:
                enc = ~c
                kinds.append("l")
                leaves.append(orig[(enc >> 3):(enc >> 3) + (enc & 7) + 1].tolist())
        out.append((q[i, :12].tobytes(), tuple(kinds), tuple(map(tuple, leaves))))
    return out


def same_trees(a, b, tag):
    """Two builds of one input: identical but for the order of the nodes within a level part
    (k_collapse hands node indices out with an atomic), compared structurally from both roots."""
    for k in ("n_nodes4", "n_nodes4_shadow", "shadow_root", "n_records", "compressed"):
        assert a[k] == b[k], (tag, k)
    assert _canon(a, 0) == _canon(b, 0), f"{tag}: closest-hit tree"
    if a["n_nodes4_shadow"]:
        assert _canon(a, a["shadow_root"]) == _canon(b, b["shadow_root"]), f"{tag}: shadow tree"
