"""The lights' cone split of the host builder's shadow tree (rt_bvh.cpp never_occludes, DESIGN.md
§4.2), checked without a GPU: tests/cpp/host_cone_dump builds the trees with the lights' radii;
the whole shadow tree still passes tests/tree_ref.py, subtree A and subtree B together hold the
kept triangles, A's levels are index ranges, the builder's rule agrees with its float64
restatement here, and no ray from a triangle of B to a light is accepted by the reference's
triangle test (the oracle's batch form of tests/devkat.py)."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import devkat
import tree_cases as tc
import tree_ref as tr
from conftest import ROOT

F32 = np.float32
SMALL = float(F32(1e-4))
PLY_LIGHT = (0.0, 4.0, 2.0, 0.5)  # scenes.ply_scene's light
MESH_CENTER = (0.0, -2.2, 0.0)
# name -> (mesh, lights [(x, y, z, r)])
SPLIT_CASES = {
    "mesh20000": (("make_mesh", 20000, 0.38), [PLY_LIGHT]),
    "mesh5000": (("make_mesh", 5000, 0.19), [PLY_LIGHT]),
    "mesh5000_two_lights": (("make_mesh", 5000, 0.19), [PLY_LIGHT, (0.0, -8.4, -2.0, 0.5)]),
    # a light whose sphere holds the top of the mesh
    "mesh5000_light_inside": (("make_mesh", 5000, 0.19), [(0.0, -2.2 + 0.19, 0.0, 0.08)]),
}
RULE_MARGIN = 1e-6  # relative: the builder (products and square roots) and this restatement (asin, acos, cos)
# round differently by some 1e-15, and may disagree only on a triangle nearer the threshold than this


@pytest.fixture(scope="module")
def tools():
    subprocess.run(["make", "-s", "-C", str(ROOT / "tests" / "cpp"), "host_tree_dump"], check=True)
    subprocess.run(["make", "-s", "-C", str(ROOT / "tests" / "cpp"), "-f", "light_cone.mk"], check=True)
    return ROOT / "tests" / "cpp" / "host_tree_dump", ROOT / "tests" / "cpp" / "host_cone_dump"


@pytest.fixture(scope="module")
def host(pt, oracle):
    return devkat.Host(pt._abi, oracle)


def dump(tool, tmp, verts, idx, lights, out="tree.bin"):
    np.ascontiguousarray(verts, F32).tofile(tmp / "verts.f32")
    np.ascontiguousarray(idx, np.int32).tofile(tmp / "idx.i32")
    np.ascontiguousarray(lights, F32).tofile(tmp / "lights.f32")
    r = subprocess.run([str(tool), str(tmp / "verts.f32"), str(tmp / "idx.i32"), str(tmp / out), str(tmp / "lights.f32")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tree = tr.read_dump(tmp / out)
    head = np.fromfile(tmp / out, np.uint32, 16)
    tree["cone_root"], tree["n_cone"] = int(head[13]), int(head[14])
    return tree


def subtree(tree, node):
    """The levels of the subtree at `node` as lists of node indices, and the record slots of its leaves."""
    L = tree["nodes4q"][:, 12:16].view(np.int32)
    levels, slots = [], []
    cur = np.array([node], np.int64)
    while len(cur):
        levels.append(cur)
        c = L[cur].reshape(-1)
        c = c[c != tr.RT_EMPTY_CHILD]
        for enc in (~c[c < 0]).tolist():
            slots.extend(range(enc >> 3, (enc >> 3) + (enc & 7) + 1))
        cur = c[c >= 0].astype(np.int64)
    return levels, np.array(slots, np.int64)


def rule_ratio(verts, idx, lights):
    """The value never_occludes compares, over its threshold, per triangle: the largest over the
    lights of 1.001 (|N| maxcos + 16 u |e1|_1 |e2|_1) / (0.999 * 1e-4f), in float64 on the float
    records (v0, e1, e2).  Below 1: the triangle is set aside."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    p = v[np.ascontiguousarray(idx, np.int32).reshape(-1, 3)]
    v0 = p[:, 0].astype(np.float64)
    e1, e2 = (p[:, 1] - p[:, 0]).astype(np.float64), (p[:, 2] - p[:, 0]).astype(np.float64)
    n = np.cross(e2, e1)
    cr = np.linalg.norm(n, axis=1)
    l1l2 = np.abs(e1).sum(axis=1) * np.abs(e2).sum(axis=1)
    cen = v0 + (e1 + e2) / 3.0
    corners = np.stack([v0, v0 + e1, v0 + e2], axis=1)
    rt = np.linalg.norm(corners - cen[:, None, :], axis=2).max(axis=1)
    worst = np.zeros(len(p))
    for x, y, z, r in lights:
        C, R = np.array([x, y, z], F32).astype(np.float64), float(F32(r))
        Lv = C - cen
        dist = np.linalg.norm(Lv, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            theta = np.arcsin(np.minimum(1.0, (1.001 * R + rt) / dist))
            phi = np.arccos(np.minimum(1.0, np.abs((Lv * n).sum(axis=1)) / (dist * cr)))
        theta = np.where(np.isfinite(theta), theta, np.pi / 2)
        phi = np.where(np.isfinite(phi), phi, 0.0)
        maxcos = np.cos(np.maximum(0.0, phi - theta))
        worst = np.maximum(worst, 1.001 * (cr * maxcos + 16.0 * tr.U * l1l2) / (0.999 * SMALL))
    return worst


def light_points(P, C, R, nrm, n_ring=32, n_fib=136):
    """Points of the light's ball for the surface points P [m, 3]: per point the two silhouette points
    that turn the ray furthest toward +-N, a ring of silhouette points, and (shared) points on and
    inside the sphere.  Returns [m, k, 3] float64, every point within R of C."""
    l = C - P
    dist = np.linalg.norm(l, axis=1, keepdims=True)
    l = l / dist
    sa = np.minimum(1.0, R / dist)  # the tangent cone's half-angle
    ca = np.sqrt(1.0 - sa * sa)
    m1 = nrm - (nrm * l).sum(axis=1, keepdims=True) * l
    ln = np.linalg.norm(m1, axis=1, keepdims=True)
    fallback = np.cross(l, np.array([1.0, 0.0, 0.0]))
    fallback = np.where(np.linalg.norm(fallback, axis=1, keepdims=True) < 1e-3, np.cross(l, np.array([0.0, 1.0, 0.0])), fallback)
    m1 = np.where(ln > 1e-12, m1 / np.maximum(ln, 1e-300), fallback / np.linalg.norm(fallback, axis=1, keepdims=True))
    m2 = np.cross(l, m1)
    az = np.concatenate([[0.0, np.pi], 2.0 * np.pi * (np.arange(n_ring) + 0.5) / n_ring])
    m = np.cos(az)[None, :, None] * m1[:, None, :] + np.sin(az)[None, :, None] * m2[:, None, :]
    shrink = 1.0 - 1e-6  # inside the ball after the float32 rounding of the ray's direction
    sil = C + shrink * R * (-sa[:, None, :] * l[:, None, :] + ca[:, None, :] * m)
    k = np.arange(n_fib) + 0.5
    zf = 1.0 - 2.0 * k / n_fib
    rf = np.sqrt(1.0 - zf * zf)
    af = np.pi * (1.0 + 5.0 ** 0.5) * k
    fib = np.stack([rf * np.cos(af), rf * np.sin(af), zf], axis=1)
    scale = np.where(np.arange(n_fib) % 3 == 2, 0.5, shrink)[:, None]  # a third of them inside
    shared = C + R * scale * fib
    return np.concatenate([sil, np.broadcast_to(shared, (len(P),) + shared.shape)], axis=1)


BARY = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5], [1 / 3, 1 / 3, 1 / 3],
                 [.8, .1, .1], [.1, .8, .1], [.1, .1, .8], [.45, .45, .1], [.2, .3, .5]])


def accepted_rays(host, abi, verts, idx, tris, lights, chunk=512):
    """Rays from 12 points of each triangle of `tris` (vertices, edge midpoints, interior) to 170 points
    of every light's ball, each given to the reference's triangle test with its direction and an
    origin one unit before the centroid — det depends on the direction and the edges alone, and the
    centroid keeps u, v and t well inside their ranges, so the test accepts exactly where
    |det| >= 1e-4 as it evaluates det.  Returns (accepted rays, rays, largest float64 |det|)."""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    p = v[np.ascontiguousarray(idx, np.int32).reshape(-1, 3)[tris]]
    rec = np.concatenate([p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]], axis=1).astype(F32)  # v0, e1, e2
    n_acc = n_rays = 0
    worst = 0.0
    for s in range(0, len(tris), chunk):
        r9 = rec[s:s + chunk]
        v0, e1, e2 = (r9[:, 0:3].astype(np.float64), r9[:, 3:6].astype(np.float64), r9[:, 6:9].astype(np.float64))
        nrm = np.cross(e2, e1)
        cen = v0 + (e1 + e2) / 3.0
        pts = v0[:, None, :] + BARY[None, :, 1:2] * e1[:, None, :] + BARY[None, :, 2:3] * e2[:, None, :]  # [m, 12, 3]
        m, nb = pts.shape[:2]
        for x, y, z, r in lights:
            C, R = np.array([x, y, z], F32).astype(np.float64), float(F32(r))
            S = light_points(pts.reshape(-1, 3), C, R, np.repeat(nrm, nb, axis=0))  # [m * 12, k, 3]
            k = S.shape[1]
            d = S - pts.reshape(-1, 1, 3)
            d = (d / np.linalg.norm(d, axis=2, keepdims=True)).astype(F32).reshape(m, nb * k, 3)
            rays = np.zeros(m * nb * k, abi.RAY_DTYPE)
            rays["d"] = d.reshape(-1, 3)
            rays["o"] = (cen[:, None, :] - d.astype(np.float64)).astype(F32).reshape(-1, 3)
            rays["tmin"] = F32(1e-4)
            rays["tmax"] = F32(np.inf)
            rays["propagation"] = 1.0
            res = host.mt_test(rays, np.repeat(r9, nb * k, axis=0))
            n_acc += int((res["hit"] != 0).sum()) + int((res["hit_any"] != 0).sum())
            n_rays += len(rays)
            worst = max(worst, float(np.abs((d.astype(np.float64) * nrm[:, None, :]).sum(axis=2)).max()))
    return n_acc, n_rays, worst


def make_case(name, pt):
    if name in SPLIT_CASES:
        (_, n, r), lights = SPLIT_CASES[name]
        verts, idx = pt.scenes.make_mesh(n, MESH_CENTER, r)
        return verts, idx, lights
    verts, idx = tc.make(name, pt.scenes)
    return verts, idx, [PLY_LIGHT]


@pytest.mark.parametrize("name", list(SPLIT_CASES) + tc.MESHES)
def test_cone_split(name, pt, tools, host, tmp_path):
    tree_tool, cone_tool = tools
    verts, idx, lights = make_case(name, pt)
    tree = dump(cone_tool, tmp_path, verts, idx, np.array(lights, F32))
    n = len(idx)
    if name in tc.NOT_ENCODABLE:
        assert tree["n_nodes4_shadow"] == 0 and tree["cone_root"] == 0
        return
    root = tree["shadow_root"]
    assert root == tree["n_nodes4"] and tree["n_nodes4_shadow"] > 0
    # the whole shadow tree: every invariant of today's, with the builder's own depth4 / stack4
    got = tr.check_tree(verts, idx, tree, root, builder="host", reported=tree["reported"][root])
    got0 = tr.check_tree(verts, idx, tree, 0, builder="host", reported=tree["reported"][0])
    assert got["n_hit"] == got0["n_hit"]
    ratio = rule_ratio(verts, idx, lights)
    if tree["cone_root"] == 0:  # no split: today's build, bit for bit
        assert name not in SPLIT_CASES
        centres = np.array(lights, F32)[:, :3]
        today = dump(tree_tool, tmp_path, verts, idx, centres, out="today.bin")
        for k in ("nodes4", "nodes4q", "tris", "nodes4_shadow"):
            assert np.array_equal(tree[k].view(np.uint32), today[k].view(np.uint32)), k
        kept = tree["tris"][n:n + got["n_hit"], 3].view(np.int32)
        aside = int((ratio[kept] < 1.0 - RULE_MARGIN).sum())
        assert aside <= tr.RT_LEAF_MAX or got["n_hit"] - aside <= tr.RT_LEAF_MAX, (aside, got["n_hit"])
        return
    # the root: exactly two children, A then B
    links = tree["nodes4q"][root, 12:16].view(np.int32)
    assert tree["cone_root"] == root + 1
    assert links.tolist() == [root + 1, root + 2, tr.RT_EMPTY_CHILD, tr.RT_EMPTY_CHILD], links
    lv_a, slots_a = subtree(tree, root + 1)
    lv_b, slots_b = subtree(tree, root + 2)
    for d, (la, lb) in enumerate(zip(lv_a, lv_b)):  # A's nodes before B's on every level
        assert la.max() < lb.min(), d
    for d, la in enumerate(lv_a):
        assert np.array_equal(la, np.arange(la[0], la[0] + len(la))), f"level {d} of A is not an index range"
    orig = tree["tris"][:, 3].view(np.int32)
    in_a, in_b = orig[slots_a], orig[slots_b]
    assert len(in_a) == tree["n_cone"]
    kept0 = orig[:got0["n_hit"]]  # the closest-hit tree's kept set
    assert len(in_a) + len(in_b) == got["n_hit"]
    assert np.array_equal(np.sort(np.concatenate([in_a, in_b])), np.sort(kept0))
    print(f"{name}: {len(in_a)} of {got['n_hit']} possible occluders, A {sum(map(len, lv_a))} nodes in {len(lv_a)} "
          f"levels, B {sum(map(len, lv_b))} nodes")
    if name in SPLIT_CASES and len(lights) == 1 and lights[0] == PLY_LIGHT:  # the cases' precondition
        assert 4 * len(in_a) >= got["n_hit"] and 4 * len(in_b) >= got["n_hit"], (len(in_a), len(in_b))
    # the rule, restated
    wrong_b = in_b[ratio[in_b] >= 1.0 + RULE_MARGIN]
    wrong_a = in_a[ratio[in_a] < 1.0 - RULE_MARGIN]
    assert len(wrong_b) == 0 and len(wrong_a) == 0, (wrong_b[:5], wrong_a[:5])
    if name == "mesh5000_light_inside":  # the triangles the inflated sphere reaches stay in A
        v = np.ascontiguousarray(verts, F32).reshape(-1, 3)[idx].astype(np.float64)
        cen = v.mean(axis=1)
        rt = np.linalg.norm(v - cen[:, None, :], axis=2).max(axis=1)
        x, y, z, r = lights[0]
        reached = np.linalg.norm(cen - np.array([x, y, z]), axis=1) <= r + rt
        reached_kept = np.intersect1d(np.flatnonzero(reached), kept0)
        assert len(reached_kept) > 50 and np.isin(reached_kept, in_a).all()
        assert len(in_b) > 100
    # no ray from a triangle of B to a light is accepted
    n_acc, n_rays, worst = accepted_rays(host, pt._abi, verts, idx, in_b, lights)
    print(f"{name}: {n_rays} rays from {len(in_b)} triangles of B, largest float64 |det| {worst:.4e}")
    assert n_rays >= 2000 * len(in_b) * len(lights)
    assert n_acc == 0, f"{n_acc} of {n_rays} rays from B were accepted"
    assert worst < SMALL
    # the same rays find occluders in A (the check can fail): a sample of A is accepted somewhere
    sample = in_a[:: max(1, len(in_a) // 64)]
    acc_a, _, _ = accepted_rays(host, pt._abi, verts, idx, sample, lights)
    assert acc_a > 0
