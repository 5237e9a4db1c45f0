"""The PLOC builder on the GPU (rt_build_gpu.hip k_ploc_*): its trees read back
(RayTracer.meshTree) against the tree verifier (tests/tree_ref.py) and, node for node, against the
numpy restatement of the rule (tests/ploc_ref.py); the traversals against the CPU oracle's linear
loop; the tree's cost against the LBVH tree's; the round cap; refit and rebuild; the builders mixed
on one context; the command line."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import ploc_cases as pc
import ploc_ref as pr
import refit_ref as rr
import tree_cases as tc
import tree_ref as tr
from conftest import ROOT, bits

pytestmark = pytest.mark.gpu

TRAVERSALS = ("linear", "bvh", "bvh4f")
CASE = "tris_64x48_sr1"


@pytest.fixture(scope="module")
def ctx(pt, tracer):
    rt = pt.RayTracer(0)
    rt.setSpheres(pt.scenes.ply_scene())
    yield rt
    rt.close()


def build(rt, pt, builder, verts, idx):
    """setMesh under `builder`: meshInfo names it, and the read-back tree passes the verifier's rules
    for a device-built tree (one tree, every triangle kept) with meshInfo's own figures."""
    rt.setBuilder(builder)
    rt.setTraversal("bvh")
    rt.setMesh(verts, idx)
    info, tree = rt.meshInfo(), rt.meshTree()
    assert info["builder"] == {"gpu": pt._abi.RT_BUILD_GPU, "ploc": pt._abi.RT_BUILD_GPU_PLOC}[builder]
    assert (tree["n_nodes4"], tree["n_nodes4_shadow"]) == (info["n_nodes4"], 0)
    assert info["n_tris_tree"] == len(idx)
    tr.check_fallback(tree, f"{builder} tree")
    rep = dict(n_hit=info["n_tris_tree"], depth4=info["depth4"], stack4=info["stack4"])
    tr.check_tree(verts, idx, tree, 0, builder="gpu", reported=rep)
    return info, tree


def rays_equal(rt, rays, exp, what):
    exp_i, exp_t, exp_o = exp
    for trav in TRAVERSALS:
        rt.setTraversal(trav)
        gi, gt = rt.traceRays(rays)
        go, _ = rt.traceRays(rays, any_hit=True)
        np.testing.assert_array_equal(gi, exp_i, err_msg=f"{what} {trav}: closest index")
        np.testing.assert_array_equal(bits(gt), bits(exp_t), err_msg=f"{what} {trav}: closest t")
        np.testing.assert_array_equal(go != 0, exp_o != 0, err_msg=f"{what} {trav}: occlusion")
    rt.setTraversal("bvh")


# ---- 1. validity and ray parity ------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.MESHES)
def test_trees_and_rays(name, ctx, pt, oracle):
    verts, idx = pc.make(name, pt.scenes)
    info, tree = build(ctx, pt, "ploc", verts, idx)
    if name in tc.NOT_ENCODABLE:
        assert tree["compressed"] == 0 and tree["nodes4q"] is None
    else:
        assert tree["compressed"] == 1
    if name == "det_bound":  # normal boxes decide results here
        assert ((tree["nodes4q"][:, 10] >> 24) != 255).mean() > 0.5
    rays, exp = tc.queries(oracle, verts, idx, tree, pt._abi.RAY_DTYPE)
    if name in tc.NOTHING_HITTABLE:
        assert not (exp[0] >= 0).any() and not exp[2].any()
    else:  # the ray set hits, occludes and misses often enough by itself
        assert len(rays) >= 2400 and (exp[0] >= 0).mean() >= 0.25
        assert (exp[2] != 0).mean() >= 0.10 and (exp[2] == 0).mean() >= 0.10
    rays_equal(ctx, rays, exp, f"{name} ploc")


# ---- 2. the device against the restatement -------------------------------------------------------
@pytest.mark.parametrize("builder", ["ploc", "gpu"])
@pytest.mark.parametrize("name", pc.MESHES)
def test_device_tree_is_the_restatements(name, builder, ctx, pt):
    """Slot by slot from the root: kind, the child box's bits, a leaf's triangles in order.  Under
    "gpu" this is the radix tree and the shared collapse: the anchor of the restatement."""
    verts, idx = pc.make(name, pt.scenes)
    _, tree = build(ctx, pt, builder, verts, idx)
    pr.same_tree4(pr.as_tree4(tree), pc.ref_tree(name, pt.scenes, builder), f"{name} {builder}")


# ---- 3. quality ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.BETTER + pc.NOT_WORSE)
def test_ploc_tree_costs_less_than_the_lbvh_tree(name, ctx, pt):
    verts, idx = pc.make(name, pt.scenes)
    cost = {b: pr.sah_cost(pr.as_tree4(build(ctx, pt, b, verts, idx)[1])) for b in ("ploc", "gpu")}
    print(f"{name}: sah_cost ploc {cost['ploc']:.6g}, lbvh {cost['gpu']:.6g}, ratio {cost['ploc'] / cost['gpu']:.4f}")
    if name in pc.BETTER:
        assert cost["ploc"] < cost["gpu"]
    else:
        assert cost["ploc"] <= cost["gpu"]


# ---- 4. a counting render ------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["gpu", "ploc"])
def test_counting_render(builder, tracer, pt, golden, golden_meta):
    """The golden progressive sequence on a device-built tree, counting: frame and seeds are the
    fixture's; the traversal's work is printed (DESIGN.md §4.6a records it), not asserted."""
    g, m = golden(CASE), golden_meta["cases"][CASE]
    W, H = m["W"], m["H"]
    t = pt.RayTracer(0)
    try:
        t.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
        t.setCamera(g["camera"])
        t.setSampleRate(m["sample_rate"])
        t.setMaxPathDepth(m["max_depth"])
        t.setNDRange(m["nd_y"])
        t.setBuilder(builder)
        t.setMesh(g["verts"], g["idx"])
        assert t.meshInfo()["builder"] == {"gpu": pt._abi.RT_BUILD_GPU, "ploc": pt._abi.RT_BUILD_GPU_PLOC}[builder]
        t.setSeeds(m["Wpad"], m["Hpad"], g["seeds_in"])
        t.setCounting(True)
        frame = np.zeros(W * H * 4, np.float32)
        for p in range(m["frames"]):
            t.rayTrace(frame, W, H, p, kernel=2)
        tot = t.counterTotals()
        print(f"{CASE} {builder}: nodes_visited {tot['nodes_visited']}, leaves_visited {tot['leaves_visited']}, "
              f"tris_tested {tot['tris_tested']}, rays {tot['rays_closest']} + {tot['rays_shadow']}")
        np.testing.assert_array_equal(bits(frame), bits(g["frames"][-1]), err_msg="frame")
        np.testing.assert_array_equal(t.getSeeds(), g["seeds_out"], err_msg="seeds")
    finally:
        t.close()


# ---- 5. the cap ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.CAP_MESHES)
def test_round_cap(name, ctx, pt, oracle):
    """The shrinking strip needs the halving rounds (tests/test_ploc_host.py has the count); the
    identical triangles pair as buddies.  Both build, verify, equal the restatement and trace."""
    verts, idx = pc.make(name, pt.scenes)
    _, tree = build(ctx, pt, "ploc", verts, idx)
    pr.same_tree4(pr.as_tree4(tree), pc.ref_tree(name, pt.scenes, "ploc"), name)
    rays, _ = tc.base_rays(verts, idx, tc.tree_planes(tree), pt._abi.RAY_DTYPE)
    rays = rays[np.linspace(0, len(rays) - 1, 480).astype(np.int64)]
    ci, ct = oracle.closest_hits(rays, verts, idx)
    assert (ci >= 0).mean() >= 0.25
    rays_equal(ctx, rays, (ci, ct, oracle.any_hits(rays, verts, idx)), name)


# ---- 6. refit and rebuild ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere257", "sphere2000"])
def test_refit(name, ctx, pt, oracle):
    verts, idx = pc.make(name, pt.scenes)
    info, before = build(ctx, pt, "ploc", verts, idx)
    up = ctx.updateMesh(verts)  # unchanged vertices: the tree word for word
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REFIT, pt._abi.RT_REFIT_OK), up
    assert up["area_ratio"] == 1.0
    same = ctx.meshTree()
    for k in ("nodes4", "nodes4q", "tris"):
        np.testing.assert_array_equal(bits(same[k]), bits(before[k]), err_msg=f"identity: {k}")
    nv = rr.wobble(verts)
    up = ctx.updateMesh(nv)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REFIT, pt._abi.RT_REFIT_OK), up
    assert ctx.meshInfo() == info
    tree = ctx.meshTree()
    rep = dict(n_hit=info["n_tris_tree"], depth4=info["depth4"], stack4=info["stack4"])
    tr.check_fallback(tree, "ploc tree, refitted")
    tr.check_tree(nv, idx, tree, 0, builder="gpu", reported=rep)
    rays, exp = tc.queries(oracle, nv, idx, tree, pt._abi.RAY_DTYPE)
    rays_equal(ctx, rays, exp, f"{name} wobble")
    want = rr.half_area_sum(tree["nodes4"]) / rr.half_area_sum(before["nodes4"])
    print(f"{name} wobble ploc: area_ratio {up['area_ratio']:.9g} (numpy {want:.9g}), refit {up['ms']:.3f} ms")
    assert abs(up["area_ratio"] - want) <= 1e-6 * want


def test_rebuild_keeps_the_builder(ctx, pt):
    """Scaled until no compressed node can hold it: rt_update_mesh rebuilds, with the mesh's own
    builder, whatever the context's builder for the next mesh has become."""
    verts, idx = pc.make("sphere2000", pt.scenes)
    big = rr.scale(verts, 10000.0)
    _, tree = build(ctx, pt, "ploc", verts, idx)
    assert tree["compressed"] == 1
    ctx.setBuilder("host")
    up = ctx.updateMesh(big)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REBUILT, pt._abi.RT_REFIT_ENCODING), up
    info, tree = ctx.meshInfo(), ctx.meshTree()
    assert info["builder"] == pt._abi.RT_BUILD_GPU_PLOC
    assert tree["compressed"] == 0 and tree["nodes4q"] is None and tree["n_nodes4_shadow"] == 0
    tr.check_tree(big, idx, tree, 0, builder="gpu")
    pr.same_tree4(pr.as_tree4(tree), pr.build(big, idx, "ploc"), "rebuilt")


# ---- 7. the builders mixed on one context --------------------------------------------------------
def test_builders_in_turn(pt, tracer, oracle):
    rt = pt.RayTracer(0)
    try:
        rt.setSpheres(pt.scenes.ply_scene())
        meshes = [("host", "sphere1000"), ("ploc", "sphere2000"), ("gpu", "sphere257"), ("ploc", "one_centre600")]
        for builder, name in meshes:
            verts, idx = pc.make(name, pt.scenes)
            rt.setBuilder(builder)
            rt.setTraversal("bvh")
            rt.setMesh(verts, idx)
            info, tree = rt.meshInfo(), rt.meshTree()
            want = {"host": pt._abi.RT_BUILD_HOST, "gpu": pt._abi.RT_BUILD_GPU, "ploc": pt._abi.RT_BUILD_GPU_PLOC}
            assert info["builder"] == want[builder], (builder, name)
            assert (tree["n_nodes4_shadow"] > 0) == (builder == "host")
            rays, exp = tc.queries(oracle, verts, idx, tree, pt._abi.RAY_DTYPE)
            rays_equal(rt, rays, exp, f"{name} {builder}")
    finally:
        rt.close()


def test_unknown_builder_is_refused(ctx, pt):
    assert ctx._lib.rt_set_builder(ctx._h, 3) == pt._abi.RT_ERR_ARG
    with pytest.raises(KeyError):
        ctx.setBuilder("sah")


# ---- 8. the command line -------------------------------------------------------------------------
def test_cli_builder(tracer, tmp_path):
    exe = str(ROOT / "pathtracer.cl_amd" / "rt_render")
    out = {}
    for b in ("host", "gpu", "ploc"):
        raw = tmp_path / f"{b}.f32"
        subprocess.run([exe, "--mesh", "2000", "--width", "64", "--height", "48", "--frames", "2", "--builder", b,
                        "--raw", str(raw)], check=True, timeout=120)
        out[b] = raw.read_bytes()
    assert len(out["host"]) == 64 * 48 * 16 and np.frombuffer(out["host"], np.float32).any()
    assert out["ploc"] == out["host"] and out["gpu"] == out["host"]
    r = subprocess.run([exe, "--mesh", "2000", "--builder", "sah"], capture_output=True, timeout=120)
    assert r.returncode == 2
