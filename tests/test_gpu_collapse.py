"""RT_COLLAPSE_SAH on the GPU (rt_build_gpu.hip k_collapse_cost / k_collapse_sah):
the device trees read back (RayTracer.meshTree) against the tree verifier (tests/tree_ref.py) and,
node for node, against the numpy restatement of the rule (tests/collapse_ref.py); the same rays and
frames as under the greedy collapse; the traversal's steps counted under both; a moving mesh; the
interface."""
from __future__ import annotations

import ctypes
import subprocess

import numpy as np
import pytest

import build_lights_cases as bl
import collapse_cases as cc
import collapse_ref as cr
import ploc_cases as pc
import ploc_ref as pr
import refit_ref as rr
import test_light_cone_host as lh
import tree_cases as tc
import tree_ref as tr
from conftest import ROOT, bits

pytestmark = pytest.mark.gpu

TRAVERSALS = ("linear", "bvh", "bvh4f")
CASE = "tris_64x48_sr1"
RT_STACK_DEPTH = 20  # rt_traverse.h: deeper stacks walk the spill tail


@pytest.fixture(scope="module")
def ctx(pt, tracer):
    rt = pt.RayTracer(0)
    rt.setSpheres(pt.scenes.ply_scene())
    yield rt
    rt.close()


def build(rt, pt, builder, verts, idx, mode="sah"):
    """setMesh under `builder` and `mode` (no build options): meshInfo names both, and the read-back
    tree passes the verifier's rules for a device-built tree, compressed and full precision, with
    meshInfo's own figures."""
    rt.setBuilder(builder)
    rt.setBuildOptions(False)
    rt.setCollapse(mode)
    rt.setTraversal("bvh")
    rt.setMesh(verts, idx)
    info, tree = rt.meshInfo(), rt.meshTree()
    assert info["builder"] == bl.builder_id(pt, builder)
    assert info["collapse"] == {"greedy": pt._abi.RT_COLLAPSE_GREEDY, "sah": pt._abi.RT_COLLAPSE_SAH}[mode]
    assert (tree["n_nodes4"], tree["n_nodes4_shadow"]) == (info["n_nodes4"], 0)
    assert info["n_tris_tree"] == len(idx)
    tr.check_fallback(tree, f"{builder} {mode} tree")
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


# ---- 1, 2. the device trees are the restatement's, and valid ---------------------------------------
@pytest.mark.parametrize("builder", cc.BUILDERS)
@pytest.mark.parametrize("name", cc.DEVICE_MESHES)
def test_device_tree_is_the_restatements(name, builder, ctx, pt):
    """Slot by slot from the root: kind, the child box's bits, a leaf's triangles in order."""
    verts, idx = pc.make(name, pt.scenes)
    info, tree = build(ctx, pt, builder, verts, idx)
    if name in tc.NOT_ENCODABLE:  # the full-precision fall-back
        assert tree["compressed"] == 0 and tree["nodes4q"] is None
    else:
        assert tree["compressed"] == 1
    ref = cc.ref_tree(name, pt.scenes, builder)
    pr.same_tree4(pr.as_tree4(tree), ref, f"{name} {builder} sah")
    assert (info["depth4"], info["stack4"]) == cr.depth_stack(ref)
    cr.check_tree4(pr.as_tree4(tree), len(idx))


@pytest.mark.parametrize("builder", cc.BUILDERS)
@pytest.mark.parametrize("name", ["mesh5000", "det_bound"])
def test_two_trees_are_the_restatements(name, builder, pt, tracer):
    """RT_BUILD_OPT_LIGHTS and the mode together: the closest-hit tree is the restatement's over
    the kept triangles, and the shadow tree's parts A and B are the restatement's over their own
    triangles, each collapsed on its own under the root of two."""
    verts, idx, lights = lh.make_case(name, pt)
    assert bl.expect_split(verts, idx, lights) is True, "precondition"
    rt = bl.context(pt, bl.spheres_for(pt.scenes, lights), builder)
    try:
        rt.setCollapse("sah")
        rt.setMesh(verts, idx)
        info, tree = bl.check_two_trees(pt, rt, builder, verts, idx, lights, f"{name} {builder} sah")
        assert info["collapse"] == pt._abi.RT_COLLAPSE_SAH
        n, n_cone, n_hit = len(idx), info["n_tris_cone"], info["n_tris_tree"]
        orig = tree["tris"][:, 3].view(np.int32)
        in_a, in_b = np.sort(orig[n:n + n_cone]), np.sort(orig[n + n_cone:n + n_hit])
        kept = np.concatenate([in_a, in_b])  # the build's list: the classes in turn, each in triangle order
        t0 = pr.as_tree4(tree)
        t0["orig"] = t0["orig"][:n]
        pr.same_tree4(t0, cr.build(verts, idx, builder, sub=kept), f"{name} {builder}: closest-hit tree")
        root = tree["shadow_root"]
        cr.same_links(tree, root + 1, cr.build(verts, idx, builder, sub=in_a), n, f"{name} {builder}: A")
        cr.same_links(tree, root + 2, cr.build(verts, idx, builder, sub=in_b), n, f"{name} {builder}: B")
    finally:
        rt.close()


# ---- 3. the same results ---------------------------------------------------------------------------
def golden_render(pt, g, m, builder, lights, mode):
    """The golden progressive sequence, counting: (last frame, seeds, counter totals, meshInfo)."""
    t = pt.RayTracer(0)
    try:
        t.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
        t.setCamera(g["camera"])
        t.setSampleRate(m["sample_rate"])
        t.setMaxPathDepth(m["max_depth"])
        t.setNDRange(m["nd_y"])
        t.setBuilder(builder)
        t.setBuildOptions(lights)
        t.setCollapse(mode)
        t.setMesh(g["verts"], g["idx"])
        info = t.meshInfo()
        t.setSeeds(m["Wpad"], m["Hpad"], g["seeds_in"])
        t.setCounting(True)
        frame = np.zeros(m["W"] * m["H"] * 4, np.float32)
        for p in range(m["frames"]):
            t.rayTrace(frame, m["W"], m["H"], p, kernel=2)
        return frame, t.getSeeds(), t.counterTotals(), info
    finally:
        t.close()


@pytest.mark.parametrize("lights", [False, True])
@pytest.mark.parametrize("builder", cc.BUILDERS)
def test_golden_sequence_and_steps(builder, lights, tracer, pt, golden, golden_meta):
    """The golden 64x48 mesh frame (2,000 triangles, 3 progressions), counting, under greedy and
    sah: the fixture's frame and seeds either way.  The traversal's steps (a node visit or a triangle
    test each) are printed, and without the build options asserted: not more under sah."""
    g, m = golden(CASE), golden_meta["cases"][CASE]
    steps = {}
    for mode in ("greedy", "sah"):
        frame, seeds, tot, info = golden_render(pt, g, m, builder, lights, mode)
        assert info["collapse"] == {"greedy": 0, "sah": 1}[mode]
        print(f"{CASE} {builder} lights {'on' if lights else 'off'} {mode}: nodes_visited {tot['nodes_visited']}, "
              f"tris_tested {tot['tris_tested']}, leaves_visited {tot['leaves_visited']}, rays {tot['rays_closest']} + "
              f"{tot['rays_shadow']}; nodes {info['n_nodes4']} + {info['n_nodes4_shadow']}, depth {info['depth4']}, "
              f"stack {info['stack4']}")
        np.testing.assert_array_equal(bits(frame), bits(g["frames"][-1]), err_msg=f"frame, {mode}")
        np.testing.assert_array_equal(seeds, g["seeds_out"], err_msg=f"seeds, {mode}")
        steps[mode] = tot["nodes_visited"] + tot["tris_tested"]
    print(f"{CASE} {builder} lights {'on' if lights else 'off'}: steps greedy {steps['greedy']} -> sah {steps['sah']} "
          f"(ratio {steps['sah'] / steps['greedy']:.4f})")
    if not lights:
        assert steps["sah"] <= steps["greedy"]


@pytest.mark.parametrize("name", ["mixed_scales", "one_centre600"])
def test_rays_through_the_spill_tail(name, ctx, pt, oracle):
    """The PLOC trees of these meshes need 29 to 38 stack entries under sah, beyond RT_STACK_DEPTH:
    closest and any-hit queries give the oracle's answers, which are the greedy tree's."""
    verts, idx = pc.make(name, pt.scenes)
    info, tree = build(ctx, pt, "ploc", verts, idx, "greedy")
    rays, exp = tc.queries(oracle, verts, idx, tree, pt._abi.RAY_DTYPE)
    rays_equal(ctx, rays, exp, f"{name} greedy")
    greedy = [ctx.traceRays(rays), ctx.traceRays(rays, any_hit=True)]
    info, _ = build(ctx, pt, "ploc", verts, idx, "sah")
    assert info["stack4"] > RT_STACK_DEPTH + 4, info
    rays_equal(ctx, rays, exp, f"{name} sah")
    sah = [ctx.traceRays(rays), ctx.traceRays(rays, any_hit=True)]
    np.testing.assert_array_equal(sah[0][0], greedy[0][0])
    np.testing.assert_array_equal(bits(sah[0][1]), bits(greedy[0][1]))
    np.testing.assert_array_equal(sah[1][0] != 0, greedy[1][0] != 0)


# ---- 5. a moving mesh ------------------------------------------------------------------------------
def small_frame(pt, rt, W=32, H=24):
    sc = pt.scenes
    Wp, Hp = sc.padded_dims(W, H)
    rt.setCamera(sc.camera_spherical(W, **sc.PLY_CAMERA))
    rt.setSampleRate(1)
    rt.setMaxPathDepth(6)
    rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp))
    frame = np.zeros(W * H * 4, np.float32)
    rt.rayTrace(frame, W, H, 0, kernel=2)
    return frame, rt.getSeeds()


def test_refit_equals_a_fresh_build(ctx, pt):
    verts, idx = pc.make("sphere2000", pt.scenes)
    nv = rr.wobble(verts)
    info, _ = build(ctx, pt, "ploc", verts, idx)
    up = ctx.updateMesh(nv)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REFIT, pt._abi.RT_REFIT_OK), up
    assert ctx.meshInfo() == info
    tree = ctx.meshTree()
    tr.check_tree(nv, idx, tree, 0, builder="gpu",
                  reported=dict(n_hit=info["n_tris_tree"], depth4=info["depth4"], stack4=info["stack4"]))
    got, got_seeds = small_frame(pt, ctx)
    build(ctx, pt, "ploc", nv, idx)
    want, want_seeds = small_frame(pt, ctx)
    assert want.any()
    np.testing.assert_array_equal(bits(got), bits(want), err_msg="frame")
    np.testing.assert_array_equal(got_seeds, want_seeds, err_msg="seeds")


def test_rebuild_keeps_the_mode(pt, tracer):
    """det_bound under refit_ref.wobble with RT_BUILD_OPT_LIGHTS (tests/test_gpu_refit.py: 75
    left-out triangles become hittable): rebuilt with the mesh's own mode, whatever the context's
    has become since."""
    verts, idx = tc.make("det_bound", pt.scenes)
    nv = rr.wobble(verts)
    rt = bl.context(pt, pt.scenes.ply_scene(), "ploc")
    try:
        rt.setCollapse("sah")
        rt.setMesh(verts, idx)
        assert rt.meshInfo()["collapse"] == pt._abi.RT_COLLAPSE_SAH
        rt.setCollapse("greedy")
        up = rt.updateMesh(nv)
        assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REBUILT, pt._abi.RT_REFIT_NEWLY_HITTABLE), up
        assert rt.getCollapse() == "greedy"
        info, tree = bl.check_two_trees(pt, rt, "ploc", nv, idx, [lh.PLY_LIGHT], "det_bound ploc sah, rebuilt")
        assert info["collapse"] == pt._abi.RT_COLLAPSE_SAH
        n = len(idx)
        orig, n_cone, n_hit = tree["tris"][:, 3].view(np.int32), info["n_tris_cone"], info["n_tris_tree"]
        kept = np.concatenate([np.sort(orig[n:n + n_cone]), np.sort(orig[n + n_cone:n + n_hit])])
        t0 = pr.as_tree4(tree)
        t0["orig"] = t0["orig"][:n]
        pr.same_tree4(t0, cr.build(nv, idx, "ploc", sub=kept), "det_bound rebuilt: closest-hit tree")
    finally:
        rt.close()


# ---- 6. the interface ------------------------------------------------------------------------------
def test_modes(pt, tracer):
    rt = pt.RayTracer(0)
    try:
        A = pt._abi
        assert rt.getCollapse() == "greedy" and A.RT_COLLAPSE_GREEDY == 0 and A.RT_COLLAPSE_SAH == 1
        rt.setCollapse("sah")
        assert rt.getCollapse() == "sah"
        for bad in (-1, 2, 7):
            assert rt._lib.rt_set_collapse(rt._h, bad) == A.RT_ERR_ARG
            assert rt.getCollapse() == "sah", "a refused call leaves the mode as it was"
        assert rt._lib.rt_get_collapse(rt._h, None) == A.RT_ERR_ARG
        with pytest.raises(KeyError):
            rt.setCollapse("dp")
        rt.setCollapse("greedy")
        assert rt.getCollapse() == "greedy"
        assert ctypes.sizeof(A.RtMeshStats) == 56
    finally:
        rt.close()


def test_default_is_greedy_and_the_tree_as_before(pt, tracer):
    verts, idx = pc.make("sphere2000", pt.scenes)
    rt = pt.RayTracer(0)
    try:
        rt.setSpheres(pt.scenes.ply_scene())
        rt.setBuilder("ploc")
        rt.setMesh(verts, idx)
        assert rt.meshInfo()["collapse"] == pt._abi.RT_COLLAPSE_GREEDY
        pr.same_tree4(pr.as_tree4(rt.meshTree()), pc.ref_tree("sphere2000", pt.scenes, "ploc"), "greedy, never set")
        rt.setCollapse("sah")
        rt.setCollapse("greedy")
        rt.setMesh(verts, idx)
        pr.same_tree4(pr.as_tree4(rt.meshTree()), pc.ref_tree("sphere2000", pt.scenes, "ploc"), "greedy, set back")
    finally:
        rt.close()


def test_host_builder_ignores_the_mode(pt, tracer):
    verts, idx = pc.make("sphere2000", pt.scenes)
    out = []
    for mode in ("greedy", "sah"):
        rt = pt.RayTracer(0)
        try:
            rt.setSpheres(pt.scenes.ply_scene())
            rt.setBuilder("host")
            rt.setCollapse(mode)
            rt.setMesh(verts, idx)
            info, tree = rt.meshInfo(), rt.meshTree()
            assert info["builder"] == pt._abi.RT_BUILD_HOST and info["collapse"] == pt._abi.RT_COLLAPSE_SAH
            out.append(({k: v for k, v in info.items() if k != "build_seconds"}, tree))
        finally:
            rt.close()
    assert out[0][0] == out[1][0]
    for k in ("nodes4", "nodes4q", "tris"):
        np.testing.assert_array_equal(bits(out[0][1][k]), bits(out[1][1][k]), err_msg=k)


def test_cli_collapse(tracer, tmp_path):
    exe = str(ROOT / "pathtracer.cl_amd" / "rt_render")
    out = {}
    for name, extra in (("host", ["--builder", "host"]), ("ploc", ["--builder", "ploc", "--collapse", "sah"]),
                        ("gpu", ["--builder", "gpu", "--build-lights", "--collapse", "sah"])):
        raw = tmp_path / f"{name}.f32"
        subprocess.run([exe, "--mesh", "2000", "--width", "64", "--height", "48", "--frames", "2", *extra,
                        "--raw", str(raw)], check=True, timeout=120)
        out[name] = raw.read_bytes()
    assert len(out["host"]) == 64 * 48 * 16 and np.frombuffer(out["host"], np.float32).any()
    assert out["ploc"] == out["host"] and out["gpu"] == out["host"]
    r = subprocess.run([exe, "--mesh", "2000", "--builder", "ploc", "--collapse", "dp"], capture_output=True, timeout=120)
    assert r.returncode == 2
