"""RT_BUILD_OPT_LIGHTS on the GPU (rt_build_gpu.hip k_classify ...): the device
builders leave the never-hit triangles out and give the shadow queries a second tree whose root
keeps the lights' possible occluders (A) and the rest (B) apart, in the host build's layout.
Culling only: the trees pass the verifier and follow the restated rules, rays and frames equal
the CPU oracle's bit for bit, a moving mesh refits both trees and keeps the split while it still
holds, a rebuild uses the mesh's own builder and options, and with the option off the build is
what it was."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import build_lights_cases as bl
import ploc_cases as pc
import ploc_ref as pr
import refit_ref as rr
import test_light_cone_host as lh
import tree_cases as tc
import tree_ref as tr
from conftest import ROOT, bits
from test_gpu_light_cone import DEPTH, H, KNOBS, MESH_CENTER, SR, W, reference, render, same_as

pytestmark = pytest.mark.gpu

TRAVERSALS = ("linear", "bvh", "bvh4f")
CASE = "tris_64x48_sr1"


# ---- 1. the trees --------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", bl.BUILDERS)
@pytest.mark.parametrize("name", list(lh.SPLIT_CASES))
def test_two_tree_build(name, builder, pt, tracer):
    """The meshes the host builder splits: a valid two-tree build; a second build of the same
    input on the same context is the same trees."""
    verts, idx, lights = lh.make_case(name, pt)
    assert bl.expect_split(verts, idx, lights) is True, "precondition"
    rt = bl.context(pt, bl.spheres_for(pt.scenes, lights), builder)
    try:
        assert rt.getBuildOptions() == pt._abi.RT_BUILD_OPT_LIGHTS
        rt.setMesh(verts, idx)
        info, tree = bl.check_two_trees(pt, rt, builder, verts, idx, lights, f"{name} {builder}")
        c = bl.classes(verts, idx, lights)
        print(f"{name} {builder}: {info['n_tris_tree']} of {info['n_tris']} kept, A {info['n_tris_cone']}, nodes "
              f"{info['n_nodes4']} + {info['n_nodes4_shadow']}, build {1e3 * info['build_seconds']:.2f} ms; restated: "
              f"{int(c['kept'].sum())} kept, {int(c['parked'].sum())} parked")
        rt.setMesh(verts, idx)
        assert {k: v for k, v in rt.meshInfo().items() if k != "build_seconds"} == \
               {k: v for k, v in info.items() if k != "build_seconds"}
        bl.same_trees(rt.meshTree(), tree, f"{name} {builder}, built twice")
    finally:
        rt.close()


# ---- 2. rays -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctxs(pt, tracer):
    out = {b: bl.context(pt, pt.scenes.ply_scene(), b) for b in bl.BUILDERS}
    yield out
    for rt in out.values():
        rt.close()


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


@pytest.mark.parametrize("name", pc.MESHES)
def test_rays(name, ctxs, pt, oracle):
    """ploc_cases' meshes under both builders with the option on: split where the restated rules
    say so, else one culled tree; the query set (from the first tree's planes, the oracle's answers
    computed once) under the three traversals."""
    verts, idx = pc.make(name, pt.scenes)
    want = bl.expect_split(verts, idx, [lh.PLY_LIGHT])
    if name in tc.NOT_ENCODABLE or name in tc.NOTHING_HITTABLE:
        want = False
    rays = exp = None
    for b in bl.BUILDERS:
        rt = ctxs[b]
        rt.setBuildOptions(True)
        rt.setMesh(verts, idx)
        if rt.meshInfo()["n_nodes4_shadow"]:
            assert want is not False, (name, b)
            _, tree = bl.check_two_trees(pt, rt, b, verts, idx, [lh.PLY_LIGHT], f"{name} {b}")
        else:
            assert want is not True, (name, b)
            info, tree = bl.check_one_tree(pt, rt, b, verts, idx, f"{name} {b}")
            if name in tc.NOT_ENCODABLE:
                assert tree["compressed"] == 0 and tree["nodes4q"] is None
            if name in tc.NOTHING_HITTABLE:
                assert info["n_tris_tree"] == 1
        if rays is None:
            rays, exp = tc.queries(oracle, verts, idx, tree, pt._abi.RAY_DTYPE)
            if name in tc.NOTHING_HITTABLE:
                assert not (exp[0] >= 0).any() and not exp[2].any()
            else:
                assert len(rays) >= 2400 and (exp[0] >= 0).mean() >= 0.25
                assert (exp[2] != 0).mean() >= 0.10 and (exp[2] == 0).mean() >= 0.10
        rays_equal(rt, rays, exp, f"{name} {b}")


# ---- 3. frames -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(pt, oracle):
    """tests/test_gpu_light_cone.py's scene (the 20,000-triangle mesh, its camera, a second light,
    the light moved, the quarter turn), and a 5,000-triangle mesh of the same place and radius 0.5:
    it splits (27 parked triangles) and keeps every triangle under refit_ref's wobble and shrink, so
    both refit it and the verifier's never-hit rule holds in the new pose too."""
    sc = pt.scenes
    verts, idx = sc.make_mesh(20_000, MESH_CENTER, 0.38)
    Wp, Hp = sc.padded_dims(W, H)
    one = sc.ply_scene()
    two = np.concatenate([one, sc.init_sphere(center=(-3.0, 1.0, -3.0), radius=0.4, emission_power=1.0,
                                              emission=(0.9, 0.8, 0.7))])
    moved = one.copy()
    moved["center"][moved["emission_power"] != 0] = (-3.0, 3.0, -2.0)
    turned = np.ascontiguousarray(np.stack([verts[:, 2], verts[:, 1], -verts[:, 0]], axis=1), np.float32)
    s = dict(verts=verts, idx=idx, cam=sc.camera_spherical(W, target=MESH_CENTER, elevation=40.0, azimuth=105.0, distance=1.3),
             Wp=Wp, Hp=Hp, seeds=sc.default_seeds(Wp, Hp, skip=3), one=one, two=two, moved=moved, turned=turned, refs={})
    v5, i5 = sc.make_mesh(5_000, MESH_CENTER, 0.5)
    small = dict(s, verts=v5, idx=i5, wobbled=rr.wobble(v5), shrunk=rr.shrink(v5), refs={})
    return dict(big=s, small=small)


def frame_context(pt, monkeypatch, s, env, builder, spheres="one", lights_opt=True):
    """A fresh context under `env` (RT_SPLIT=0 unless it says otherwise, as tests/test_gpu_light_cone.py)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {"RT_SPLIT": "0", **env}.items():
        monkeypatch.setenv(k, v)
    rt = pt.RayTracer(0)
    rt.setSpheres(s[spheres])
    rt.setCamera(s["cam"])
    rt.setSampleRate(SR)
    rt.setMaxPathDepth(DEPTH)
    rt.setBuilder(builder)
    rt.setBuildOptions(lights_opt)
    rt.setMesh(s["verts"], s["idx"])
    return rt


@pytest.mark.parametrize("builder", bl.BUILDERS)
def test_frames(builder, pt, oracle, monkeypatch, scene):
    """One light, plain and counting; the light moved (the whole shadow tree) and put back."""
    s = scene["big"]
    ref = reference(s, oracle, "one")
    rt = frame_context(pt, monkeypatch, s, {}, builder)
    info = rt.meshInfo()
    assert info["cone_root"] == info["n_nodes4"] + 1 and info["n_nodes4_shadow"] > 0, info
    got = render(rt, s)
    same_as(got, ref, f"{builder}")
    counted = render(rt, s, counting=True)
    same_as(counted, ref, f"{builder}, counting")
    assert got[3]["shadow_start"] == counted[3]["shadow_start"] == info["cone_root"]
    rt.setSpheres(s["moved"])
    got = render(rt, s)
    assert rt.meshInfo() == info
    assert got[3]["shadow_start"] == info["n_nodes4"], got[3]
    same_as(got, reference(s, oracle, "moved"), f"{builder}, moved light")
    rt.setSpheres(s["one"])
    back = render(rt, s)
    rt.close()
    assert back[3]["shadow_start"] == info["cone_root"]
    same_as(back, ref, f"{builder}, light put back")


@pytest.mark.parametrize("builder", bl.BUILDERS)
def test_two_lights(builder, pt, oracle, monkeypatch, scene):
    s = scene["big"]
    rt = frame_context(pt, monkeypatch, s, {}, builder, spheres="two")
    info = rt.meshInfo()
    got = render(rt, s)
    rt.close()
    assert info["cone_root"] and got[3]["shadow_start"] == info["cone_root"], (info, got[3])
    same_as(got, reference(s, oracle, "two"), f"{builder}, two lights")


@pytest.mark.parametrize("builder", bl.BUILDERS)
@pytest.mark.parametrize("knob", ["RT_LIGHT_CONE", "RT_CULL_UNHITTABLE"])
def test_knobs_off(knob, builder, pt, oracle, monkeypatch, scene):
    """RT_LIGHT_CONE=0: one culled tree.  RT_CULL_UNHITTABLE=0: nothing left out, no split (the
    split is made among the kept triangles of a culled build): the build without the option."""
    s = scene["big"]
    rt = frame_context(pt, monkeypatch, s, {knob: "0"}, builder)
    info = rt.meshInfo()
    got = render(rt, s)
    rt.close()
    assert (info["n_nodes4_shadow"], info["cone_root"], info["n_tris_cone"]) == (0, 0, 0), info
    assert got[3]["shadow_start"] == 0
    if knob == "RT_LIGHT_CONE":
        assert info["n_tris_tree"] < info["n_tris"]
    else:
        assert info["n_tris_tree"] == info["n_tris"]
    same_as(got, reference(s, oracle, "one"), f"{builder}, {knob}=0")


@pytest.mark.parametrize("builder", bl.BUILDERS)
def test_split_tile(builder, pt, oracle, monkeypatch, scene):
    """A 2-way row-stripe tile through the sample-split path: the oracle's frame and seeds; the ray
    counts are the oracle's plus the repaired pixels' waste (tests/test_gpu_light_cone.py)."""
    s = scene["big"]
    tile = (8, 2, 1)
    rows = np.flatnonzero((np.arange(H) // tile[0]) % tile[1] == tile[2])
    pix = (rows[:, None] * W + np.arange(W)[None, :]).reshape(-1).astype(np.uint32)
    exp, sd, (closest, shadow) = reference(s, oracle, "one", pixels=pix)
    rt = frame_context(pt, monkeypatch, s, {"RT_SPLIT": "1"}, builder)
    info = rt.meshInfo()
    frame, seeds, c, ri = render(rt, s, tile=tile)
    rt.close()
    assert ri["split_chunks"] > 0 and ri["shadow_start"] == info["cone_root"] != 0, ri
    np.testing.assert_array_equal(bits(frame), bits(exp.reshape(H, W * 4)[rows].reshape(-1)), err_msg="frame")
    np.testing.assert_array_equal(seeds, sd, err_msg="seeds")
    assert c["rays_closest"] >= closest and c["rays_shadow"] >= shadow
    if ri["split_repaired"] == 0:
        assert (c["rays_closest"], c["rays_shadow"]) == (closest, shadow)


@pytest.mark.parametrize("builder", bl.BUILDERS)
@pytest.mark.parametrize("depth", [1, 4, 7, 8, 9, 64])
def test_shadow_cache_cuts(depth, builder, pt, oracle, monkeypatch, scene):
    """RT_SHADOW_CACHE_DEPTH from 1 to beyond the tree: the cut is a level of subtree A, or none."""
    s = scene["big"]
    rt = frame_context(pt, monkeypatch, s, {"RT_SHADOW_CACHE_DEPTH": str(depth)}, builder)
    info = rt.meshInfo()
    got = render(rt, s)
    rt.close()
    assert got[3]["shadow_start"] == info["cone_root"] != 0
    same_as(got, reference(s, oracle, "one"), f"{builder}, cut {depth}")


@pytest.mark.parametrize("builder", bl.BUILDERS)
def test_golden_sequence(builder, tracer, pt, golden, golden_meta):
    """The golden progressive sequence, counting, with the option on and off: the fixture's last
    frame and seeds either way; the traversal's work is printed, not asserted."""
    g, m = golden(CASE), golden_meta["cases"][CASE]
    Wg, Hg = m["W"], m["H"]
    for on in (False, True):
        t = pt.RayTracer(0)
        try:
            t.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
            t.setCamera(g["camera"])
            t.setSampleRate(m["sample_rate"])
            t.setMaxPathDepth(m["max_depth"])
            t.setNDRange(m["nd_y"])
            t.setBuilder(builder)
            t.setBuildOptions(on)
            t.setMesh(g["verts"], g["idx"])
            info = t.meshInfo()
            t.setSeeds(m["Wpad"], m["Hpad"], g["seeds_in"])
            t.setCounting(True)
            frame = np.zeros(Wg * Hg * 4, np.float32)
            for p in range(m["frames"]):
                t.rayTrace(frame, Wg, Hg, p, kernel=2)
            tot = t.counterTotals()
            print(f"{CASE} {builder} option {'on' if on else 'off'}: nodes_visited {tot['nodes_visited']}, leaves_visited "
                  f"{tot['leaves_visited']}, tris_tested {tot['tris_tested']}, rays {tot['rays_closest']} + "
                  f"{tot['rays_shadow']}; tree {info['n_tris_tree']} of {info['n_tris']}, A {info['n_tris_cone']}, "
                  f"shadow nodes {info['n_nodes4_shadow']}")
            np.testing.assert_array_equal(bits(frame), bits(g["frames"][-1]), err_msg=f"frame, option {on}")
            np.testing.assert_array_equal(t.getSeeds(), g["seeds_out"], err_msg=f"seeds, option {on}")
        finally:
            t.close()


# ---- 4. a moving mesh ----------------------------------------------------------------------------
def refit_ok(pt, up):
    return (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REFIT, pt._abi.RT_REFIT_OK)


@pytest.mark.parametrize("builder", bl.BUILDERS)
def test_update_unchanged(builder, pt, oracle, monkeypatch, scene):
    """(a) The vertices the trees were built from: both trees word for word, the split holds."""
    s = scene["big"]
    rt = frame_context(pt, monkeypatch, s, {}, builder)
    info, before = rt.meshInfo(), rt.meshTree()
    up = rt.updateMesh(s["verts"])
    assert refit_ok(pt, up) and up["area_ratio"] == 1.0 and up["ms"] > 0, up
    after = rt.meshTree()
    for k in ("nodes4", "nodes4q", "tris"):
        np.testing.assert_array_equal(bits(after[k]), bits(before[k]), err_msg=f"identity: {k}")
    assert rt.meshInfo() == info
    got = render(rt, s)
    rt.close()
    assert got[3]["shadow_start"] == info["cone_root"] != 0
    same_as(got, reference(s, oracle, "one"), f"{builder}, unchanged vertices")


@pytest.mark.parametrize("builder", bl.BUILDERS)
@pytest.mark.parametrize("pose", ["wobbled", "shrunk"])
def test_update_refits(pose, builder, pt, oracle, monkeypatch, scene):
    """(b) refit_ref.wobble and shrink on the mesh that keeps its never-hit set: a refit, both roots
    pass the verifier, rays and the frame are the oracle's for the new pose.  The queries start at
    A exactly when every parked triangle still never occludes — by the restated rule: after the
    wobble some can (the whole shadow tree), after the shrink none (A)."""
    s = scene["small"]
    verts, idx, nv = s["verts"], s["idx"], s[pose]
    lights = [lh.PLY_LIGHT]
    c0, c1 = bl.classes(verts, idx, lights), bl.classes(nv, idx, lights)
    assert not (c0["out"] ^ c1["out"]).any() and c0["unsure"] == c1["unsure"] == 0, "precondition: a refit, no flips"
    assert bl.expect_split(verts, idx, lights) is True, "precondition"
    broken = int((c0["parked"] & c1["occluder"]).sum())
    assert (broken > 0) == (pose == "wobbled"), "precondition"
    rt = frame_context(pt, monkeypatch, s, {}, builder)
    info = rt.meshInfo()
    assert info["cone_root"] == info["n_nodes4"] + 1
    up = rt.updateMesh(nv)
    assert refit_ok(pt, up) and up["ms"] > 0, up
    assert rt.meshInfo() == info
    tree = rt.meshTree()
    tr.check_tree(nv, idx, tree, 0, builder="host", reported=dict(n_hit=info["n_tris_tree"], depth4=info["depth4"],
                                                                  stack4=info["stack4"]))
    tr.check_tree(nv, idx, tree, tree["shadow_root"], builder="host", reported=dict(n_hit=info["n_tris_tree"]))
    rays, exp = tc.queries(oracle, nv, idx, tree, pt._abi.RAY_DTYPE)
    rays_equal(rt, rays, exp, f"{builder} {pose}")
    got = render(rt, s)
    rt.close()
    print(f"{builder} {pose}: refit {up['ms']:.3f} ms, {broken} parked triangles can occlude now, shadow_start "
          f"{got[3]['shadow_start']} (A {info['cone_root']}, root {info['n_nodes4']})")
    assert got[3]["shadow_start"] == (info["n_nodes4"] if broken else info["cone_root"])
    same_as(got, reference(s, oracle, "one", verts=pose), f"{builder}, {pose}")


@pytest.mark.parametrize("builder", bl.BUILDERS)
def test_update_quarter_turn(builder, pt, oracle, monkeypatch, scene):
    """(c) The mesh turned a quarter: other triangles face the light, some parked triangle can
    occlude: the whole shadow tree, the oracle's frame."""
    s = scene["big"]
    c0, c1 = bl.classes(s["verts"], s["idx"], [lh.PLY_LIGHT]), bl.classes(s["turned"], s["idx"], [lh.PLY_LIGHT])
    assert (c0["parked"] & c1["occluder"]).sum() > 0, "precondition"
    rt = frame_context(pt, monkeypatch, s, {}, builder)
    info = rt.meshInfo()
    assert info["cone_root"]
    up = rt.updateMesh(s["turned"])
    assert refit_ok(pt, up), up
    got = render(rt, s)
    rt.close()
    assert got[3]["shadow_start"] == info["n_nodes4"], got[3]
    same_as(got, reference(s, oracle, "one", verts="turned"), f"{builder}, turned")


@pytest.mark.parametrize("builder", bl.BUILDERS)
def test_rebuild_keeps_builder_and_options(builder, pt, tracer, oracle):
    """(d) det_bound under refit_ref.wobble (tests/test_gpu_refit.py: 75 left-out triangles become
    hittable): rebuilt by the mesh's own builder with its own options, whatever the context's have
    become since."""
    verts, idx = tc.make("det_bound", pt.scenes)
    nv = rr.wobble(verts)
    lights = [lh.PLY_LIGHT]
    assert bl.expect_split(verts, idx, lights) is True and bl.expect_split(nv, idx, lights) is True, "precondition"
    c0, c1 = bl.classes(verts, idx, lights), bl.classes(nv, idx, lights)
    newly = int((c0["out"] & c1["kept"]).sum())
    assert newly == 75 and c0["unsure"] == c1["unsure"] == 0, "precondition"
    rt = bl.context(pt, pt.scenes.ply_scene(), builder)
    try:
        rt.setMesh(verts, idx)
        bl.check_two_trees(pt, rt, builder, verts, idx, lights, f"det_bound {builder}")
        rt.setBuilder("host")
        rt.setBuildOptions(False)
        up = rt.updateMesh(nv)
        assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REBUILT, pt._abi.RT_REFIT_NEWLY_HITTABLE), up
        assert up["newly_hittable"] == newly
        assert rt.getBuildOptions() == 0
        _, tree = bl.check_two_trees(pt, rt, builder, nv, idx, lights, f"det_bound {builder}, rebuilt")
        rays, exp = tc.queries(oracle, nv, idx, tree, pt._abi.RAY_DTYPE)
        rays_equal(rt, rays, exp, f"det_bound {builder}, rebuilt")
        up = rt.updateMesh(nv)  # and the rebuilt mesh can be updated in turn
        assert refit_ok(pt, up) and up["area_ratio"] == 1.0, up
    finally:
        rt.close()


def test_host_built_mesh_still_loses_its_cone(pt, oracle, monkeypatch, scene):
    """(e) On a context with the option set, a host-built mesh is refitted as before: the queries
    walk the whole shadow tree afterwards, even with unchanged vertices."""
    s = scene["big"]
    rt = frame_context(pt, monkeypatch, s, {}, "host")
    info = rt.meshInfo()
    assert info["builder"] == pt._abi.RT_BUILD_HOST and info["cone_root"]
    up = rt.updateMesh(s["verts"])
    assert refit_ok(pt, up), up
    got = render(rt, s)
    rt.close()
    assert got[3]["shadow_start"] == info["n_nodes4"], got[3]
    same_as(got, reference(s, oracle, "one"), "host-built, refitted")


# ---- 5. off means off ----------------------------------------------------------------------------
@pytest.mark.parametrize("builder", bl.BUILDERS)
@pytest.mark.parametrize("name", ["mesh5000", "det_bound"])
def test_off_means_off(name, builder, pt, tracer):
    """The option never set, and set and then cleared before setMesh: the build of a context that
    never heard of it — one tree over every triangle, structurally the same arrays."""
    verts, idx, _ = lh.make_case(name, pt)
    trees = []
    for mode in ("never", "cleared"):
        rt = pt.RayTracer(0)
        try:
            rt.setSpheres(pt.scenes.ply_scene())
            rt.setBuilder(builder)
            if mode == "cleared":
                rt.setBuildOptions(True)
                rt.setBuildOptions(False)
            rt.setTraversal("bvh")
            rt.setMesh(verts, idx)
            info, tree = bl.check_one_tree(pt, rt, builder, verts, idx, f"{name} {builder} {mode}", culled=False)
            assert info["n_tris_tree"] == len(idx)
            trees.append((info, tree))
        finally:
            rt.close()
    (ia, ta), (ib, tb) = trees
    assert {k: v for k, v in ia.items() if k != "build_seconds"} == {k: v for k, v in ib.items() if k != "build_seconds"}
    pr.same_tree4(pr.as_tree4(ta), pr.as_tree4(tb), f"{name} {builder}")
    pr.same_tree4(pr.as_tree4(ta), pr.build(verts, idx, builder), f"{name} {builder} against the restatement")
    np.testing.assert_array_equal(np.sort(ta["tris"][:, 3].view(np.int32)), np.arange(len(idx)))


# ---- 6. the interface ----------------------------------------------------------------------------
def test_option_bits(pt, tracer):
    rt = pt.RayTracer(0)
    try:
        assert rt.getBuildOptions() == 0
        rt.setBuildOptions(True)
        assert rt.getBuildOptions() == pt._abi.RT_BUILD_OPT_LIGHTS == 1
        for bad in (2, 3, 0x80000000):
            assert rt._lib.rt_set_build_options(rt._h, bad) == pt._abi.RT_ERR_ARG
            assert rt.getBuildOptions() == 1, "a refused call leaves the options as they were"
        rt.setBuildOptions(False)
        assert rt.getBuildOptions() == 0
        assert rt._lib.rt_get_build_options(rt._h, None) == pt._abi.RT_ERR_ARG
    finally:
        rt.close()


def test_host_builder_ignores_the_option(pt, tracer):
    verts, idx, _ = lh.make_case("mesh5000", pt)
    out = []
    for on in (False, True):
        rt = bl.context(pt, pt.scenes.ply_scene(), "host", lights_opt=on)
        try:
            rt.setMesh(verts, idx)
            info, tree = rt.meshInfo(), rt.meshTree()
            out.append(({k: v for k, v in info.items() if k != "build_seconds"}, tree))
        finally:
            rt.close()
    assert out[0][0] == out[1][0] and out[0][0]["builder"] == pt._abi.RT_BUILD_HOST
    for k in ("nodes4", "nodes4q", "tris"):
        np.testing.assert_array_equal(bits(out[0][1][k]), bits(out[1][1][k]), err_msg=k)


def test_cli_build_lights(tracer, tmp_path):
    exe = str(ROOT / "pathtracer.cl_amd" / "rt_render")
    out = {}
    for name, extra in (("host", ["--builder", "host"]), ("ploc", ["--builder", "ploc", "--build-lights"]),
                        ("gpu", ["--builder", "gpu", "--build-lights"])):
        raw = tmp_path / f"{name}.f32"
        subprocess.run([exe, "--mesh", "2000", "--width", "64", "--height", "48", "--frames", "2", *extra,
                        "--raw", str(raw)], check=True, timeout=120)
        out[name] = raw.read_bytes()
    assert len(out["host"]) == 64 * 48 * 16 and np.frombuffer(out["host"], np.float32).any()
    assert out["ploc"] == out["host"] and out["gpu"] == out["host"]
