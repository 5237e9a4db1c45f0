"""rt_update_mesh on the GPU (csrc/rt_refit.hip): the refitted trees read back
(RayTracer.meshTree) against the numpy restatement (tests/refit_ref.py) and the tree verifier
(tests/tree_ref.py), the traversals against the CPU oracle's linear loop on the moved vertices,
the fallbacks to a rebuild, dynamic mode, frames with their caches, the off-mesh bounds, the
feature buffers and the errors.

The shadow tree's full-precision nodes exist only in the refit's workspace; they are compared
through the compressed nodes: check_tree, given refit_ref's full shadow nodes, pins every plane
of a compressed node to them (origin, smallest exponent, outward rounding within one step)."""
from __future__ import annotations

import numpy as np
import pytest

import features_ref as fr
import refit_ref as rr
import tree_cases as tc
import tree_ref as tr
from conftest import bits

pytestmark = pytest.mark.gpu

TRAVERSALS = ("linear", "bvh", "bvh4f")
KNOBS = ("RT_INLINE_LIST", "RT_INLINE_CHAIN", "RT_LIST_MB", "RT_PIXEL_LISTS", "RT_SPLIT", "RTMI_GRID_BLOCKS",
         "RT_SHADOW_CACHE", "RT_DET_CULL", "RT_CULL_UNHITTABLE", "RT_BVH_LIGHT_W")
NO_CULLED = ("sphere200_first1", "sphere200_first5", "sphere200_first9", "sphere2000", "one_centre600", "flat_grid",
             "far_grid", "mesh20000")
CULLED = ("mixed_scales", "det_bound")
BUILDERS = ("host", "gpu")


def mesh(name, pt):
    """tree_cases' meshes, and make_mesh(20000): more than 256 nodes on a level, many record blocks."""
    return pt.scenes.make_mesh(20000) if name == "mesh20000" else tc.make(name, pt.scenes)


def ratios(verts, idx):
    r = tr.never_hit_rule(tr.triangle_terms(verts, idx))
    assert (np.abs(r - 1.0) > 1e-6).all(), "precondition: no triangle within 1e-6 of the never-hit bound"
    return r


def flips(verts, new_verts, idx):
    """(left-out triangles that become hittable, tree triangles that become never-hit, left out before)"""
    b, a = ratios(verts, idx) < 1.0, ratios(new_verts, idx) < 1.0
    if b.all():  # nothing hittable: the builder keeps triangle 0
        b = b.copy()
        b[0] = False
    return int((b & ~a).sum()), int((~b & a).sum()), int(b.sum())


@pytest.fixture(scope="module")
def ctx(pt, tracer):
    """A context with the mesh scene's light: the host build makes the shadow tree."""
    rt = pt.RayTracer(0)
    rt.setSpheres(pt.scenes.ply_scene())
    yield rt
    rt.close()


def build(rt, builder, verts, idx, dynamic=False):
    rt.setMeshDynamic(dynamic)
    rt.setBuilder(builder)
    rt.setTraversal("bvh")
    try:
        rt.setMesh(verts, idx)
    finally:
        rt.setMeshDynamic(False)
    return rt.meshTree()


def same_tree(a, b, what):
    for k in ("nodes4", "nodes4q", "tris"):
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=f"{what}: {k}")


def rays_equal_oracle(rt, pt, oracle, verts, idx, tree, what):
    rays, (exp_i, exp_t, exp_o) = tc.queries(oracle, verts, idx, tree, pt._abi.RAY_DTYPE)
    for trav in TRAVERSALS:
        rt.setTraversal(trav)
        gi, gt = rt.traceRays(rays)
        go, _ = rt.traceRays(rays, any_hit=True)
        np.testing.assert_array_equal(gi, exp_i, err_msg=f"{what} {trav}: closest index")
        np.testing.assert_array_equal(bits(gt), bits(exp_t), err_msg=f"{what} {trav}: closest t")
        np.testing.assert_array_equal(go != 0, exp_o != 0, err_msg=f"{what} {trav}: occlusion")
    rt.setTraversal("bvh")
    return exp_i


# ---- 1. identity ---------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", ["sphere200_first5", "sphere2000", "one_centre600", "far_grid", "det_bound", "mesh20000"])
def test_identity(name, builder, ctx, pt):
    """updateMesh with the vertices the tree was built from: every array the kernels read is bit
    for bit what the builder made — the device's quantisation agrees with the host's."""
    verts, idx = mesh(name, pt)
    before = build(ctx, builder, verts, idx)
    info = ctx.meshInfo()
    up = ctx.updateMesh(verts)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REFIT, pt._abi.RT_REFIT_OK), up
    assert up["area_ratio"] == 1.0 and up["newly_hittable"] == 0 and up["ms"] > 0
    same_tree(ctx.meshTree(), before, f"{name} {builder}")
    assert ctx.meshInfo() == info
    assert ctx.lastMeshUpdate() == up


# ---- 2. refit ------------------------------------------------------------------------------------
REFIT_CASES = [(n, d) for n in NO_CULLED for d in ("rigid", "wobble")] + [(n, "rigid") for n in CULLED]


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name,deform", REFIT_CASES)
def test_refit(name, deform, builder, ctx, pt, oracle):
    verts, idx = mesh(name, pt)
    nv = rr.DEFORM[deform](verts)
    newly, unhit, culled = flips(verts, nv, idx)
    assert (newly, unhit) == (0, 0) and (culled == 0 or name in CULLED), "precondition"
    before = build(ctx, builder, verts, idx)
    info = ctx.meshInfo()
    up = ctx.updateMesh(nv)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REFIT, pt._abi.RT_REFIT_OK), up
    assert (up["newly_hittable"], up["now_unhittable"]) == (0, 0)
    assert ctx.meshInfo() == info, "rt_mesh_info's numbers stay the build's"
    tree = ctx.meshTree()
    # the structure is the build's
    np.testing.assert_array_equal(tree["nodes4"][:, 24:28].view(np.int32), before["nodes4"][:, 24:28].view(np.int32))
    np.testing.assert_array_equal(tree["nodes4q"][:, 12:16], before["nodes4q"][:, 12:16])
    np.testing.assert_array_equal(tree["tris"][:, 3].view(np.int32), before["tris"][:, 3].view(np.int32))
    # the records and boxes are the reference's
    ref = rr.refit(before, nv, idx)
    np.testing.assert_array_equal(bits(tree["tris"]), bits(ref["tris"]), err_msg="records")
    np.testing.assert_array_equal(bits(tree["nodes4"]), bits(ref["nodes4"]), err_msg="closest-hit tree")
    # and a tree the verifier accepts like a built one, the shadow tree pinned to the reference's full boxes
    tree["nodes4_shadow"] = ref["nodes4_shadow"]
    rep = dict(n_hit=info["n_tris_tree"], depth4=info["depth4"], stack4=info["stack4"])
    tr.check_fallback(tree, f"{builder} tree")
    tr.check_tree(nv, idx, tree, 0, builder=builder, reported=rep)
    assert (tree["n_nodes4_shadow"] > 0) == (builder == "host")
    if tree["n_nodes4_shadow"]:
        tr.check_tree(nv, idx, tree, tree["shadow_root"], builder=builder, reported=dict(n_hit=rep["n_hit"]))
    hit = rays_equal_oracle(ctx, pt, oracle, nv, idx, tree, f"{name} {deform} {builder}")
    assert (hit >= 0).mean() >= 0.25
    want = rr.half_area_sum(tree["nodes4"]) / rr.half_area_sum(before["nodes4"])
    print(f"{name} {deform} {builder}: area_ratio {up['area_ratio']:.9g} (numpy {want:.9g}), refit {up['ms']:.3f} ms")
    assert abs(up["area_ratio"] - want) <= 1e-6 * want


# ---- 3. fallbacks --------------------------------------------------------------------------------
def test_newly_hittable_triangles_rebuild(ctx, pt, oracle):
    verts, idx = mesh("det_bound", pt)
    nv = rr.wobble(verts)
    newly, unhit, _ = flips(verts, nv, idx)
    assert (newly, unhit) == (75, 46), "precondition"
    build(ctx, "host", verts, idx)
    up = ctx.updateMesh(nv)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REBUILT, pt._abi.RT_REFIT_NEWLY_HITTABLE), up
    assert up["newly_hittable"] == 75 and up["ms"] == 0
    info, tree = ctx.meshInfo(), ctx.meshTree()
    assert info["builder"] == pt._abi.RT_BUILD_HOST
    rep = dict(n_hit=info["n_tris_tree"], depth4=info["depth4"], stack4=info["stack4"])
    tr.check_tree(nv, idx, tree, 0, builder="host", reported=rep)
    tr.check_tree(nv, idx, tree, tree["shadow_root"], builder="host", reported=dict(n_hit=rep["n_hit"]))
    rays_equal_oracle(ctx, pt, oracle, nv, idx, tree, "det_bound wobble rebuilt")
    # and the rebuilt mesh can be updated in turn
    up = ctx.updateMesh(nv)
    assert up["action"] == pt._abi.RT_MESH_UPDATE_REFIT and up["area_ratio"] == 1.0


def test_triangles_that_become_unhittable_stay(ctx, pt, oracle):
    verts, idx = mesh("det_bound", pt)
    nv = rr.shrink(verts)
    newly, unhit, _ = flips(verts, nv, idx)
    assert (newly, unhit) == (0, 271), "precondition"
    build(ctx, "host", verts, idx)
    info = ctx.meshInfo()
    up = ctx.updateMesh(nv)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REFIT, pt._abi.RT_REFIT_OK), up
    assert (up["newly_hittable"], up["now_unhittable"]) == (0, 271)
    assert ctx.meshInfo() == info
    rays_equal_oracle(ctx, pt, oracle, nv, idx, ctx.meshTree(), "det_bound shrink")


def test_mixed_scales_preconditions_and_shrink(ctx, pt, oracle):
    verts, idx = mesh("mixed_scales", pt)
    assert flips(verts, rr.wobble(verts), idx)[:2] == (68, 59), "precondition"
    nv = rr.shrink(verts)
    assert flips(verts, nv, idx)[:2] == (0, 369), "precondition"
    build(ctx, "host", verts, idx)
    up = ctx.updateMesh(nv)
    assert (up["action"], up["now_unhittable"]) == (pt._abi.RT_MESH_UPDATE_REFIT, 369), up
    rays_equal_oracle(ctx, pt, oracle, nv, idx, ctx.meshTree(), "mixed_scales shrink")
    up = ctx.updateMesh(rr.wobble(verts))
    assert (up["action"], up["reason"], up["newly_hittable"]) == (
        pt._abi.RT_MESH_UPDATE_REBUILT, pt._abi.RT_REFIT_NEWLY_HITTABLE, 68), up


def test_unhittable_mesh_scaled_up_rebuilds(ctx, pt):
    verts, idx = mesh("unhittable", pt)
    nv = rr.scale(verts, 40.0)
    assert int((ratios(nv, idx) >= 1.0).sum()) == 63 and (ratios(verts, idx) < 1.0).all(), "precondition"
    build(ctx, "host", verts, idx)
    assert ctx.meshInfo()["n_tris_tree"] == 1
    up = ctx.updateMesh(nv)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REBUILT, pt._abi.RT_REFIT_NEWLY_HITTABLE), up
    assert up["newly_hittable"] in (62, 63)  # triangle 0 is in the one-leaf tree whatever its ratio
    info, tree = ctx.meshInfo(), ctx.meshTree()
    assert info["n_tris_tree"] == 63
    tr.check_tree(nv, idx, tree, 0, builder="host", reported=dict(n_hit=63))


@pytest.mark.parametrize("builder", BUILDERS)
def test_encodability_change_rebuilds(builder, ctx, pt):
    """sphere2000 scaled until a node spans more than 255 * 128: no compressed nodes any more, a
    rebuild; scaled back, the tree without compressed nodes fits again: a rebuild too."""
    verts, idx = mesh("sphere2000", pt)
    big = rr.scale(verts, 10000.0)
    v = big.astype(np.float64)
    assert (v.max(axis=0) - v.min(axis=0)).max() > 255.0 * 128.0 + 1000.0, "precondition"
    assert build(ctx, builder, verts, idx)["compressed"] == 1
    up = ctx.updateMesh(big)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REBUILT, pt._abi.RT_REFIT_ENCODING), up
    tree = ctx.meshTree()
    assert tree["compressed"] == 0 and tree["nodes4q"] is None and tree["n_nodes4_shadow"] == 0
    tr.check_fallback(tree, f"{builder} tree, scaled up")
    tr.check_tree(big, idx, tree, 0, builder=builder)
    # a refit of the tree without compressed nodes, still not encodable
    big2 = rr.scale(verts, 9000.0)
    up = ctx.updateMesh(big2)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REFIT, pt._abi.RT_REFIT_OK), up
    tree = ctx.meshTree()
    assert tree["compressed"] == 0
    tr.check_fallback(tree, f"{builder} tree, refitted without compressed nodes")
    tr.check_tree(big2, idx, tree, 0, builder=builder)
    up = ctx.updateMesh(verts)
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REBUILT, pt._abi.RT_REFIT_ENCODING), up
    tree = ctx.meshTree()
    assert tree["compressed"] == 1
    tr.check_fallback(tree, f"{builder} tree, scaled back")
    tr.check_tree(verts, idx, tree, 0, builder=builder)


# ---- 4. dynamic mode -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", CULLED)
def test_dynamic_mode_always_refits(name, ctx, pt, oracle):
    verts, idx = mesh(name, pt)
    nv = rr.wobble(verts)
    newly, unhit, culled = flips(verts, nv, idx)
    assert newly > 0 and unhit > 0 and culled > 0, "precondition: the default build would have to rebuild"
    before = build(ctx, "host", verts, idx, dynamic=True)
    info = ctx.meshInfo()
    assert info["n_tris_tree"] == info["n_tris"] == len(idx)
    up = ctx.updateMesh(nv)
    assert (up["action"], up["reason"], up["newly_hittable"]) == (pt._abi.RT_MESH_UPDATE_REFIT, pt._abi.RT_REFIT_OK, 0), up
    assert up["now_unhittable"] == unhit  # of the triangles a ray could hit at the build
    assert ctx.meshInfo() == info
    tree = ctx.meshTree()
    ref = rr.refit(before, nv, idx)
    np.testing.assert_array_equal(bits(tree["nodes4"]), bits(ref["nodes4"]))
    rays_equal_oracle(ctx, pt, oracle, nv, idx, tree, f"{name} wobble dynamic")
    # the mode is the mesh's, not the context's: the next default build culls again
    build(ctx, "host", verts, idx)
    assert ctx.meshInfo()["n_tris_tree"] == len(idx) - culled


# ---- 5 - 7. frames, caches, bounds, features ------------------------------------------------------
def oracle_frame(oracle, sc, cam, verts, idx, W, H, sr, seeds):
    Wp, Hp = sc.padded_dims(W, H)
    sd = seeds.copy()
    exp = np.zeros(W * H * 4, np.float32)
    bvh = oracle.build_bvh(verts, idx)
    counts = oracle.render_tris(exp, cam, sc.ply_scene(), W, H, Wp, Hp, sr, 6, 0, sd, verts, idx, bvh=bvh)
    bvh.close()
    return bits(exp).copy(), sd, tuple(counts)


def gpu_frame(rt, sc, W, H, seeds):
    Wp, Hp = sc.padded_dims(W, H)
    rt.setSeeds(Wp, Hp, seeds.copy())
    got = np.zeros(W * H * 4, np.float32)
    rt.rayTrace(got, W, H, 0, kernel=2)
    c = rt.counters()
    return bits(got).copy(), rt.getSeeds().copy(), (c["rays_closest"], c["rays_shadow"])


def frame_ctx(pt, monkeypatch, W, sr, builder, verts, idx, camera=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    sc = pt.scenes
    rt = pt.RayTracer(0)
    rt.setSpheres(sc.ply_scene())
    cam = sc.camera_spherical(W, **(camera or sc.PLY_CAMERA))
    rt.setCamera(cam)
    rt.setSampleRate(sr)
    rt.setMaxPathDepth(6)
    rt.setBuilder(builder)
    rt.setMesh(verts, idx)
    return rt, cam


def assert_frame(got, exp, what):
    np.testing.assert_array_equal(got[0], exp[0], err_msg=f"{what}: frame")
    np.testing.assert_array_equal(got[1], exp[1], err_msg=f"{what}: seeds")
    assert got[2] == exp[2], f"{what}: ray counts {got[2]} != {exp[2]}"


@pytest.mark.parametrize("builder", BUILDERS)
def test_frames_and_caches(builder, pt, oracle, monkeypatch):
    """A frame on the built mesh (so schedule and candidate lists exist), the update, a frame on
    the moved mesh: frame, both seed planes and ray counts equal the oracle's BVH mode on the new
    vertices, and the lists were built again."""
    sc = pt.scenes
    W, H, sr = 16, 12, 4
    verts, idx = mesh("sphere2000", pt)
    nv = rr.wobble(verts)
    seeds = sc.default_seeds(*sc.padded_dims(W, H), skip=3)
    rt, cam = frame_ctx(pt, monkeypatch, W, sr, builder, verts, idx)
    try:
        old = oracle_frame(oracle, sc, cam, verts, idx, W, H, sr, seeds)
        new = oracle_frame(oracle, sc, cam, nv, idx, W, H, sr, seeds)
        assert not np.array_equal(old[0], new[0]), "precondition: the deformation shows"
        assert_frame(gpu_frame(rt, sc, W, H, seeds), old, "built mesh")
        assert rt.renderInfo()["lists"] == 1, "precondition: the frame uses candidate lists"
        for _ in range(2):  # (the first build sizes the next one's list area: the second frame may build again)
            assert_frame(gpu_frame(rt, sc, W, H, seeds), old, "built mesh again")
        assert rt.renderInfo()["lists_rebuilt"] == 0, "precondition: the same view keeps its lists"
        assert rt.updateMesh(nv)["action"] == pt._abi.RT_MESH_UPDATE_REFIT
        assert_frame(gpu_frame(rt, sc, W, H, seeds), new, "moved mesh")
        assert rt.renderInfo()["lists_rebuilt"] == 1
    finally:
        rt.close()


def test_off_mesh_bounds_follow_the_vertices(pt, oracle, monkeypatch):
    """A small mesh translated out of its own padded bounds: a box-path query is answered without a
    traversal when it misses the bounds, so stale bounds would lose the mesh."""
    sc = pt.scenes
    W = H = 8
    verts, idx = sc.make_mesh(2000, center=(-1.2, -3.6, 0.3), radius=0.5)
    nv = np.ascontiguousarray((verts.astype(np.float64) + np.array([2.4, 0.0, 0.0])).astype(np.float32))
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    pad = 1e-3 * float((hi - lo).max()) + 1e-4
    assert nv[:, 0].min() - pad > hi[0] + pad, "precondition: the padded bounds are disjoint"
    seeds = sc.default_seeds(*sc.padded_dims(W, H), skip=3)
    rt, cam = frame_ctx(pt, monkeypatch, W, 1, "host", verts, idx)
    try:
        old = oracle_frame(oracle, sc, cam, verts, idx, W, H, 1, seeds)
        new = oracle_frame(oracle, sc, cam, nv, idx, W, H, 1, seeds)
        assert not np.array_equal(old[0], new[0]), "precondition: the mesh shows in the frame"
        assert_frame(gpu_frame(rt, sc, W, H, seeds), old, "built mesh")
        assert rt.updateMesh(nv)["action"] == pt._abi.RT_MESH_UPDATE_REFIT
        assert_frame(gpu_frame(rt, sc, W, H, seeds), new, "translated mesh")
    finally:
        rt.close()


@pytest.mark.parametrize("builder", BUILDERS)
def test_features_after_update(builder, ctx, pt, oracle):
    W, H = 16, 8
    verts, idx = mesh("sphere2000", pt)
    nv = rr.wobble(verts)
    build(ctx, builder, verts, idx)
    ctx.setCamera(pt.scenes.camera_spherical(W, **pt.scenes.PLY_CAMERA))
    assert ctx.updateMesh(nv)["action"] == pt._abi.RT_MESH_UPDATE_REFIT
    exp = fr.features_tris(oracle, ctx.primaryRays(W, H), nv, idx)
    old = fr.features_tris(oracle, ctx.primaryRays(W, H), verts, idx)
    assert (fr.feature_ids(exp.reshape(-1)) >= 0).sum() >= 16 and not np.array_equal(bits(exp), bits(old))
    for trav in ("bvh", "bvh4f"):
        ctx.setTraversal(trav)
        feat = np.full(2 * W * H * 4, np.nan, np.float32)
        ctx.renderFeatures(feat, W, H, kernel=2)
        np.testing.assert_array_equal(bits(feat), bits(exp.reshape(-1)), err_msg=trav)
    ctx.setTraversal("bvh")


# ---- 8. errors -----------------------------------------------------------------------------------
def test_errors_leave_the_mesh_as_it_was(pt, oracle, monkeypatch):
    sc = pt.scenes
    W, H, sr = 16, 12, 1
    verts, idx = mesh("sphere2000", pt)
    seeds = sc.default_seeds(*sc.padded_dims(W, H), skip=3)
    rt = pt.RayTracer(0)
    with pytest.raises(pt.RtError) as e:
        rt.updateMesh(verts)
    assert e.value.status == pt._abi.RT_ERR_NO_MESH
    rt.close()
    rt, cam = frame_ctx(pt, monkeypatch, W, sr, "host", verts, idx)
    try:
        before = rt.meshTree()
        with pytest.raises(pt.RtError) as e:
            rt.lastMeshUpdate()
        with pytest.raises(pt.RtError) as e:
            rt.updateMesh(verts[:-1])
        assert e.value.status == pt._abi.RT_ERR_ARG
        bad = rr.wobble(verts)
        bad[len(bad) // 2, 1] = np.nan
        with pytest.raises(pt.RtError) as e:
            rt.updateMesh(bad)
        assert e.value.status == pt._abi.RT_ERR_ARG
        bad[len(bad) // 2, 1] = np.inf
        with pytest.raises(pt.RtError) as e:
            rt.updateMesh(bad)
        assert e.value.status == pt._abi.RT_ERR_ARG
        same_tree(rt.meshTree(), before, "after the refused updates")
        assert_frame(gpu_frame(rt, sc, W, H, seeds), oracle_frame(oracle, sc, cam, verts, idx, W, H, sr, seeds),
                     "after the refused updates")
    finally:
        rt.close()


def test_cpp_view_drops_what_shows_the_old_mesh(tracer, tmp_path):
    """RayTracerHIP::updateMesh and ProgressiveViewHIP::updateMesh (tests/cpp/view_update_mesh.cpp):
    with the temporal and the variance-guided display on, the frames displayed after an update equal
    those of a second view that got the moved vertices by a fresh setMesh and dropped its history through
    the stages' own switches (the program's header says why both refine the same accumulation)."""
    import subprocess

    from test_refit_host import build_view_program

    r = subprocess.run([str(build_view_program(tmp_path)), "32", "24", "2000"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("builder", BUILDERS)
def test_device_pointer_update(builder, ctx, pt):
    import torch

    verts, idx = mesh("mesh20000", pt)
    nv = rr.wobble(verts)
    build(ctx, builder, verts, idx)
    up_h = ctx.updateMesh(nv)
    host = ctx.meshTree()
    # the same tree moved away and back again through device memory (two GPU builds of one mesh
    # need not number their nodes alike)
    assert ctx.updateMesh(rr.rigid(verts))["action"] == pt._abi.RT_MESH_UPDATE_REFIT
    dv = torch.from_numpy(nv).cuda()
    torch.cuda.synchronize()
    up_d = ctx.updateMesh(dv, device=True)
    same_tree(ctx.meshTree(), host, "device pointer against host pointer")
    assert {k: v for k, v in up_d.items() if k != "ms"} == {k: v for k, v in up_h.items() if k != "ms"}
