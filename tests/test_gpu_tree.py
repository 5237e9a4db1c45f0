"""The trees as the kernels read them (RayTracer.meshTree) under both builders, checked node by node
by tests/tree_ref.py; the traversals against the CPU oracle's linear loop on rays built to sit on
their edges (tests/tree_cases.py); and the spill tail of the traversal stack (rt_traverse.h Stack),
on a mesh whose rays are proved to reach it."""
from __future__ import annotations

import numpy as np
import pytest

import features_ref as fr
import tree_cases as tc
import tree_ref as tr
from conftest import bits

pytestmark = pytest.mark.gpu

TRAVERSALS = ("linear", "bvh", "bvh4f")
KNOBS = ("RT_INLINE_LIST", "RT_INLINE_CHAIN", "RT_LIST_MB", "RT_PIXEL_LISTS", "RT_SPLIT", "RTMI_GRID_BLOCKS",
         "RT_SHADOW_CACHE", "RT_DET_CULL", "RT_CULL_UNHITTABLE", "RT_BVH_LIGHT_W")


@pytest.fixture(scope="module")
def ctx(pt, tracer):
    """A context of this module's own, with the mesh scene's light (the host build then makes the
    shadow tree); `tracer` only proves that a GPU is there."""
    rt = pt.RayTracer(0)
    rt.setSpheres(pt.scenes.ply_scene())
    yield rt
    rt.close()


def build_and_check(rt, builder, verts, idx):
    """setMesh under `builder`, the read-back trees verified against meshInfo's figures."""
    rt.setBuilder(builder)
    rt.setTraversal("bvh")
    rt.setMesh(verts, idx)
    info, tree = rt.meshInfo(), rt.meshTree()
    assert (tree["n_nodes4"], tree["n_nodes4_shadow"]) == (info["n_nodes4"], info["n_nodes4_shadow"])
    tr.check_fallback(tree, f"{builder} tree")
    rep = dict(n_hit=info["n_tris_tree"], depth4=info["depth4"], stack4=info["stack4"])
    got = {0: tr.check_tree(verts, idx, tree, 0, builder=builder, reported=rep)}
    if tree["n_nodes4_shadow"]:
        got[1] = tr.check_tree(verts, idx, tree, tree["shadow_root"], builder=builder, reported=dict(n_hit=rep["n_hit"]))
    return info, tree, got


@pytest.mark.parametrize("builder", ["host", "gpu"])
@pytest.mark.parametrize("name", tc.MESHES)
def test_trees_and_rays(name, builder, ctx, pt, oracle):
    verts, idx = tc.make(name, pt.scenes)
    n = len(idx)
    info, tree, got = build_and_check(ctx, builder, verts, idx)
    if name in tc.NOT_ENCODABLE:  # the full-precision fallback, under both builders
        assert tree["compressed"] == 0 and tree["nodes4q"] is None and tree["n_nodes4_shadow"] == 0
    else:
        assert tree["compressed"] == 1
        assert (tree["n_nodes4_shadow"] > 0) == (builder == "host")
    if builder == "host" and name in tc.NOTHING_HITTABLE:
        assert tree["n_nodes4"] == 1 and info["n_tris_tree"] == 1
    if builder == "host" and name == "det_bound":
        assert 0 < info["n_tris_tree"] < n
    if name == "det_bound":  # normal boxes decide results here, under the GPU builder too
        assert ((tree["nodes4q"][:, 10] >> 24) != 255).mean() > 0.5

    # the oracle's answers first: the ray set must hit, occlude and miss often enough by itself
    rays, (exp_i, exp_t, exp_o) = tc.queries(oracle, verts, idx, tree, pt._abi.RAY_DTYPE)
    if name in tc.NOTHING_HITTABLE:
        assert not (exp_i >= 0).any() and not exp_o.any()
    else:
        assert len(rays) >= 2400
        assert (exp_i >= 0).mean() >= 0.25
        assert (exp_o != 0).mean() >= 0.10 and (exp_o == 0).mean() >= 0.10
    for trav in TRAVERSALS:
        ctx.setTraversal(trav)
        gi, gt = ctx.traceRays(rays)
        go, _ = ctx.traceRays(rays, any_hit=True)
        np.testing.assert_array_equal(gi, exp_i, err_msg=f"{name} {builder} {trav}: closest index")
        np.testing.assert_array_equal(bits(gt), bits(exp_t), err_msg=f"{name} {builder} {trav}: closest t")
        np.testing.assert_array_equal(go != 0, exp_o != 0, err_msg=f"{name} {builder} {trav}: occlusion")
    ctx.setTraversal("bvh")


# ---- the spill tail ------------------------------------------------------------------------------
def spill_rays(pt, n_each=288, seed=3):
    """Rays along z from z = -4 (a few from z = 4 back, a few slightly tilted) at two places: inside
    every box and outside every triangle ((x, y) in [0.7, 1.1]^2: x + y > r), and through every
    triangle ((x, y) in [-0.3, 0.3]^2); the lanes differ, so overlapping tails would show.  The first
    ray of each set is the plain one, (0.9, 0.9) and (0, 0), straight along z: the model walk's
    (tree_ref.live_stack).  Then the same rays as any-hit
    queries with finite tmax."""
    rng = np.random.default_rng(seed)
    rays = np.zeros(2 * n_each, pt._abi.RAY_DTYPE)
    xy = np.concatenate([rng.uniform(0.7, 1.1, (n_each, 2)), rng.uniform(-0.3, 0.3, (n_each, 2))])
    xy[0], xy[n_each] = (0.9, 0.9), (0.0, 0.0)
    back = (np.arange(2 * n_each) % 8 == 5)
    d = np.zeros((2 * n_each, 3))
    d[:, 2] = np.where(back, -1.0, 1.0)
    tilt = (np.arange(2 * n_each) % 4 == 3)
    d[tilt, :2] = rng.uniform(-0.004, 0.004, (int(tilt.sum()), 2))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["o"] = np.concatenate([xy, np.where(back, 4.0, -4.0)[:, None]], axis=1).astype(np.float32)
    rays["d"] = d.astype(np.float32)
    rays["tmin"], rays["tmax"] = np.float32(1e-4), np.float32(np.inf)
    rays["propagation"] = 1.0
    short = rays.copy()
    short["tmax"] = rng.choice(np.array([0.5, 1.0, 2.2, 3.7, 6.9, 7.0, 8.0], np.float32), 2 * n_each)
    return rays, short, n_each


def down_z_camera(pixel):
    """Camera (view, up, right, position) at (0.5, 0.5, 4) looking down -z, `pixel` apart per pixel at
    distance 1: over the frame the rays pass through every triangle, inside every box beside them,
    and past the mesh."""
    cam = np.zeros(16, np.float32)
    cam[0:3] = (0.0, 0.0, -1.0)
    cam[4:7] = (0.0, pixel, 0.0)
    cam[8:11] = (pixel, 0.0, 0.0)
    cam[12:15] = (0.5, 0.5, 4.0)
    return cam


@pytest.fixture(scope="module", params=["host", "gpu"])
def spill(request, tracer, pt, oracle):
    """The spill mesh built under one builder, with the preconditions that make it one: the reported
    stack4 is past the LDS part, and the model walk of the read-back tree keeps at least
    RT_STACK_DEPTH + 3 entries live for a ray of each set."""
    builder = request.param
    verts, idx = tc.spill_stack(tc.SPILL_COUNT[builder])
    rt = pt.RayTracer(0)  # a context of the mesh's own: the tests below find it as it was built
    rt.setSpheres(pt.scenes.ply_scene())
    info, tree, got = build_and_check(rt, builder, verts, idx)
    rays, short, n_each = spill_rays(pt)
    live = tr.live_stack(tree, 0, rays[[0, n_each]])
    print(f"spill mesh, {builder} builder: {len(idx)} triangles, stack4 {info['stack4']}, depth4 {info['depth4']}, "
          f"live entries {live.tolist()} (miss, hit)")
    assert info["stack4"] >= tr.RT_STACK_DEPTH + 4, "precondition: the builder's stack bound is in the spill tail"
    assert live.min() >= tr.RT_STACK_DEPTH + 3, f"precondition: the rays reach the spill tail ({live})"
    yield dict(builder=builder, rt=rt, verts=verts, idx=idx, rays=rays, short=short)
    rt.close()


def linear_oracle(oracle, fn, rays, v, i, parts=8):
    """The oracle's linear loop over `rays` in `parts` threads (the library call releases the
    interpreter lock): the large spill mesh's answers in a second or two."""
    from concurrent.futures import ThreadPoolExecutor

    chunks = [np.ascontiguousarray(c) for c in np.array_split(rays, parts)]
    with ThreadPoolExecutor(parts) as ex:
        res = list(ex.map(lambda c: fn(c, v, i), chunks))
    if isinstance(res[0], tuple):
        return tuple(np.concatenate(x) for x in zip(*res))
    return np.concatenate(res)


def test_spill_trace_rays(spill, oracle):
    ctx, v, i = spill["rt"], spill["verts"], spill["idx"]
    exp_i, exp_t = linear_oracle(oracle, oracle.closest_hits, spill["rays"], v, i)
    exp_o = linear_oracle(oracle, oracle.any_hits, spill["short"], v, i)
    half = len(exp_i) // 2
    assert not (exp_i[:half] >= 0).any() and (exp_i[half:] >= 0).all()  # the two places
    assert 0.2 < (exp_o[half:] != 0).mean() < 0.9 and not exp_o[:half].any()
    for trav in ("bvh", "bvh4f"):
        ctx.setTraversal(trav)
        gi, gt = ctx.traceRays(spill["rays"])
        go, _ = ctx.traceRays(spill["short"], any_hit=True)
        ga, _ = ctx.traceRays(spill["rays"], any_hit=True)
        np.testing.assert_array_equal(gi, exp_i, err_msg=f"{trav}: closest index")
        np.testing.assert_array_equal(bits(gt), bits(exp_t), err_msg=f"{trav}: closest t")
        np.testing.assert_array_equal(go != 0, exp_o != 0, err_msg=f"{trav}: occlusion, finite tmax")
        np.testing.assert_array_equal(ga != 0, exp_i >= 0, err_msg=f"{trav}: occlusion")
    ctx.setTraversal("bvh")


def test_spill_features(spill, oracle):
    W, H = 16, 8
    ctx = spill["rt"]
    ctx.setCamera(down_z_camera(0.06))
    rays = ctx.primaryRays(W, H)
    exp = fr.features_tris(oracle, rays, spill["verts"], spill["idx"])
    ids = fr.feature_ids(exp.reshape(-1))
    assert (ids >= 0).sum() >= 16 and (ids == fr.RT_FEAT_BOX).sum() >= 16
    for trav in ("bvh", "bvh4f"):
        ctx.setTraversal(trav)
        feat = np.full(2 * W * H * 4, np.nan, np.float32)
        ctx.renderFeatures(feat, W, H, kernel=2)
        np.testing.assert_array_equal(bits(feat), bits(exp.reshape(-1)), err_msg=trav)
    ctx.setTraversal("bvh")


@pytest.mark.parametrize("lists", ["off", "default"])
def test_spill_frame(lists, spill, pt, oracle, monkeypatch):
    """An 8 x 8 frame, 1 sample, depth 6, through k_tris (and with the default settings whatever
    pre-passes it chooses): frame, seeds and ray counts equal the oracle's BVH mode."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if lists == "off":
        monkeypatch.setenv("RT_PIXEL_LISTS", "0")
    sc = pt.scenes
    W = H = 8
    Wp, Hp = sc.padded_dims(W, H)
    cam = down_z_camera(0.12)
    v, i = spill["verts"], spill["idx"]
    sd = sc.default_seeds(Wp, Hp, skip=3)
    exp = np.zeros(W * H * 4, np.float32)
    bvh = oracle.build_bvh(v, i)
    counts = oracle.render_tris(exp, cam, sc.ply_scene(), W, H, Wp, Hp, 1, 6, 0, sd, v, i, bvh=bvh)
    bvh.close()
    rt = pt.RayTracer(0)
    try:
        rt.setSpheres(sc.ply_scene())
        rt.setCamera(cam)
        rt.setSampleRate(1)
        rt.setMaxPathDepth(6)
        rt.setBuilder(spill["builder"])
        rt.setMesh(v, i)
        assert rt.meshInfo()["stack4"] >= tr.RT_STACK_DEPTH + 4
        rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp, skip=3))
        got = np.zeros(W * H * 4, np.float32)
        rt.rayTrace(got, W, H, 0, kernel=2)
        c = rt.counters()
        np.testing.assert_array_equal(bits(got), bits(exp), err_msg="frame")
        np.testing.assert_array_equal(rt.getSeeds(), sd, err_msg="seeds")
        assert (c["rays_closest"], c["rays_shadow"]) == tuple(counts)
        assert (exp.reshape(-1, 4)[:, :3] > 0).any()
    finally:
        rt.close()
