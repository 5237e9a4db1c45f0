"""The lights' cone split of the shadow tree on the GPU (rt_bvh.cpp never_occludes):
the shadow queries start at the subtree over the triangles that can occlude the lights the tree was
built for.  Culling only: frames, seeds and ray counts equal the CPU oracle's bit for bit with the
split, without it (RT_LIGHT_CONE=0), with two lights, with the GPU builder, on a sample-split tile
and at every cut of the shadow cache; after a light has moved or the mesh was refitted the queries
start at the whole shadow tree's root again (renderInfo's shadow_start).
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

W, H, SR, DEPTH = 64, 48, 4, 6
MESH_CENTER = (0.0, -2.2, 0.0)
KNOBS = ("RT_LIGHT_CONE", "RT_SHADOW_CACHE", "RT_SHADOW_CACHE_DEPTH", "RT_SPLIT", "RT_SPLIT_SPEC", "RT_CULL_UNHITTABLE",
         "RT_BVH_LIGHT_W")


@pytest.fixture(scope="module")
def scene(pt, oracle):
    """The 20,000-triangle mesh of the host test (radius 0.38 at the mesh scene's place) with the camera
    aimed at it, the mesh scene's spheres, and its variants: a second light on the other side, the
    light moved, the mesh turned a quarter about its vertical axis (exact in float: the same
    never-hit set, so an update refits)."""
    sc = pt.scenes
    verts, idx = sc.make_mesh(20_000, MESH_CENTER, 0.38)
    cam = sc.camera_spherical(W, target=MESH_CENTER, elevation=40.0, azimuth=105.0, distance=1.3)
    Wp, Hp = sc.padded_dims(W, H)
    one = sc.ply_scene()
    two = np.concatenate([one, sc.init_sphere(center=(-3.0, 1.0, -3.0), radius=0.4, emission_power=1.0,
                                              emission=(0.9, 0.8, 0.7))])
    moved = one.copy()
    moved["center"][moved["emission_power"] != 0] = (-3.0, 3.0, -2.0)
    turned = np.ascontiguousarray(np.stack([verts[:, 2], verts[:, 1], -verts[:, 0]], axis=1), np.float32)
    bvh = oracle.build_bvh(verts, idx)
    hit, _ = oracle.closest_hits_bvh(sc.camera_rays(cam, W, H), bvh)
    bvh.close()
    assert (hit >= 0).mean() >= 0.25, "precondition: a quarter of the pixels hit the mesh"
    return dict(verts=verts, idx=idx, cam=cam, Wp=Wp, Hp=Hp, seeds=sc.default_seeds(Wp, Hp, skip=3), one=one, two=two,
                moved=moved, turned=turned, refs={})


def reference(scene, oracle, spheres, verts="verts", pixels=None):
    """The oracle's frame, seeds and (closest, shadow) ray counts, computed once per variant."""
    key = (spheres, verts, None if pixels is None else len(pixels))
    if key not in scene["refs"]:
        s = scene
        sd = s["seeds"].copy()
        exp = np.zeros(W * H * 4, np.float32)
        bvh = oracle.build_bvh(s[verts], s["idx"])
        counts = oracle.render_tris(exp, s["cam"], s[spheres], W, H, s["Wp"], s["Hp"], SR, DEPTH, 0, sd, s[verts], s["idx"],
                                    pixels=pixels, bvh=bvh)
        bvh.close()
        for a in (exp, sd):
            a.setflags(write=False)
        scene["refs"][key] = (exp, sd, tuple(counts))
    return scene["refs"][key]


def context(pt, monkeypatch, scene, env, spheres="one", builder="host"):
    """A fresh context under `env`.  RT_SPLIT=0 unless `env` says otherwise: a frame of so few pixels
    would take the sample-split path by itself, whose ray counts include the chunks its repair pass
    renders a second time (test_split_tile)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {"RT_SPLIT": "0", **env}.items():
        monkeypatch.setenv(k, v)
    rt = pt.RayTracer(0)  # the knobs are read here and in setMesh
    rt.setSpheres(scene[spheres])
    rt.setCamera(scene["cam"])
    rt.setSampleRate(SR)
    rt.setMaxPathDepth(DEPTH)
    rt.setBuilder(builder)
    rt.setMesh(scene["verts"], scene["idx"])
    return rt


def render(rt, scene, tile=None, counting=False):
    rt.setSeeds(scene["Wp"], scene["Hp"], scene["seeds"])
    rt.setCounting(counting)
    rows = H if tile is None else int(((np.arange(H) // tile[0]) % tile[1] == tile[2]).sum())
    got = np.zeros(rows * W * 4, np.float32)
    rt.rayTrace(got, W, H, 0, kernel=2, tile=tile)
    return got, rt.getSeeds(), rt.counters(), rt.renderInfo()


def same_as(got, ref, what):
    frame, seeds, c, _ = got
    exp, sd, (closest, shadow) = ref
    np.testing.assert_array_equal(bits(frame), bits(exp), err_msg=f"{what}: frame")
    np.testing.assert_array_equal(seeds, sd, err_msg=f"{what}: seeds")
    assert (c["rays_closest"], c["rays_shadow"]) == (closest, shadow), (what, c, closest, shadow)


def test_frames_and_counts(pt, oracle, monkeypatch, scene):
    """With the split and without it: both the oracle's frame; the split's counting launch visits no
    more nodes."""
    ref = reference(scene, oracle, "one")
    out = {}
    for cone in ("1", "0"):
        rt = context(pt, monkeypatch, scene, {"RT_LIGHT_CONE": cone})
        info = rt.meshInfo()
        got = render(rt, scene)
        same_as(got, ref, f"RT_LIGHT_CONE={cone}")
        counted = render(rt, scene, counting=True)
        same_as(counted, ref, f"RT_LIGHT_CONE={cone}, counting")
        rt.close()
        root = info["n_nodes4"]
        assert info["n_nodes4_shadow"] > 0
        if cone == "1":
            assert info["cone_root"] == root + 1 and 0 < info["n_tris_cone"] < info["n_tris_tree"], info
            assert 4 * info["n_tris_cone"] >= info["n_tris_tree"], info
            assert 4 * (info["n_tris_tree"] - info["n_tris_cone"]) >= info["n_tris_tree"], info
            assert got[3]["shadow_start"] == counted[3]["shadow_start"] == info["cone_root"]
        else:
            assert info["cone_root"] == 0 and info["n_tris_cone"] == 0, info
            assert got[3]["shadow_start"] == counted[3]["shadow_start"] == root
        out[cone] = counted[2]
    print("nodes_visited, tris_tested: split", out["1"]["nodes_visited"], out["1"]["tris_tested"], "whole tree",
          out["0"]["nodes_visited"], out["0"]["tris_tested"])
    assert out["1"]["nodes_visited"] <= out["0"]["nodes_visited"]


def test_default_is_the_knob_on_or_off(pt, oracle, monkeypatch, scene):
    """Without the knob: the library's default, either way the oracle's frame."""
    rt = context(pt, monkeypatch, scene, {})
    same_as(render(rt, scene), reference(scene, oracle, "one"), "default")
    rt.close()


def test_two_lights(pt, oracle, monkeypatch, scene):
    rt = context(pt, monkeypatch, scene, {"RT_LIGHT_CONE": "1"}, spheres="two")
    info = rt.meshInfo()
    got = render(rt, scene)
    rt.close()
    assert info["cone_root"] and got[3]["shadow_start"] == info["cone_root"], (info, got[3])
    same_as(got, reference(scene, oracle, "two"), "two lights")


def test_moved_light_starts_at_the_whole_tree(pt, oracle, monkeypatch, scene):
    """setSpheres with the light elsewhere, no new setMesh: the split was made for another light, the
    queries walk the whole shadow tree; the light put back, they start at the subtree again."""
    rt = context(pt, monkeypatch, scene, {"RT_LIGHT_CONE": "1"})
    info = rt.meshInfo()
    assert info["cone_root"]
    rt.setSpheres(scene["moved"])
    got = render(rt, scene)
    assert rt.meshInfo() == info
    assert got[3]["shadow_start"] == info["n_nodes4"], got[3]
    same_as(got, reference(scene, oracle, "moved"), "moved light")
    rt.setSpheres(scene["one"])
    back = render(rt, scene)
    rt.close()
    assert back[3]["shadow_start"] == info["cone_root"]
    same_as(back, reference(scene, oracle, "one"), "light put back")


def test_refit_starts_at_the_whole_tree(pt, oracle, monkeypatch, scene):
    """updateMesh that refits (the mesh turned a quarter: other triangles face the light now): the
    split is the old records', the queries walk the whole shadow tree."""
    rt = context(pt, monkeypatch, scene, {"RT_LIGHT_CONE": "1"})
    info = rt.meshInfo()
    assert info["cone_root"]
    up = rt.updateMesh(scene["turned"])
    assert (up["action"], up["reason"]) == (pt._abi.RT_MESH_UPDATE_REFIT, pt._abi.RT_REFIT_OK), up
    got = render(rt, scene)
    rt.close()
    assert got[3]["shadow_start"] == info["n_nodes4"], got[3]
    same_as(got, reference(scene, oracle, "one", verts="turned"), "refitted")


def test_gpu_builder(pt, oracle, monkeypatch, scene):
    rt = context(pt, monkeypatch, scene, {"RT_LIGHT_CONE": "1"}, builder="gpu")
    info = rt.meshInfo()
    got = render(rt, scene)
    rt.close()
    assert info["builder"] == pt._abi.RT_BUILD_GPU and info["cone_root"] == 0 and got[3]["shadow_start"] == 0
    same_as(got, reference(scene, oracle, "one"), "gpu builder")


def test_split_tile(pt, oracle, monkeypatch, scene):
    """A 2-way row-stripe tile through the sample-split path (RT_SPLIT=1: chunk tasks): the oracle's
    frame and seeds.  The split path counts the rays of a speculated pixel's discarded chunks as well as
    those of its repair (rt_tris.hip: a camera ray that misses the mesh), so its ray counts are the
    oracle's plus that waste: equal to the oracle's when nothing was repaired, never below them, and
    the same with the split and without it."""
    tile = (8, 2, 1)
    rows = np.flatnonzero((np.arange(H) // tile[0]) % tile[1] == tile[2])
    pix = (rows[:, None] * W + np.arange(W)[None, :]).reshape(-1).astype(np.uint32)
    exp, sd, (closest, shadow) = reference(scene, oracle, "one", pixels=pix)
    rays = {}
    for cone in ("1", "0"):
        rt = context(pt, monkeypatch, scene, {"RT_LIGHT_CONE": cone, "RT_SPLIT": "1"})
        info = rt.meshInfo()
        frame, seeds, c, ri = render(rt, scene, tile=tile)
        rt.close()
        assert ri["split_chunks"] > 0 and ri["shadow_start"] == (info["cone_root"] if cone == "1" else info["n_nodes4"]), ri
        assert (info["cone_root"] != 0) == (cone == "1")
        np.testing.assert_array_equal(bits(frame), bits(exp.reshape(H, W * 4)[rows].reshape(-1)), err_msg=f"frame, cone {cone}")
        np.testing.assert_array_equal(seeds, sd, err_msg=f"seeds, cone {cone}")
        rays[cone] = (c["rays_closest"], c["rays_shadow"])
        print(f"split tile, RT_LIGHT_CONE={cone}: rays {rays[cone]}, oracle {(closest, shadow)}, repaired {ri['split_repaired']}")
        assert rays[cone][0] >= closest and rays[cone][1] >= shadow
        if ri["split_repaired"] == 0:
            assert rays[cone] == (closest, shadow)
    assert rays["1"] == rays["0"]


@pytest.mark.parametrize("depth", [1, 4, 7, 8, 9, 64])
def test_shadow_cache_cuts(pt, oracle, monkeypatch, scene, depth):
    """RT_SHADOW_CACHE_DEPTH from 1 to beyond the subtree's depth (its deepest level is 8: tests/
    test_light_cone_host.py prints the levels of the same build): the cut is a level of the subtree,
    or none."""
    rt = context(pt, monkeypatch, scene, {"RT_LIGHT_CONE": "1", "RT_SHADOW_CACHE_DEPTH": str(depth)})
    info = rt.meshInfo()
    got = render(rt, scene)
    rt.close()
    assert got[3]["shadow_start"] == info["cone_root"] != 0
    same_as(got, reference(scene, oracle, "one"), f"cut {depth}")
