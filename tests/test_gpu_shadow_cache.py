"""The shadow cache of the triangle megakernel (rt_traverse.h ShadowCut): a shadow
query from a mesh hit starts at the node of one tree level (the cut) under which the pixel's last
occluder was found, and restarts at the root when that subtree holds none.  An any-hit answer is
existential, so frames, seeds and ray counts must not move by a bit, whatever the cut:
RT_SHADOW_CACHE (0: off) and RT_SHADOW_CACHE_DEPTH (the cut's level) are read when a context is
created.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

RAYS = ("rays_closest", "rays_shadow", "rays_skipped")


def _render(pt, monkeypatch, env, verts, idx, W, H, sr, seeds, builder="host", tile=None, frames=1):
    """One fresh context under `env`: (frame bits of the last frame, both seed planes, ray counts
    per frame, mesh info)."""
    for k in ("RT_SHADOW_CACHE", "RT_SHADOW_CACHE_DEPTH", "RT_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = pt.scenes
    Wp, Hp = sc.padded_dims(W, H)
    rt = pt.RayTracer(0)  # the knobs are read here
    rt.setSpheres(sc.ply_scene())
    rt.setCamera(sc.camera_spherical(W, **sc.PLY_CAMERA))
    rt.setSampleRate(sr)
    rt.setMaxPathDepth(6)
    rt.setBuilder(builder)
    rt.setMesh(verts, idx)
    rt.setSeeds(Wp, Hp, seeds)
    rows = H if tile is None else int(((np.arange(H) // tile[0]) % tile[1] == tile[2]).sum())
    got = np.zeros(rows * W * 4, np.float32)
    rays = []
    for p in range(frames):
        rt.rayTrace(got, W, H, p, kernel=2, tile=tile)
        c = rt.counters()
        rays.append(tuple(c[k] for k in RAYS))
    out = (bits(got).copy(), rt.getSeeds().copy(), rays, rt.meshInfo(), rt.renderInfo())
    rt.close()
    return out


def _same(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=f"{what}: frame")
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"{what}: seeds")
    assert a[2] == b[2], f"{what}: ray counts {a[2]} != {b[2]}"


@pytest.fixture(scope="module")
def mesh20k(pt):
    return pt.scenes.make_mesh(20_000)


@pytest.fixture(scope="module")
def oracle20k(pt, oracle, mesh20k):
    """The 20 k mesh at 96x64, sampleRate 4, two progressive frames, by the oracle's BVH mode:
    (frame bits, seeds, (closest, shadow) per frame)."""
    sc = pt.scenes
    W, H, sr = 96, 64, 4
    Wp, Hp = sc.padded_dims(W, H)
    verts, idx = mesh20k
    seeds = sc.default_seeds(Wp, Hp, skip=5)
    sd = seeds.copy()
    exp = np.zeros(W * H * 4, np.float32)
    bvh = oracle.build_bvh(verts, idx)
    counts = []
    for p in range(2):
        counts.append(oracle.render_tris(exp, sc.camera_spherical(W, **sc.PLY_CAMERA), sc.ply_scene(), W, H, Wp, Hp, sr,
                                         6, p, sd, verts, idx, bvh=bvh))
    bvh.close()
    return dict(W=W, H=H, sr=sr, seeds=seeds, frame=bits(exp).copy(), seeds_out=sd, counts=counts)


@pytest.fixture(scope="module")
def off20k(pt, mesh20k, oracle20k):
    """The same two frames with the cache off (the form the whole-frame tests pin to the oracle)."""
    mp = pytest.MonkeyPatch()
    try:
        o = oracle20k
        return _render(pt, mp, {"RT_SHADOW_CACHE": "0"}, *mesh20k, o["W"], o["H"], o["sr"], o["seeds"], frames=2)
    finally:
        mp.undo()


def _vs_oracle(got, o, what):
    np.testing.assert_array_equal(got[0], o["frame"], err_msg=f"{what}: frame")
    np.testing.assert_array_equal(got[1], o["seeds_out"], err_msg=f"{what}: seeds")
    for p, (closest, shadow) in enumerate(o["counts"]):
        assert got[2][p][0] == closest and got[2][p][1] == shadow, (what, p, got[2][p], closest, shadow)


def test_default_cut_vs_oracle(pt, monkeypatch, mesh20k, oracle20k, off20k):
    """Cache on at the default cut: the oracle's BVH mode bit for bit, frames, seeds and ray counts."""
    o = oracle20k
    got = _render(pt, monkeypatch, {}, *mesh20k, o["W"], o["H"], o["sr"], o["seeds"], frames=2)
    _vs_oracle(got, o, "default cut")
    _vs_oracle(off20k, o, "cache off")
    _same(got, off20k, "on against off")


@pytest.mark.parametrize("depth", ["1", "deepest-1", "deepest", "beyond"])
def test_cut_extremes(pt, monkeypatch, mesh20k, oracle20k, off20k, depth):
    """A cut right below the root (nearly every try is answered), at the tree's deepest levels (most
    tries fail and restart at the root) and beyond the tree (an empty range, never armed): all
    bit-equal to the cache off."""
    o = oracle20k
    d4 = off20k[3]["depth4"]
    d = {"1": 1, "deepest-1": max(1, d4 - 1), "deepest": max(1, d4), "beyond": 64}[depth]
    got = _render(pt, monkeypatch, {"RT_SHADOW_CACHE_DEPTH": str(d)}, *mesh20k, o["W"], o["H"], o["sr"], o["seeds"],
                  frames=2)
    print(f"cut {d} (depth4 {d4}): rays {got[2]}")
    _same(got, off20k, f"cut {d}")


def test_tree_shallower_than_any_cut(pt, oracle, monkeypatch):
    """A 12-triangle mesh (one or two nodes): no level can be the cut, or only the last one; equal to
    the oracle with the default cut and with cuts 1 and 2 (no node outside the array is read: a cut
    is only ever a level the host found in the links)."""
    sc = pt.scenes
    W, H, sr = 32, 32, 2
    Wp, Hp = sc.padded_dims(W, H)
    verts, idx = sc.make_mesh(12)
    seeds = sc.default_seeds(Wp, Hp, skip=2)
    sd = seeds.copy()
    exp = np.zeros(W * H * 4, np.float32)
    closest, shadow = oracle.render_tris(exp, sc.camera_spherical(W, **sc.PLY_CAMERA), sc.ply_scene(), W, H, Wp, Hp, sr,
                                         6, 0, sd, verts, idx)
    for env in ({}, {"RT_SHADOW_CACHE_DEPTH": "1"}, {"RT_SHADOW_CACHE_DEPTH": "2"}, {"RT_SHADOW_CACHE": "0"}):
        got = _render(pt, monkeypatch, env, verts, idx, W, H, sr, seeds)
        np.testing.assert_array_equal(got[0], bits(exp), err_msg=str(env))
        np.testing.assert_array_equal(got[1], sd, err_msg=str(env))
        assert got[2][0][:2] == (closest, shadow), (env, got[2])


@pytest.fixture(scope="module")
def bunny(pt):
    """The bunny-class mesh at 1024x512, sampleRate 2: more pixels than resident lanes, so every
    lane takes many pixels in turn."""
    sc = pt.scenes
    W, H = 1024, 512
    Wp, Hp = sc.padded_dims(W, H)
    verts, idx = sc.make_mesh(sc.MESH_CONFIGS["bunny"])
    return dict(verts=verts, idx=idx, W=W, H=H, sr=2, seeds=sc.default_seeds(Wp, Hp, skip=1))


def test_lanes_take_many_pixels(pt, monkeypatch, bunny):
    """A lane's cache must not leak from one pixel to the next (it would still be exact, but the
    step counts would depend on the queue order): cache on equals cache off over a frame of more
    pixels than resident lanes."""
    b = bunny
    args = (b["verts"], b["idx"], b["W"], b["H"], b["sr"], b["seeds"])
    off = _render(pt, monkeypatch, {"RT_SHADOW_CACHE": "0"}, *args)
    on = _render(pt, monkeypatch, {}, *args)
    _same(on, off, "whole frame")


def test_split_tile(pt, monkeypatch, bunny):
    """The same frame's 8-way row-stripe tile through the sample-split path (RT_SPLIT=1: chunk
    tasks), on against off."""
    b = bunny
    args = (b["verts"], b["idx"], b["W"], b["H"], b["sr"], b["seeds"])
    tile = (8, 8, 3)
    off = _render(pt, monkeypatch, {"RT_SHADOW_CACHE": "0", "RT_SPLIT": "1"}, *args, tile=tile)
    on = _render(pt, monkeypatch, {"RT_SPLIT": "1"}, *args, tile=tile)
    assert on[4]["split_chunks"] > 0 and off[4]["split_chunks"] > 0, (on[4], off[4])
    _same(on, off, "split tile")


def test_gpu_builder_tree(pt, monkeypatch, mesh20k, oracle20k):
    """The GPU builder's one tree (the shadow queries walk the closest-hit tree from node 0): on
    against off, and against the oracle."""
    o = oracle20k
    args = (*mesh20k, o["W"], o["H"], o["sr"], o["seeds"])
    off = _render(pt, monkeypatch, {"RT_SHADOW_CACHE": "0"}, *args, builder="gpu", frames=2)
    on = _render(pt, monkeypatch, {}, *args, builder="gpu", frames=2)
    assert on[3]["builder"] == off[3]["builder"] == pt._abi.RT_BUILD_GPU
    _same(on, off, "gpu builder")
    _vs_oracle(on, o, "gpu builder, cache on")
