"""One context across frame sizes (csrc/rt_ctx.h DevBuf): its device buffers grow, are used again
after they grew, and are used again at a smaller size.  Most GPU tests keep one frame size per
context; here one context renders 16x8, then 64x40, then 24x16, and everything it returns is
compared bit for bit with a fresh context that has only ever seen that size — the triangle
kernel's frames (whole pixels, and sample-split with speculation and repairs), the display-side
stages through their host staging area against the same call on device buffers, and
rt_update_mesh after the sizes changed."""
from __future__ import annotations

import math

import numpy as np
import pytest

import refit_ref as rr
import tree_cases as tc
from conftest import bits

pytestmark = pytest.mark.gpu

SIZES = ((16, 8), (64, 40), (24, 16))
KNOBS = ("RT_INLINE_LIST", "RT_INLINE_CHAIN", "RT_LIST_MB", "RT_PIXEL_LISTS", "RT_SPLIT", "RT_SPLIT_SPEC", "RT_SPLIT_MB",
         "RT_SEED_WIDTH", "RT_REPAIR_SLOTS", "RT_PILOT", "RTMI_GRID_BLOCKS", "RT_SCHEDULE", "RT_SHADOW_CACHE")


def scene(sc):
    """The mesh scene with a second emissive sphere."""
    second = sc.init_sphere(center=(-3.0, 3.0, -1.0), radius=0.4, emission_power=1.0, emission=(0.6, 0.9, 1.3))
    return np.concatenate([sc.ply_scene(), second])


def context(pt, verts, idx, builder="host"):
    rt = pt.RayTracer(0)
    rt.setSpheres(scene(pt.scenes))
    rt.setMaxPathDepth(6)
    rt.setBuilder(builder)
    rt.setMesh(verts, idx)
    return rt


def frames(rt, sc, W, H, sr, n=2):
    """n progressive frames from explicitly set seeds: (frame bits, seed planes) after each."""
    Wp, Hp = sc.padded_dims(W, H)
    rt.setCamera(sc.camera_spherical(W, **sc.PLY_CAMERA))
    rt.setSampleRate(sr)
    rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp, skip=3))
    out = np.zeros(W * H * 4, np.float32)
    got = []
    for p in range(n):
        rt.rayTrace(out, W, H, p, kernel=2)
        got.append((bits(out).copy(), rt.getSeeds().copy()))
    return got


def same_frames(got, exp, what):
    for p, (g, e) in enumerate(zip(got, exp)):
        np.testing.assert_array_equal(g[0], e[0], err_msg=f"{what}, frame {p}")
        np.testing.assert_array_equal(g[1], e[1], err_msg=f"{what}, seeds after frame {p}")


# ---- 1. the triangle kernel's frames ---------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"RT_SPLIT": "1", "RT_SPLIT_SPEC": "2"}], ids=["default", "split_spec2"])
def test_frames_across_sizes(env, pt, tracer, monkeypatch):
    """Every frame of the one context equals a fresh context's with the same seeds.  With RT_SPLIT=1
    RT_SPLIT_SPEC=2 (every probe-hit pixel speculated, so repairs happen) the split, speculation and
    repair buffers, the box list and the list area all regrow."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = pt.scenes
    verts, idx = sc.make_mesh(2000)
    rt = context(pt, verts, idx)
    try:
        for sr in (2, 4):
            for W, H in SIZES:
                got = frames(rt, sc, W, H, sr)
                info = rt.renderInfo()
                fresh = context(pt, verts, idx)
                try:
                    exp = frames(fresh, sc, W, H, sr)
                finally:
                    fresh.close()
                same_frames(got, exp, f"{W}x{H} sampleRate {sr}")
                if env:
                    assert info["split_chunks"] > 0, "precondition: the frame is sample-split"
    finally:
        rt.close()


# ---- 2. the display-side stages through the staging area ---------------------------------------------
def display_calls(rt, pt, W, H, dev):
    """Every display-side call once at W x H, with host buffers or (dev) device buffers; the outputs
    as host arrays by name.  The inputs are functions of W, H alone."""
    import torch

    sc = pt.scenes
    px = W * H
    rng = np.random.default_rng(1000 * W + H)
    host_in = dict(rgba=rng.random(px * 4, np.float32), prev=rng.random(px * 4, np.float32),
                   hist=rng.random(px * 4, np.float32), mom=rng.random(px * 4, np.float32),
                   length=np.floor(rng.random(px, np.float32) * 9.0).astype(np.float32),
                   var=rng.random(px, np.float32))
    host_in["length1"] = host_in["length"] + 1.0

    def buf(a):
        if not dev:
            return a.copy()
        t = torch.from_numpy(a.copy()).cuda()
        torch.cuda.synchronize()
        return t

    def new(n):
        if not dev:
            return np.full(n, np.nan, np.float32)
        t = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (the library writes it on a stream of its own)
        return t

    def host(a):
        return bits(a.cpu().numpy() if dev else a).copy()

    out = {}
    rt.setCamera(sc.camera_spherical(W, **sc.MAIN_CAMERA))
    prev_cam = rt.getCamera(W)
    prev_feat = new(px * 8)
    rt.renderFeatures(prev_feat, W, H, kernel=2)
    rt.setCamera(sc.camera_spherical(W, **sc.PLY_CAMERA))
    feat = new(px * 8)
    rt.renderFeatures(feat, W, H, kernel=2)
    out["features"] = host(feat)
    i = {k: buf(v) for k, v in host_in.items()}
    for n in (1, 3):
        d = new(px * 4)
        rt.denoise(i["rgba"], feat, d, W, H, iterations=n)
        out[f"denoise{n}"] = host(d)
    o_rgba, o_len = new(px * 4), new(px)
    rt.reproject(i["prev"], i["length"], prev_feat, prev_cam, feat, o_rgba, o_len, W, H)
    out["reproject"], out["reproject_len"] = host(o_rgba), host(o_len)
    m_rgba, m_len = new(px * 4), new(px)
    rt.temporalMerge(i["hist"], i["length1"], i["rgba"], 2.0, m_rgba, m_len, W, H)
    out["merge"], out["merge_len"] = host(m_rgba), host(m_len)
    mom1, mom3 = new(px * 4), new(px * 4)
    rt.momentsAccumulate(None, i["rgba"], 1.0, None, mom1, W, H)
    rt.momentsAccumulate(i["prev"], i["rgba"], 3.0, i["mom"], mom3, W, H)
    out["moments_first"], out["moments_later"] = host(mom1), host(mom3)
    v = new(px)
    rt.variance(i["rgba"], i["mom"], i["length"], feat, v, W, H)
    out["variance"] = host(v)
    f1, f2, fv = new(px * 4), new(px * 4), new(px)
    rt.denoiseVar(i["rgba"], i["var"], feat, f1, None, W, H, iterations=3)
    rt.denoiseVar(i["rgba"], i["var"], feat, f2, fv, W, H, iterations=3)
    out["denoise_var"], out["denoise_var2"], out["denoise_var2_var"] = host(f1), host(f2), host(fv)
    for k, a in host_in.items():
        np.testing.assert_array_equal(host(i[k]), bits(a), err_msg=f"input {k} was written")
    return out


def stage_times(rt):
    return {"features": rt.lastFeaturesMs, "denoise": rt.lastDenoiseMs, "reproject": rt.lastReprojectMs,
            "merge": lambda: rt.lastReprojectMs(merge=True), "moments": lambda: rt.lastVarianceMs("moments"),
            "variance": lambda: rt.lastVarianceMs("variance"), "denoise_var": lambda: rt.lastVarianceMs("denoise_var")}


def test_display_stages_across_sizes(pt, tracer):
    """Host buffers (the staging area regrows, is reused, is reused at a smaller size) against device
    buffers on a fresh context, and every rt_last_*_ms: RT_ERR_STATE before its stage has run, a
    finite non-negative time after."""
    verts, idx = pt.scenes.make_mesh(2000)
    rt = context(pt, verts, idx)
    try:
        for name, get in stage_times(rt).items():
            with pytest.raises(pt.RtError) as e:
                get()
            assert e.value.status == pt._abi.RT_ERR_STATE, name
        for W, H in SIZES:
            got = display_calls(rt, pt, W, H, dev=False)
            fresh = context(pt, verts, idx)
            try:
                exp = display_calls(fresh, pt, W, H, dev=True)
            finally:
                fresh.close()
            assert got.keys() == exp.keys()
            for k in got:
                np.testing.assert_array_equal(got[k], exp[k], err_msg=f"{W}x{H}: {k}")
            assert (got["features"] != bits(np.full(8 * W * H, np.nan, np.float32))).any()
            for name, get in stage_times(rt).items():
                ms = get()
                assert math.isfinite(ms) and ms >= 0.0, (name, ms)
    finally:
        rt.close()


# ---- 3. rt_update_mesh after the sizes changed -----------------------------------------------------
@pytest.mark.parametrize("deform,action", [("rigid", "RT_MESH_UPDATE_REFIT"), ("wobble", "RT_MESH_UPDATE_REBUILT")])
def test_update_mesh_after_size_changes(deform, action, pt, tracer, monkeypatch):
    """det_bound (tests/tree_cases.py): moved rigidly it is refitted, wobbled it has newly hittable
    triangles and is rebuilt.  Either way the frames after the update equal a fresh rt_set_mesh of
    the moved vertices, and the rebuilt trees are that build's, bit for bit."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    sc = pt.scenes
    verts, idx = tc.make("det_bound", sc)
    nv = rr.DEFORM[deform](verts)
    rt = context(pt, verts, idx)
    fresh = context(pt, nv, idx)
    try:
        for W, H in SIZES:
            frames(rt, sc, W, H, 2, n=1)
        up = rt.updateMesh(nv)
        assert up["action"] == getattr(pt._abi, action), up
        if deform == "wobble":
            a, b = rt.meshTree(), fresh.meshTree()
            for k in ("nodes4", "nodes4q", "tris"):
                np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)
        for W, H in (SIZES[2], SIZES[1]):
            same_frames(frames(rt, sc, W, H, 2), frames(fresh, sc, W, H, 2), f"{deform}, {W}x{H}")
    finally:
        rt.close()
        fresh.close()
