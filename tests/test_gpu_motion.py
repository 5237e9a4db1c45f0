"""GPU: carrying the displayed frame across rt_update_mesh.  rt_warp_features
against its float32 numpy restatement (tests/motion_ref.py), bit for bit, on rendered and on synthetic
feature buffers; rt_mesh_pose; that the new calls leave a render's state alone; that the carry is not
vacuous; ProgressiveViewHIP::setMotionCarry through the rt_render CLI; and its effect on a turning mesh
of 1-spp frames.  Run on the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

import features_ref as fr
import motion_ref as mr
import refit_ref as rr
import render_state as rs
import temporal_ref as tr
import tree_cases as tc
import view_ref as vr
from conftest import bits
from test_motion_host import small_move

pytestmark = pytest.mark.gpu

F = np.float32
TARGET = (0.0, -4.0, 0.0)
EL0, AZ0, DIST = 40.0, 105.0, 5.0  # the golden view
SIZES = [(1, 1), (5, 3), (37, 29), (64, 48)]
MOTION_CAP = 8.0  # setMotionCarry's default


def new_tracer(pt, verts=None, idx=None):
    t = pt.RayTracer(0)
    t.setSpheres(pt.scenes.ply_scene())
    t.setSampleRate(1)
    t.setMaxPathDepth(6)
    t.setCameraSpherical(TARGET, EL0, AZ0, DIST)
    if verts is not None:
        t.setMesh(verts, idx)
    return t


@pytest.fixture(scope="module")
def mesh(pt):
    return pt.scenes.make_mesh(2000)  # the --mesh 2000 class (rt_make_mesh(2000, ...))


@pytest.fixture(scope="module")
def rt(pt, mesh):
    t = new_tracer(pt, *mesh)
    yield t
    t.close()


@pytest.fixture(scope="module")
def moved(rt, mesh):
    """deformation name -> the moved vertices; the tracer is left in that pose (rest -> moved by one
    rt_update_mesh), with the rest pose as the earlier one."""
    verts, idx = mesh
    cache = {}

    def get(name, move=None):
        if name not in cache:
            cache[name] = (move or rr.DEFORM[name])(verts)
        rt.setMesh(verts, idx)
        rt.updateMesh(cache[name])
        return cache[name]

    return get


def features(rt, w, h):
    feat = np.zeros(2 * w * h * 4, F)
    rt.renderFeatures(feat, w, h, kernel=2)
    return feat


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("deform", list(rr.DEFORM))
def test_warp_equals_numpy(deform, w, h, rt, mesh, moved):
    """The golden view of the moved mesh warped back into the rest pose: host pointers and device
    tensors, apart and in place; the inputs are only read."""
    import torch

    verts, idx = mesh
    cur = moved(deform)
    feat = features(rt, w, h)
    exp = mr.warp(feat, idx, cur, verts)
    keep = feat.copy(), verts.copy()
    out = np.full(2 * w * h * 4, np.nan, F)
    rt.warpFeatures(feat, verts, out, w, h)
    assert np.array_equal(bits(out), bits(exp))
    assert np.array_equal(bits(feat), bits(keep[0])) and np.array_equal(bits(verts), bits(keep[1]))
    assert rt.lastWarpMs() > 0.0
    inplace = feat.copy()
    rt.warpFeatures(inplace, verts, inplace, w, h)
    assert np.array_equal(bits(inplace), bits(exp))
    dfeat, dprev = torch.from_numpy(feat).cuda(), torch.from_numpy(verts).cuda()
    dout = torch.zeros_like(dfeat)
    rt.warpFeatures(dfeat, dprev, dout, w, h)
    assert np.array_equal(bits(dout.cpu().numpy()), bits(exp))
    assert np.array_equal(bits(dfeat.cpu().numpy()), bits(feat)) and np.array_equal(bits(dprev.cpu().numpy()), bits(verts))
    rt.warpFeatures(dfeat, dprev, dfeat, w, h)
    assert np.array_equal(bits(dfeat.cpu().numpy()), bits(exp))
    with pytest.raises(ValueError):
        rt.warpFeatures(feat, dprev, out, w, h)  # host and device buffers mixed
    if (w, h) == (64, 48):  # mesh pixels are there, and they moved
        ids = fr.feature_ids(exp)
        assert (ids >= 0).sum() > 1000 and not np.array_equal(bits(exp), bits(feat))


DEGENERATE = (10, 500, 1000)  # triangles of the 2000-triangle mesh that share no vertex


def _synthetic(verts, idx, w, h, seed):
    """A feature buffer no scene produces: every kind of id, among the triangle ids the first, the
    last, the one past the last and INT32_MAX; P on the triangle, or off its plane; three triangles
    (DEGENERATE) whose earlier pose test_warp_synthetic makes a point, a line, and one that overflows."""
    rng = np.random.default_rng(seed)
    n, nt = w * h, len(idx)
    pool = np.array([0, nt - 1, nt, 2 ** 31 - 1, fr.RT_FEAT_BOX, fr.RT_FEAT_NONE, fr.RT_FEAT_SPHERE0, fr.RT_FEAT_SPHERE0 - 5,
                     *DEGENERATE], np.int32)
    ids = np.where(rng.random(n) < 0.5, pool[rng.integers(0, len(pool), n)], rng.integers(0, nt, n)).astype(np.int32)
    ids[:len(pool)] = pool
    tri = verts[idx[np.clip(ids, 0, nt - 1)]]
    uv = rng.uniform(0.05, 0.45, (n, 2)).astype(F)
    P = (tri[:, 0] + uv[:, :1] * (tri[:, 1] - tri[:, 0]) + uv[:, 1:] * (tri[:, 2] - tri[:, 0])).astype(F)
    off = rng.random(n) < 0.3
    P[off] += rng.uniform(-0.5, 0.5, (int(off.sum()), 3)).astype(F)
    feat = np.zeros((2, n, 4), F)
    feat[0, :, :3], feat[0, :, 3] = P, rng.uniform(0.5, 9.0, n).astype(F)
    feat[1, :, :3] = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    feat[1, :, 3] = ids.view(F)
    return feat.reshape(-1), ids


def test_warp_synthetic(rt, mesh, moved):
    """Every pixel, none excepted, comes out "no surface" or finite, and equal to the restatement: ids
    that are no triangle's never reach an address, degenerate and overflowing earlier poses are dropped."""
    verts, idx = mesh
    cur = moved("wobble")
    w, h = 37, 29
    feat, ids = _synthetic(cur, idx, w, h, 11)
    prev = verts.copy()
    a, b, c = (idx[t] for t in DEGENERATE)
    assert len(set(a) | set(b) | set(c)) == 9
    prev[a] = prev[a[0]]                        # a point
    prev[b[2]] = prev[b[1]]                     # a line: e2' = e1', their cross product is exactly 0
    prev[c[0], 0], prev[c[1], 0] = -3e38, 3e38  # e1'.x and with it P'.x overflow
    exp = mr.warp(feat, idx, cur, prev)
    out = np.full_like(feat, np.nan)
    rt.warpFeatures(feat, prev, out, w, h)
    assert np.array_equal(bits(out), bits(exp))
    o, f = out.reshape(2, -1, 4), feat.reshape(2, -1, 4)
    oid = fr.feature_ids(out)
    none = oid == fr.RT_FEAT_NONE
    dropped = none & (ids != fr.RT_FEAT_NONE)
    assert np.array_equal(o[0, dropped], np.tile(np.array([0, 0, 0, np.inf], F), (int(dropped.sum()), 1)))
    assert not o[1, dropped, :3].any()
    kept = oid >= 0
    assert np.isfinite(o[:, kept, :3]).all() and np.array_equal(oid[kept], ids[kept])
    assert np.array_equal(bits(o[0, kept, 3]), bits(f[0, kept, 3]))
    assert dropped[(ids >= len(idx)) | np.isin(ids, DEGENERATE)].all()
    assert kept[(ids == 0) | (ids == len(idx) - 1)].all() and kept.sum() > 300
    assert np.array_equal(bits(o[:, ids < 0]), bits(f[:, ids < 0]))  # box, spheres, none: copied bit for bit


def test_mesh_pose(pt, mesh):
    """rt_mesh_pose after setMesh, after a refit, after a rebuild and after a refused update."""
    import torch

    ab = pt._abi
    verts, idx = mesh
    t = new_tracer(pt)
    try:
        with pytest.raises(ab.RtError) as e:
            t.meshPose()
        assert e.value.status == ab.RT_ERR_NO_MESH
        buf = np.zeros(3 * len(verts), F)
        assert t._lib.rt_mesh_pose(t._h, ab.ptr(buf), len(verts), 0) == ab.RT_ERR_NO_MESH
        t.setMesh(verts, idx)
        assert np.array_equal(bits(t.meshPose()), bits(verts))
        nv = rr.rigid(verts)
        assert t.updateMesh(nv)["action"] == ab.RT_MESH_UPDATE_REFIT
        assert np.array_equal(bits(t.meshPose()), bits(nv))
        dev = t.meshPose(device=True)
        assert dev.is_cuda and np.array_equal(bits(dev.cpu().numpy()), bits(nv))
        bad = rr.wobble(verts)
        bad[7, 1] = np.nan
        with pytest.raises(ab.RtError) as e:
            t.updateMesh(bad)
        assert e.value.status == ab.RT_ERR_ARG
        assert np.array_equal(bits(t.meshPose()), bits(nv))
        assert t._lib.rt_mesh_pose(t._h, ab.ptr(buf), len(verts) - 1, 0) == ab.RT_ERR_ARG
        assert t._lib.rt_mesh_pose(t._h, None, len(verts), 0) == ab.RT_ERR_ARG
        assert not buf.any()
        dverts, didx = tc.make("det_bound", pt.scenes)  # wobbled, it has newly hittable triangles: a rebuild
        t.setMesh(dverts, didx)
        assert np.array_equal(bits(t.meshPose()), bits(dverts))
        dn = rr.wobble(dverts)
        assert t.updateMesh(dn)["action"] == ab.RT_MESH_UPDATE_REBUILT
        assert np.array_equal(bits(t.meshPose()), bits(dn))
        out = torch.zeros(len(dn) * 3, dtype=torch.float32, device="cuda:0")
        t.meshPose(out)
        assert np.array_equal(bits(out.cpu().numpy().reshape(-1, 3)), bits(dn))
    finally:
        t.close()


def test_warp_argument_checks(pt, rt, mesh, moved):
    ab = pt._abi
    verts, idx = mesh
    moved("shrink")
    w, h = 5, 3
    feat = features(rt, w, h)
    out = np.zeros_like(feat)
    lib, p = rt._lib, ab.ptr
    nv = len(verts)
    assert lib.rt_warp_features(rt._h, None, p(verts), nv, p(out), w, h, 0) == ab.RT_ERR_ARG
    assert lib.rt_warp_features(rt._h, p(feat), None, nv, p(out), w, h, 0) == ab.RT_ERR_ARG
    assert lib.rt_warp_features(rt._h, p(feat), p(verts), nv, None, w, h, 0) == ab.RT_ERR_ARG
    assert lib.rt_warp_features(rt._h, p(feat), p(verts), nv, p(out), 0, h, 0) == ab.RT_ERR_ARG
    assert lib.rt_warp_features(rt._h, p(feat), p(verts), nv, p(out), w, 0, 0) == ab.RT_ERR_ARG
    assert lib.rt_warp_features(rt._h, p(feat), p(verts), nv - 1, p(out), w, h, 0) == ab.RT_ERR_ARG
    assert lib.rt_warp_features(rt._h, p(feat), p(verts), nv, p(out), w, h, 2) == ab.RT_ERR_ARG
    assert not out.any()
    t = new_tracer(pt)
    try:
        import ctypes

        ms = ctypes.c_float()
        assert t._lib.rt_last_warp_ms(t._h, ctypes.byref(ms)) == ab.RT_ERR_STATE
        assert t._lib.rt_warp_features(t._h, p(feat), p(verts), nv, p(out), w, h, 0) == ab.RT_ERR_NO_MESH
    finally:
        t.close()
    assert not out.any()


def test_render_state_untouched(pt, golden, golden_meta):
    """The golden progressive frames with rt_warp_features and rt_mesh_pose in between — device tensors
    on a side stream behind a render enqueued without a wait, host buffers on the context's stream — are
    the frames, seeds, counter totals, render info and rt_read of the sequence without them
    (tests/render_state.py)."""
    import torch

    with rs.untouched(pt, golden, golden_meta) as (t, frame, g, m):
        W, H = m["W"], m["H"]
        verts, idx = g["verts"], g["idx"]
        feat = np.zeros(2 * W * H * 4, F)
        t.renderFeatures(feat, W, H, kernel=2)
        prev = rr.shrink(verts)
        exp = mr.warp(feat, idx, verts, prev)
        dfeat, dprev = torch.from_numpy(feat).cuda(), torch.from_numpy(prev).cuda()
        douts = [torch.zeros_like(dfeat) for _ in range(m["frames"])]
        host_out = np.zeros_like(feat)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        for p in range(m["frames"]):
            t.rayTrace(frame, W, H, p, kernel=2, sync=False)
            t.warpFeatures(dfeat, dprev, douts[p], W, H, stream=side.cuda_stream, sync=False)
            if p == 1:  # and host buffers on the context's own stream
                t.warpFeatures(feat, prev, host_out, W, H)
                assert np.array_equal(bits(t.meshPose()), bits(verts))
    for d in douts:
        assert np.array_equal(bits(d.cpu().numpy()), bits(exp))
    assert np.array_equal(bits(host_out), bits(exp))


def test_not_vacuous(rt, mesh, moved):
    """After small_move (tests/test_motion_host.py: 5 degrees and a quarter of rigid's translation; the
    restatement over the oracle's features gives 0.8696 there, and 0.378 for rigid itself, whose 20
    degrees bring in what lay outside the frame the mesh overfills) at 64 x 48: at least half of the
    view's mesh pixels find history through warp + rt_reproject, and what they carry is not what an
    unwarped rt_reproject carries."""
    verts, idx = mesh
    w, h = 64, 48
    rt.setMesh(verts, idx)
    cam = rt.getCamera(w)
    pfeat = features(rt, w, h)
    cur = moved("small", small_move)
    cfeat = features(rt, w, h)
    warped = np.zeros_like(cfeat)
    rt.warpFeatures(cfeat, verts, warped, w, h)
    rng = np.random.default_rng(4)
    col = rng.random(w * h * 4, dtype=F)
    ln = (F(1.0) + rng.random(w * h, dtype=F) * F(3.0)).astype(F)
    res = {}
    for label, cf in (("warp", warped), ("plain", cfeat)):
        out, ol = np.full(w * h * 4, np.nan, F), np.full(w * h, np.nan, F)
        rt.reproject(col, ln, pfeat, cam, cf, out, ol, w, h, max_history=MOTION_CAP)
        res[label] = (out, ol)
    assert np.array_equal(bits(res["warp"][0]), bits(tr.reproject(col, ln, pfeat, cam, mr.warp(cfeat, idx, cur, verts), w, h,
                                                                   max_history=MOTION_CAP)[0]))
    meshpx = fr.feature_ids(cfeat) >= 0
    share = float((res["warp"][1] > 0)[meshpx].mean())
    plain_share = float((res["plain"][1] > 0)[meshpx].mean())
    print(f"mesh pixels with history: {share:.4f} through the warp, {plain_share:.4f} without it")
    assert share >= 0.5
    both = meshpx & (res["warp"][1] > 0) & (res["plain"][1] > 0)
    a, b = res["warp"][0].reshape(-1, 4)[both, :3], res["plain"][0].reshape(-1, 4)[both, :3]
    assert both.sum() > 50 and (np.abs(a - b).max(axis=1) > 1e-3).mean() > 0.9
    box = fr.feature_ids(cfeat) == fr.RT_FEAT_BOX  # off the mesh the warp changes nothing
    assert np.array_equal(bits(res["warp"][0].reshape(-1, 4)[box]), bits(res["plain"][0].reshape(-1, 4)[box]))


EVENTS = "d,d,p:1,d,p:2,l,d,d"
# (pose, azimuth, progression) of the five displayed frames: an update restarts the progression like a key press
SHOWN = [(0, AZ0, 0), (0, AZ0, 1), (1, AZ0, 1), (2, AZ0 + 3.0, 1), (2, AZ0 + 3.0, 2)]


@pytest.mark.parametrize("denoise", [False, True])
def test_progressive_view_motion_carry(denoise, rt, pt, mesh, tmp_path):
    """ProgressiveViewHIP::setMotionCarry through the rt_render CLI: two displays, a mesh update, a
    display, another update and a key press, two displays.  With --motion-carry every displayed frame is
    the recomposition of warpFeatures / reproject / temporalMerge (/ denoise) through the Python API
    (tests/view_ref.py); without it the history is dropped at every update, as before; the accumulation
    buffers of both runs are the same; and the runs differ exactly from the first display after an
    update on."""
    W, H = 64, 48
    px = W * H * 4
    verts, idx = mesh
    poses = np.stack([verts, small_move(verts), rr.wobble(verts)]).astype(F)
    pfile = tmp_path / "poses.f32"
    poses.tofile(pfile)
    flags = vr.Flags(temporal=True, denoise=denoise, motion_carry=True)
    variants = {"off": flags.without("motion_carry"), "on": flags}
    runs = {}
    for name, fl in variants.items():
        runs[name] = run = vr.run_view(tmp_path, ["--mesh", "2000", "--poses", str(pfile), "--events", EVENTS] + fl.cli())
        lines = run["lines"]
        ups = [l for l in lines if l.get("event", "").startswith("p:")]
        assert len(ups) == 2 and all(l["mesh_update"] in ("refit", "rebuilt") and l["progression"] == 0 for l in ups)
        assert all("mesh_update" not in l for l in lines if l not in ups)
        pose, seen = 0, []
        for l in lines:
            if l in ups:
                pose = int(l["event"][2:])
            if l.get("rendered"):
                seen.append((pose, l["azimuth"], l["progression"]))
        assert seen == SHOWN
    on, off = runs["on"], runs["off"]
    assert on["shown"].size == off["shown"].size == on["raw"].size == len(SHOWN) * px and on["feat"].size == 2 * len(SHOWN) * px
    assert np.array_equal(bits(on["raw"]), bits(off["raw"])) and np.array_equal(bits(on["feat"]), bits(off["feat"]))
    for name, run in runs.items():
        exp = vr.displayed(rt, pt.scenes, variants[name], EVENTS, run["raw"], run["feat"], W, H, mesh=mesh, poses=poses)
        assert len(exp.frames) == len(SHOWN)
        for k, disp in enumerate(exp.frames):
            assert np.array_equal(bits(run["shown"][px * k:px * (k + 1)]), bits(disp)), f"{name}: displayed frame {k}"
        if name == "on":
            assert (exp.lengths[-1] > 2).mean() > 0.3  # the last view's two frames on top of what was carried into it
    for k in range(len(SHOWN)):
        same = np.array_equal(bits(on["shown"][px * k:px * (k + 1)]), bits(off["shown"][px * k:px * (k + 1)]))
        assert same == (k < 2), f"displayed frame {k} against the run without --motion-carry"


def turn(verts, deg, centre):
    """`deg` degrees about the vertical axis through `centre`, binary64, rounded to float32."""
    v, c = np.asarray(verts, F).astype(np.float64), np.array(centre, np.float64)
    a = np.deg2rad(deg)
    d = v - c
    out = np.stack([np.cos(a) * d[:, 0] + np.sin(a) * d[:, 2], d[:, 1], -np.sin(a) * d[:, 0] + np.cos(a) * d[:, 2]], axis=1)
    return np.ascontiguousarray((out + c).astype(F))


def test_motion_quality(rt, pt, mesh):
    """The golden view at 128 x 96 (camera[0:4] *= 2), the camera static, 12 poses of the mesh turning 2
    degrees per pose about the vertical axis through its centre, 1 spp each, the history carried from
    pose to pose through the warp (motion cap 8, the default; temporal cap 32); mean squared errors of
    the last pose's frames against a sampleRate-16 frame of it from other seeds.  Evaluated beforehand
    with the restatements over the oracle's frames (its BVH mode) of exactly these inputs:
        1-spp frame 2.2609e-3, merged (unfiltered) 3.2429e-4: 6.97 times lower (motion cap 2 / 4 / 16:
        4.17 / 5.96 / 7.01 times; carried without the warp: 3.4051e-4);
        a-trous alone 7.9107e-5 / 5.3483e-5 / 5.4875e-5 at 2 / 3 / 5 passes, merged then 3 passes
        3.2123e-5: 1.66 times below the best of them.
    The conditions, set in advance at half the measured gain and never below 1: the merged frame's
    error is at most 1 / 3.48 of the 1-spp frame's; merged then 3 passes is no worse than the best
    a-trous-alone frame (half of 1.66 is below 1).
    The whole-frame error is the box's: the tenth of the frame that is not mesh carries nine tenths of
    it and keeps its history with or without the warp.  On the mesh pixels alone (0.896 of the frame)
    the same evaluation gives 1-spp 2.012e-5, merged 1.132e-5 (1.78 times lower; motion cap 2: 2.36
    times), carried without the warp 2.943e-5 (worse than the 1-spp frame), and with 3 a-trous passes
    8.88e-6 merged against 6.29e-6 alone: on this turning, diffusely lit mesh the carried radiance
    lags the shading, and the cap bounds that lag, not the noise.  The third condition holds the warp
    to what it is for: on the mesh pixels the merged frame is no worse than the 1-spp frame (half of
    1.78 is below 1)."""
    sc = pt.scenes
    W, H = 128, 96
    Wp, Hp = sc.padded_dims(W, H)
    verts, idx = mesh
    cam = sc.camera_spherical(64, target=TARGET, elevation=EL0, azimuth=AZ0, distance=DIST)
    cam[0:4] *= 2
    rt.setMesh(verts, idx)
    rt.setCamera(cam)
    rt.setSampleRate(1)
    rt.setMaxPathDepth(6)
    rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp))
    poses = [turn(verts, 2.0 * k, sc.MESH_CENTER) for k in range(12)]
    hist = hl = pfeat = None
    try:
        for k in range(12):
            if k:
                rt.updateMesh(poses[k])
            frame = np.zeros(W * H * 4, F)
            rt.rayTrace(frame, W, H, 0, kernel=2)
            feat = features(rt, W, H)
            car, cl = np.zeros(W * H * 4, F), np.zeros(W * H, F)
            if hist is not None:
                warped = np.zeros_like(feat)
                rt.warpFeatures(feat, poses[k - 1], warped, W, H)
                rt.reproject(hist, hl, pfeat, cam, warped, car, cl, W, H, max_history=min(32.0, MOTION_CAP))
            hist, hl = np.zeros(W * H * 4, F), np.zeros(W * H, F)
            rt.temporalMerge(car, cl, frame, 1.0, hist, hl, W, H)
            pfeat = feat
        ref = np.zeros(W * H * 4, F)
        rt.setSampleRate(16)
        rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp, skip=12345))
        rt.rayTrace(ref, W, H, 0, kernel=2)
    finally:
        rt.setSampleRate(1)
        rt.setCameraSpherical(TARGET, EL0, AZ0, DIST)
    meshpx = fr.feature_ids(feat) >= 0

    def mse(a, sel=slice(None)):
        d = a.reshape(-1, 4)[sel, :3].astype(np.float64) - ref.reshape(-1, 4)[sel, :3].astype(np.float64)
        return float((d * d).mean())

    def filtered(src, it):
        out = np.zeros_like(src)
        rt.denoise(src, feat, out, W, H, iterations=it)
        return out

    alone = {it: mse(filtered(frame, it)) for it in (2, 3, 5)}
    merged3 = mse(filtered(hist, 3))
    print(f"mse 1-spp {mse(frame):.4e} merged {mse(hist):.4e} ratio {mse(frame) / mse(hist):.2f}; a-trous alone "
          f"{alone}; merged then 3 passes {merged3:.4e} ratio {min(alone.values()) / merged3:.2f}; mesh pixels "
          f"({meshpx.mean():.3f}): 1-spp {mse(frame, meshpx):.4e} merged {mse(hist, meshpx):.4e}")
    assert mse(hist) <= mse(frame) / 3.48
    assert merged3 <= min(alone.values())
    assert mse(hist, meshpx) <= mse(frame, meshpx)
