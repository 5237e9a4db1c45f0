"""GPU: carrying the displayed frame across sphere moves.  rt_warp_features_spheres
against its float32 numpy restatement (tests/sphere_motion_ref.py), bit for bit, on rendered and on
synthetic feature buffers; its argument checks; that the call leaves a render's state alone; that the
carry is not vacuous; ProgressiveViewHIP::setSphereCarry through the rt_render CLI; and its effect on a
dragged sphere of 1-spp frames.  Run on the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

import ctypes
from dataclasses import replace

import numpy as np
import pytest

import features_ref as fr
import sphere_motion_ref as sm
import temporal_ref as tr
import view_ref as vr
from conftest import bits
from test_sphere_motion_host import MOVES, moved_scene

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(1, 1), (5, 3), (37, 29), (64, 48)]
SPHERE_CAP = 8.0  # setSphereCarry's default
ALL_MOVES = dict(MOVES, nothing={})


def new_tracer(pt, spheres=None):
    t = pt.RayTracer(0)
    if spheres is not None:
        t.setSpheres(spheres)
    t.setSampleRate(1)
    t.setMaxPathDepth(6)
    c = pt.scenes.MAIN_CAMERA
    t.setCameraSpherical(c["target"], c["elevation"], c["azimuth"], c["distance"])
    return t


@pytest.fixture(scope="module")
def rt(pt):
    t = new_tracer(pt, pt.scenes.main_scene())
    yield t
    t.close()


def features(rt, w, h):
    feat = np.zeros(2 * w * h * 4, F)
    rt.renderFeatures(feat, w, h, kernel=rt.KERNEL_SPHERES)
    return feat


def device_bytes(spheres):
    import torch

    return torch.from_numpy(np.ascontiguousarray(spheres).view(np.uint8).copy()).cuda()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("move", list(ALL_MOVES))
def test_warp_equals_numpy(move, w, h, rt, pt):
    """The sphere golden view of the moved scene warped back onto main_scene(): host pointers and device
    tensors, apart and in place; the inputs are only read."""
    import torch

    prev, cur = moved_scene(pt, {}), moved_scene(pt, ALL_MOVES[move])
    rt.setSpheres(cur)
    feat = features(rt, w, h)
    exp = sm.warp_spheres(feat, cur, prev)
    keep = feat.copy(), prev.copy()
    out = np.full(2 * w * h * 4, np.nan, F)
    rt.warpFeaturesSpheres(feat, prev, out, w, h)
    assert np.array_equal(bits(out), bits(exp))
    assert np.array_equal(bits(feat), bits(keep[0])) and prev.tobytes() == keep[1].tobytes()
    assert rt.lastSphereWarpMs() > 0.0
    inplace = feat.copy()
    rt.warpFeaturesSpheres(inplace, prev, inplace, w, h)
    assert np.array_equal(bits(inplace), bits(exp))
    dfeat, dprev = torch.from_numpy(feat).cuda(), device_bytes(prev)
    dout = torch.zeros_like(dfeat)
    rt.warpFeaturesSpheres(dfeat, dprev, dout, w, h)
    assert np.array_equal(bits(dout.cpu().numpy()), bits(exp))
    assert np.array_equal(bits(dfeat.cpu().numpy()), bits(feat)) and dprev.cpu().numpy().tobytes() == prev.tobytes()
    rt.warpFeaturesSpheres(dfeat, dprev, dfeat, w, h)
    assert np.array_equal(bits(dfeat.cpu().numpy()), bits(exp))
    with pytest.raises(ValueError):
        rt.warpFeaturesSpheres(feat, dprev, out, w, h)  # host and device buffers mixed
    if move == "nothing":
        assert np.array_equal(bits(exp), bits(feat))
    elif (w, h) == (64, 48) and move != "light":  # the moved spheres are in view (the light is above it)
        changed = (bits(exp).reshape(2, -1, 4) != bits(feat).reshape(2, -1, 4)).any(axis=(0, 2))
        print(f"{move}: {changed.sum()} pixels differ from the input")
        assert changed.sum() > 100


BAD = [("radius", 0.0), ("radius", -1.0), ("radius", np.nan), ("radius", np.inf), ("radius", 1e38), ("center", np.inf),
       ("center", -np.inf), ("center", np.nan)]


def _synthetic(n_cur, w, h, seed):
    """A feature buffer no scene produces: every kind of id, normals with NaN components, and normals
    large enough to overflow against a radius of 1e38."""
    rng = np.random.default_rng(seed)
    n = w * h
    pool = np.array([0, 5, 2 ** 31 - 1, fr.RT_FEAT_BOX, fr.RT_FEAT_NONE, *range(-15, -2), fr.RT_FEAT_SPHERE0,
                     fr.RT_FEAT_SPHERE0 - (n_cur - 1), fr.RT_FEAT_SPHERE0 - n_cur, fr.RT_FEAT_SPHERE0 - (n_cur + 1), -2 ** 31],
                    np.int64).astype(np.int32)
    ids = np.where(rng.random(n) < 0.3, pool[rng.integers(0, len(pool), n)],
                   fr.RT_FEAT_SPHERE0 - rng.integers(0, n_cur + 2, n)).astype(np.int32)
    ids[:len(pool)] = pool
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm.astype(F)
    nrm[rng.random(n) < 0.2] *= F(10.0)  # 1e38 * 10 overflows
    nan = rng.random(n) < 0.1
    nrm[nan, rng.integers(0, 3, int(nan.sum()))] = np.nan
    feat = np.zeros((2, n, 4), F)
    feat[0, :, :3], feat[0, :, 3] = rng.uniform(-6, 6, (n, 3)).astype(F), rng.uniform(0.5, 9.0, n).astype(F)
    feat[1, :, :3], feat[1, :, 3] = nrm, ids.view(F)
    return feat.reshape(-1), ids


@pytest.mark.parametrize("n_cur", [1, 6, 70])
def test_warp_synthetic(n_cur, pt):
    """Every pixel, none excepted, equals the restatement: ids that name no sphere of both lists never
    reach an address, earlier spheres that cannot hold a point are dropped, NaN normals are."""
    w, h = 37, 29
    rng = np.random.default_rng(100 + n_cur)
    cur = np.zeros(n_cur, pt._abi.SPHERE_DTYPE)
    cur["center"], cur["radius"] = rng.uniform(-6, 6, (n_cur, 3)), rng.uniform(0.1, 3.0, n_cur)
    base = np.zeros(n_cur + 1, pt._abi.SPHERE_DTYPE)
    base["center"], base["radius"] = rng.uniform(-6, 6, (n_cur + 1, 3)), rng.uniform(0.1, 3.0, n_cur + 1)
    base[n_cur // 2] = cur[n_cur // 2]  # one that stands where it stood
    feat, ids = _synthetic(n_cur, w, h, n_cur)
    t = new_tracer(pt, cur)
    try:
        for n_prev in sorted({0, 1, n_cur - 1, n_cur, n_cur + 1}):
            for field, value in BAD if n_prev else BAD[:1]:
                prev = base[:n_prev].copy()
                for j in range(0, n_prev, 3):  # every third earlier sphere is a bad one
                    if field == "radius":
                        prev["radius"][j] = value
                    else:
                        prev["center"][j, j % 3] = value
                exp = sm.warp_spheres(feat, cur, prev)
                out = np.full_like(feat, np.nan)
                t.warpFeaturesSpheres(feat, prev, out, w, h)
                assert np.array_equal(bits(out), bits(exp)), (n_prev, field, value)
                o, f = out.reshape(2, -1, 4), feat.reshape(2, -1, 4)
                oid = fr.feature_ids(out)
                assert np.array_equal(bits(o[:, ids > fr.RT_FEAT_SPHERE0]), bits(f[:, ids > fr.RT_FEAT_SPHERE0]))
                s = fr.RT_FEAT_SPHERE0 - ids.astype(np.int64)
                outside = (ids <= fr.RT_FEAT_SPHERE0) & ((s >= n_cur) | (s >= n_prev))
                assert outside.any() and (oid[outside] == fr.RT_FEAT_NONE).all()
                kept = (ids <= fr.RT_FEAT_SPHERE0) & (oid != fr.RT_FEAT_NONE)
                moved = kept & (s != n_cur // 2)
                assert np.isfinite(o[0, moved, :3]).all() and np.array_equal(oid[kept], ids[kept])
                if n_cur >= 6 and n_prev >= n_cur:  # spheres 1, 2, 4, 5, ... have an earlier self that can hold a point
                    assert kept.any()
    finally:
        t.close()


def test_errors_and_state(pt, rt):
    """Every RT_ERR_ARG / RT_ERR_NO_SCENE case; a render before and after the call gives the frame, the
    seeds and the ray counts of the renders without it; no mesh is ever set."""
    ab = pt._abi
    w, h = 37, 29
    S = moved_scene(pt, {})
    prev = moved_scene(pt, MOVES["sphere2"])
    rt.setSpheres(S)
    big = np.zeros(2 * (8 * w * h) + 64, F)  # room for overlapping views
    feat, out = big[:8 * w * h], big[8 * w * h + 32:16 * w * h + 32]
    feat[:] = features(rt, w, h)
    lib, p, H_ = rt._lib, ab.ptr, rt._h
    call = lib.rt_warp_features_spheres
    assert call(H_, None, p(prev), 6, p(out), w, h, 0) == ab.RT_ERR_ARG
    assert call(H_, p(feat), p(prev), 6, None, w, h, 0) == ab.RT_ERR_ARG
    assert call(H_, p(feat), None, 6, p(out), w, h, 0) == ab.RT_ERR_ARG
    assert call(H_, p(feat), p(prev), 6, p(out), 0, h, 0) == ab.RT_ERR_ARG
    assert call(H_, p(feat), p(prev), 6, p(out), w, 0, 0) == ab.RT_ERR_ARG
    assert call(H_, p(feat), p(prev), 6, p(out), 1 << 14, 1 << 14, 0) == ab.RT_ERR_ARG
    assert call(H_, p(feat), p(prev), 6, p(out), w, h, 2) == ab.RT_ERR_ARG
    assert call(H_, p(feat), p(prev), 6, p(out), w, h, ab.RT_OUT_DEVICE | 4) == ab.RT_ERR_ARG
    # out_feat overlapping cur_feat other than exactly, from either side, and overlapping the earlier spheres
    assert call(H_, p(feat), p(prev), 6, p(big[4:]), w, h, 0) == ab.RT_ERR_ARG
    assert call(H_, p(big[4:]), p(prev), 6, p(feat), w, h, 0) == ab.RT_ERR_ARG
    assert call(H_, p(feat), p(big[8 * w * h - 4:]), 6, p(out), w, h, 0) == ab.RT_ERR_ARG
    assert call(H_, p(feat), p(out[-20:]), 1, p(out), w, h, 0) == ab.RT_ERR_ARG
    assert lib.rt_warp_features_spheres_async(H_, p(feat), p(out[-20:]), 1, p(out), w, h, 0, None) == ab.RT_ERR_ARG
    assert not out.any()
    # legal: no earlier spheres at all (a null list), and exactly in place
    exp0 = sm.warp_spheres(feat, S, S[:0])
    assert call(H_, p(feat), None, 0, p(out), w, h, 0) == ab.RT_OK
    assert np.array_equal(bits(out), bits(exp0)) and (fr.feature_ids(out) > fr.RT_FEAT_SPHERE0).all()
    t = pt.RayTracer(0)
    try:
        ms = ctypes.c_float()
        assert t._lib.rt_last_sphere_warp_ms(t._h, ctypes.byref(ms)) == ab.RT_ERR_STATE
        assert t._lib.rt_warp_features_spheres(t._h, p(feat), p(prev), 6, p(out), w, h, 0) == ab.RT_ERR_NO_SCENE
        t.setSpheres(S[:0])
        t._sync_scene()
        assert t._lib.rt_warp_features_spheres(t._h, p(feat), p(prev), 6, p(out), w, h, 0) == ab.RT_ERR_NO_SCENE
        assert t._lib.rt_last_sphere_warp_ms(t._h, ctypes.byref(ms)) == ab.RT_ERR_STATE
    finally:
        t.close()
    # the render state: frames 0 and 1 of a progressive render with the call between them and after them
    sc = pt.scenes
    Wp, Hp = sc.padded_dims(w, h)
    res = {}
    for name in ("plain", "with"):
        t = new_tracer(pt, S)
        try:
            t.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp))
            t.setCounting(True)
            frame = np.zeros(w * h * 4, F)
            rays = []
            for prog in (0, 1):
                t.rayTrace(frame, w, h, prog, kernel=t.KERNEL_SPHERES)
                c = t.counters()
                rays.append((c["rays_closest"], c["rays_shadow"]))
                if name == "with":
                    o2 = np.zeros(8 * w * h, F)
                    t.warpFeaturesSpheres(np.ascontiguousarray(feat), prev, o2, w, h)
                    assert np.array_equal(bits(o2), bits(sm.warp_spheres(feat, S, prev)))
            back = np.zeros(w * h * 4, F)
            t.read(back)
            res[name] = (frame.copy(), back, t.getSeeds(), rays)
        finally:
            t.close()
    a, b = res["plain"], res["with"]
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[0]), bits(a[1]))
    assert np.array_equal(a[2], b[2]) and a[3] == b[3] and all(r[0] > 0 for r in a[3])


def test_not_vacuous(rt, pt):
    """Sphere 2 moved by (0.25, 0, 0.1) at 64 x 48, a history of ones.  The precondition, on the
    restatement over the device's features: at least half of sphere 2's pixels in the new view receive
    history through the warped features, and fewer than a fifth through the unwarped ones (the
    restatement over restated features, tests/test_sphere_motion_host.py: 0.9646 and 0).  Then the device's
    warp + rt_reproject equals the restatement chain bit for bit."""
    w, h = 64, 48
    prev, cur = moved_scene(pt, {}), moved_scene(pt, MOVES["sphere2"])
    rt.setSpheres(prev)
    cam = rt.getCamera(w)
    pfeat = features(rt, w, h)
    rt.setSpheres(cur)
    cfeat = features(rt, w, h)
    col, ln = np.ones(w * h * 4, F), np.ones(w * h, F)
    px2 = fr.feature_ids(cfeat) == fr.RT_FEAT_SPHERE0 - 2
    exp_warp = tr.reproject(col, ln, pfeat, cam, sm.warp_spheres(cfeat, cur, prev), w, h, max_history=SPHERE_CAP)
    exp_plain = tr.reproject(col, ln, pfeat, cam, cfeat, w, h, max_history=SPHERE_CAP)
    share, plain_share = float((exp_warp[1] > 0)[px2].mean()), float((exp_plain[1] > 0)[px2].mean())
    print(f"sphere 2's {px2.sum()} pixels with history: {share:.4f} through the warp, {plain_share:.4f} without it")
    assert px2.sum() > 200 and share >= 0.5 and plain_share < 0.2
    warped = np.zeros_like(cfeat)
    rt.warpFeaturesSpheres(cfeat, prev, warped, w, h)
    out, ol = np.full(w * h * 4, np.nan, F), np.full(w * h, np.nan, F)
    rt.reproject(col, ln, pfeat, cam, warped, out, ol, w, h, max_history=SPHERE_CAP)
    assert np.array_equal(bits(out), bits(exp_warp[0])) and np.array_equal(bits(ol), bits(exp_warp[1]))
    rt.reproject(col, ln, pfeat, cam, cfeat, out, ol, w, h, max_history=SPHERE_CAP)
    assert np.array_equal(bits(out), bits(exp_plain[0])) and np.array_equal(bits(ol), bits(exp_plain[1]))


# ---- ProgressiveViewHIP::setSphereCarry through rt_render --events ----

VW, VH = 64, 48
EVENTS = "d,d,o:2:0.25:0:0.1,d,d,o:2:0.1:0:0,o:0:0:0.2:0,d,l,d,s:48:40,d"
N_SHOWN = 7
VIEW_FLAGS = {
    "plain": (vr.Flags(temporal=True), []),
    "variance": (vr.Flags(temporal=True, variance_guided=True), []),
    "trust": (vr.Flags(temporal=True, history_trust=True), []),
    "denoise": (vr.Flags(temporal=True, denoise=True), []),
    "tonemap": (vr.Flags(temporal=True), ["--tonemap"]),
}


@pytest.mark.parametrize("flags", list(VIEW_FLAGS))
def test_view_sphere_carry(flags, rt, pt, tmp_path):
    """Two displays, a move of sphere 2, two displays, moves of spheres 2 and 0 (the oldest list is the
    one kept), a display, a key press, a display, a reshape, a display.  With --sphere-carry every
    displayed frame is the recomposition of warpFeaturesSpheres / reproject / (historyTrust) / temporalMerge
    / (the filters) through the Python API; without it the frames are those of sceneChanged() as it was
    (the history dropped at every o event, or with --history-trust kept where it was); the accumulation
    buffers and the features of both runs are the same, and the runs differ from the first display after
    a move on."""
    fl, extra = VIEW_FLAGS[flags]
    tone = "--tonemap" in extra
    outputs = ("shown", "raw", "feat") + (("f8",) if tone else ())
    spheres0 = moved_scene(pt, {})
    px = VW * VH * 4
    variants = {"off": fl, "on": replace(fl, sphere_carry=True)}
    runs = {}
    for name, v in variants.items():
        runs[name] = vr.run_view(tmp_path, ["--events", EVENTS] + v.cli() + extra, outputs, VW, VH)
        lines = runs[name]["lines"]
        moves = [l for l in lines if l.get("event", "").startswith("o:")]
        assert len(moves) == 3 and all(l["progression"] == 0 and not l["rendered"] for l in moves)
        sizes = [(l["width"], l["height"]) for l in lines if l.get("rendered")]
        assert sizes == [(VW, VH)] * 6 + [(48, 40)]
    on, off = runs["on"], runs["off"]
    total = 6 * px + 48 * 40 * 4
    assert on["shown"].size == off["shown"].size == on["raw"].size == total and on["feat"].size == 2 * total
    assert np.array_equal(bits(on["raw"]), bits(off["raw"])) and np.array_equal(bits(on["feat"]), bits(off["feat"]))
    try:
        for name, run in runs.items():
            exp = vr.displayed(rt, pt.scenes, variants[name], EVENTS, run["raw"], run["feat"], VW, VH, spheres0=spheres0).frames
            assert len(exp) == N_SHOWN
            at = at8 = 0
            exposure = np.zeros(1, F)
            for k, (e, (w, h)) in enumerate(zip(exp, sizes)):
                assert np.array_equal(bits(run["shown"][at:at + e.size]), bits(e)), f"{name}: displayed frame {k}"
                if tone:  # the last stage reads what is shown; the exposure starts afresh at the reshape
                    assert e.size == 4 * w * h
                    if k and sizes[k - 1] != (w, h):
                        exposure[:] = 0.0
                    out8 = np.zeros(w * h, np.uint32)
                    rt.meterExposure(e, exposure, w, h)
                    rt.toneMap(e, out8, w, h, exposure=exposure)
                    assert np.array_equal(run["f8"][at8:at8 + w * h], out8), f"{name}: 8-bit frame {k}"
                    at8 += w * h
                at += e.size
    finally:
        rt.setSpheres(spheres0)
    same = [np.array_equal(bits(on["shown"][px * k:px * (k + 1)]), bits(off["shown"][px * k:px * (k + 1)])) for k in range(6)]
    assert same[:2] == [True, True] and not same[2] and not all(same[2:]), same


@pytest.mark.parametrize("flags", list(VIEW_FLAGS))
def test_view_tris_unchanged(flags, tmp_path):
    """An RT_KERNEL_TRIS view (--mesh 2000: its spheres are lights only) with a light move: the same bytes
    with and without --sphere-carry."""
    fl, extra = VIEW_FLAGS[flags]
    outputs = ("shown", "raw") + (("f8",) if "--tonemap" in extra else ())
    args = ["--mesh", "2000", "--events", "d,d,e:0.3:0:0,d,d"] + extra
    off = vr.run_view(tmp_path, args + fl.cli(), outputs, VW, VH)
    on = vr.run_view(tmp_path, args + replace(fl, sphere_carry=True).cli(), outputs, VW, VH)
    assert on["lines"] == off["lines"]
    for k in outputs:
        assert on[k].size and np.array_equal(on[k].view(np.uint32), off[k].view(np.uint32)), k


def test_sphere_motion_quality(rt, pt):
    """The main scene with sphere 2 given sphere 0's diffuse material at 128 x 96, the camera static, 12
    steps of sphere 2 moving 0.05 along x, 1 spp each, the history carried from step to step through the
    warp (sphere cap 8, the default; temporal cap 32); mean squared errors of the last step's frames
    against a sampleRate-16 frame of it from other seeds.  Evaluated beforehand with the restatements over
    the oracle's frames of exactly these inputs (profiles/sphere_motion/evaluate.py):
        whole frame: 1-spp 9.8088e-2, merged 1.2458e-2: 7.87 times lower (cap 2 / 4 / 16: 4.77 / 7.23 /
        7.70 times; carried without the warp: 1.4274e-2);
        sphere 2's pixels (0.126 of the frame): 1-spp 2.0595e-2, merged 2.8414e-3: 7.25 times lower (cap 2
        / 4 / 16: 5.62 / 7.82 / 7.06 times), carried without the warp 1.7251e-2 (1.19 times).
    The conditions: on sphere 2's pixels the merged frame is no worse than the 1-spp frame, and better
    than the frame merged without the warp; over the whole frame the merged frame's error is at most 1 /
    3.936 of the 1-spp frame's — half the measured gain (7.873), set in advance."""
    sc, ab = pt.scenes, pt._abi
    W, H = 128, 96
    Wp, Hp = sc.padded_dims(W, H)
    scenes = [sm.quality_spheres(sc, ab.SPHERE_DTYPE, k) for k in range(sm.QUALITY_STEPS)]
    cam = rt.getCamera(W)
    res = {}
    try:
        for label in ("warp", "no warp"):
            rt.setSampleRate(1)
            rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp))
            hist = hl = pfeat = None
            for k, S in enumerate(scenes):
                rt.setSpheres(S)
                frame = np.zeros(W * H * 4, F)
                rt.rayTrace(frame, W, H, 0, kernel=rt.KERNEL_SPHERES)
                feat = features(rt, W, H)
                car, cl = np.zeros(W * H * 4, F), np.zeros(W * H, F)
                if hist is not None:
                    cf = feat
                    if label == "warp":
                        cf = np.zeros_like(feat)
                        rt.warpFeaturesSpheres(feat, scenes[k - 1], cf, W, H)
                    rt.reproject(hist, hl, pfeat, cam, cf, car, cl, W, H, max_history=min(32.0, SPHERE_CAP))
                hist, hl = np.zeros(W * H * 4, F), np.zeros(W * H, F)
                rt.temporalMerge(car, cl, frame, 1.0, hist, hl, W, H)
                pfeat = feat
            res[label] = hist
        ref = np.zeros(W * H * 4, F)
        rt.setSampleRate(16)
        rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp, skip=12345))
        rt.rayTrace(ref, W, H, 0, kernel=rt.KERNEL_SPHERES)
    finally:
        rt.setSampleRate(1)
        rt.setSpheres(sc.main_scene())
    px2 = fr.feature_ids(feat) == fr.RT_FEAT_SPHERE0 - 2

    def mse(a, sel=slice(None)):
        d = a.reshape(-1, 4)[sel, :3].astype(np.float64) - ref.reshape(-1, 4)[sel, :3].astype(np.float64)
        return float((d * d).mean())

    print(f"mse whole frame: 1-spp {mse(frame):.4e} merged {mse(res['warp']):.4e} ratio {mse(frame) / mse(res['warp']):.2f} "
          f"(without the warp {mse(res['no warp']):.4e}); sphere 2 ({px2.mean():.3f}): 1-spp {mse(frame, px2):.4e} merged "
          f"{mse(res['warp'], px2):.4e} without the warp {mse(res['no warp'], px2):.4e}")
    assert px2.sum() > 1000
    assert mse(res["warp"], px2) <= mse(frame, px2)
    assert mse(res["warp"], px2) < mse(res["no warp"], px2)
    assert mse(res["warp"]) <= mse(frame) / 3.936
