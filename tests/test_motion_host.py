"""Host side of the motion carry (CPU only): the new ABI and the C++ methods, the
float32 restatement of rt_warp_features (tests/motion_ref.py) against its binary64 twin, the
identity pose, and the carry of a history across a mesh move through the restatements of the warp
and of rt_reproject."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

import features_ref as fr
import motion_ref as mr
import refit_ref as rr
import temporal_ref as tr
import tree_cases as tc
from conftest import ROOT, bits

F = np.float32
NEW_SYMBOLS = ["rt_mesh_pose", "rt_warp_features", "rt_warp_features_async", "rt_last_warp_ms"]

CPP_USE = r"""
#include "ProgressiveViewHIP.hpp"
int use(RayTracerHIP &rt, ProgressiveViewHIP &view, const float *feat, float *pose, float *out, uint32_t n_verts)
{
    rt.meshPose(pose, n_verts, true);
    rt.warpFeatures(feat, pose, n_verts, out, 64, 48, true);
    view.setMotionCarry(true);
    view.setMotionCarry(true, 4.0f);
    return view.motionCarry() && rt.lastWarpMs() > 0.0f;
}
"""


def test_new_entries_exist(pt, tmp_path):
    """The library exports the new entries, _abi.py binds them, RayTracer wraps them, and a
    translation unit that calls the new C++ methods compiles."""
    lib = pt.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(pt._abi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_\w+)", nm))
    for n in NEW_SYMBOLS:
        assert n in exported, f"librtmi.so does not export {n}"
        assert n in pt._abi.SIGNATURES, f"_abi.py does not bind {n}"
        assert getattr(lib, n).argtypes is not None
    for m in ("meshPose", "warpFeatures", "lastWarpMs"):
        assert callable(getattr(pt.RayTracer, m))
    src = tmp_path / "use_motion.cpp"
    src.write_text(CPP_USE)
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", "-c", "-o",
                    str(tmp_path / "use_motion.o"), str(src)], check=True, timeout=300)


def test_null_context_checks(pt):
    ab, lib = pt._abi, pt.load_library()
    buf, out = np.zeros(64, F), np.zeros(64, F)
    p, o = ab.ptr(buf), ab.ptr(out)
    assert lib.rt_mesh_pose(None, o, 3, 0) == ab.RT_ERR_ARG
    assert lib.rt_warp_features(None, p, p, 3, o, 2, 2, 0) == ab.RT_ERR_ARG
    assert lib.rt_warp_features_async(None, p, p, 3, o, 2, 2, 0, None) == ab.RT_ERR_ARG
    ms = ctypes.c_float()
    assert lib.rt_last_warp_ms(None, ctypes.byref(ms)) == ab.RT_ERR_ARG
    assert not out.any()


def aimed_rays(pt, verts, idx, n=600, seed=3):
    """n rays from outside the mesh toward points inside random triangles, no direction component 0."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(verts, F).reshape(-1, 3)[np.asarray(idx, np.int32).reshape(-1, 3)]
    lo, hi = tri.min(axis=(0, 1)), tri.max(axis=(0, 1))
    diag = max(float(np.linalg.norm(hi.astype(np.float64) - lo)), 1e-2)
    k = rng.integers(0, len(tri), n)
    ab = rng.uniform(0.05, 0.45, (n, 2))
    tg = tri[k, 0] + ab[:, :1] * (tri[k, 1] - tri[k, 0]) + ab[:, 1:] * (tri[k, 2] - tri[k, 0])
    dr = rng.normal(size=(n, 3))
    dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    o = (tg + dr * (rng.uniform(0.3, 1.2, (n, 1)) * diag)).astype(F)
    d = (tg - o).astype(F)
    d = (d / np.sqrt((d * d).sum(axis=1, dtype=F))[:, None]).astype(F)
    rays = np.zeros(n, pt._abi.RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    rays["tmin"], rays["tmax"] = F(1e-4), F(np.inf)
    rays["propagation"] = 1.0
    return rays[np.all(d != 0, axis=1)]


@pytest.fixture(scope="module")
def mesh_features(pt, oracle):
    """mesh name -> (verts, idx, features of 600 aimed rays by the oracle's linear loop), made once."""
    cache = {}

    def get(name):
        if name not in cache:
            verts, idx = tc.make(name, pt.scenes)
            cache[name] = (verts, idx, fr.features_tris(oracle, aimed_rays(pt, verts, idx), verts, idx))
        return cache[name]

    return get


# The largest float32-to-binary64 difference of P' that the restatement shows on these inputs (every
# mesh of tree_cases.MESHES, 600 aimed rays each, the three deformations), in units of the mesh's
# largest coordinate magnitude (at least 1): 3.784e-7, on one_centre600 / rigid (absolute 7.6e-7 at
# coordinates up to 2; sphere2000: 4.7e-7 at coordinates up to 4.9; far_grid at 1000: 6.0e-5; huge8 at
# 20000: 3.7e-3).  The normals differ by at most 3.4e-7.  The bound is four times that, for a device
# that evaluates the identical arithmetic.
MEASURED_REL = 3.784e-7
BOUND_REL = 4.0 * MEASURED_REL


@pytest.mark.parametrize("deform", list(rr.DEFORM))
@pytest.mark.parametrize("name", tc.MESHES)
def test_restatement_against_binary64_twin(name, deform, mesh_features):
    """P' of the float32 restatement lies on the earlier triangle at the twin's barycentrics (the
    twin's P') within BOUND_REL of the coordinates' magnitude, N' within 4 x 3.4e-7; both forms keep and
    drop the same pixels."""
    verts, idx, feat = mesh_features(name)
    prev = rr.DEFORM[deform](verts)
    out = mr.warp(feat, idx, verts, prev).reshape(2, -1, 4)
    k, P64, N64, ok64, u, v = mr.warp64(feat, idx, verts, prev)
    ids_in, ids_out = fr.feature_ids(feat), fr.feature_ids(out)
    assert np.array_equal(np.flatnonzero(ids_in >= 0), k)
    if name in tc.NOTHING_HITTABLE:
        assert k.size == 0
        assert np.array_equal(bits(out), bits(feat.reshape(2, -1, 4)))
        return
    assert k.size >= 100
    ok32 = ids_out[k] >= 0
    assert np.array_equal(ok32, ok64) and ok32.all()
    scale = max(1.0, float(np.abs(verts).max()), float(np.abs(prev).max()))
    eP = np.abs(out[0, k, :3].astype(np.float64) - P64).max()
    eN = np.abs(out[1, k, :3].astype(np.float64) - N64).max()
    print(f"{name} {deform}: P' {eP:.3e} ({eP / scale:.3e} of the scale {scale:.1f}), N' {eN:.3e}")
    assert eP <= BOUND_REL * scale
    assert eN <= 4 * 3.4e-7
    # the twin's point is the earlier triangle's point at (u, v): inside it for these hits
    assert u.min() > -1e-3 and v.min() > -1e-3 and (u + v).max() < 1 + 1e-3
    # t and id stay; everything that is not on the mesh is copied bit for bit
    f = feat.reshape(2, -1, 4)
    assert np.array_equal(bits(out[0, :, 3]), bits(f[0, :, 3])) and np.array_equal(ids_out, ids_in)
    other = ids_in < 0
    assert np.array_equal(bits(out[:, other]), bits(f[:, other]))


@pytest.mark.parametrize("name", ["sphere2000", "mixed_scales", "det_bound", "far_grid"])
def test_identity_pose(name, mesh_features):
    """The earlier pose is the current one: N' is N bit for bit, id and t are untouched, and P' is P
    within BOUND_REL of the coordinates' magnitude."""
    verts, idx, feat = mesh_features(name)
    out = mr.warp(feat, idx, verts, verts).reshape(2, -1, 4)
    f = feat.reshape(2, -1, 4)
    assert np.array_equal(bits(out[1]), bits(f[1]))
    assert np.array_equal(bits(out[0, :, 3]), bits(f[0, :, 3]))
    mesh = fr.feature_ids(feat) >= 0
    assert mesh.sum() >= 100
    scale = max(1.0, float(np.abs(verts).max()))
    assert np.abs(out[0, mesh, :3].astype(np.float64) - f[0, mesh, :3]).max() <= BOUND_REL * scale


def test_restatement_drops_what_it_cannot_carry():
    """ids past the triangle count, indices outside the vertices, degenerate triangles in either pose
    and an overflowing P' all give "no surface"; ids below 0 are copied."""
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 2, 2)], F)
    idx = np.array([(0, 1, 2), (0, 1, 7), (0, -1, 2), (0, 1, 1), (3, 3, 3)], np.int32)
    ids = np.array([0, 1, 2, 3, 4, 5, 2 ** 31 - 1, fr.RT_FEAT_BOX, fr.RT_FEAT_NONE, fr.RT_FEAT_SPHERE0 - 3, 0, 0, 0], np.int32)
    n = len(ids)
    feat = np.zeros((2, n, 4), F)
    feat[0, :, :3], feat[0, :, 3] = (0.25, 0.25, 0.5), 3.0  # off the triangle's plane: projected along its normal
    feat[1, :, 2] = -1.0
    feat[1, :, 3] = ids.view(F)
    out = mr.warp(feat, idx, verts, verts + F(1.0)).reshape(2, n, 4)
    oid = fr.feature_ids(out)
    assert list(oid[:10]) == [0] + [fr.RT_FEAT_NONE] * 6 + [fr.RT_FEAT_BOX, fr.RT_FEAT_NONE, fr.RT_FEAT_SPHERE0 - 3]
    assert np.array_equal(out[0, 0], np.array([1.25, 1.25, 1.0, 3.0], F)) and np.array_equal(out[1, 0, :3], np.array([0, 0, -1], F))
    none = oid == fr.RT_FEAT_NONE
    assert np.array_equal(out[0, none & (ids != fr.RT_FEAT_NONE)], np.tile(np.array([0, 0, 0, np.inf], F), (6, 1)))
    assert np.array_equal(bits(out[:, 7:10]), bits(feat[:, 7:10]))
    for prev in (np.array([(5, 5, 5)] * 4, F), np.array([(0, 0, 0), (1, 1, 1), (2, 2, 2), (0, 0, 0)], F),
                 np.array([(0, 0, 0), (3e38, 0, 0), (0, 3e38, 0), (0, 0, 0)], F)):  # a point, a line, an overflow
        o = mr.warp(feat, idx, verts, prev).reshape(2, n, 4)
        assert (fr.feature_ids(o)[[0, 10, 11, 12]] == fr.RT_FEAT_NONE).all()
        assert np.isfinite(o[0, :, :3]).all() and np.isfinite(o[1, :, :3]).all()


def small_move(verts, deg=5.0, part=0.25):
    """A quarter of refit_ref.rigid: `deg` degrees about the vertical axis through the box centre, then
    `part` of its translation (binary64, rounded to float32)."""
    v, c, _ = rr._frame(verts)
    a = np.deg2rad(deg)
    d = v - c
    out = np.stack([np.cos(a) * d[:, 0] + np.sin(a) * d[:, 2], d[:, 1], -np.sin(a) * d[:, 0] + np.cos(a) * d[:, 2]], axis=1)
    return np.ascontiguousarray((out + c + part * np.array([0.3, -0.2, 0.1])).astype(F))


def carry_case(pt, orc, move, W=64, H=48):
    """The 2000-triangle mesh in the golden view, before and after `move`: (camera, idx, the two
    poses, previous features, current features) with the features by the oracle's linear loop."""
    sc = pt.scenes
    verts, idx = sc.make_mesh(2000)
    cam = sc.camera_spherical(W, **sc.PLY_CAMERA)
    rays = np.zeros(W * H, pt._abi.RAY_DTYPE)
    assert pt.load_library().rt_primary_rays(pt._abi.ptr(cam), W, H, pt._abi.ptr(rays)) == pt._abi.RT_OK
    moved = move(verts)
    return (cam, idx, verts, moved, fr.features_tris(orc, rays, verts, idx).reshape(-1),
            fr.features_tris(orc, rays, moved, idx).reshape(-1))


def rest_positions(cfeat, idx, moved, verts):
    """Per pixel the binary64 rest-pose position of the material point it shows (NaN off the mesh) and
    how far the move has displaced it."""
    k, P64, _, ok, _, _ = mr.warp64(cfeat, idx, moved, verts)
    assert ok.all()
    rest = np.full((len(cfeat) // 8, 3), np.nan)
    rest[k] = P64
    disp = np.linalg.norm(cfeat.reshape(2, -1, 4)[0, :, :3].astype(np.float64) - rest, axis=1)
    return rest, disp


def test_carry_through_the_restatements(pt, oracle):
    """The rigid move (20 degrees and a translation: every mesh point moves by 0.76 to 1.1) in the
    golden view at 64 x 48.  The history's colour is each previous pixel's own position, so a carried
    colour says which material point the history came from.  Measured beforehand, as a fraction of the
    pixel's displacement, over the mesh pixels that find history: with the warp the carried colour is
    within 0.0617 of the pixel's own rest-pose position at worst (median 2.3e-4; 1156 of 3057 mesh
    pixels find history, the others' earlier places lie outside the frame, which the mesh overfills);
    without the warp the 26 pixels that still pass rt_reproject's plane test are off by 0.977 at
    least.  The bound is halfway between the two on a log scale: sqrt(0.0617 * 0.977) = 0.245."""
    W, H = 64, 48
    cam, idx, verts, moved, pfeat, cfeat = carry_case(pt, oracle, rr.rigid)
    n = W * H
    hist = np.zeros((n, 4), F)
    hist[:, :3] = pfeat.reshape(2, n, 4)[0, :, :3]
    ln = np.ones(n, F)
    rest, disp = rest_positions(cfeat, idx, moved, verts)
    mesh = fr.feature_ids(cfeat) >= 0
    err = {}
    for label, cf in (("warp", mr.warp(cfeat, idx, moved, verts)), ("no warp", cfeat)):
        out, ol = tr.reproject(hist.reshape(-1), ln, pfeat, cam, cf, W, H)
        got = mesh & (ol > 0)
        err[label] = (np.linalg.norm(out.reshape(n, 4)[:, :3].astype(np.float64) - rest, axis=1) / disp)[got]
        print(f"{label}: {got.sum()} of {mesh.sum()} mesh pixels find history, error / displacement "
              f"{err[label].min():.4f} .. {err[label].max():.4f}")
    assert err["warp"].size >= 1000 and err["no warp"].size >= 1
    assert err["warp"].max() <= 0.245
    assert err["no warp"].min() > 0.245


def test_small_move_finds_history(pt, oracle):
    """What tests/test_gpu_motion.py asks of the device, checked on the restatements first: after
    small_move (5 degrees, a quarter of rigid's translation) 0.8696 of the mesh pixels find history
    through warp + reproject (2501 of 2876), 0.0897 without the warp.  (rigid itself: 0.378 — the mesh
    overfills the 64 x 48 frame, and a 20 degree turn brings in what was outside it.)"""
    W, H = 64, 48
    cam, idx, verts, moved, pfeat, cfeat = carry_case(pt, oracle, small_move)
    ln = np.ones(W * H, F)
    col = np.zeros(W * H * 4, F)
    mesh = fr.feature_ids(cfeat) >= 0
    with_warp = (tr.reproject(col, ln, pfeat, cam, mr.warp(cfeat, idx, moved, verts), W, H)[1] > 0)[mesh].mean()
    without = (tr.reproject(col, ln, pfeat, cam, cfeat, W, H)[1] > 0)[mesh].mean()
    print(f"share of mesh pixels with history: {with_warp:.4f} with the warp, {without:.4f} without")
    assert with_warp >= 0.8 and without <= 0.2
