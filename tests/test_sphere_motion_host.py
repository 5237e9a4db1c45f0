"""Host side of the sphere carry (CPU only): the new ABI and the C++ methods, the
float32 restatement of rt_warp_features_spheres (tests/sphere_motion_ref.py) against its binary64 twin,
the sets that give the input back, the carry of a history across a sphere move through the restatements
of the warp and of rt_reproject, and what rt_render refuses."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

import features_ref as fr
import sphere_motion_ref as sm
import temporal_ref as tr
from conftest import ROOT, bits

F = np.float32
NEW_SYMBOLS = ["rt_warp_features_spheres", "rt_warp_features_spheres_async", "rt_last_sphere_warp_ms"]
MOVE = (0.25, 0.0, 0.1)  # of the central sphere (index 2), the issue's drag step

CPP_USE = r"""
#include "ProgressiveViewHIP.hpp"
int use(RayTracerHIP &rt, ProgressiveViewHIP &view, const float *feat, float *out)
{
    const std::vector<rt_sphere> &now = rt.spheres();
    rt.warpFeaturesSpheres(feat, now.data(), (uint32_t)now.size(), out, 64, 48, true);
    view.setSphereCarry(true);
    view.setSphereCarry(true, 4.0f);
    return view.sphereCarry() && rt.lastSphereWarpMs() > 0.0f;
}
"""


def test_new_entries_exist(pt, tmp_path):
    """The library exports the new entries, the header declares them, _abi.py binds them, RayTracer wraps
    them, and a translation unit that calls the new C++ methods compiles."""
    lib = pt.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(pt._abi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_\w+)", nm))
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pathtracer_rt.h").read_text(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert n in exported, f"librtmi.so does not export {n}"
        assert re.search(rf"\bint {n}\s*\(", header), f"pathtracer_rt.h does not declare {n}"
        assert n in pt._abi.SIGNATURES, f"_abi.py does not bind {n}"
        assert getattr(lib, n).argtypes is not None
    for m in ("warpFeaturesSpheres", "lastSphereWarpMs"):
        assert callable(getattr(pt.RayTracer, m))
    src = tmp_path / "use_sphere_motion.cpp"
    src.write_text(CPP_USE)
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", "-c", "-o",
                    str(tmp_path / "use_sphere_motion.o"), str(src)], check=True, timeout=300)


def test_null_context_checks(pt):
    ab, lib = pt._abi, pt.load_library()
    buf, out = np.zeros(64, F), np.zeros(64, F)
    prev = np.zeros(1, ab.SPHERE_DTYPE)
    p, o, s = ab.ptr(buf), ab.ptr(out), ab.ptr(prev)
    assert lib.rt_warp_features_spheres(None, p, s, 1, o, 2, 2, 0) == ab.RT_ERR_ARG
    assert lib.rt_warp_features_spheres_async(None, p, s, 1, o, 2, 2, 0, None) == ab.RT_ERR_ARG
    ms = ctypes.c_float()
    assert lib.rt_last_sphere_warp_ms(None, ctypes.byref(ms)) == ab.RT_ERR_ARG
    assert not out.any()


def main_view(pt, W, H, spheres):
    """(camera, features by the restatement of k_features_sph) of the sphere golden view."""
    sc = pt.scenes
    cam = sc.camera_spherical(W, **sc.MAIN_CAMERA)
    rays = np.zeros(W * H, pt._abi.RAY_DTYPE)
    assert pt.load_library().rt_primary_rays(pt._abi.ptr(cam), W, H, pt._abi.ptr(rays)) == pt._abi.RT_OK
    return cam, sm.features_spheres(rays, spheres).reshape(-1)


def moved_scene(pt, moves):
    """main_scene() with (dx, dy, dz, dr) added to sphere i for every i in `moves` (float32 sums)."""
    s = np.asarray(pt.scenes.main_scene(), pt._abi.SPHERE_DTYPE).reshape(-1).copy()
    for i, (dx, dy, dz, dr) in moves.items():
        s["center"][i] = s["center"][i] + np.array((dx, dy, dz), F)
        s["radius"][i] = s["radius"][i] + F(dr)
    return s


def synthetic(rng, n, n_spheres):
    """n pixels of spheres 0 .. n_spheres - 1 with unit normals (rounded to float32), and a few others."""
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ids = (fr.RT_FEAT_SPHERE0 - rng.integers(0, n_spheres, n)).astype(np.int32)
    ids[:4] = (5, fr.RT_FEAT_BOX, fr.RT_FEAT_NONE, fr.RT_FEAT_SPHERE0 + 1)
    feat = np.zeros((2, n, 4), F)
    feat[0, :, :3], feat[0, :, 3] = rng.uniform(-6, 6, (n, 3)).astype(F), rng.uniform(0.5, 9.0, n).astype(F)
    feat[1, :, :3], feat[1, :, 3] = nrm.astype(F), ids.view(F)
    return feat.reshape(-1)


def test_identical_set_and_material_change_give_the_input(pt):
    """Rule 3: an unmoved scene gives the input's bits, and so does one whose materials alone changed —
    on a synthetic buffer and on the main view."""
    S = moved_scene(pt, {})
    other = S.copy()
    other["diffuse"][2], other["kd"][2], other["ks"][2], other["emission_power"][0] = (0.0, 0.7, 0.7), 1.0, 0.0, 0.5
    assert S.tobytes() != other.tobytes()
    for feat in (synthetic(np.random.default_rng(1), 500, len(S)), main_view(pt, 37, 29, S)[1]):
        assert (fr.feature_ids(feat) <= fr.RT_FEAT_SPHERE0).sum() > 100
        for prev in (S, S.copy(), other):
            assert np.array_equal(bits(sm.warp_spheres(feat, S, prev)), bits(feat))


# The largest float32-to-binary64 difference of a component of P' that the restatement shows on the
# inputs below (4000 synthetic pixels per sphere count over spheres with centres in [-6, 6]^3 and radii in
# [0.1, 3], and the main view at 64 x 48 after the moves "sphere2", "all" and "radius" below), in
# units of the scale max(1, |C'|_inf + r'): 7.839e-8 (synthetic, 6 spheres; 7.211e-8 and 6.473e-8 with 1 and
# 70), 4.768e-8 (main view, the radius change) — P' = fl(C' + fl(N r')) is two roundings, each at most half
# an ulp (2^-24 relative) of a number no larger than the scale: 1.19e-7 at worst.  The bound is twice the
# measured figure.  With unit normals |P' - C'| is held against r' under the same bound; the normals
# k_features_sph writes are (P - C) * (1 / r), off unit length by up to 8.4e-6 in the main view, so there
# |P' - C'| is held against r' |N|.
MEASURED_REL = 7.839e-8
BOUND_REL = 2.0 * MEASURED_REL


def _check_against_twin(feat, cur, prev, label, unit_normals):
    out = sm.warp_spheres(feat, cur, prev).reshape(2, -1, 4)
    k, s, P64, ok64 = sm.warp_spheres64(feat, cur, prev)
    assert k.size >= 100 and ok64.all()
    assert (fr.feature_ids(out.reshape(-1))[k] <= fr.RT_FEAT_SPHERE0).all()  # both forms keep the same pixels
    g = sm._geometry(prev).astype(np.float64)[s]
    scale = np.maximum(1.0, np.abs(g[:, :3]).max(axis=1) + g[:, 3])
    P32 = out[0, k, :3].astype(np.float64)
    eP = (np.abs(P32 - P64).max(axis=1) / scale).max()
    nrm = np.linalg.norm(feat.reshape(2, -1, 4)[1, k, :3].astype(np.float64), axis=1)
    # |P' - C'| is r' |N|: the distance from the earlier centre against that, and |N| itself against 1
    eR = (np.abs(np.linalg.norm(P32 - g[:, :3], axis=1) - g[:, 3] * nrm) / scale).max()
    eR1 = (np.abs(np.linalg.norm(P32 - g[:, :3], axis=1) - g[:, 3]) / scale).max()
    print(f"{label}: P' off its binary64 twin by {eP:.3e} of the scale, |P' - C'| off r'|N| by {eR:.3e} and off r' by "
          f"{eR1:.3e}, |N| off 1 by {np.abs(nrm - 1).max():.3e}")
    assert eP <= BOUND_REL
    assert (eR1 if unit_normals else eR) <= BOUND_REL
    f = feat.reshape(2, -1, 4)
    assert np.array_equal(bits(out[1]), bits(f[1])) and np.array_equal(bits(out[0, :, 3]), bits(f[0, :, 3]))  # N, id and t stay
    rest = np.ones(f.shape[1], bool)
    rest[k] = False
    assert np.array_equal(bits(out[:, rest]), bits(f[:, rest]))


@pytest.mark.parametrize("n_spheres", [1, 6, 70])
def test_restatement_against_binary64_twin_synthetic(pt, n_spheres):
    rng = np.random.default_rng(n_spheres)
    cur = np.zeros(n_spheres, pt._abi.SPHERE_DTYPE)
    cur["center"], cur["radius"] = rng.uniform(-6, 6, (n_spheres, 3)), rng.uniform(0.1, 3.0, n_spheres)
    prev = cur.copy()
    prev["center"] = prev["center"] + rng.uniform(-0.5, 0.5, (n_spheres, 3)).astype(F)
    prev["radius"] = prev["radius"] * rng.uniform(0.8, 1.25, n_spheres).astype(F)
    _check_against_twin(synthetic(rng, 4000, n_spheres), cur, prev, f"synthetic, {n_spheres} spheres", True)


MOVES = {
    "sphere2": {2: (*MOVE, 0.0)},
    "all": {i: (0.05 * (i + 1), -0.03 * i, 0.04 * (3 - i), 0.0) for i in range(6)},
    "radius": {2: (0.0, 0.0, 0.0, 0.2)},
    "light": {5: (0.3, -0.2, 0.1, 0.0)},
}


@pytest.mark.parametrize("move", ["sphere2", "all", "radius"])
def test_restatement_against_binary64_twin_main_view(pt, move):
    """The main view after a move, warped back onto the spheres of main_scene(): besides the twin's
    bound, a moved sphere's warped points lie on the sphere it was."""
    prev, cur = moved_scene(pt, {}), moved_scene(pt, MOVES[move])
    _, feat = main_view(pt, 64, 48, cur)
    _check_against_twin(feat, cur, prev, f"main view, {move}", False)


def test_restatement_drops_what_it_cannot_carry(pt):
    """Indices past either count, INT32_MIN, earlier radii that are not positive and finite and an
    overflowing P' give "no surface"; every id above RT_FEAT_SPHERE0 is copied."""
    cur = moved_scene(pt, {})
    ids = np.array([7, 0, fr.RT_FEAT_BOX, fr.RT_FEAT_NONE, -3, -15, fr.RT_FEAT_SPHERE0, fr.RT_FEAT_SPHERE0 - 5,
                    fr.RT_FEAT_SPHERE0 - 6, fr.RT_FEAT_SPHERE0 - 7, -2 ** 31], np.int32)
    n = len(ids)
    feat = np.zeros((2, n, 4), F)
    feat[0, :, :3], feat[0, :, 3], feat[1, :, 0], feat[1, :, 3] = (1.0, 2.0, 3.0), 4.0, 1.0, ids.view(F)
    prev = cur.copy()
    prev["center"][:, 0] += F(1.0)
    out = sm.warp_spheres(feat, cur, prev).reshape(2, n, 4)
    oid = fr.feature_ids(out.reshape(-1))
    assert list(oid) == list(ids[:8]) + [fr.RT_FEAT_NONE] * 3
    assert np.array_equal(bits(out[:, :6]), bits(feat[:, :6]))
    assert np.array_equal(out[0, 6], np.array([-2.0 + 1.0 + 1.0, -4.0, -2.0, 4.0], F))  # C' + N r' with N = (1, 0, 0)
    assert np.array_equal(out[0, 8:], np.tile(np.array([0, 0, 0, np.inf], F), (3, 1))) and not out[1, 8:, :3].any()
    for n_prev in (0, 5):  # sphere 5 has no earlier self
        o = fr.feature_ids(sm.warp_spheres(feat, cur, prev[:n_prev]))
        assert o[7] == fr.RT_FEAT_NONE and (o[6] == fr.RT_FEAT_NONE) == (n_prev == 0)
    for r in (0.0, -1.0, np.nan, np.inf, 1e38):
        bad = prev.copy()
        bad["radius"][0] = r
        f = feat.copy()
        f[1, 6, 0] = 10.0  # 1e38 * 10 overflows
        o = sm.warp_spheres(f, cur, bad).reshape(2, n, 4)
        assert fr.feature_ids(o.reshape(-1))[6] == fr.RT_FEAT_NONE and np.array_equal(o[0, 6], np.array([0, 0, 0, np.inf], F))


def test_carry_through_the_restatements(pt):
    """What tests/test_gpu_sphere_motion.py asks of the device, checked on the restatements first: the
    main view at 64 x 48 before and after sphere 2 moves by MOVE.  Of sphere 2's pixels in the new view,
    0.9646 find history through warp + reproject (245 of 254) and none without the warp; where a pixel
    finds history, the carried colour — the previous pixels' own positions — lies on the sphere as it
    stood (off it by 6.4e-3 at most: a blend of points on a unit sphere lies inside it)."""
    W, H = 64, 48
    prev, cur = moved_scene(pt, {}), moved_scene(pt, MOVES["sphere2"])
    cam, pfeat = main_view(pt, W, H, prev)
    _, cfeat = main_view(pt, W, H, cur)
    n = W * H
    hist = np.zeros((n, 4), F)
    hist[:, :3] = pfeat.reshape(2, n, 4)[0, :, :3]
    ln = np.ones(n, F)
    px2 = fr.feature_ids(cfeat) == fr.RT_FEAT_SPHERE0 - 2
    share = {}
    for label, cf in (("warp", sm.warp_spheres(cfeat, cur, prev)), ("no warp", cfeat)):
        out, ol = tr.reproject(hist.reshape(-1), ln, pfeat, cam, cf, W, H)
        got = px2 & (ol > 0)
        share[label] = got.sum() / px2.sum()
        print(f"{label}: {got.sum()} of {px2.sum()} pixels of sphere 2 find history ({share[label]:.4f})")
        if label == "warp":
            c = np.asarray(prev["center"][2], np.float64)
            off = np.abs(np.linalg.norm(out.reshape(n, 4)[got, :3].astype(np.float64) - c, axis=1) - 1.0)
            print(f"the carried positions are off the earlier sphere by {off.max():.3e} at most")
            assert off.max() < 0.02
    assert px2.sum() > 200
    assert share["warp"] >= 0.5 and share["no warp"] < 0.2


def test_cli_refuses(pt):
    """rt_render refuses --sphere-carry without --temporal and an o event that names no sphere of the
    scene, each with exit code 2 and a message, before it touches a device."""
    exe = ROOT / "pathtracer.cl_amd" / "rt_render"
    if not exe.exists():
        subprocess.run(["make", "-s", "-C", str(ROOT / "pathtracer.cl_amd" / "csrc")], check=True)
    r = subprocess.run([str(exe), "--events", "d", "--sphere-carry"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--sphere-carry needs --temporal" in r.stderr
    for ev in ("o:6:0.1:0:0", "d,o:100:0:0:0:0.5"):
        r = subprocess.run([str(exe), "--events", ev, "--temporal", "--sphere-carry"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "holds no sphere" in r.stderr, (ev, r.returncode, r.stderr)
