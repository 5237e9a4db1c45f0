"""Host side of the temporal reprojection (CPU only): the new ABI, the defaults, the checks that need
no device, and the restatement's inverse projection (tests/temporal_ref.py) against the pixel-centre
rays of rt_primary_rays."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

import temporal_ref as tr

NEW_SYMBOLS = ["rt_reproject_defaults", "rt_reproject", "rt_reproject_async", "rt_temporal_merge",
               "rt_temporal_merge_async", "rt_last_reproject_ms"]


def test_new_symbols_exported_and_bound(pt):
    lib = pt.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(pt._abi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_\w+)", nm))
    for n in NEW_SYMBOLS:
        assert n in exported, f"librtmi.so does not export {n}"
        assert n in pt._abi.SIGNATURES, f"_abi.py does not bind {n}"
        assert getattr(lib, n).argtypes is not None
    for m in ("reproject", "temporalMerge", "lastReprojectMs", "reprojectDefaults"):
        assert callable(getattr(pt.RayTracer, m))


def test_reproject_defaults(pt):
    ab = pt._abi
    lib = pt.load_library()
    prm = ab.RtReprojectParams(-1.0, -1.0, -1.0)
    assert lib.rt_reproject_defaults(ctypes.byref(prm)) == ab.RT_OK
    assert (np.float32(prm.plane_tol), np.float32(prm.normal_min), np.float32(prm.max_history)) == (
        np.float32(0.01), np.float32(0.9), np.float32(32.0))
    assert lib.rt_reproject_defaults(None) == ab.RT_ERR_ARG
    assert ctypes.sizeof(ab.RtReprojectParams) == 12


def test_null_context_checks(pt):
    """The context entries refuse a null context before touching a device."""
    ab = pt._abi
    lib = pt.load_library()
    prm = ab.RtReprojectParams(0.01, 0.9, 32.0)
    buf = np.zeros(64, np.float32)
    out = np.zeros(64, np.float32)
    cam = np.zeros(16, np.float32)
    p, o = ab.ptr(buf), ab.ptr(out)
    assert lib.rt_reproject(None, p, p, p, ab.ptr(cam), p, o, o, 2, 2, ctypes.byref(prm), 0) == ab.RT_ERR_ARG
    assert lib.rt_reproject_async(None, p, p, p, ab.ptr(cam), p, o, o, 2, 2, ctypes.byref(prm), 0, None) == ab.RT_ERR_ARG
    assert lib.rt_temporal_merge(None, p, p, p, 1.0, 32.0, o, o, 2, 2, 0) == ab.RT_ERR_ARG
    assert lib.rt_temporal_merge_async(None, p, p, p, 1.0, 32.0, o, o, 2, 2, 0, None) == ab.RT_ERR_ARG
    ms = ctypes.c_float()
    assert lib.rt_last_reproject_ms(None, ctypes.byref(ms), None) == ab.RT_ERR_ARG
    assert not out.any()


def _skewed(cam):
    """A camera that is neither orthogonal nor normalised (an explicit rt_set_camera override may be)."""
    c = np.array(cam, np.float32).reshape(4, 4)
    c[1, :3] = c[1, :3] * np.float32(1.3) + c[2, :3] * np.float32(0.2)
    c[2, :3] = c[2, :3] + c[0, :3] * np.float32(0.001)
    return c.reshape(-1)


@pytest.mark.parametrize("W,H", [(64, 48), (333, 7)])
@pytest.mark.parametrize("skew", [False, True])
def test_inverse_projection_recovers_pixels(pt, golden, W, H, skew):
    """A point at any depth along the pixel-centre ray of (x, y) projects back to fx = x, fy = y.
    Bound: P = o + d t carries a rounding error of about an ulp of its magnitude (|P| < 16: 1e-6),
    which the projection magnifies by |view| / t <= 333 / 0.5 pixels per unit; a few such terms stay
    below 5e-3 pixels — a hundredth of the half pixel at which a tap would change."""
    kat = golden("kat")
    cam = np.ascontiguousarray(kat["cams"][list(kat["cam_widths"]).index(W)], np.float32)
    if skew:
        cam = _skewed(cam)
    lib = pt.load_library()
    rays = np.zeros(W * H, pt._abi.RAY_DTYPE)
    assert lib.rt_primary_rays(pt._abi.ptr(cam), W, H, pt._abi.ptr(rays)) == pt._abi.RT_OK
    rng = np.random.default_rng(W + skew)
    t = (np.float32(0.5) + rng.random(W * H, dtype=np.float32) * np.float32(8.0)).astype(np.float32)
    P = (rays["o"] + rays["d"] * t[:, None]).astype(np.float32)
    s, fx, fy, det = tr.project(cam, P, W, H)
    assert det != 0 and np.all(s > 0)
    ys, xs = np.divmod(np.arange(W * H), W)
    assert np.abs(fx.astype(np.float64) - xs).max() < 5e-3
    assert np.abs(fy.astype(np.float64) - ys).max() < 5e-3
    # s is the ray parameter of the unnormalised direction: t / |view + a right + b up|
    behind = (rays["o"] - rays["d"] * t[:, None]).astype(np.float32)
    assert np.all(tr.project(cam, behind, W, H)[0] < 0)


def test_restatement_edge_cases():
    """The restatement itself on a tiny frame: a singular camera and a point behind the camera leave
    no history; the merge returns the current frame's bits where the history is empty."""
    f = np.float32
    W, H = 2, 2
    cam = np.array([0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], f)  # view +z, up +y, right +x
    feat = np.zeros((2, 4, 4), f)
    feat[0, :, :3] = [(-0.5, -0.5, 1), (0.5, -0.5, 1), (-0.5, 0.5, 1), (0.5, 0.5, 1)]  # the four pixel centres at z = 1
    feat[0, :, 3] = 1.0
    feat[1, :, 2] = -1.0
    feat[1, :, 3] = np.array([5, 5, 5, 5], np.int32).view(f)
    col = np.arange(16, dtype=f)
    ln = np.array([1, 2, 3, 4], f)
    out, ol = tr.reproject(col, ln, feat, cam, feat, W, H)
    assert np.array_equal(out.reshape(4, 4)[:, :3], col.reshape(4, 4)[:, :3]) and np.array_equal(ol, ln)
    assert not out.reshape(4, 4)[:, 3].any()
    sing = cam.copy()
    sing[4:8] = sing[8:12]  # up = right
    out, ol = tr.reproject(col, ln, feat, sing, feat, W, H)
    assert not out.any() and not ol.any()
    back = feat.copy()
    back[0, :, 2] = -1.0
    out, ol = tr.reproject(col, ln, feat, cam, back, W, H)
    assert not out.any() and not ol.any()
    cur = (col * f(0.37)).astype(f)
    cur[0] = f(-0.0)
    mo, ml = tr.merge(col, np.array([0, 2, 0, 40], f), cur, 3.0, 32.0)
    assert np.array_equal(mo.view(np.uint32).reshape(4, 4)[[0, 2]], cur.view(np.uint32).reshape(4, 4)[[0, 2]])
    assert np.array_equal(ml, np.array([3, 5, 3, 32], f))
    assert np.array_equal(mo[3::4], cur[3::4])
