"""Host side of the first-hit features and the display denoiser (CPU only): the pixel-centre
camera rays, the argument checks that need no device, the filter's defaults and the new ABI."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import bits

NEW_SYMBOLS = ["rt_get_camera", "rt_primary_rays", "rt_render_features", "rt_render_features_async",
               "rt_denoise_defaults", "rt_denoise", "rt_denoise_async", "rt_last_features_ms", "rt_last_denoise_ms"]


def primary_rays_numpy(cam16, W, H):
    """float32 restatement of rt_primary_rays: raytracer.cl:221-224 with the stratified draw
    replaced by 0.5, normalize over the float4 lanes incl. w as v / sqrt(dot(v, v))."""
    f = np.float32
    cam = np.asarray(cam16, f).reshape(4, 4)
    view, up, right, pos = cam
    x = np.arange(W, dtype=f)[None, :]
    y = np.arange(H, dtype=f)[:, None]
    a = (x + f(0.5)) - f(W) / f(2.0)
    b = (y + f(0.5)) - f(H) / f(2.0)
    v = [(view[k] + right[k] * a) + up[k] * b for k in range(4)]
    v = [np.broadcast_to(c, (H, W)).astype(f) for c in v]
    ln = np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
    d = np.stack([v[0] / ln, v[1] / ln, v[2] / ln], axis=-1).reshape(-1, 3)
    return d, np.broadcast_to(pos[:3], d.shape)


@pytest.mark.parametrize("W,H", [(64, 48), (333, 7)])
def test_primary_rays_match_numpy(pt, golden, W, H):
    kat = golden("kat")
    cam = np.ascontiguousarray(kat["cams"][list(kat["cam_widths"]).index(W)], np.float32)
    lib = pt.load_library()
    rays = np.zeros(W * H, pt._abi.RAY_DTYPE)
    rays["diffuse_bounce"] = 7
    assert lib.rt_primary_rays(pt._abi.ptr(cam), W, H, pt._abi.ptr(rays)) == pt._abi.RT_OK
    d, o = primary_rays_numpy(cam, W, H)
    assert np.array_equal(bits(rays["d"]), bits(d))
    assert np.array_equal(bits(rays["o"]), bits(o))
    assert np.all(rays["tmin"] == np.float32(1e-4)) and np.all(np.isposinf(rays["tmax"]))
    assert np.all(rays["propagation"] == 1.0) and np.all(rays["extinction"] == 0.0)
    assert np.all(rays["diffuse_bounce"] == 0)
    # unit directions (the tree's culled triangles are those no unit ray can hit)
    n2 = (rays["d"].astype(np.float64) ** 2).sum(axis=1)
    assert np.abs(n2 - 1.0).max() < 1e-6


def test_primary_rays_argument_checks(pt):
    ab = pt._abi
    lib = pt.load_library()
    cam = np.zeros(16, np.float32)
    rays = np.zeros(4, ab.RAY_DTYPE)
    assert lib.rt_primary_rays(None, 2, 2, ab.ptr(rays)) == ab.RT_ERR_ARG
    assert lib.rt_primary_rays(ab.ptr(cam), 2, 2, None) == ab.RT_ERR_ARG
    assert lib.rt_primary_rays(ab.ptr(cam), 0, 2, ab.ptr(rays)) == ab.RT_ERR_ARG
    assert lib.rt_primary_rays(ab.ptr(cam), 2, 0, ab.ptr(rays)) == ab.RT_ERR_ARG
    # the context entries refuse a null context before touching a device
    prm = ab.RtDenoiseParams(5, 2.0, 0.3, 0.1)
    buf = np.zeros(32, np.float32)
    assert lib.rt_get_camera(None, 4, ab.ptr(cam)) == ab.RT_ERR_ARG
    assert lib.rt_render_features(None, ab.ptr(buf), 2, 2, ab.RT_KERNEL_TRIS, 0) == ab.RT_ERR_ARG
    assert lib.rt_render_features_async(None, ab.ptr(buf), 2, 2, ab.RT_KERNEL_TRIS, 0, None) == ab.RT_ERR_ARG
    assert lib.rt_denoise(None, ab.ptr(buf), ab.ptr(buf), ab.ptr(buf), 2, 2, ctypes.byref(prm), 0) == ab.RT_ERR_ARG
    assert lib.rt_denoise_async(None, ab.ptr(buf), ab.ptr(buf), ab.ptr(buf), 2, 2, ctypes.byref(prm), 0,
                                None) == ab.RT_ERR_ARG
    ms = ctypes.c_float()
    assert lib.rt_last_features_ms(None, ctypes.byref(ms)) == ab.RT_ERR_ARG
    assert lib.rt_last_denoise_ms(None, ctypes.byref(ms)) == ab.RT_ERR_ARG


def test_denoise_defaults(pt):
    ab = pt._abi
    lib = pt.load_library()
    prm = ab.RtDenoiseParams(0, 0.0, 0.0, 0.0)
    assert lib.rt_denoise_defaults(ctypes.byref(prm)) == ab.RT_OK
    assert prm.iterations == 5
    assert (np.float32(prm.sigma_color), np.float32(prm.sigma_normal), np.float32(prm.sigma_plane)) == (
        np.float32(2.0), np.float32(0.3), np.float32(0.1))
    assert lib.rt_denoise_defaults(None) == ab.RT_ERR_ARG
    assert ctypes.sizeof(ab.RtDenoiseParams) == 16
    assert (ab.RT_FEAT_BOX, ab.RT_FEAT_NONE, ab.RT_FEAT_SPHERE0) == (-1, -2, -16)


def test_new_symbols_exported_and_bound(pt):
    lib = pt.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(pt._abi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_\w+)", nm))
    for n in NEW_SYMBOLS:
        assert n in exported, f"librtmi.so does not export {n}"
        assert n in pt._abi.SIGNATURES, f"_abi.py does not bind {n}"
        assert getattr(lib, n).argtypes is not None
    for m in ("primaryRays", "renderFeatures", "denoise", "getCamera", "lastFeaturesMs", "lastDenoiseMs"):
        assert callable(getattr(pt.RayTracer, m))
