"""CPU: the tone-mapped 8-bit display output — the new symbols and their defaults, and
the properties of the restatement tests/tonemap_ref.py that the GPU tests compare the kernels with."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

import tonemap_ref as tm
from conftest import ROOT

F = np.float32
NEW_SYMBOLS = ["rt_tonemap_defaults", "rt_meter_defaults", "rt_meter_exposure", "rt_meter_exposure_async", "rt_tonemap",
               "rt_tonemap_async", "rt_last_tonemap_ms"]


def test_new_symbols_exported_and_bound(pt):
    lib = pt.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(pt._abi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_\w+)", nm))
    for n in NEW_SYMBOLS:
        assert n in exported, f"librtmi.so does not export {n}"
        assert n in pt._abi.SIGNATURES, f"_abi.py does not bind {n}"
        assert getattr(lib, n).argtypes is not None
    for m in ("toneMap", "meterExposure", "toneMapDefaults", "meterDefaults", "lastToneMapMs"):
        assert callable(getattr(pt.RayTracer, m))
    ab = pt._abi
    assert (ab.RT_TONE_CLAMP, ab.RT_TONE_REINHARD, ab.RT_TONE_ACES, ab.RT_METER_BINS) == (0, 1, 2, 384)


def test_defaults(pt):
    ab = pt._abi
    lib = pt.load_library()
    t = ab.RtTonemapParams(9, 9, 9, -1.0, -1.0)
    assert lib.rt_tonemap_defaults(ctypes.byref(t)) == ab.RT_OK
    assert (t.curve, t.srgb, t.dither, F(t.exposure), F(t.white)) == (ab.RT_TONE_ACES, 1, 1, F(1.0), F(4.0))
    m = ab.RtMeterParams(*[-1.0] * 6)
    assert lib.rt_meter_defaults(ctypes.byref(m)) == ab.RT_OK
    assert (F(m.key), F(m.lo), F(m.hi), F(m.e_min), F(m.e_max), F(m.rate)) == \
           (F(0.18), F(0.10), F(0.95), F(2.0 ** -8), F(2.0 ** 12), F(1.0))
    assert lib.rt_tonemap_defaults(None) == ab.RT_ERR_ARG and lib.rt_meter_defaults(None) == ab.RT_ERR_ARG
    assert ctypes.sizeof(ab.RtTonemapParams) == 20 and ctypes.sizeof(ab.RtMeterParams) == 24
    for k, v in tm.TONE_DEFAULTS.items():
        assert F(getattr(t, k)) == F(v)
    for k, v in tm.METER_DEFAULTS.items():
        assert F(getattr(m, k)) == F(v)


def test_null_context_checks(pt):
    """The context entries refuse a null context before touching a device."""
    ab = pt._abi
    lib = pt.load_library()
    t, m = ab.RtTonemapParams(2, 1, 1, 1.0, 4.0), ab.RtMeterParams(0.18, 0.1, 0.95, 0.01, 10.0, 1.0)
    a = np.zeros(4, F)
    e = np.zeros(1, F)
    o = np.zeros(1, np.uint32)
    p = ab.ptr
    assert lib.rt_meter_exposure(None, p(a), p(e), None, 1, 1, ctypes.byref(m), 0) == ab.RT_ERR_ARG
    assert lib.rt_meter_exposure_async(None, p(a), p(e), None, 1, 1, ctypes.byref(m), 0, None) == ab.RT_ERR_ARG
    assert lib.rt_tonemap(None, p(a), None, p(o), 1, 1, ctypes.byref(t), 0) == ab.RT_ERR_ARG
    assert lib.rt_tonemap_async(None, p(a), None, p(o), 1, 1, ctypes.byref(t), 0, None) == ab.RT_ERR_ARG
    ms = ctypes.c_float()
    assert lib.rt_last_tonemap_ms(None, ctypes.byref(ms), None) == ab.RT_ERR_ARG


def test_bayer_matrix():
    b = tm.bayer()
    assert sorted(b.reshape(-1).tolist()) == list(range(64))
    assert b[0].tolist() == [0, 32, 8, 40, 2, 34, 10, 42]
    assert b[1].tolist() == [48, 16, 56, 24, 50, 18, 58, 26]


def test_bins(monkeypatch):
    """The bin of 2^k is 16 (k + 16) for k = -16..7; below 2^-16 bin 0, from 2^8 bin 383; 0, -1, NaN and
    inf are uncounted.  bins() is run on the luminance itself (lum patched to return the red channel)."""
    monkeypatch.setattr(tm, "lum", lambda rgb: np.asarray(rgb, F)[..., 0])

    def run(L):
        L = np.asarray(L, F)
        return tm.bins(np.stack([L, L, L, L], axis=1))

    ks = np.arange(-16, 8)
    counted, b = run(np.ldexp(F(1.0), ks))
    assert counted.all() and b.tolist() == [16 * (k + 16) for k in ks]
    assert np.array([tm.BIN0 << 19], np.uint32).view(F)[0] == F(2.0 ** -16)
    counted, b = run([2.0 ** -17, 1e-30, 1e-45, np.nextafter(F(2.0 ** -16), F(0))])
    assert counted.all() and (b == 0).all()
    counted, b = run([2.0 ** 8, 1e10, 3e38, np.nextafter(F(2.0 ** 8), F(0))])
    assert counted.all() and b.tolist() == [383, 383, 383, 383]
    counted, _ = run([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf])
    assert not counted.any()
    h = tm.histogram(np.stack([np.array([1.0, 1.0, 0.0, -1.0], F)] * 4, axis=1))
    assert h.sum() == 2 and h[16 * 16] == 2


@pytest.mark.parametrize("srgb", [0, 1])
@pytest.mark.parametrize("curve", [tm.CLAMP, tm.REINHARD, tm.ACES])
def test_curves_monotone(curve, srgb, oracle):
    """Each curve, then encode and quantise, is monotone non-decreasing over a sorted sample of [0, 8]
    (grey pixels: Reinhard scales by the pixel's luminance)."""
    rng = np.random.default_rng(5)
    x = np.sort(np.concatenate([rng.uniform(0, 8, 20000), rng.uniform(0, 0.02, 5000), [0.0, 8.0, 1.0, 0.0031308]]).astype(F))
    v = tm.curve_apply(np.stack([x, x, x], axis=1), curve)
    q = tm.encode(oracle, v, srgb, F(0.5))[:, 0].astype(np.int64)
    assert (np.diff(q) >= 0).all()
    assert q[0] == 0 and q.max() <= 255


def test_clamp_is_identity_on_the_8_bit_grid(oracle):
    """RT_TONE_CLAMP with srgb and dither off maps k / 255.0f to k for every k."""
    k = np.arange(256)
    x = (k.astype(F) / F(255.0)).astype(F)
    rgba = np.stack([x, x, x, np.ones_like(x)], axis=1).reshape(-1)
    out = tm.tonemap(oracle, rgba, 256, 1, 1.0, curve=tm.CLAMP, srgb=0, dither=0)
    for sh in (0, 8, 16):
        assert np.array_equal((out >> sh) & 255, k)
    assert ((out >> 24) == 255).all()


def test_gl_pbo_rgba8_target_builds():
    """The RGBA8 form of GlPboTargetHIP compiles and links (no GL context anywhere: nothing is run)."""
    subprocess.run(["make", "-s", "-B", "-C", str(ROOT / "tests" / "cpp"), "-f", "gl_pbo_rgba8.mk"], check=True, timeout=300)
    assert (ROOT / "tests" / "cpp" / "gl_pbo_rgba8").exists()
