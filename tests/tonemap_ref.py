"""numpy restatement of the tone-mapped 8-bit display output: the meter's histogram
in integers, the exposure in Python integers, binary64 and float32, and the tone map in float32, every
operation one IEEE operation in the order the definition gives.  rt_powf is the pinned one, through the
oracle.  Shared by tests/test_tonemap_host.py and tests/test_gpu_tonemap.py."""
from __future__ import annotations

import numpy as np

F = np.float32
BINS = 384
BIN0 = 1776  # bits(2^-16) >> 19
CLAMP, REINHARD, ACES = 0, 1, 2
TONE_DEFAULTS = dict(curve=ACES, srgb=1, dither=1, exposure=1.0, white=4.0)
METER_DEFAULTS = dict(key=0.18, lo=0.10, hi=0.95, e_min=2.0 ** -8, e_max=2.0 ** 12, rate=1.0)


def lum(rgb):
    """(0.2126f x + 0.7152f y) + 0.0722f z over the last axis, in float32."""
    c = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def bins(rgba):
    """(counted, bin) per pixel of an RGBA frame (any shape ending in 4, or flat)."""
    u = np.ascontiguousarray(lum(np.asarray(rgba, F).reshape(-1, 4))).view(np.uint32)
    counted = (u > 0) & (u < 0x7F800000)
    b = np.clip((u >> 19).astype(np.int64) - BIN0, 0, BINS - 1)
    return counted, b


def histogram(rgba):
    counted, b = bins(rgba)
    return np.bincount(b[counted], minlength=BINS).astype(np.uint32)


def pow_f(orc, x, y):
    x = np.ascontiguousarray(x, F)
    return orc.math("pow_xy", x, np.full(x.shape, y, F))


def exposure(orc, hist, prev, key=0.18, lo=0.10, hi=0.95, e_min=2.0 ** -8, e_max=2.0 ** 12, rate=1.0):
    """The float32 exposure from the counts and the previous exposure."""
    prev, key, lo, hi, e_min, e_max, rate = (F(v) for v in (prev, key, lo, hi, e_min, e_max, rate))
    n = [int(v) for v in hist]
    N = sum(n)
    if N == 0:
        return prev if prev > 0 else F(1.0)
    lo_n = min(int(np.float64(lo) * np.float64(N)), N - 1)
    hi_n = min(max(int(np.float64(hi) * np.float64(N)), lo_n + 1), N)
    c = S = 0
    for i, ni in enumerate(n):
        a, b = max(c, lo_n), min(c + ni, hi_n)
        if b > a:
            S += (b - a) * (2 * i + 1)
        c += ni
    K = hi_n - lo_n
    m = F(F(np.float64(S) / np.float64(32 * K)) - F(16.0))
    t = F(key * pow_f(orc, np.array([2.0], F), F(-m))[0])
    t = e_min if t < e_min else t  # rt_maxf(t, e_min)
    t = e_max if e_max < t else t  # rt_minf(., e_max)
    if not (prev > 0) or not np.isfinite(prev):
        return F(t)
    return F(prev + F(F(t - prev) * rate))


def bayer():
    """The 8 x 8 matrix B[y, x]."""
    y, x = np.mgrid[0:8, 0:8]
    a, b = x ^ y, y
    return ((a & 1) << 5 | (b & 1) << 4 | (a >> 1 & 1) << 3 | (b >> 1 & 1) << 2 | (a >> 2 & 1) << 1 | (b >> 2 & 1)).astype(np.int64)


def _clamp01(v):
    v = np.where(v < F(0.0), F(0.0), v)  # rt_maxf(v, 0)
    return np.where(F(1.0) < v, F(1.0), v).astype(F)  # rt_minf(., 1)


def encode(orc, v, srgb, d):
    """After the curve: clamp, encode, clamp, quantise; d a float32 scalar or array."""
    v = _clamp01(np.asarray(v, F))
    if srgb:
        hi = F(1.055) * pow_f(orc, v, 0.41666666) - F(0.055)
        v = _clamp01(np.where(v <= F(0.0031308), F(12.92) * v, hi).astype(F))
    q = (v * F(255.0) + d).astype(F).astype(np.int64)
    return np.minimum(q, 255).astype(np.uint32)


def curve_apply(v, curve, white=4.0):
    """The curve on exposed, clamped components v [n, 3]."""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        if curve == REINHARD:
            iw = F(1.0) / F(F(white) * F(white))
            L = lum(v)
            s = (F(1.0) + L * iw) / (F(1.0) + L)
            return (v * s[..., None]).astype(F)
        if curve == ACES:
            return ((v * (F(2.51) * v + F(0.03))) / (v * (F(2.43) * v + F(0.59)) + F(0.14))).astype(F)
    return v


def tonemap(orc, rgba, W, H, E, curve=ACES, srgb=1, dither=1, white=4.0):
    """The W*H RGBA8 words of the frame under exposure E."""
    c = np.asarray(rgba, F).reshape(H * W, 4)[:, :3]
    with np.errstate(all="ignore"):
        v = (c * F(E)).astype(F)
        v = np.where(v > 0, v, F(0.0)).astype(F)
        v = np.where(F(65536.0) < v, F(65536.0), v).astype(F)
    v = curve_apply(v, curve, white)
    if dither:
        y, x = np.mgrid[0:H, 0:W]
        d = ((bayer()[y & 7, x & 7].astype(F) + F(0.5)) * F(0.015625)).astype(F).reshape(-1, 1)
    else:
        d = F(0.5)
    q = encode(orc, v, srgb, d)
    return (q[:, 0] | q[:, 1] << 8 | q[:, 2] << 16 | np.uint32(255 << 24)).astype(np.uint32)
