"""Host side of the variance-guided display filter (CPU only): the new ABI, the defaults, the checks
that need no device, and the restatement (tests/variance_ref.py) against what it must compute
independently of any kernel: the moments of known per-frame images, and the a-trous filter of
DESIGN.md §4.9 when the luminance term is off."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

import features_ref as fr
import variance_ref as vr
from conftest import bits

F = np.float32
CASE = "tris_64x48_sr1"
NEW_SYMBOLS = ["rt_denoise_var_defaults", "rt_moments_accumulate", "rt_moments_accumulate_async", "rt_variance",
               "rt_variance_async", "rt_denoise_var", "rt_denoise_var_async", "rt_last_variance_ms"]


def test_new_symbols_exported_and_bound(pt):
    lib = pt.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(pt._abi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_\w+)", nm))
    for n in NEW_SYMBOLS:
        assert n in exported, f"librtmi.so does not export {n}"
        assert n in pt._abi.SIGNATURES, f"_abi.py does not bind {n}"
        assert getattr(lib, n).argtypes is not None
    for m in ("momentsAccumulate", "variance", "denoiseVar", "denoiseVarDefaults", "lastVarianceMs"):
        assert callable(getattr(pt.RayTracer, m))


def test_denoise_var_defaults(pt):
    ab = pt._abi
    lib = pt.load_library()
    prm = ab.RtDenoiseVarParams(0, -1.0, -1.0, -1.0, -1.0)
    assert lib.rt_denoise_var_defaults(ctypes.byref(prm)) == ab.RT_OK
    assert prm.iterations == 5
    assert (F(prm.sigma_lum), F(prm.sigma_normal), F(prm.sigma_plane), F(prm.min_len)) == (F(4.0), F(0.3), F(0.1), F(4.0))
    assert lib.rt_denoise_var_defaults(None) == ab.RT_ERR_ARG
    assert ctypes.sizeof(ab.RtDenoiseVarParams) == 20


def test_null_context_checks(pt):
    """The context entries refuse a null context before touching a device."""
    ab = pt._abi
    lib = pt.load_library()
    prm = ab.RtDenoiseVarParams(5, 4.0, 0.3, 0.1, 4.0)
    buf, out = np.zeros(64, F), np.zeros(64, F)
    p, o, pr = ab.ptr(buf), ab.ptr(out), ctypes.byref(prm)
    assert lib.rt_moments_accumulate(None, p, p, 2.0, p, o, 2, 2, 0) == ab.RT_ERR_ARG
    assert lib.rt_moments_accumulate_async(None, p, p, 2.0, p, o, 2, 2, 0, None) == ab.RT_ERR_ARG
    assert lib.rt_variance(None, p, p, p, p, o, 2, 2, pr, 0) == ab.RT_ERR_ARG
    assert lib.rt_variance_async(None, p, p, p, p, o, 2, 2, pr, 0, None) == ab.RT_ERR_ARG
    assert lib.rt_denoise_var(None, p, p, p, o, o, 2, 2, pr, 0) == ab.RT_ERR_ARG
    assert lib.rt_denoise_var_async(None, p, p, p, o, o, 2, 2, pr, 0, None) == ab.RT_ERR_ARG
    ms = ctypes.c_float()
    assert lib.rt_last_variance_ms(None, ctypes.byref(ms), None, None) == ab.RT_ERR_ARG
    assert not out.any()


@pytest.mark.parametrize("n_frames", [1, 2, 17, 64])
def test_moments_recover_known_frames(n_frames):
    """Known per-frame images s_1..s_n with components in [0, 1), accumulated as the progressive render
    does (float32 mix(acc, s_k, 1 / k)); the restatement's moments, fed the accumulation before and
    after every frame, against the float64 mean of lum(s_k) and of its square.

    The bound.  u = 2^-24 is the unit roundoff at magnitudes below 1.  The mix rounds four times
    (difference, reciprocal, product, sum): acc_k carries at most 4 u of its own.  The inversion
    prev + (cur - prev) k multiplies that by k and rounds three times more: a recovered component is
    within (4 k + 3) u of s_k, and so is its luminance (weights summing to 1) up to 3 u more of
    its own rounding; its square within twice that plus u.  The running mean damps an earlier error by
    (k - 1) / k per step and adds at most 3 u per step, which at the end weighs k / n: in all the
    mean of the sample errors, at most (2 (n + 1) + 6) u, plus 1.5 (n + 1) u, and for the second
    moment twice the former plus u — both below 8 (n + 2) u, the bound asserted."""
    rng = np.random.default_rng(n_frames)
    px = 257
    s = rng.random((n_frames, px, 4), dtype=F)
    acc = np.zeros((px, 4), F)
    mom = None
    for k in range(1, n_frames + 1):
        prev = acc.copy()
        acc = vr.mix(prev, s[k - 1], k)
        mom = vr.moments(prev.reshape(-1), acc.reshape(-1), k, mom)
    L = (0.2126 * s[:, :, 0].astype(np.float64) + 0.7152 * s[:, :, 1]) + 0.0722 * s[:, :, 2]
    m = mom.reshape(px, 4)
    e1 = np.abs(m[:, 0] - L.mean(axis=0)).max()
    e2 = np.abs(m[:, 1] - (L * L).mean(axis=0)).max()
    bound = 8 * (n_frames + 2) * 2.0 ** -24
    print(f"n {n_frames}: first moment off by {e1:.3e}, second by {e2:.3e}, bound {bound:.3e}")
    assert e1 <= bound and e2 <= bound
    assert not m[:, 2:].any()


def test_moments_clamp_and_first_frame():
    """n = 1 takes the current frame as the sample and reads no history; a recovered sample below 0
    counts as 0."""
    cur = np.array([0.5, 0.25, 1.0, 9.0, -0.5, -0.25, -1.0, 9.0], F)
    m = vr.moments(None, cur, 1.0, None).reshape(2, 4)
    L = vr.lum(cur.reshape(2, 4)[:1])[0]
    assert np.array_equal(bits(m[0]), bits(np.array([L, L * L, 0, 0], F)))
    assert not m[1].any()
    prev = np.array([0.5, 0.5, 0.5, 0.0], F)
    cur = np.array([0.25, 0.5, 0.75, 0.0], F)  # n = 4: the samples are -0.5, 0.5, 1.5
    m = vr.moments(prev, cur, 4.0, np.zeros(4, F))
    L = F(0.7152) * F(0.5) + F(0.0722) * F(1.5)
    assert np.array_equal(bits(m), bits(np.array([L * F(0.25), (L * L) * F(0.25), 0, 0], F)))


def _cpu_features(pt, oracle, golden, W, H):
    g = golden(CASE)
    rays = np.zeros(W * H, pt._abi.RAY_DTYPE)
    cam = np.ascontiguousarray(g["camera"], F)
    assert pt.load_library().rt_primary_rays(pt._abi.ptr(cam), W, H, pt._abi.ptr(rays)) == pt._abi.RT_OK
    return fr.features_tris(oracle, rays, g["verts"], g["idx"]).reshape(-1)


def test_luminance_term_off_is_the_feature_filter(pt, oracle, golden):
    """sigma_lum = +INFINITY: the colour output is that of the a-trous filter of §4.9 with its colour
    term off, bit for bit, whatever the variance plane holds; and the variance output is the input's
    filtered by the squared weights (a constant plane under weights w: sum(w^2) / sum(w)^2 of it,
    never above it)."""
    W, H = 37, 29
    feat = _cpu_features(pt, oracle, golden, W, H)
    rng = np.random.default_rng(3)
    col = (rng.random(W * H * 4, dtype=F) * F(1.5)).astype(F)
    var = (rng.random(W * H, dtype=F) * F(0.01)).astype(F)
    for it in (1, 3):
        out, ov = vr.denoise_var(oracle, col, var, feat, W, H, iterations=it, sigma_lum=np.inf)
        exp = fr.atrous(oracle, col, feat, W, H, iterations=it, sigma_color=np.inf)
        assert np.array_equal(bits(out), bits(exp))
        assert np.isfinite(ov).all() and (ov >= 0).all()
    out1, ov1 = vr.denoise_var(oracle, col, np.full(W * H, 0.5, F), feat, W, H, iterations=1, sigma_lum=np.inf)
    assert (ov1 <= F(0.5) * (1 + 1e-6)).all() and ov1.min() < 0.25


def test_variance_estimates(pt, oracle, golden):
    """The restatement of rt_variance where the answer is known: constant luminance has no variance in
    either estimate; moments (mu, mu^2 + d) over l >= min_len frames give d / (l - 1); below min_len
    the spatial estimate of an image that is L0 on even columns and L1 on odd ones over a featureless
    plane is the weighted variance of those two values, scaled by min_len / max(l, 1)."""
    W, H = 16, 9
    n = W * H
    feat = np.zeros((2, n, 4), F)
    feat[0, :, 3] = 1.0
    feat[1, :, 2] = -1.0  # one plane, one normal: every tap weighs 1
    feat[1, :, 3] = np.full(n, 5, np.int32).view(F)
    feat = feat.reshape(-1)
    flat = np.tile(np.array([0.25, 0.25, 0.25, 1.0], F), n)
    mom = np.tile(np.array([0.25, 0.0625, 0, 0], F), n)
    for l in (0.0, 1.0, 3.0, 4.0, 40.0):
        assert not vr.variance(oracle, flat, mom, np.full(n, l, F), feat, W, H).any()
    mom = np.tile(np.array([0.5, 0.25 + 0.125, 0, 0], F), n)
    v = vr.variance(oracle, flat, mom, np.full(n, 9.0, F), feat, W, H)
    assert np.array_equal(v, np.full(n, 0.125 / 8.0, F))
    stripes = np.zeros((H, W, 4), F)
    stripes[:, 0::2, :3] = 0.0
    stripes[:, 1::2, :3] = 1.0
    for l, scale in ((0.0, 4.0), (1.0, 4.0), (2.0, 2.0), (3.0, 4.0 / 3.0)):
        v = vr.variance(oracle, stripes.reshape(-1), mom, np.full(n, l, F), feat, W, H).reshape(H, W)
        # an interior window holds 3 columns of one value and 4 of the other: variance 12 / 49
        assert np.allclose(v[:, 3:-3], scale * 12.0 / 49.0, rtol=1e-5)
