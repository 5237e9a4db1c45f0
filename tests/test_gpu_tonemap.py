"""GPU: the tone-mapped 8-bit display output with histogram auto-exposure.
rt_meter_exposure and rt_tonemap against their numpy restatement (tests/tonemap_ref.py), bit for bit
over every pixel; that the calls leave a render's state alone; their argument checks; and
ProgressiveViewHIP::setToneMap through the rt_render CLI.  Run on the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

import ctypes
import json
import subprocess

import numpy as np
import pytest

import render_state as rs
import tonemap_ref as tm
import view_ref as vr
from conftest import ROOT, bits
from test_gpu_trust import TOL
from test_motion_host import small_move

pytestmark = pytest.mark.gpu

CASE = "tris_64x48_sr1"
F = np.float32
U = np.uint32
TW, TH = 37, 29  # the tone-map frame: every Bayer cell, no multiple of 8, more than one block
SIZES = [(1, 1), (63, 1), (65, 3), (37, 29), (300, 200), (520, 512)]


@pytest.fixture(scope="module")
def rt(pt):
    t = pt.RayTracer(0)
    yield t
    t.close()


def f_bits(u):
    return np.asarray(u, U).view(F)


def with_luminance(target):
    """Pixels (0, g, 0, 1) whose luminance (0.7152f g, exactly one product) is `target` where a float g
    gives it, else the nearest it gives."""
    t = np.asarray(target, F)
    with np.errstate(all="ignore"):
        g0 = (t / F(0.7152)).astype(F)
        best = g0.copy()
        for k in range(-3, 4):
            g = f_bits((bits(g0).astype(np.int64) + k).clip(0, 0x7F7FFFFF).astype(U))
            hit = (F(0.7152) * g).astype(F) == t
            best = np.where(hit, g, best)
    px = np.zeros((t.size, 4), F)
    px[:, 1], px[:, 3] = best, 1.0
    return px


def constructed_pixels():
    """The histogram's edge cases as RGBA pixels [n, 4]."""
    i = np.arange(tm.BINS, dtype=np.int64)
    edges = ((tm.BIN0 + i) << 19).astype(U)
    rows = [with_luminance(f_bits(edges)), with_luminance(f_bits(edges - 1))]
    rows.append(with_luminance(f_bits(np.array([1, 2, 0x7FFFFF, 0x400000, 0x800000], U))))  # subnormals, the first normal
    rows.append(with_luminance(np.array([1e-10, 1e-30, 2.0 ** -17, 300.0, 1e10, 3e38], F)))  # beyond both ends
    nan, inf = np.nan, np.inf
    rows.append(np.array([[0, 0, 0, 1], [-0.0, -0.0, -0.0, 1], [-1, -1, -1, 1], [nan, nan, nan, 1], [inf, inf, inf, 1],
                          # single channels: lum decides, not a channel
                          [nan, 1, 1, 1], [1, nan, 1, 1], [1, 1, nan, 1], [inf, 1, 1, 1], [1, 1, inf, 1], [inf, -inf, 1, 1],
                          [-1, 1, 0, 1], [1, -1, 1, 1], [-5, 1, 1, 1], [0, 0, -0.0, 1], [0, 0, 1e-3, 1], [-0.0, 1, 0, 1],
                          [1, 1, 1, nan], [1, 1, 1, -1]], F))
    return np.concatenate(rows)


def lognormal(n, seed):
    rng = np.random.default_rng(seed)
    px = np.exp(rng.normal(-3.0, 2.5, (n, 4))).astype(F)
    px[:, 3] = 1.0
    return px


def hist_frame(w, h, seed):
    """w*h pixels: the constructed ones (as many as fit, from a rotating start) among lognormal ones."""
    n = w * h
    cons = np.roll(constructed_pixels(), -seed * 97, axis=0)
    px = lognormal(n, seed)
    k = min(len(cons), n if n < 100 else n // 2 + 1)
    where = np.random.default_rng(seed + 1).permutation(n)[:k]
    px[where] = cons[:k]
    return np.ascontiguousarray(px.reshape(-1))


def device(a):
    import torch

    t = torch.from_numpy(a.view(np.int32) if a.dtype == U else a)
    return t.cuda()


def test_constructed_inputs_reach_every_bin():
    """What the histogram cases rely on: the constructed pixels occupy all 384 bins, and some are not
    counted."""
    h = tm.histogram(constructed_pixels())
    assert (h > 0).all()
    counted, _ = tm.bins(constructed_pixels())
    assert (~counted).sum() >= 12


@pytest.mark.parametrize("w,h", SIZES)
def test_histogram_equals_numpy(w, h, rt, oracle):
    """Host arrays and device tensors, with and without hist_out; 300 x 200 has 235 blocks, so the flush
    into global memory runs many times; 520 x 512 has 1040 blocks of 256 pixels against the grid's 1024, so
    some blocks take a second trip through the grid-stride loop; the frame is only read."""
    for seed in (0, 1, 2) if w * h < 1000 else (0,):
        frame = hist_frame(w, h, seed)
        keep = frame.copy()
        exp_h = tm.histogram(frame)
        for prev in (0.0, 0.37):
            exp_e = tm.exposure(oracle, exp_h, prev)
            e = np.array([prev], F)
            hist = np.full(tm.BINS, 7, U)
            rt.meterExposure(frame, e, w, h, hist=hist)
            assert np.array_equal(hist, exp_h)
            assert bits(e)[0] == bits(np.array([exp_e], F))[0]
            e2 = np.array([prev], F)
            rt.meterExposure(frame, e2, w, h)  # no hist_out
            assert bits(e2)[0] == bits(e)[0]
            dframe, de, dh = device(frame), device(np.array([prev], F)), device(np.full(tm.BINS, 7, U))
            rt.meterExposure(dframe, de, w, h, hist=dh)
            assert np.array_equal(dh.cpu().numpy().view(U), exp_h)
            assert bits(de.cpu().numpy())[0] == bits(e)[0]
            de2 = device(np.array([prev], F))
            rt.meterExposure(dframe, de2, w, h)
            assert bits(de2.cpu().numpy())[0] == bits(e)[0]
            assert np.array_equal(bits(dframe.cpu().numpy()), bits(keep))
        assert np.array_equal(bits(frame), bits(keep))
    assert rt.lastToneMapMs(meter=True) > 0.0
    with pytest.raises(ValueError):
        rt.meterExposure(frame, device(np.zeros(1, F)), w, h)  # host and device buffers mixed


def test_histogram_all_equal_frame(rt):
    """The worst case of the LDS counting: every pixel in one bin, the count exactly 60,000."""
    w, h = 300, 200
    frame = np.tile(np.array([0.25, 0.5, 0.125, 1.0], F), w * h)
    exp_h = tm.histogram(frame)
    assert exp_h.max() == 60000 and (exp_h > 0).sum() == 1
    for dev in (False, True):
        hist, e = np.zeros(tm.BINS, U), np.zeros(1, F)
        if dev:
            dh, de = device(hist), device(e)
            rt.meterExposure(device(frame), de, w, h, hist=dh)
            hist = dh.cpu().numpy().view(U)
        else:
            rt.meterExposure(frame, e, w, h, hist=hist)
        assert np.array_equal(hist, exp_h)


def grey(values_counts):
    px = np.concatenate([np.full((n, 4), v, F) for v, n in values_counts])
    px[:, 3] = 1.0
    return np.ascontiguousarray(px.reshape(-1))


EXPOSURE_FRAMES = {
    "black": grey([(0.0, 100)]),
    "one_bin": grey([(0.5, 100)]),
    "three_bins": grey([(0.01, 50), (0.3, 30), (5.0, 20)]),  # lo_n = 10 and hi_n = 95 fall inside bins
    "bright": grey([(1e5, 60), (3e5, 40)]),  # the target is below e_min
    "dark": grey([(1e-6, 100)]),  # ... above e_max
    "lognormal": np.ascontiguousarray(lognormal(100, 11).reshape(-1)),
}
EXPOSURE_PARAMS = [dict(), dict(lo=0.0, hi=1.0), dict(rate=0.25), dict(lo=0.33, hi=0.34), dict(key=0.5, e_min=0.25, e_max=2.0),
                   dict(lo=0.999, hi=1.0, rate=0.5)]


@pytest.mark.parametrize("name", list(EXPOSURE_FRAMES))
def test_exposure_equals_numpy(name, rt, oracle):
    """Every frame under every parameter set, without a previous exposure (0, NaN, inf, negative) and with
    one on either side of every target: the float's bits are the restatement's."""
    frame = EXPOSURE_FRAMES[name]
    h = tm.histogram(frame)
    seen = set()
    for prm in EXPOSURE_PARAMS:
        for prev in (0.0, -1.0, np.nan, np.inf, 2.5, 1e-3, 3000.0, 1e-5, 1e6):
            exp = tm.exposure(oracle, h, prev, **prm)
            e = np.array([prev], F)
            rt.meterExposure(frame, e, 10, 10, **prm)
            assert bits(e)[0] == bits(np.array([exp], F))[0], (name, prm, prev, e[0], exp)
            seen.add(float(exp))
    if name == "black":
        assert seen == {1.0, float("inf"), 2.5, float(F(1e-3)), 3000.0, float(F(1e-5)), 1e6}  # N == 0: prev > 0 ? prev : 1
    if name == "bright":
        assert float(F(2.0 ** -8)) in seen  # e_min
    if name == "dark":
        assert 4096.0 in seen  # e_max
    if name == "three_bins":
        assert len(seen) >= 12  # the parameters and the previous exposure both matter


# ---- the tone map ----------------------------------------------------------------------------------

def pattern_frames():
    """Every 4099th float bit pattern in [0, 8] as the colour components of 37 x 29 frames."""
    v = f_bits(np.arange(0, 0x41000000 + 1, 4099, dtype=np.int64).astype(U))
    per = TW * TH * 3
    n = (v.size + per - 1) // per
    c = np.zeros(n * per, F)
    c[:v.size] = v
    fr = np.ones((n, TW * TH, 4), F)
    fr[:, :, :3] = c.reshape(n, TW * TH, 3)
    return [np.ascontiguousarray(f.reshape(-1)) for f in fr]


def ulps(x, ks):
    return f_bits((int(bits(np.array([x], F))[0]) + np.asarray(ks, np.int64)).astype(U))


def special_frames(E, dither):
    """Two frames made for the exposure E: the sRGB knee and the odd values; and components whose
    v 255 + d sits on an integer at their own pixel's d (red), one float above (green) and below (blue)."""
    E = F(E)
    knee = ulps(0.0031308, range(-2, 3))
    vals = np.concatenate([knee, (knee / E).astype(F), ulps(F(0.0031308) / E, range(-2, 3)),
                           np.array([-1.0, -1e-30, -0.0, np.nan, np.inf, -np.inf, 1e30, 65536.0, 65537.0, 1e-45, 1e-38], F)])
    a = lognormal(TW * TH, 3)
    n = vals.size
    for ch in range(3):  # each value in each channel, the other two from the random frame
        a[ch * n:(ch + 1) * n, ch] = vals
    a[3 * n:3 * n + 40, :3] = 0.5  # a component that differs from its neighbours in one channel only
    a[3 * n:3 * n + 40:3, 0] = 0.6
    a[3 * n + 1:3 * n + 40:3, 1] = 0.4
    a[3 * n + 2:3 * n + 40:3, 2] = 0.5000001
    y, x = np.mgrid[0:TH, 0:TW]
    d = ((tm.bayer()[y & 7, x & 7].astype(F) + F(0.5)) * F(0.015625)).reshape(-1) if dither else np.full(TW * TH, 0.5, F)
    k = (np.arange(TW * TH) * 7 % 255 + 1).astype(F)
    v0 = (((k - d).astype(F) / F(255.0)).astype(F) / E).astype(F)
    q = np.ones((TW * TH, 4), F)
    q[:, 0] = v0
    q[:, 1] = f_bits(bits(v0) + 1)
    q[:, 2] = f_bits(bits(v0) - 1)
    return [np.ascontiguousarray(a.reshape(-1)), np.ascontiguousarray(q.reshape(-1))]


@pytest.fixture(scope="module")
def patterns():
    return pattern_frames()


@pytest.mark.parametrize("metered", [True, False])
@pytest.mark.parametrize("dither", [0, 1])
@pytest.mark.parametrize("srgb", [0, 1])
@pytest.mark.parametrize("curve", [tm.CLAMP, tm.REINHARD, tm.ACES])
def test_tonemap_equals_numpy(curve, srgb, dither, metered, rt, oracle, patterns):
    """3 curves x srgb x dither x (an exposure the meter wrote, params.exposure) over the pattern frames and
    the two special frames; the special frames as device tensors too.  rgba is unchanged."""
    assert len(patterns) == 83
    prm = dict(curve=curve, srgb=srgb, dither=dither, white=3.0)
    if metered:
        base = np.ascontiguousarray(lognormal(TW * TH, 21).reshape(-1))
        e = np.zeros(1, F)
        rt.meterExposure(base, e, TW, TH)
        E = e[0]
        assert bits(e)[0] == bits(np.array([tm.exposure(oracle, tm.histogram(base), 0.0)], F))[0] and E not in (1.0, 0.0)
    else:
        e, E = 0.7, F(0.7)  # a number: params.exposure
    specials = special_frames(E, dither)
    for k, frame in enumerate(specials + patterns):
        keep = frame.copy()
        exp = tm.tonemap(oracle, frame, TW, TH, E, curve, srgb, dither, white=3.0)
        out = np.zeros(TW * TH, U)
        rt.toneMap(frame, out, TW, TH, exposure=e, **prm)
        assert np.array_equal(out, exp), f"frame {k}: {(out != exp).sum()} pixels differ"
        assert np.array_equal(bits(frame), bits(keep))
        if k < 2:
            dframe, dout = device(frame), device(np.zeros(TW * TH, U))
            rt.toneMap(dframe, dout, TW, TH, exposure=device(e) if metered else e, **prm)
            assert np.array_equal(dout.cpu().numpy().view(U), exp)
            assert np.array_equal(bits(dframe.cpu().numpy()), bits(keep))
    assert rt.lastToneMapMs() > 0.0


def test_rendered_frame(rt, oracle, golden, golden_meta):
    """The golden 64 x 48 triangle frame through meter and tone map, defaults and Reinhard."""
    g, m = golden(CASE), golden_meta["cases"][CASE]
    W, H = m["W"], m["H"]
    frame = np.ascontiguousarray(g["frames"][-1], F).reshape(-1)
    keep = frame.copy()
    h = tm.histogram(frame)
    assert (h > 0).sum() > 20
    E = tm.exposure(oracle, h, 0.0)
    e, hist, out = np.zeros(1, F), np.zeros(tm.BINS, U), np.zeros(W * H, U)
    rt.meterExposure(frame, e, W, H, hist=hist)
    assert np.array_equal(hist, h) and bits(e)[0] == bits(np.array([E], F))[0]
    for prm in (dict(), dict(curve=tm.REINHARD), dict(curve=tm.CLAMP, srgb=0, dither=0)):
        rt.toneMap(frame, out, W, H, exposure=e, **prm)
        exp = tm.tonemap(oracle, frame, W, H, E, **{**dict(curve=tm.ACES, srgb=1, dither=1), **prm})
        assert np.array_equal(out, exp)
        assert len(np.unique(out)) > 50  # an image, not a constant
    assert np.array_equal(bits(frame), bits(keep))


def test_argument_checks(pt, rt):
    ab = pt._abi
    lib, p = rt._lib, ab.ptr
    w, h = 5, 3
    frame = np.ascontiguousarray(lognormal(w * h, 1).reshape(-1))
    e, out, hist = np.ones(1, F), np.zeros(w * h, U), np.zeros(tm.BINS, U)
    nan = float("nan")

    def failed(status, kw):
        assert status == ab.RT_ERR_ARG, kw
        assert lib.rt_last_error(rt._h), kw  # the message is set

    def meter(rgba=frame, e_=e, w_=w, h_=h, prm=(0.18, 0.1, 0.95, 2.0 ** -8, 4096.0, 1.0), flags=0):
        pr = ab.RtMeterParams(*prm) if prm else None
        return lib.rt_meter_exposure(rt._h, p(rgba), p(e_), p(hist), w_, h_, ctypes.byref(pr) if pr else None, flags)

    def tone(rgba=frame, e_=None, out_=out, w_=w, h_=h, prm=(2, 1, 1, 1.0, 4.0), flags=0):
        pr = ab.RtTonemapParams(*prm) if prm else None
        return lib.rt_tonemap(rt._h, p(rgba), p(e_), p(out_), w_, h_, ctypes.byref(pr) if pr else None, flags)

    assert meter() == ab.RT_OK and tone() == ab.RT_OK and tone(e_=e) == ab.RT_OK
    assert tone(e_=e, prm=(2, 1, 1, -1.0, 4.0)) == ab.RT_OK  # params->exposure is not used
    assert meter(prm=(0.18, 0.0, 1.0, 1.0, 1.0, 1.0)) == ab.RT_OK  # the ends of the ranges
    out[:] = 0
    e[:] = 1.0
    M = (0.18, 0.1, 0.95, 2.0 ** -8, 4096.0, 1.0)

    def m(i, v):
        return dict(prm=M[:i] + (v,) + M[i + 1:])

    for kw in (dict(rgba=None), dict(e_=None), dict(prm=None), dict(w_=0), dict(h_=0), dict(flags=2),
               m(0, 0.0), m(0, -1.0), m(0, nan), m(1, -0.1), m(1, 1.0), m(1, nan), m(2, 0.1), m(2, 0.05), m(2, 1.5), m(2, nan),
               m(3, 0.0), m(3, -1.0), m(3, nan), m(3, 5000.0), m(4, nan), m(5, 0.0), m(5, -0.5), m(5, 1.5), m(5, nan)):
        failed(meter(**kw), kw)
    for kw in (dict(rgba=None), dict(out_=None), dict(prm=None), dict(w_=0), dict(h_=0), dict(flags=2),
               dict(prm=(3, 1, 1, 1.0, 4.0)), dict(prm=(2, 1, 1, 1.0, 0.0)), dict(prm=(2, 1, 1, 1.0, -4.0)),
               dict(prm=(0, 1, 1, 1.0, nan)), dict(prm=(2, 1, 1, 0.0, 4.0)), dict(prm=(2, 1, 1, -1.0, 4.0)),
               dict(prm=(2, 1, 1, nan, 4.0))):
        failed(tone(**kw), kw)
    assert not out.any() and e[0] == 1.0
    t = pt.RayTracer(0)
    try:
        ms = ctypes.c_float()
        assert t._lib.rt_last_tonemap_ms(t._h, ctypes.byref(ms), None) == ab.RT_ERR_STATE
        assert t._lib.rt_last_tonemap_ms(t._h, None, ctypes.byref(ms)) == ab.RT_ERR_STATE
        assert t._lib.rt_last_tonemap_ms(t._h, None, None) == ab.RT_ERR_ARG
    finally:
        t.close()


MIXED = ["denoise", "reproject", "temporalMerge", "historyTrust", "warpFeatures", "warpFeaturesSpheres",
         "momentsAccumulate", "variance", "denoiseVar", "meterExposure", "toneMap", "noiseMeter"]


@pytest.fixture(scope="module")
def untouched(pt):
    """A tracer no call has failed on: its last error is empty."""
    t = pt.RayTracer(0)
    yield t
    t.close()


@pytest.mark.parametrize("method", MIXED)
def test_mixed_host_and_device_buffers(method, pt, untouched):
    """Every display method of RayTracer, with one buffer a CUDA tensor and the rest numpy arrays: a
    ValueError before any call crosses the ABI, so the library's last error stays empty."""
    t = untouched
    w, h = 5, 3
    px = w * h
    c4, f8, l1 = np.zeros(px * 4, F), np.zeros(px * 8, F), np.ones(px, F)
    d4, d8, d1 = device(c4), device(f8), device(l1)
    cam = np.zeros(pt._abi.CAMERA_FLOATS, F)
    calls = {
        "denoise": lambda: t.denoise(c4, f8, d4, w, h),
        "reproject": lambda: t.reproject(c4, l1, f8, cam, f8, c4.copy(), d1, w, h),
        "temporalMerge": lambda: t.temporalMerge(c4, l1, c4.copy(), 2.0, c4.copy(), d1, w, h),
        "historyTrust": lambda: t.historyTrust(c4, l1, c4.copy(), 2.0, f8, d1, w, h),
        "warpFeatures": lambda: t.warpFeatures(f8, np.zeros((0, 3), F), d8, w, h),
        "warpFeaturesSpheres": lambda: t.warpFeaturesSpheres(f8, np.zeros(0, pt._abi.SPHERE_DTYPE), d8, w, h),
        "momentsAccumulate": lambda: t.momentsAccumulate(c4, c4.copy(), 2.0, c4.copy(), d4, w, h),
        "variance": lambda: t.variance(c4, c4.copy(), l1, f8, d1, w, h),
        "denoiseVar": lambda: t.denoiseVar(c4, l1, f8, c4.copy(), d1, w, h),
        "meterExposure": lambda: t.meterExposure(c4, device(np.zeros(1, F)), w, h),
        "toneMap": lambda: t.toneMap(c4, device(np.zeros(px, U)), w, h),
        "noiseMeter": lambda: t.noiseMeter(c4, d1, w, h),
    }
    assert sorted(calls) == sorted(MIXED)
    with pytest.raises(ValueError, match="must all be host arrays or all device tensors"):
        calls[method]()
    assert t._lib.rt_last_error(t._h) == b""


def test_render_state_untouched(pt, golden, golden_meta, oracle):
    """The golden progressive frames with rt_meter_exposure and rt_tonemap in between — device tensors on
    a side stream behind a render enqueued without a wait, host buffers on the context's stream — are
    the frames, seeds, counter totals, render info and rt_read of the sequence without them
    (tests/render_state.py)."""
    import torch

    with rs.untouched(pt, golden, golden_meta) as (t, frame, g, m):
        W, H = m["W"], m["H"]
        src = np.ascontiguousarray(g["frames"][-1], F).reshape(-1)
        E = tm.exposure(oracle, tm.histogram(src), 0.0)
        exp = tm.tonemap(oracle, src, W, H, E)
        dsrc = torch.from_numpy(src).cuda()
        des = [torch.zeros(1, dtype=torch.float32, device="cuda:0") for _ in range(m["frames"])]
        douts = [torch.zeros(W * H, dtype=torch.int32, device="cuda:0") for _ in range(m["frames"])]
        he, hout = np.zeros(1, F), np.zeros(W * H, U)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        for p in range(m["frames"]):
            t.rayTrace(frame, W, H, p, kernel=2, sync=False)
            t.meterExposure(dsrc, des[p], W, H, stream=side.cuda_stream, sync=False)
            t.toneMap(dsrc, douts[p], W, H, exposure=des[p], stream=side.cuda_stream, sync=False)
            if p == 1:  # and host buffers on the context's own stream
                t.meterExposure(src, he, W, H)
                t.toneMap(src, hout, W, H, exposure=he)
    for d, de in zip(douts, des):
        assert np.array_equal(d.cpu().numpy().view(U), exp)
        assert bits(de.cpu().numpy())[0] == bits(np.array([E], F))[0]
    assert np.array_equal(hout, exp) and bits(he)[0] == bits(np.array([E], F))[0]
    assert np.array_equal(bits(dsrc.cpu().numpy()), bits(src))


# ---- ProgressiveViewHIP through rt_render --events ----------------------------------------------

VW, VH = 64, 48
# displays, a key, a drag, a pose update and a reshape (to the 37 x 29 of the tone-map tests)
EVENTS = "d,d,l,d,m:5:-3,d,d,p:1,d,s:37:29,d,d"
ALL_ON = vr.Flags(temporal=True, motion_carry=True, history_trust=True, tolerance=TOL, variance_guided=True)
TONE = ["--tonemap", "aces", "--exposure", "auto", "--adapt", "0.25"]


@pytest.fixture(scope="module")
def view_runs(pt, tmp_path_factory):
    """The event stream with every display stage on, without and with the tone map."""
    tmp = tmp_path_factory.mktemp("tonemap_view")
    verts = pt.scenes.make_mesh(2000)[0]
    np.stack([verts, small_move(verts)]).astype(F).tofile(tmp / "poses.f32")
    args = ["--mesh", "2000", "--poses", str(tmp / "poses.f32"), "--events", EVENTS] + ALL_ON.cli()
    return {"plain": vr.run_view(tmp, args, ("shown",), VW, VH),
            "tone": vr.run_view(tmp, args + TONE, ("shown", "f8", "elog", "ppm"), VW, VH)}


def test_progressive_view_tone_map(view_runs, oracle):
    """The stage alters nothing upstream: every float frame (and every JSON line) of the run with --tonemap
    is that of the run without.  Every 8-bit frame is the restatement applied to that float frame under
    the exposure carried from the previous displayed frame at rate 0.25 — through the key, the drag and
    the pose update — and started afresh after the reshape; the exposure log holds those exposures; the
    PPM is the last 8-bit frame, top row first."""
    plain, tone = view_runs["plain"], view_runs["tone"]
    assert plain["lines"] == tone["lines"]
    assert np.array_equal(bits(plain["shown"]), bits(tone["shown"]))
    sizes = [(l["width"], l["height"]) for l in tone["lines"] if l.get("rendered")]
    assert sizes == [(VW, VH)] * 6 + [(TW, TH)] * 2
    f8 = tone["f8"]
    log = [int(l, 16) for l in tone["elog"].read_text().split()]
    assert f8.size == sum(w * h for w, h in sizes) and len(log) == len(sizes)
    at = at8 = 0
    prev, exposures = F(0.0), []
    for k, (w, h) in enumerate(sizes):
        if k and sizes[k - 1] != (w, h):
            prev = F(0.0)  # the reshape: a new allocation, no exposure yet
        frame = tone["shown"][at:at + 4 * w * h]
        at += 4 * w * h
        E = tm.exposure(oracle, tm.histogram(frame), prev, rate=0.25)
        assert log[k] == int(bits(np.array([E], F))[0]), f"displayed frame {k}: exposure"
        exp = tm.tonemap(oracle, frame, w, h, E)
        assert np.array_equal(f8[at8:at8 + w * h], exp), f"displayed frame {k}"
        at8 += w * h
        prev = E
        exposures.append(float(E))
    assert len(set(exposures)) == len(exposures)  # it adapts at every display
    # rate 0.25 does carry: the second frame's exposure is not its own target
    second = tone["shown"][4 * VW * VH:8 * VW * VH]
    assert exposures[1] != float(tm.exposure(oracle, tm.histogram(second), 0.0, rate=0.25))
    # the PPM: binary P6, top row first
    raw = tone["ppm"].read_bytes()
    head = f"P6\n{TW} {TH}\n255\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + 3 * TW * TH
    rgb = np.frombuffer(raw[len(head):], np.uint8).reshape(TH, TW, 3)
    last = f8[-TW * TH:].reshape(TH, TW)[::-1]
    for c in range(3):
        assert np.array_equal(rgb[:, :, c], (last >> (8 * c)) & 255)


def test_cli_flags(tmp_path, oracle):
    """The flags' checks, and a still frame: --tonemap needs no --events, the 8-bit outputs need --tonemap;
    the still frame's PPM is the restatement of its raw frame under the flags."""
    exe = str(ROOT / "pathtracer.cl_amd" / "rt_render")
    r = subprocess.run([exe, "--width", "16", "--height", "8", "--ppm", str(tmp_path / "a.ppm")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--tonemap" in r.stderr
    r = subprocess.run([exe, "--width", "16", "--height", "8", "--tonemap", "--frames8-out", str(tmp_path / "a.u32")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--events" in r.stderr
    r = subprocess.run([exe, "--width", "16", "--height", "8", "--tonemap", "reinhard", "--exposure", "2.5", "--no-srgb", "--no-dither",
                        "--ppm", str(tmp_path / "b.ppm"), "--raw", str(tmp_path / "b.f32")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    info = [json.loads(l) for l in r.stdout.splitlines()]
    assert info[0]["exposure"] == 2.5 and "frames" in info[-1]
    raw = (tmp_path / "b.ppm").read_bytes()
    head = b"P6\n16 8\n255\n"
    assert raw.startswith(head) and len(raw) == len(head) + 3 * 16 * 8
    exp = tm.tonemap(oracle, np.fromfile(tmp_path / "b.f32", F), 16, 8, 2.5, tm.REINHARD, 0, 0, white=4.0).reshape(8, 16)[::-1]
    rgb = np.frombuffer(raw[len(head):], np.uint8).reshape(8, 16, 3)
    for c in range(3):
        assert np.array_equal(rgb[:, :, c], (exp >> (8 * c)) & 255)
