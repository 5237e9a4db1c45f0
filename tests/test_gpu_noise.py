"""GPU: the noise meter and the view's stop rule.  rt_noise_meter against its numpy
restatement (tests/noise_ref.py), bit for bit over every output word — histogram, stats and tile plane;
that the call leaves a render's state alone; its argument checks; the meter on real progressive frames;
and ProgressiveViewHIP::setConverge through the rt_render CLI.  Run on the MI355X box with
`pytest -m gpu`."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import noise_ref as nr
import render_state as rs
import view_ref as vr
from conftest import bits

pytestmark = pytest.mark.gpu

CASE = "tris_64x48_sr1"
F = np.float32
U = np.uint32
# 1 x 1; one partial tile; one whole wave; a second tile to the right and above; no multiple of 8; the
# golden frame's size; many blocks; and 65 x 64 tiles = 1,088 groups of four, more than one trip of the
# persistent grid's 1,024 blocks covers
SHAPES = [(1, 1), (7, 5), (8, 8), (9, 8), (8, 9), (37, 29), (64, 48), (300, 200), (520, 512)]


@pytest.fixture(scope="module")
def rt(pt):
    t = pt.RayTracer(0)
    yield t
    t.close()


def device(a):
    import torch

    return torch.from_numpy(a.view(np.int32) if a.dtype == U else a).cuda()


def constructed():
    """(rgba [n, 4], var [n]): the odd variances under a grey pixel and the odd colours over v = 1 (first: the
    small frames hold them); then, with lum_floor = 1, black pixels with v = fl(x x), whose e is x exactly,
    x the two floats at every bin edge."""
    i = np.arange(nr.BINS, dtype=np.int64)
    edges = ((nr.BIN0 + i) << 19).astype(U)
    x = nr.f_bits(np.concatenate([edges, edges - 1]))
    nan, inf = np.nan, np.inf
    odd_v = np.array([0.0, -0.0, -1.0, -1e-30, nan, inf, -inf, 1e-45, 1e-38, 3e38, 1e-12], F)
    odd_c = np.array([[nan, 1, 1, 1], [1, nan, 1, 1], [1, 1, nan, 1], [inf, 1, 1, 1], [1, 1, inf, 1], [inf, -inf, 1, 1],
                      [-1, -1, -1, 1], [-5, 1, 1, 1], [1, -1, 1, 1], [0, 0, 0, 1], [-0.0, -0.0, -0.0, 1], [1, 1, 1, nan],
                      [3e38, 3e38, 3e38, 1], [1e-30, 1e-30, 1e-30, 1]], F)
    rgba = np.concatenate([np.full((odd_v.size, 4), 0.5, F), odd_c, np.zeros((x.size, 4), F)])
    var = np.concatenate([odd_v, np.ones(len(odd_c), F), (x * x).astype(F)])
    return rgba, var


def lognormal_frame(n, seed):
    rng = np.random.default_rng(seed)
    px = np.exp(rng.normal(-2.0, 1.5, (n, 4))).astype(F)
    px[:, 3] = 1.0
    var = np.exp(rng.normal(-6.0, 3.0, n)).astype(F)
    return px, var


def frame(w, h, seed):
    """w*h pixels: the constructed ones (as many as fit, from a rotating start) among lognormal ones."""
    n = w * h
    px, var = lognormal_frame(n, seed)
    c_px, c_var = (np.roll(a, -seed * 7, axis=0) for a in constructed())
    k = min(len(c_var), n if n < 100 else n // 2 + 1)
    where = np.random.default_rng(seed + 1).permutation(n)[:k]
    px[where], var[where] = c_px[:k], c_var[:k]
    return np.ascontiguousarray(px.reshape(-1)), np.ascontiguousarray(var)


def run(rt, rgba, var, w, h, dev=False, optional=True, **prm):
    """One call: (stats, hist or None, tiles or None), host arrays or device tensors."""
    n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
    hist, tiles = (np.full(nr.BINS, 7, U), np.full(2 * n_tiles, np.nan, F)) if optional else (None, None)
    if not dev:
        st = rt.noiseMeter(rgba, var, w, h, tiles=tiles, hist=hist, **prm)
        return st, hist, tiles
    dh, dt = (device(hist), device(tiles)) if optional else (None, None)
    st = rt.noiseMeter(device(rgba), device(var), w, h, tiles=dt, hist=dh, **prm)
    return st, (dh.cpu().numpy().view(U) if optional else None), (dt.cpu().numpy() if optional else None)


def check(got, exp, what):
    st, hist, tiles = got
    e_st, e_hist, e_tiles = exp
    assert nr.same_stats(st, e_st), (what, st, e_st)
    if hist is not None:
        assert np.array_equal(hist, e_hist), what
        assert np.array_equal(bits(tiles), bits(e_tiles)), (what, int((bits(tiles) != bits(e_tiles)).sum()))


def test_constructed_inputs_reach_every_bin():
    rgba, var = constructed()
    valid, e = nr.errors(rgba, var, lum_floor=1.0)
    assert (nr.histogram(valid, e) > 0).all() and (~valid).sum() >= 10
    assert np.isinf(e[valid]).sum() == 0 and (e.view(U) == 0x80000000).any()  # -0 among the errors


@pytest.mark.parametrize("w,h", SHAPES)
def test_meter_equals_numpy(w, h, rt):
    """Host arrays and device tensors, with and without the optional outputs, lum_floor 1 (the constructed
    pixels sit on the bin edges) and the default, percentiles 0.5, 0.95 and 1; the inputs are only read."""
    for seed in (0, 1, 2) if w * h < 1000 else (0,):
        rgba, var = frame(w, h, seed)
        keep = rgba.copy(), var.copy()
        for prm in (dict(lum_floor=1.0, percentile=0.5), dict(), dict(percentile=1.0, threshold=0.3)):
            exp = nr.meter(rgba, var, w, h, **prm)
            for dev in (False, True):
                for optional in (True, False):
                    check(run(rt, rgba, var, w, h, dev, optional, **prm), exp, (w, h, seed, prm, dev, optional))
        assert np.array_equal(bits(rgba), bits(keep[0])) and np.array_equal(bits(var), bits(keep[1]))
    assert exp[0]["skipped"] > 0 or w * h < 64
    assert rt.lastNoiseMs() > 0.0
    with pytest.raises(ValueError):
        rt.noiseMeter(rgba, device(var), w, h)  # host and device buffers mixed


def test_all_equal_and_all_different(rt):
    """The leader path: every pixel in one bin, the count exactly 60,000; and the other end: a tile whose
    64 lanes fall into 64 different bins (every lane adds itself)."""
    w, h = 300, 200
    rgba = np.tile(np.array([0.25, 0.5, 0.125, 1.0], F), w * h)
    var = np.full(w * h, 1e-4, F)
    exp = nr.meter(rgba, var, w, h)
    assert exp[1].max() == 60000 and (exp[1] > 0).sum() == 1 and exp[0]["below"] == 60000
    for dev in (False, True):
        check(run(rt, rgba, var, w, h, dev), exp, ("equal", dev))
    w, h = 16, 8
    x = nr.f_bits(((nr.BIN0 + 3 * np.arange(128, dtype=np.int64)) << 19).astype(U))
    rgba, var = np.zeros(4 * w * h, F), (x * x).astype(F)
    exp = nr.meter(rgba, var, w, h, lum_floor=1.0)
    assert exp[1].max() == 1 and (exp[1] > 0).sum() == 128
    for dev in (False, True):
        check(run(rt, rgba, var, w, h, dev, lum_floor=1.0), exp, ("different", dev))


def test_thresholds_at_a_bin_edge(rt):
    """`below` with the threshold on a bin's upper edge and on its float neighbours, and the level of a
    frame whose percentile lands in the last bin (+inf)."""
    w, h = 10, 10
    e = nr.f_bits(np.array([(nr.BIN0 + 100) << 19] * 60 + [(nr.BIN0 + 101) << 19] * 40, U))
    rgba, var = np.zeros(4 * w * h, F), (e * e).astype(F)
    edge = nr.upper_edge(100)
    seen = []
    for t in (np.nextafter(edge, F(0)), edge, np.nextafter(edge, F(1)), nr.upper_edge(101), 0.0, 3e38):
        exp = nr.meter(rgba, var, w, h, lum_floor=1.0, threshold=t)
        check(run(rt, rgba, var, w, h, lum_floor=1.0, threshold=t), exp, t)
        seen.append(exp[0]["below"])
    assert seen == [0, 60, 60, 100, 0, 100]
    var[:] = 1e12
    st = rt.noiseMeter(rgba, var, w, h, lum_floor=1.0, threshold=3e38)
    assert st["level"] == np.inf and st["below"] == 0 and st["counted"] == 100
    var[:] = np.nan
    st = rt.noiseMeter(rgba, var, w, h)
    assert (bits(np.array([st["level"]], F))[0], st["counted"], st["skipped"], st["below"]) == (0, 0, 100, 0)


def test_golden_frame_with_lognormal_noise(rt, golden, golden_meta):
    g, m = golden(CASE), golden_meta["cases"][CASE]
    W, H = m["W"], m["H"]
    rgba = np.ascontiguousarray(g["frames"][-1], F).reshape(-1)
    var = np.exp(np.random.default_rng(9).normal(-7.0, 2.5, W * H)).astype(F)
    for prm in (dict(), dict(percentile=0.5, threshold=0.01)):
        exp = nr.meter(rgba, var, W, H, **prm)
        assert (exp[1] > 0).sum() > 50
        for dev in (False, True):
            check(run(rt, rgba, var, W, H, dev, **prm), exp, (prm, dev))


def test_argument_checks(pt, rt):
    ab = pt._abi
    lib, p = rt._lib, ab.ptr
    w, h = 9, 3
    rgba, var = frame(w, h, 1)
    stats, tiles, hist = np.zeros(4, U), np.zeros(2 * 2, F), np.zeros(nr.BINS, U)
    nan, inf = float("nan"), float("inf")

    def call(rgba_=rgba, var_=var, st_=stats, tl_=tiles, hs_=hist, w_=w, h_=h, prm=(0.95, 0.05, 1e-3), flags=0):
        pr = ab.RtNoiseParams(*prm) if prm else None
        return lib.rt_noise_meter(rt._h, p(rgba_), p(var_), p(st_), p(tl_), p(hs_), w_, h_, ctypes.byref(pr) if pr else None, flags)

    assert call() == ab.RT_OK and call(tl_=None, hs_=None) == ab.RT_OK
    assert call(prm=(1.0, 0.0, 1e-30)) == ab.RT_OK  # the ends of the ranges
    stats[:] = 0
    for kw in (dict(rgba_=None), dict(var_=None), dict(st_=None), dict(prm=None), dict(w_=0), dict(h_=0), dict(w_=1 << 14, h_=1 << 14),
               dict(flags=2), dict(prm=(0.0, 0.05, 1e-3)), dict(prm=(-0.5, 0.05, 1e-3)), dict(prm=(1.5, 0.05, 1e-3)),
               dict(prm=(nan, 0.05, 1e-3)), dict(prm=(0.95, -0.1, 1e-3)), dict(prm=(0.95, nan, 1e-3)), dict(prm=(0.95, 0.05, 0.0)),
               dict(prm=(0.95, 0.05, -1.0)), dict(prm=(0.95, 0.05, inf)), dict(prm=(0.95, 0.05, nan)),
               # an output that is, or lies inside, an input or another output
               dict(st_=var), dict(tl_=var), dict(tl_=rgba[4:]), dict(hs_=rgba.view(U)), dict(st_=hist[8:]), dict(tl_=hist.view(F)[100:])):
        assert call(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
        assert lib.rt_last_error(rt._h)
    assert not stats.any()
    t = pt.RayTracer(0)
    try:
        ms = ctypes.c_float()
        assert t._lib.rt_last_noise_ms(t._h, ctypes.byref(ms)) == ab.RT_ERR_STATE
        assert t._lib.rt_last_noise_ms(t._h, None) == ab.RT_ERR_ARG
    finally:
        t.close()


def test_render_state_untouched(pt, golden, golden_meta):
    """The golden progressive frames with rt_noise_meter in between — device tensors on a side stream
    behind a render enqueued without a wait, host buffers on the context's stream — are the frames, seeds,
    counter totals, render info and rt_read of the sequence without it (tests/render_state.py)."""
    import torch

    with rs.untouched(pt, golden, golden_meta) as (t, frame_dev, g, m):
        W, H = m["W"], m["H"]
        n_tiles = ((W + 7) // 8) * ((H + 7) // 8)
        src = np.ascontiguousarray(g["frames"][-1], F).reshape(-1)
        var = np.exp(np.random.default_rng(2).normal(-7.0, 2.0, W * H)).astype(F)
        exp = nr.meter(src, var, W, H)
        dsrc, dvar = device(src), device(var)
        dst = [torch.zeros(4, dtype=torch.int32, device="cuda:0") for _ in range(m["frames"])]
        dtl = [torch.zeros(2 * n_tiles, dtype=torch.float32, device="cuda:0") for _ in range(m["frames"])]
        dhs = [torch.zeros(nr.BINS, dtype=torch.int32, device="cuda:0") for _ in range(m["frames"])]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        host = None
        for p in range(m["frames"]):
            t.rayTrace(frame_dev, W, H, p, kernel=2, sync=False)
            assert t.noiseMeter(dsrc, dvar, W, H, tiles=dtl[p], hist=dhs[p], stats=dst[p], stream=side.cuda_stream, sync=False) is None
            if p == 1:  # and host buffers on the context's own stream
                host = run(t, src, var, W, H)
    for s, tl, hs in zip(dst, dtl, dhs):
        w = s.cpu().numpy().view(U)
        st = dict(level=w[:1].view(F)[0], counted=w[1], skipped=w[2], below=w[3])
        check((st, hs.cpu().numpy().view(U), tl.cpu().numpy()), exp, "side stream")
    check(host, exp, "host")
    assert np.array_equal(bits(dsrc.cpu().numpy()), bits(src)) and np.array_equal(bits(dvar.cpu().numpy()), bits(var))


def test_level_falls_on_real_frames(pt, golden, golden_meta):
    """The golden triangle view at 64 x 48, progressive 1-spp frames from the default seeds (progression
    1..64), the moments and the variance through the library (min_len 4, lengths n everywhere): the level
    at n = 4, 16 and 64 is the restatement's, and strictly decreases.  Evaluated beforehand on the CPU
    with the restatements over the oracle's frames of exactly these inputs: 0.59375, 0.328125, 0.1640625
    (bits 3f180000, 3ea80000, 3e280000), `below` 2646, 2532, 2495 of 3072."""
    import torch

    g, m = golden(CASE), golden_meta["cases"][CASE]
    sc = pt.scenes
    W, H = m["W"], m["H"]
    Wp, Hp = sc.padded_dims(W, H)
    rt = pt.RayTracer(0)
    rt.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
    rt.setCamera(g["camera"])
    rt.setSampleRate(1)
    rt.setMaxPathDepth(m["max_depth"])
    rt.setMesh(g["verts"], g["idx"])
    rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp))

    def dev(n_floats):
        return torch.zeros(n_floats, dtype=torch.float32, device="cuda:0")

    feat, acc, prev, mom, var = dev(W * H * 8), dev(W * H * 4), dev(W * H * 4), dev(W * H * 4), dev(W * H)
    rt.renderFeatures(feat, W, H, kernel=2)
    levels = []
    for n in range(1, 65):
        prev.copy_(acc)
        torch.cuda.synchronize()
        rt.rayTrace(acc, W, H, n, kernel=2)
        rt.momentsAccumulate(prev, acc, n, mom, mom, W, H)
        if n in (4, 16, 64):
            ln = torch.full((W * H,), float(n), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            rt.variance(acc, mom, ln, feat, var, W, H, min_len=4.0)
            st = rt.noiseMeter(acc, var, W, H)
            exp = nr.meter(acc.cpu().numpy(), var.cpu().numpy(), W, H)[0]
            print(f"n {n}: level {st['level']!r} bits {bits(np.array([st['level']], F))[0]:08x} below {st['below']}")
            assert nr.same_stats(st, exp), (n, st, exp)
            assert st["counted"] == W * H
            levels.append(float(st["level"]))
    rt.close()
    assert levels[0] > levels[1] > levels[2] > 0.0


# ---- ProgressiveViewHIP through rt_render --events ----------------------------------------------

VW, VH = 64, 48
PX = VW * VH
TILE_FLOATS = 2 * (VW // 8) * (VH // 8)
# Measured beforehand with the restatements on the CPU, over the oracle's frames of this view (the mesh of
# 2,000 triangles, the CLI's camera, the default seeds), the level of the view's 5th..10th traced display
# (4..9 frames in its moments): 0.59375, 0.625, 0.53125, 0.484375, 0.4375, 0.421875.  T lies between the
# 5th's and the 8th's: the 7th display is the first at or under it.
T = 0.55
STOPS_AT = 7
MIN_FRAMES = 4
EVENTS = ",".join(["d"] * 10 + ["l"] + ["d"] * 10)
CONVERGE = ["--converge", str(T), "--converge-min-frames", str(MIN_FRAMES)]


def read_log(path):
    rows = [l.split() for l in path.read_text().splitlines()]
    return [dict(level=nr.f_bits(np.array([int(r[0], 16)], U))[0], counted=int(r[1]), skipped=int(r[2]), below=int(r[3]),
                 converged=int(r[4])) for r in rows]


def run_converge(tmp, args, outputs):
    """vr.run_view with the meter's two files beside its own."""
    log, tiles = tmp / "noise.log", tmp / "noise_map.f32"
    for f in (log, tiles):
        f.unlink(missing_ok=True)
    r = vr.run_view(tmp, args + ["--noise-log", str(log), "--noise-map-out", str(tiles)], outputs, VW, VH)
    r["log"], r["map"] = read_log(log), np.fromfile(tiles, F)
    return r


@pytest.fixture(scope="module")
def converge_run(tmp_path_factory):
    """The non-temporal run with --converge alone."""
    tmp = tmp_path_factory.mktemp("converge_view")
    return run_converge(tmp, ["--mesh", "2000", "--events", EVENTS] + CONVERGE, ("shown", "raw", "feat"))


def test_view_stops_and_resumes(converge_run, rt):
    """Ten displays, a key, ten displays.  Moments, variance and stats of every traced display are
    recomposed from the run's raw frames and features through the stage methods: every line of the noise
    log and every tile plane is theirs; tracing stops at the display the recomposition says (the 7th, by
    the CPU evaluation above), the later displays render nothing and ask for no redisplay, the key's line
    asks for one, tracing resumes and stops again."""
    run = converge_run
    lines = run["lines"][:-1]  # (the last line is the run's summary)
    assert [l["event"] for l in lines] == EVENTS.split(",")
    raw, feats, log = run["raw"], run["feat"], run["log"]
    k = 0  # traced displays so far
    mom = last = None
    frames = 0
    converged, mom_valid, realloc, progression = False, False, True, 0
    stops = []
    for l in lines:
        if l["event"] == "l":
            assert l["redisplay"] is converged and l["converged"] is False and not l["rendered"]
            converged, progression = False, 0
            continue
        trace = realloc or not converged
        assert l["rendered"] is trace, l
        if not trace:
            assert l["redisplay"] is False and l["converged"] is True
            continue
        progression = 0 if realloc else progression + 1
        realloc = False
        n = max(progression, 1)
        assert l["progression"] == progression
        cur, feat = (np.ascontiguousarray(a[c * PX * k:c * PX * (k + 1)]) for a, c in ((raw, 4), (feats, 8)))
        n_mom = n if mom_valid else 1
        new = np.zeros(4 * PX, F)
        rt.momentsAccumulate(last if n_mom > 1 else None, cur, n_mom, mom if n_mom > 1 else None, new, VW, VH)
        mom, mom_valid, last = new, True, cur
        frames = 1 if n_mom == 1 else frames + 1
        var, tiles = np.zeros(PX, F), np.zeros(TILE_FLOATS, F)
        rt.variance(cur, mom, np.full(PX, n, F), feat, var, VW, VH)
        st = rt.noiseMeter(cur, var, VW, VH, threshold=T, tiles=tiles)
        assert nr.same_stats(st, nr.meter(cur, var, VW, VH, threshold=T)[0])
        assert nr.same_stats(log[k], st), (k, log[k], st)
        assert np.array_equal(bits(run["map"][TILE_FLOATS * k:TILE_FLOATS * (k + 1)]), bits(tiles)), k
        converged = bool(frames >= MIN_FRAMES and st["counted"] > 0 and st["level"] <= F(T))
        print(f"traced display {k + 1}: frames {frames} level {st['level']!r} converged {converged}")
        assert log[k]["converged"] == int(converged) and l["converged"] is converged and l["redisplay"] is (not converged)
        k += 1
        if converged:
            stops.append(k)
    assert k == len(log) and raw.size == 4 * PX * k and run["map"].size == TILE_FLOATS * k
    assert len(stops) == 2 and stops[0] == STOPS_AT and stops[1] < 17  # it stopped, resumed after the key and stopped again
    assert lines[-1]["converged"] is True and lines[-1]["rendered"] is False


def test_converge_alone_shows_the_raw_frames(converge_run):
    """--converge without --variance-guided keeps the moments and the variance plane, and displays what it
    displayed before: the accumulation buffer."""
    assert converge_run["shown"].size and np.array_equal(bits(converge_run["shown"]), bits(converge_run["raw"]))


def test_prefix_property(tmp_path):
    """With every display stage on, the shown, raw and 8-bit frames of the --converge run are the first
    frames of the same run without it; each log line says converged exactly when the view's moments hold
    min frames, a pixel was counted and the level is at or under T."""
    events = ",".join(["d"] * 14)
    stages = ["--temporal", "--variance-guided", "--history-trust", "--tonemap"]
    args = ["--mesh", "2000", "--events", events] + stages
    off = vr.run_view(tmp_path, args, ("shown", "raw", "f8"), VW, VH)
    on = run_converge(tmp_path, args + CONVERGE, ("shown", "raw", "f8"))
    k = len(on["log"])
    print([(float(r["level"]), r["converged"]) for r in on["log"]])
    assert MIN_FRAMES < k < 14  # it stopped by itself
    for name, per in (("shown", 4 * PX), ("raw", 4 * PX), ("f8", PX)):
        assert on[name].size == per * k and off[name].size == per * 14
        assert np.array_equal(bits(on[name]), bits(off[name][:per * k])), name
    for i, r in enumerate(on["log"]):
        frames = max(i, 1)  # the second display starts the accumulation, and the moments, afresh
        assert r["converged"] == int(frames >= MIN_FRAMES and r["counted"] > 0 and r["level"] <= F(T)), (i, r)
    assert [r["converged"] for r in on["log"]] == [0] * (k - 1) + [1]
    assert "converged" not in off["lines"][0] and on["lines"][k - 1]["converged"] is True
    assert [l["rendered"] for l in on["lines"][:-1]] == [True] * k + [False] * (14 - k)
