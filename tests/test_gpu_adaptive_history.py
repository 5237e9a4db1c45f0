"""GPU: adaptive sampling under the temporal stage.  The four entries against their float32
numpy restatements (tests/adaptive_history_ref.py) and against their scalar twins, word for word; their
argument checks; that they leave a render's state alone; and ProgressiveViewHIP::setAdaptiveHistory through
the rt_render CLI against the restatement of the view's chain over the oracle's frames — alone, with --budget
and with --history-trust — with the point of the feature as a condition on its planes, and the runs without
the flag against the restatements they had.  Run on the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import adaptive_history_ref as ahr
import adaptive_ref as ar
import budget_ref as br
import render_state as rs
import trust_cases as tc
import view_ref as vr
from conftest import bits
from test_adaptive_history_host import CONVERGE, EVENTS, FIRST, MIN_FRAMES, RULE, feat_with, stopped_on_history
from test_gpu_adaptive import ADAPTIVE, device, host, tile_maps
from test_gpu_budget import PX, TILES, VH, VW, check_against, golden_views, restated
from test_gpu_budget import run_cli as run_budget_cli

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
MERGE_SIZES = [(1, 1), (7, 5), (37, 29), (64, 48)]
TRUST_SIZES = [(37, 29), (64, 48)]
PLANE_SIZES = MERGE_SIZES + [(300, 200)]
ODD_COUNTS = np.array([0.0, 0.5, np.nan, 1.0, 33.0, 1e6, -2.0, 1.5], F)


def counts_plane(W, H, seed, odd=True):
    """Frame counts as a view keeps them — one per 8x8 tile — with, per pixel, the odd ones in: 0, 0.5, NaN, 1,
    values above max_history."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 20, ar.n_tiles(W, H)).astype(F)[ar.pixel_tiles(W, H)]
    if odd:
        k = min(W * H, 3 * len(ODD_COUNTS))
        c[rng.permutation(W * H)[:k]] = np.resize(ODD_COUNTS, k)
    return c


# ---- 1. the merge ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", MERGE_SIZES)
def test_merge_len_equals_numpy(tracer, W, H):
    """Host arrays and device tensors, apart and in place (the outputs are the history's buffers); the inputs
    are only read; a constant plane gives rt_temporal_merge's words."""
    px = W * H
    rng = np.random.default_rng(W * 100 + H)
    hist, cur = rng.normal(0.5, 1.0, 4 * px).astype(F), rng.normal(0.5, 1.0, 4 * px).astype(F)
    m = np.array([0.0, 0.0, 1.0, 2.5, 30.5, 32.0], F)[rng.integers(0, 6, px)]
    cl = counts_plane(W, H, W + H)
    for cap in (32.0, 8.0):
        exp, exp_len = ahr.merge_len(hist, m, cur, cl, cap)
        out, out_len = np.full(4 * px, np.nan, F), np.full(px, np.nan, F)
        keep = [a.copy() for a in (hist, m, cur, cl)]
        tracer.temporalMergeLen(hist, m, cur, cl, out, out_len, W, H, max_history=cap)
        assert np.array_equal(bits(out), bits(exp)) and np.array_equal(bits(out_len), bits(exp_len)), (W, H, cap)
        for a, b in zip((hist, m, cur, cl), keep):
            assert np.array_equal(bits(a), bits(b))
        h2, m2 = hist.copy(), m.copy()
        tracer.temporalMergeLen(h2, m2, cur, cl, h2, m2, W, H, max_history=cap)  # in place
        assert np.array_equal(bits(h2), bits(exp)) and np.array_equal(bits(m2), bits(exp_len))
        dh, dm, dc, dl = (device(a) for a in (hist, m, cur, cl))
        do, dol = device(np.zeros(4 * px + 4, F)), device(np.zeros(px + 1, F))
        tracer.temporalMergeLen(dh, dm, dc, dl, do, dol, W, H, max_history=cap)
        assert np.array_equal(bits(host(do)[:4 * px]), bits(exp)) and np.array_equal(bits(host(dol)[:px]), bits(exp_len))
        assert not host(do)[4 * px:].any() and not host(dol)[px:].any()
        tracer.temporalMergeLen(dh, dm, dc, dl, dh, dm, W, H, max_history=cap)  # in place on the device
        assert np.array_equal(bits(host(dh)), bits(exp)) and np.array_equal(bits(host(dm)), bits(exp_len))
        assert np.array_equal(bits(host(dc)), bits(cur)) and np.array_equal(bits(host(dl)), bits(cl))
    for n in (1.0, 7.0):
        a, a_len, b, b_len = np.zeros(4 * px, F), np.zeros(px, F), np.zeros(4 * px, F), np.zeros(px, F)
        tracer.temporalMerge(hist, m, cur, n, a, a_len, W, H)
        tracer.temporalMergeLen(hist, m, cur, np.full(px, n, F), b, b_len, W, H)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a_len), bits(b_len))
    assert tracer.lastReprojectMs(merge=True) > 0.0


# ---- 2. the trust test -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trust_view(pt, golden, golden_meta):
    """A tracer on the golden triangle view and its feature buffer at 64 x 48 (tests/test_gpu_trust.py's)."""
    g, m = golden(rs.CASE), golden_meta["cases"][rs.CASE]
    rt = pt.RayTracer(0)
    rt.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
    rt.setCamera(g["camera"])
    rt.setSampleRate(1)
    rt.setMaxPathDepth(m["max_depth"])
    rt.setMesh(g["verts"], g["idx"])
    feat = np.zeros(2 * tc.W0 * tc.H0 * 4, F)
    rt.renderFeatures(feat, tc.W0, tc.H0, kernel=2)
    yield rt, feat, g
    rt.close()


@pytest.mark.parametrize("source", ["golden", "synthetic"])
@pytest.mark.parametrize("w,h", TRUST_SIZES)
def test_trust_len_equals_numpy(trust_view, oracle, w, h, source):
    """The counts change at 8x8 tile borders, so the 7 x 7 windows straddle them; host and device, apart and in
    place; a constant plane gives rt_history_trust's words; tolerance inf returns hist_len."""
    rt, feat0, g = trust_view
    hist, ln, cur, feat = tc.golden_inputs(g, feat0, w, h) if source == "golden" else tc.synthetic_inputs(w, h, 100 * w + h)
    cl = counts_plane(w, h, w, odd=source == "synthetic")
    exp = ahr.trust_len(oracle, hist, ln, cur, cl, feat, w, h)
    out = np.full(w * h, np.nan, F)
    keep = [a.copy() for a in (hist, ln, cur, cl, feat)]
    rt.historyTrustLen(hist, ln, cur, cl, feat, out, w, h)
    assert np.array_equal(bits(out), bits(exp))
    for a, b in zip((hist, ln, cur, cl, feat), keep):
        assert np.array_equal(bits(a), bits(b))
    assert (source == "golden" or (exp != ln).any()) and rt.lastTrustMs() > 0.0
    inplace = ln.copy()
    rt.historyTrustLen(hist, inplace, cur, cl, feat, inplace, w, h)
    assert np.array_equal(bits(inplace), bits(exp))
    dh, dn, dc, dl, df = (device(a) for a in (hist, ln, cur, cl, feat))
    dout = device(np.zeros(w * h + 1, F))
    rt.historyTrustLen(dh, dn, dc, dl, df, dout, w, h)
    assert np.array_equal(bits(host(dout)[:w * h]), bits(exp)) and host(dout)[w * h] == 0
    rt.historyTrustLen(dh, dn, dc, dl, df, dn, w, h)  # in place on the device
    assert np.array_equal(bits(host(dn)), bits(exp)) and np.array_equal(bits(host(dl)), bits(cl))
    for n in (1.0, 5.0):
        a, b = np.zeros(w * h, F), np.zeros(w * h, F)
        rt.historyTrust(hist, ln, cur, n, feat, a, w, h)
        rt.historyTrustLen(hist, ln, cur, np.full(w * h, n, F), feat, b, w, h)
        assert np.array_equal(bits(a), bits(b))
    rt.historyTrustLen(hist, ln, cur, cl, feat, out, w, h, tolerance=np.inf)
    assert np.array_equal(bits(out), bits(ln))


# ---- 3. the tile minimum ------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", PLANE_SIZES)
def test_tile_len_min_equals_numpy(tracer, W, H):
    px, n_t = W * H, ar.n_tiles(W, H)
    rng = np.random.default_rng(W * 7 + H)
    ln = rng.uniform(0.0, 40.0, px).astype(F)
    ln[rng.permutation(px)[:max(px // 20, 1)]] = np.resize(np.array([np.nan, -1.0, 0.0, np.inf, -np.inf, 1e-30], F), max(px // 20, 1))
    ids = rng.integers(0, 50, px).astype(np.int32)
    ids[rng.random(px) < 0.3] = -2
    tile = ar.pixel_tiles(W, H)
    ids[tile == n_t // 2] = -2  # a tile of background only
    feat = feat_with(ids)
    for ft in (feat, None):
        exp = ahr.tile_len_min(ln, ft, W, H)
        out = np.full(n_t, np.nan, F)
        tracer.tileLenMin(ln, ft, out, W, H)
        assert np.array_equal(bits(out), bits(exp)), (W, H, ft is None)
        dout = device(np.full(n_t + 1, -7.0, F))
        dl, df = device(ln), None if ft is None else device(ft)
        tracer.tileLenMin(dl, df, dout, W, H)
        assert np.array_equal(bits(host(dout)[:n_t]), bits(exp)) and host(dout)[n_t] == -7.0
        assert np.array_equal(bits(host(dl)), bits(ln))
    assert np.isinf(ahr.tile_len_min(ln, feat, W, H)[n_t // 2]) and tracer.lastTileLenMs() > 0.0


# ---- 4. the stop rule --------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", PLANE_SIZES)
def test_select_frames_equals_numpy(tracer, W, H):
    n_t = ar.n_tiles(W, H)
    rng = np.random.default_rng(W + 3 * H)
    for seed, prm in enumerate((dict(), dict(min_frames=4, dilate=0), dict(threshold=0.08, max_ratio=np.inf, min_frames=1, dilate=2),
                                dict(min_frames=7, dilate=4))):
        tiles = tile_maps(W, H, seed)
        frames = rng.integers(0, 24, n_t).astype(F)
        frames[rng.permutation(n_t)[:min(n_t, 4)]] = np.array([np.nan, np.inf, 15.999, 16.0], F)[:min(n_t, 4)]
        stop = ((rng.random(n_t) < 0.25) * rng.integers(1, 1 << 32, n_t)).astype(U)
        full = {**ar.DEFAULTS, **prm}
        exp, exp_st = ahr.select_frames(tiles, frames, stop, 3, W, H, **full)
        got = stop.copy()
        assert tracer.tileStopSelectFrames(tiles, frames, got, 3, W, H, **prm) == exp_st and np.array_equal(got, exp), (W, H, prm)
        d_tiles, d_frames, d_stop = device(tiles), device(frames), device(np.append(stop, U(0xDEADBEEF)))
        assert tracer.tileStopSelectFrames(d_tiles, d_frames, d_stop, 3, W, H, **prm) == exp_st
        assert np.array_equal(host(d_stop)[:n_t], exp) and host(d_stop)[n_t] == 0xDEADBEEF
        assert np.array_equal(bits(host(d_frames)), bits(frames)) and np.array_equal(bits(host(d_tiles)), bits(tiles))
        for n in (3, 16, 40):  # a constant plane: the scalar form's plane and stats
            a, b = stop.copy(), stop.copy()
            st_a = tracer.tileStopSelect(tiles, a, n, W, H, **prm)
            st_b = tracer.tileStopSelectFrames(tiles, np.full(n_t, n, F), b, n, W, H, **prm)
            assert st_a == st_b and np.array_equal(a, b)
    assert tracer.lastAdaptiveMs() > 0.0


def test_select_frames_on_hand_made_planes(tracer):
    """tests/test_adaptive_history_host.py's planes through the kernel, at dilate 0 and 1."""
    W, H = 40, 8
    tiles = np.full((5, 2), 0.01, F)
    frames = np.array([4.0, np.nextafter(F(4), F(0)), np.nan, np.inf, 32.0], F)
    for d, start, n, want in ((0, [0] * 5, 1, [1, 0, 0, 1, 1]), (1, [0] * 5, 1, [0, 0, 0, 0, 1]), (1, [0, 7, 7, 0, 0], 2, [2, 7, 7, 2, 2])):
        stop = np.array(start, U)
        st = tracer.tileStopSelectFrames(tiles, frames, stop, n, W, H, threshold=0.05, max_ratio=4.0, min_frames=4, dilate=d)
        assert stop.tolist() == want and st == ahr.select_frames(tiles, frames, np.array(start, U), n, W, H, 0.05, 4.0, 4, d)[1]


# ---- 5. argument checks and the render state -----------------------------------------------------------------

def test_argument_checks(pt):
    """Every RT_ERR_ARG, on a context that has run none of the stages (the tile minimum's time is RT_ERR_STATE)."""
    ab = pt._abi
    t = pt.RayTracer(0)
    try:
        lib, p, h = t._lib, ab.ptr, t._h
        W, H = 20, 9  # 3 x 2 tiles
        n, px = ar.n_tiles(W, H), W * H
        nan = float("nan")
        assert lib.rt_last_tile_len_ms(h, ctypes.byref(ctypes.c_float())) == ab.RT_ERR_STATE
        assert lib.rt_last_tile_len_ms(h, None) == ab.RT_ERR_ARG
        hist, cur, out, big = (np.zeros(4 * px, F) for _ in range(4))
        m, cl, ol = np.ones(px, F), np.ones(px, F), np.zeros(px, F)
        feat = np.zeros(8 * px, F)

        def merge(hs_=hist, m_=m, cr_=cur, cl_=cl, cap=32.0, o_=out, ol_=ol, w_=W, h_=H, flags=0):
            return lib.rt_temporal_merge_len(h, p(hs_), p(m_), p(cr_), p(cl_), cap, p(o_), p(ol_), w_, h_, flags)

        for kw in (dict(hs_=None), dict(m_=None), dict(cr_=None), dict(cl_=None), dict(o_=None), dict(ol_=None), dict(w_=0), dict(h_=0),
                   dict(w_=1 << 14, h_=1 << 14), dict(flags=2), dict(cap=0.5), dict(cap=nan), dict(o_=cur), dict(ol_=cl),
                   dict(o_=big, cl_=big[4:4 + px]), dict(cl_=big[:px], ol_=big[px - 1:2 * px - 1])):
            assert merge(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
            assert lib.rt_last_error(h)
        assert not out.any() and not ol.any()
        assert merge() == ab.RT_OK and merge(o_=hist, ol_=m) == ab.RT_OK

        def trust(hs_=hist, m_=m, cr_=cur, cl_=cl, f_=feat, ol_=ol, w_=W, h_=H, prm=(1.5, 0.3, 0.1), flags=0):
            pr = ab.RtTrustParams(*(prm or (1.5, 0.3, 0.1)))
            return lib.rt_history_trust_len(h, p(hs_), p(m_), p(cr_), p(cl_), p(f_), p(ol_), w_, h_, ctypes.byref(pr) if prm else None, flags)

        ol[:] = 0.0
        for kw in (dict(hs_=None), dict(m_=None), dict(cr_=None), dict(cl_=None), dict(f_=None), dict(ol_=None), dict(prm=None), dict(w_=0),
                   dict(h_=0), dict(flags=2), dict(prm=(0.0, 0.3, 0.1)), dict(prm=(nan, 0.3, 0.1)), dict(prm=(1.5, 0.0, 0.1)),
                   dict(prm=(1.5, 0.3, nan)), dict(ol_=hist), dict(ol_=cur), dict(ol_=feat), dict(ol_=cl), dict(cl_=big[:px], ol_=big[1:px + 1])):
            assert trust(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
        assert not ol.any()
        assert trust() == ab.RT_OK and trust(ol_=m.copy()) == ab.RT_OK and trust(prm=(float("inf"), 0.3, 0.1)) == ab.RT_OK

        tl = np.zeros(n, F)

        def len_min(ln_=m, f_=feat, tl_=tl, w_=W, h_=H, flags=0):
            return lib.rt_tile_len_min(h, p(ln_), p(f_), p(tl_), w_, h_, flags)

        for kw in (dict(ln_=None), dict(tl_=None), dict(w_=0), dict(h_=0), dict(w_=1 << 14, h_=1 << 14), dict(flags=2), dict(tl_=m),
                   dict(tl_=feat[8 * px - n:]), dict(tl_=m[px - 1:px - 1 + n])):
            assert len_min(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
        assert not tl.any()
        m[:] = 3.0
        assert len_min() == ab.RT_OK and len_min(f_=None) == ab.RT_OK and (tl == 3.0).all()

        tiles, frames, stop, stats = np.full(2 * n, 0.01, F), np.full(n, 9.0, F), np.zeros(n, U), np.zeros(4, U)

        def select(tm_=tiles, fr_=frames, sp_=stop, n_=5, st_=stats, w_=W, h_=H, prm=(0.05, 4.0, 4, 1), flags=0):
            pr = ab.RtAdaptiveParams(*(prm or (0.05, 4.0, 4, 1)))
            return lib.rt_tile_stop_select_frames(h, p(tm_), p(fr_), p(sp_), n_, p(st_), w_, h_, ctypes.byref(pr) if prm else None, flags)

        for kw in (dict(tm_=None), dict(fr_=None), dict(sp_=None), dict(st_=None), dict(prm=None), dict(w_=0), dict(h_=0), dict(flags=2),
                   dict(n_=0), dict(prm=(-0.1, 4.0, 4, 1)), dict(prm=(nan, 4.0, 4, 1)), dict(prm=(0.05, 0.5, 4, 1)), dict(prm=(0.05, nan, 4, 1)),
                   dict(prm=(0.05, 4.0, 4, 5)), dict(sp_=tiles.view(U)), dict(st_=stop), dict(st_=tiles.view(U)[2:6]), dict(sp_=frames.view(U)),
                   dict(fr_=stop.view(F)), dict(st_=frames.view(U)[1:5])):
            assert select(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
        assert not stop.any() and not stats.any()
        assert select() == ab.RT_OK and (stop == 5).all() and stats.tolist() == [n, 0, n, 5]
    finally:
        t.close()


def test_render_state_untouched(pt, oracle, golden, golden_meta):
    """The golden progressive frames with the four entries in between — device tensors on a side stream behind a
    render enqueued without a wait, host buffers on the context's stream — are the frames, seeds, counter totals,
    render info and rt_read of the sequence without them."""
    import torch

    with rs.untouched(pt, golden, golden_meta) as (t, frame_dev, g, m):
        W, H = m["W"], m["H"]
        n, px = ar.n_tiles(W, H), W * H
        feat0 = np.zeros(8 * px, F)
        t.renderFeatures(feat0, W, H, kernel=2)
        hist, ln, cur, feat = tc.golden_inputs(g, feat0, W, H)
        cl = counts_plane(W, H, 5)
        tiles, frames, stop = tile_maps(W, H, 2), np.random.default_rng(1).integers(0, 30, n).astype(F), (np.arange(n) % 5 == 0).astype(U) * U(3)
        exp_trust = ahr.trust_len(oracle, hist, ln, cur, cl, feat, W, H)
        exp_merge = ahr.merge_len(hist, exp_trust, cur, cl)
        exp_min = ahr.tile_len_min(exp_merge[1], feat, W, H)
        rule = dict(threshold=0.1, max_ratio=8.0, min_frames=4, dilate=0)
        exp_stop, exp_st = ahr.select_frames(tiles, frames, stop, 6, W, H, **rule)
        dh, dn, dc, dl, df, dt, dfr = (device(a) for a in (hist, ln, cur, cl, feat, tiles, frames))
        per = range(m["frames"])
        d_trust, d_len = ([torch.zeros(px, dtype=torch.float32, device="cuda:0") for _ in per] for _ in range(2))
        d_out = [torch.zeros(4 * px, dtype=torch.float32, device="cuda:0") for _ in per]
        d_min = [torch.zeros(n, dtype=torch.float32, device="cuda:0") for _ in per]
        d_stop, d_stats = [device(stop) for _ in per], [torch.zeros(4, dtype=torch.int32, device="cuda:0") for _ in per]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        on_host = None
        for p in per:
            t.rayTrace(frame_dev, W, H, p, kernel=2, sync=False)
            kw = dict(stream=side.cuda_stream, sync=False)
            t.historyTrustLen(dh, dn, dc, dl, df, d_trust[p], W, H, **kw)
            t.temporalMergeLen(dh, d_trust[p], dc, dl, d_out[p], d_len[p], W, H, **kw)
            t.tileLenMin(d_len[p], df, d_min[p], W, H, **kw)
            assert t.tileStopSelectFrames(dt, dfr, d_stop[p], 6, W, H, stats=d_stats[p], **rule, **kw) is None
            if p == 1:  # and host buffers on the context's own stream
                h_trust, h_out, h_len, h_min, h_stop = np.zeros(px, F), np.zeros(4 * px, F), np.zeros(px, F), np.zeros(n, F), stop.copy()
                t.historyTrustLen(hist, ln, cur, cl, feat, h_trust, W, H)
                t.temporalMergeLen(hist, h_trust, cur, cl, h_out, h_len, W, H)
                t.tileLenMin(h_len, feat, h_min, W, H)
                on_host = (h_trust, h_out, h_len, h_min, h_stop, t.tileStopSelectFrames(tiles, frames, h_stop, 6, W, H, **rule))
    for p in per:
        for got, exp in ((d_trust[p], exp_trust), (d_out[p], exp_merge[0]), (d_len[p], exp_merge[1]), (d_min[p], exp_min)):
            assert np.array_equal(bits(host(got)), bits(exp))
        assert np.array_equal(host(d_stop[p]), exp_stop) and host(d_stats[p]).tolist() == [exp_st[k] for k in ("tiles", "active", "stopped_now", "frames")]
    for got, exp in zip(on_host[:4], (exp_trust, exp_merge[0], exp_merge[1], exp_min)):
        assert np.array_equal(bits(got), bits(exp))
    assert np.array_equal(on_host[4], exp_stop) and on_host[5] == exp_st and 0 < exp_st["stopped_now"]


# ---- 6. ProgressiveViewHIP::setAdaptiveHistory through rt_render --events --------------------------------------

N_DISPLAYS = EVENTS.count("d")
BASE = ["--mesh", "2000", "--events", EVENTS, "--converge", str(CONVERGE), "--converge-min-frames", str(MIN_FRAMES)]
HISTORY = BASE + ["--temporal"] + ADAPTIVE + ["--adaptive-history"]
TOLERANCE = 1.5  # rt_trust_defaults


def run_cli(tmp, args, budget=False):
    """tests/test_gpu_budget.py's run_cli with the kept history lengths beside its files."""
    lens = tmp / "history_len.f32"
    lens.unlink(missing_ok=True)
    r = run_budget_cli(tmp, args + ["--history-len-out", str(lens)], budget=budget)
    r["lens"] = np.fromfile(lens, F)
    return r


@pytest.fixture(scope="module")
def view_runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("adaptive_history_view")
    return dict(plain=run_cli(tmp, HISTORY), budget=run_cli(tmp, HISTORY + ["--budget", "4"], budget=True),
                trust=run_cli(tmp, HISTORY + ["--history-trust"]))


def check_view(run, seq, budget):
    """Every display of `run` against the restatement's: the shown frame, the kept lengths, the accumulation
    buffer, the stop plane, the tile map, the noise-log line and the event line's figures; with a budget the
    counts, the budget log and the line's."""
    assert len(seq) == N_DISPLAYS and run["raw"].size == 4 * PX * N_DISPLAYS == run["shown"].size and run["lens"].size == PX * N_DISPLAYS
    for k, d in enumerate(seq):
        assert np.array_equal(bits(run["raw"][4 * PX * k:4 * PX * (k + 1)]), bits(d["acc"])), k
        assert np.array_equal(bits(run["shown"][4 * PX * k:4 * PX * (k + 1)]), bits(d["shown"])), k
        assert np.array_equal(bits(run["lens"][PX * k:PX * (k + 1)]), bits(d["length"])), k
        assert np.array_equal(run["stops"][TILES * k:TILES * (k + 1)], d["stop"]), k
        assert np.array_equal(bits(run["map"][2 * TILES * k:2 * TILES * (k + 1)]), bits(d["tiles"])), k
        s = d["stats"]
        level = int(np.array([s["level"]], F).view(U)[0])
        assert run["noise"][k] == "%08x %u %u %u %d" % (level, s["counted"], s["skipped"], s["below"], int(d["converged"])), k
        line = run["lines"][k if k < FIRST else k + 1]
        assert line["rendered"] and line["tiles_active"] == d["active"] and line["converged"] == d["converged"], k
        if budget:
            assert np.array_equal(run["counts"][TILES * k:TILES * (k + 1)], d["count"]), k
            assert run["budget"][k] == [d["rounds"], d["tile_passes"]] + d["by_passes"], k
            assert line["rounds"] == d["rounds"] and line["tile_passes"] == d["tile_passes"], k


@pytest.mark.parametrize("name", ["plain", "budget", "trust"])
def test_view_follows_the_restatement(view_runs, pt, oracle, golden, golden_meta, name):
    """--temporal --converge --adaptive --adaptive-history, alone, with --budget 4 and with --history-trust: every
    displayed frame, kept length plane, accumulation buffer, stop plane and count plane is the restatement's over
    the oracle's frames, before and after the key.  And the point of the feature: at the first display after the
    key tiles are stopped with a word below min_frames — on their history — while others are live."""
    run = view_runs[name]
    kw = dict(budget_prm=dict(br.DEFAULTS)) if name == "budget" else dict(tolerance=TOLERANCE) if name == "trust" else {}
    seq = ahr.golden_view(pt, oracle, golden, golden_meta, EVENTS, CONVERGE, MIN_FRAMES, RULE, feats=run["feat"], **kw)
    check_view(run, seq, budget=name == "budget")
    stop = run["stops"][TILES * FIRST:TILES * (FIRST + 1)]
    early, live = int(((stop != 0) & (stop < RULE["min_frames"])).sum()), int((stop == 0).sum())
    print(name, "after the key: stopped on history", early, "live", live, "restated", [stopped_on_history(d) for d in seq[FIRST:]])
    assert (early, live) == stopped_on_history(seq[FIRST]) and early >= 1 and live >= 1
    if name == "budget":
        assert all(d["budget"] for d in seq) and max(d["rounds"] for d in seq) >= 2
    if name == "trust":  # (the test judged: some length differs from the run without it)
        assert not np.array_equal(bits(run["lens"]), bits(view_runs["plain"]["lens"]))


def test_opt_in_off_changes_nothing(tmp_path, pt, oracle, golden, golden_meta):
    """Without --adaptive-history: --temporal --converge is view_ref.displayed's bytes (the merged frame, from the
    run's raw frames through the library's scalar stages), --converge --adaptive and --converge --adaptive --budget
    are test_gpu_budget.restated's over the oracle's frames."""
    views = golden_views(pt, oracle, golden, golden_meta)
    for extra, prm in ((ADAPTIVE, None), (ADAPTIVE + ["--budget", "4"], dict(br.DEFAULTS))):
        run = run_budget_cli(tmp_path, BASE + extra, budget=prm is not None)
        seq = restated(views, run, CONVERGE, prm)
        assert len(seq) == N_DISPLAYS
        check_against(run, seq, budget=prm is not None)
        assert np.array_equal(bits(run["shown"]), bits(run["raw"]))
    run = vr.run_view(tmp_path, BASE + ["--temporal"], width=VW, height=VH)
    t = pt.RayTracer(0)
    try:
        got = vr.displayed(t, pt.scenes, vr.Flags(temporal=True), EVENTS, run["raw"], run["feat"], VW, VH)
    finally:
        t.close()
    assert len(got.frames) == N_DISPLAYS
    assert np.array_equal(bits(run["shown"]), bits(np.concatenate(got.frames)))
    assert all("tiles_active" not in l for l in run["lines"])
