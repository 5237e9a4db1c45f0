"""CPU: adaptive sampling on the noise meter's tile map — the new symbols, their defaults
and the argument checks that need no device; the stop rule's restatement (tests/adaptive_ref.py) on
hand-made planes; the CLI's refusals; and, over the oracle's frames, the precondition of the GPU view test:
that its configuration stops tiles at several displays and never all or none of them."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
import noise_ref as nr
from conftest import ROOT

F = np.float32
U = np.uint32
NEW_SYMBOLS = ["rt_set_tile_stop", "rt_adaptive_defaults", "rt_tile_stop_select", "rt_tile_stop_select_async",
               "rt_tile_stop_order", "rt_tile_stop_order_async", "rt_moments_accumulate_tiles",
               "rt_moments_accumulate_tiles_async", "rt_last_adaptive_ms"]
# the view test's configuration (tests/test_gpu_adaptive.py)
RULE = dict(threshold=0.2, max_ratio=4.0, min_frames=4, dilate=0)


def test_new_symbols_exported_and_bound(pt):
    lib = pt.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(pt._abi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_\w+)", nm))
    for n in NEW_SYMBOLS:
        assert n in exported, f"librtmi.so does not export {n}"
        assert n in pt._abi.SIGNATURES, f"_abi.py does not bind {n}"
        assert getattr(lib, n).argtypes is not None
    for m in ("setTileStop", "tileStopSelect", "tileStopOrder", "momentsAccumulateTiles", "adaptiveDefaults", "lastAdaptiveMs"):
        assert callable(getattr(pt.RayTracer, m))
    hpp = (ROOT / "include" / "RayTracerHIP.hpp").read_text()
    for m in ("setTileStop", "tileStopSelect", "momentsAccumulateTiles", "adaptiveDefaults", "lastAdaptiveMs"):
        assert re.search(rf"\b{m}\(", hpp), m
    view = (ROOT / "include" / "ProgressiveViewHIP.hpp").read_text()
    for m in ("setAdaptive", "adaptiveInEffect", "adaptiveStats", "stopMap"):
        assert re.search(rf"\b{m}\(", view), m


def test_defaults(pt):
    ab = pt._abi
    lib = pt.load_library()
    p = ab.RtAdaptiveParams(-1.0, -1.0, 99, 99)
    assert lib.rt_adaptive_defaults(ctypes.byref(p)) == ab.RT_OK
    assert (F(p.threshold), F(p.max_ratio), p.min_frames, p.dilate) == (F(0.05), F(4.0), 16, 1)
    assert lib.rt_adaptive_defaults(None) == ab.RT_ERR_ARG
    assert ctypes.sizeof(ab.RtAdaptiveParams) == 16 and ctypes.sizeof(ab.RtAdaptiveStats) == 16
    assert {k: (F(v) if isinstance(v, float) else v) for k, v in ar.DEFAULTS.items()} == \
        dict(threshold=F(p.threshold), max_ratio=F(p.max_ratio), min_frames=p.min_frames, dilate=p.dilate)
    # the meter's threshold is the rule's
    n = ab.RtNoiseParams()
    assert lib.rt_noise_defaults(ctypes.byref(n)) == ab.RT_OK and F(n.threshold) == F(p.threshold)


def test_null_context_checks(pt):
    """The context entries refuse a null context before touching a device."""
    ab = pt._abi
    lib = pt.load_library()
    p = ab.ptr
    prm = ab.RtAdaptiveParams(0.05, 4.0, 16, 1)
    t, s, st, a, ln = np.zeros(2, F), np.zeros(1, U), np.zeros(4, U), np.zeros(4, F), np.zeros(1, F)
    assert lib.rt_set_tile_stop(None, p(s), 1, 1, 0) == ab.RT_ERR_ARG
    assert lib.rt_tile_stop_select(None, p(t), p(s), 1, p(st), 1, 1, ctypes.byref(prm), 0) == ab.RT_ERR_ARG
    assert lib.rt_tile_stop_select_async(None, p(t), p(s), 1, p(st), 1, 1, ctypes.byref(prm), 0, None) == ab.RT_ERR_ARG
    assert lib.rt_tile_stop_order(None, None, p(s), 1, p(st), p(st[1:]), 0) == ab.RT_ERR_ARG
    assert lib.rt_tile_stop_order_async(None, None, p(s), 1, p(st), p(st[1:]), 0, None) == ab.RT_ERR_ARG
    assert lib.rt_moments_accumulate_tiles(None, None, p(a), 1.0, None, p(a.copy()), p(s), p(ln), 1, 1, 0) == ab.RT_ERR_ARG
    assert lib.rt_moments_accumulate_tiles_async(None, None, p(a), 1.0, None, p(a.copy()), p(s), p(ln), 1, 1, 0, None) == ab.RT_ERR_ARG
    ms = ctypes.c_float()
    assert lib.rt_last_adaptive_ms(None, ctypes.byref(ms), None) == ab.RT_ERR_ARG
    assert not st.any() and not s.any()


# ---- the rule on hand-made planes -------------------------------------------------------------------

def plane(W, H, mean, mx):
    """A tile map with every tile at (mean, mx)."""
    t = np.empty((ar.n_tiles(W, H), 2), F)
    t[:, 0], t[:, 1] = mean, mx
    return t


def test_each_term_on_its_edge():
    """mean <= threshold, max <= fl(threshold max_ratio) and n_frames >= min_frames, each on its edge and
    on its float neighbours; NaN is under nothing; +inf switches the maximum's term off."""
    thr, ratio = F(0.05), F(4.0)
    lim = F(thr * ratio)
    up, down = (lambda x: np.nextafter(F(x), F(np.inf))), (lambda x: np.nextafter(F(x), F(-np.inf)))
    cases = [((thr, lim), True), ((down(thr), down(lim)), True), ((up(thr), lim), False), ((thr, up(lim)), False),
             ((0.0, 0.0), True), ((-0.0, -0.0), True), ((np.nan, 0.0), False), ((0.0, np.nan), False), ((thr, np.inf), False)]
    for (mean, mx), want in cases:
        q = ar.quiet(np.array([[mean, mx]], F), 16, thr, ratio, 16)
        assert bool(q[0]) is want, (mean, mx)
    assert not ar.quiet(np.array([[0.0, 0.0]], F), 15, thr, ratio, 16)[0]
    assert ar.quiet(np.array([[0.0, 0.0]], F), 16, thr, ratio, 16)[0] and ar.quiet(np.array([[0.0, 0.0]], F), 17, thr, ratio, 16)[0]
    assert ar.quiet(np.array([[thr, np.inf]], F), 16, thr, np.inf, 16)[0] and ar.max_limit(0.0, np.inf) == F(np.inf)
    assert ar.max_limit(0.0, 4.0) == F(0.0) and ar.quiet(np.array([[0.0, 0.0]], F), 1, 0.0, 4.0, 1)[0]
    assert ar.max_limit(0.05, 4.1) == F(F(0.05) * F(4.1))  # one product, rounded once, in float32


def test_dilate_edges_and_neighbours():
    W, H = 72, 56  # 9 x 7 tiles
    tw, th = ar.tile_grid(W, H)
    t = plane(W, H, 0.01, 0.02).reshape(th, tw, 2)
    t[3, 4] = (1.0, 1.0)  # one noisy tile in the middle
    zero = np.zeros(tw * th, U)
    for d in (0, 1, 4):
        new, st = ar.select(t, zero, 16, W, H, dilate=d)
        held = np.zeros((th, tw), bool)
        held[max(3 - d, 0):3 + d + 1, max(4 - d, 0):4 + d + 1] = True  # its Chebyshev ball, cut at the frame
        assert np.array_equal(new.reshape(th, tw) == 0, held), d
        assert np.array_equal(new.reshape(th, tw)[~held], np.full((~held).sum(), 16, U))
        assert st == dict(tiles=63, active=int(held.sum()), stopped_now=63 - int(held.sum()), frames=16)
    # a noisy corner: the frame's edge cuts the ball, and nothing outside the frame objects
    t = plane(W, H, 0.01, 0.02).reshape(th, tw, 2)
    t[0, 0] = (1.0, 1.0)
    new, st = ar.select(t, zero, 16, W, H, dilate=1)
    assert st["active"] == 4 and (new.reshape(th, tw)[:2, :2] == 0).all()
    # a 1 x 1 grid
    for mean, want in ((0.01, 7), (1.0, 0)):
        for d in (0, 1, 4):
            new, st = ar.select(np.array([[mean, mean]], F), np.zeros(1, U), 7, 5, 3, min_frames=7, dilate=d)
            assert new.tolist() == [want] and st == dict(tiles=1, active=int(want == 0), stopped_now=int(want != 0), frames=7)


def test_stopped_neighbour_counts_as_settled_and_old_plane_decides():
    W, H = 24, 8  # 3 x 1 tiles
    t = np.array([[1.0, 1.0], [0.01, 0.01], [0.01, 0.01]], F)  # tile 0 is noisy now ...
    stop = np.array([5, 0, 0], U)  # ... but stopped earlier: it is settled
    new, st = ar.select(t, stop, 16, W, H, dilate=1)
    assert new.tolist() == [5, 16, 16] and st["stopped_now"] == 2 and st["active"] == 0
    # decisions come from the old plane: tile 1 is noisy and live, so tile 0 (quiet) may not stop because of
    # it, and tile 2 may not either — whatever order the tiles are visited in
    t = np.array([[0.01, 0.01], [1.0, 1.0], [0.01, 0.01]], F)
    new, _ = ar.select(t, np.zeros(3, U), 16, W, H, dilate=1)
    assert new.tolist() == [0, 0, 0]
    # a chain: each call settles what the call before allowed, never more
    t = np.array([[0.01, 0.01]] * 3, F)
    new, _ = ar.select(t, np.zeros(3, U), 16, W, H, dilate=1)
    assert new.tolist() == [16, 16, 16]
    # a stopped tile keeps its word whatever the map says now
    new, st = ar.select(np.array([[9.0, 9.0]] * 3, F), np.array([3, 0, 8], U), 20, W, H, dilate=0)
    assert new.tolist() == [3, 0, 8] and st == dict(tiles=3, active=1, stopped_now=0, frames=20)


def test_stopping_is_monotone():
    """Random maps over a sequence of calls: a word that is set never changes, the live count never rises,
    and the words are the frame counts of the calls that set them."""
    rng = np.random.default_rng(11)
    for W, H, d in ((64, 48, 0), (64, 48, 1), (37, 29, 2), (300, 200, 4), (8, 8, 1)):
        stop = np.zeros(ar.n_tiles(W, H), U)
        last = stop.size
        for n in range(1, 30):
            t = np.exp(rng.normal(-3.0, 1.0, (stop.size, 2))).astype(F)
            t[:, 1] = t[:, 0] * rng.uniform(1.0, 6.0, stop.size).astype(F)
            new, st = ar.select(t, stop, n, W, H, threshold=0.05, max_ratio=4.0, min_frames=4, dilate=d)
            was = stop != 0
            assert np.array_equal(new[was], stop[was]) and set(np.unique(new[~was]).tolist()) <= {0, n}
            assert st["active"] == int((new == 0).sum()) <= last and st["stopped_now"] == int((new != 0).sum() - was.sum())
            assert n >= 4 or not new.any()
            stop, last = new, st["active"]


def test_masked_order_restatement():
    rng = np.random.default_rng(5)
    for n in (1, 7, 48, 4097):
        base = rng.permutation(n).astype(U)
        stop = (rng.random(n) < 0.4).astype(U) * U(9)
        out, live = ar.order(base, stop)
        kept = [int(b) for b in base if stop[b] == 0]
        assert out.size == n and live == len(kept) and out[:live].tolist() == kept and (out[live:] == n).all() and out.max() <= n
        ident, live_i = ar.order(None, stop)
        assert ident[:live_i].tolist() == np.flatnonzero(stop == 0).tolist() and (ident[live_i:] == n).all()
    out, live = ar.order(np.array([2, 7, 0, 1], U), np.zeros(4, U))  # an entry that is no tile index
    assert out.tolist() == [2, 0, 1, 4] and live == 3


def test_masked_moments_restatement():
    import variance_ref as vr

    W, H = 11, 9
    rng = np.random.default_rng(2)
    prev, cur, mom = (rng.random(W * H * 4).astype(F) for _ in range(3))
    stop = np.array([0, 6, 3, 0], U)
    out, ln = ar.moments_tiles(prev, cur, 7, mom, stop, W, H)
    full = vr.moments(prev, cur, 7, mom)
    live = ar.pixel_mask(stop, W, H).reshape(H, W)
    assert live[:8, :8].all() and not live[:8, 8:].any() and not live[8:, :8].any() and live[8:, 8:].all()
    o, f, m = (a.reshape(H, W, 4) for a in (out, full, mom))
    assert np.array_equal(o[live].view(U), f[live].view(U)) and np.array_equal(o[~live].view(U), m[~live].view(U))
    ln = ln.reshape(H, W)
    assert (ln[live] == 7).all() and (ln[:8, 8:] == 6).all() and (ln[8:, :8] == 3).all()


# ---- the CLI's refusals -----------------------------------------------------------------------------

def test_cli_refusals():
    exe = str(ROOT / "pathtracer.cl_amd" / "rt_render")
    base = [exe, "--width", "16", "--height", "8"]

    def refused(args, word):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)

    refused(["--mesh", "100", "--events", "d", "--adaptive"], "--converge")
    refused(["--mesh", "100", "--events", "d", "--converge", "--temporal", "--adaptive", "0.1"], "--temporal")
    refused(["--events", "d", "--converge", "--adaptive"], "--mesh")
    refused(["--mesh", "100", "--events", "d", "--converge", "--stop-map-out", "x"], "--adaptive")
    refused(["--mesh", "100", "--converge", "--adaptive"], "--events")


# ---- the precondition of the GPU view test ----------------------------------------------------------

@pytest.fixture(scope="module")
def view(pt, oracle, golden, golden_meta):
    """The golden triangle view at 64 x 48, 1 spp, default seeds: the oracle and what it renders."""
    from oracle import MeshBVH

    g, m = golden("tris_64x48_sr1"), golden_meta["cases"]["tris_64x48_sr1"]
    sc = pt.scenes
    W, H = m["W"], m["H"]
    Wp, Hp = sc.padded_dims(W, H)
    spheres = g["spheres"].view(pt._abi.SPHERE_DTYPE)
    bvh = MeshBVH(oracle, g["verts"], g["idx"])

    def render(acc, progression, seeds):
        oracle.render_tris(acc, g["camera"], spheres, W, H, Wp, Hp, 1, m["max_depth"], progression, seeds, g["verts"], g["idx"],
                           bvh=bvh)

    return dict(W=W, H=H, Wp=Wp, Hp=Hp, seeds=sc.default_seeds(Wp, Hp), render=render)


def live_tiles(view, first_progression, displays, **rule):
    """Per display from n = 4 on: (live tiles after it, the meter's level).  Display k renders progression k
    under the plane the displays before it left; stopped tiles keep accumulation, moments and length."""
    W, H, Wp, Hp = view["W"], view["H"], view["Wp"], view["Hp"]
    seeds = view["seeds"].copy()
    acc, mom = np.zeros(W * H * 4, F), None
    stop = np.zeros(ar.n_tiles(W, H), U)
    seq = []
    for k in range(first_progression, displays + 1):
        n = max(k, 1)
        prev, seeds_prev, full = acc.copy(), seeds.copy(), acc.copy()
        view["render"](full, k, seeds)
        acc, seeds = ar.masked(stop, W, H, Wp, Hp, prev, full, seeds_prev, seeds)
        mom, length = ar.moments_tiles(prev, acc, n, mom, stop, W, H)
        if n >= 4:
            stats, _, tiles = nr.meter(acc, ar.variance_temporal(mom, length), W, H)
            stop, st = ar.select(tiles, stop, n, W, H, **rule)
            seq.append((st["active"], float(stats["level"])))
    return seq


def enough_events(active):
    return len(set(active)) >= 4 and 0 < min(active) and max(active) < 48  # three distinct stopping displays after the first


def test_precondition_frames_from_progression_one(view):
    """Frames of progression 1 .. 12 from the default seeds (test_gpu_noise's test_level_falls_on_real_frames
    renders these): the figures the rule was designed on, at dilate 0 and 1, and the meter's level at n = 4."""
    seq = live_tiles(view, 1, 12, **RULE)
    assert [a for a, _ in seq] == [17, 17, 15, 13, 13, 13, 13, 12, 11] and seq[0][1] == 0.59375
    assert enough_events([a for a, _ in seq])
    seq = live_tiles(view, 1, 12, **{**RULE, "dilate": 1})
    assert [a for a, _ in seq] == [39, 39, 37, 30, 30, 30, 30, 28, 28]


def test_precondition_the_views_displays(view):
    """What ProgressiveViewHIP displays: progression 0 first, which draws from the seeds before progression 1
    overwrites its frame, so every later frame differs from the ones above — and the sequence with them
    (17, 15, 13, ... against 17, 17, 15, ...).  This is the run tests/test_gpu_adaptive.py makes through the
    CLI: displays 4 to 12 stop tiles at four different displays and never all or none."""
    seq = live_tiles(view, 0, 12, **RULE)
    assert [a for a, _ in seq] == [17, 15, 13, 13, 13, 13, 12, 12, 11] and seq[0][1] == 0.59375
    assert enough_events([a for a, _ in seq])
    seq = live_tiles(view, 0, 12, **{**RULE, "dilate": 1})
    assert [a for a, _ in seq] == [39, 39, 30, 30, 30, 30, 28, 28, 28]
    # at the defaults' threshold, ratio and ring too few tiles stop for a test: of 48, 7 at the first allowed
    # display (n = 4 here, n = 16 at the default min_frames) and one more at n = 17, within 24 frames
    for min_frames in (4, 16):
        active = [a for a, _ in live_tiles(view, 1, 24, **{**ar.DEFAULTS, "min_frames": min_frames})]
        first = min_frames - 4
        assert active[:first] == [48] * first and active[first:13] == [41] * (13 - first) and active[13:] == [40] * 8
