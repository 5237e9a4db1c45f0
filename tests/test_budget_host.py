"""CPU: per-tile sample counts — the new symbols, their defaults and the argument checks
that need no device (those that need a context are in tests/test_gpu_budget.py); the budget rule's and the
pass mask's restatement (tests/budget_ref.py) on hand-made maps; the fold's restatement at uniform counts against the progressive mix and the moments of
tests/variance_ref.py; and the CLI's refusals."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np

import adaptive_ref as ar
import budget_ref as br
import variance_ref as vr
from conftest import ROOT, bits

F = np.float32
U = np.uint32
NEW_SYMBOLS = ["rt_fold_tiles", "rt_fold_tiles_async", "rt_budget_defaults", "rt_tile_budget", "rt_tile_budget_async",
               "rt_tile_pass_mask", "rt_tile_pass_mask_async", "rt_last_budget_ms"]


def test_new_symbols_exported_and_bound(pt):
    lib = pt.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(pt._abi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_\w+)", nm))
    for n in NEW_SYMBOLS:
        assert n in exported, f"librtmi.so does not export {n}"
        assert n in pt._abi.SIGNATURES, f"_abi.py does not bind {n}"
        assert getattr(lib, n).argtypes is not None
    methods = ("foldTiles", "tileBudget", "tilePassMask", "budgetDefaults", "lastBudgetMs")
    for m in methods:
        assert callable(getattr(pt.RayTracer, m))
    hpp = (ROOT / "include" / "RayTracerHIP.hpp").read_text()
    for m in methods:
        assert re.search(rf"\b{m}\(", hpp), m
    view = (ROOT / "include" / "ProgressiveViewHIP.hpp").read_text()
    for m in ("setSampleBudget", "budgetStats", "setSampleCountReadback", "sampleCounts"):
        assert re.search(rf"\b{m}\(", view), m


def test_defaults(pt):
    ab = pt._abi
    lib = pt.load_library()
    p = ab.RtBudgetParams()
    p.max_passes = 99
    assert lib.rt_budget_defaults(ctypes.byref(p)) == ab.RT_OK
    assert p.max_passes == 4 and [F(v) for v in p.limits][:3] == [F(0.1), F(0.2), F(0.4)]
    assert all(F(p.limits[k + 1]) > F(p.limits[k]) for k in range(6))  # the whole table is usable at max_passes 8
    assert lib.rt_budget_defaults(None) == ab.RT_ERR_ARG
    assert ctypes.sizeof(ab.RtBudgetParams) == 32 and ctypes.sizeof(ab.RtBudgetStats) == 52
    assert br.DEFAULTS["max_passes"] == p.max_passes and [F(v) for v in br.DEFAULTS["limits"]] == [F(v) for v in p.limits][:3]
    assert br.MAX_PASSES == ab.RT_BUDGET_MAX_PASSES
    # the meter's threshold x 2, 4, 8
    n = ab.RtNoiseParams()
    assert lib.rt_noise_defaults(ctypes.byref(n)) == ab.RT_OK
    assert [F(v) for v in p.limits][:3] == [F(n.threshold) * F(k) for k in (2, 4, 8)]


def test_null_context_checks(pt):
    """The context entries refuse a null context before touching a device."""
    ab = pt._abi
    lib = pt.load_library()
    p = ab.ptr
    prm = ab.RtBudgetParams()
    lib.rt_budget_defaults(ctypes.byref(prm))
    a, b, c, w, st, t = np.zeros(4, F), np.zeros(4, F), np.zeros(1, U), np.zeros(1, U), np.zeros(13, U), np.zeros(2, F)
    assert lib.rt_fold_tiles(None, p(a), p(b), p(c), None, 0, None, None, None, 1, 1, 0) == ab.RT_ERR_ARG
    assert lib.rt_fold_tiles_async(None, p(a), p(b), p(c), None, 0, None, None, None, 1, 1, 0, None) == ab.RT_ERR_ARG
    assert lib.rt_tile_budget(None, p(t), None, p(w), p(st), 1, 1, ctypes.byref(prm), 0) == ab.RT_ERR_ARG
    assert lib.rt_tile_budget_async(None, p(t), None, p(w), p(st), 1, 1, ctypes.byref(prm), 0, None) == ab.RT_ERR_ARG
    assert lib.rt_tile_pass_mask(None, None, p(c), 0, p(w), 1, 1, 0) == ab.RT_ERR_ARG
    assert lib.rt_tile_pass_mask_async(None, None, p(c), 0, p(w), 1, 1, 0, None) == ab.RT_ERR_ARG
    ms = ctypes.c_float()
    assert lib.rt_last_budget_ms(None, ctypes.byref(ms), None, None) == ab.RT_ERR_ARG
    assert not b.any() and not c.any() and not w.any() and not st.any()


# ---- the budget rule and the pass mask on hand-made maps ---------------------------------------------

def test_budget_rule_on_its_edges():
    """A mean exactly on a limit and its two float neighbours; NaN, +inf and -0; a stop word."""
    up, down = (lambda x: np.nextafter(F(x), F(np.inf))), (lambda x: np.nextafter(F(x), F(-np.inf)))
    lim = [F(0.1), F(0.2), F(0.4)]
    means = [lim[0], down(lim[0]), up(lim[0]), lim[1], down(lim[1]), up(lim[1]), lim[2], down(lim[2]), up(lim[2]), np.nan, np.inf,
             -0.0, 0.0, -1.0, 1e30]
    want = [1, 1, 2, 2, 2, 3, 3, 3, 4, 1, 4, 1, 1, 1, 4]
    tiles = np.zeros((len(means), 2), F)
    tiles[:, 0] = means
    tiles[:, 1] = np.nan  # the maximum is not read
    passes, st = br.budget(tiles, None, 4, lim)
    assert passes.tolist() == want
    assert st == dict(tiles=15, rounds=4, tile_passes=sum(want), by_passes=[0, 6, 3, 3, 3, 0, 0, 0, 0])
    stop = np.zeros(len(means), U)
    stop[[2, 8, 9]] = [7, 0xFFFFFFFF, 1]
    passes, st = br.budget(tiles, stop, 4, lim)
    assert passes.tolist() == [0 if s else w for s, w in zip(stop, want)] and st["by_passes"][:5] == [3, 5, 2, 3, 2]
    assert st["tile_passes"] == sum(want) - 2 - 4 - 1 and st["rounds"] == 4
    # max_passes caps the limits read: 1 reads none
    for mp in range(1, 5):
        passes, st = br.budget(tiles, None, mp, lim)
        assert passes.tolist() == [min(w, mp) for w in want] and st["rounds"] == mp
    passes, st = br.budget(tiles, np.ones(len(means), U), 4, lim)
    assert not passes.any() and st["rounds"] == 0 and st["tile_passes"] == 0 and st["by_passes"][0] == 15
    # eight passes
    lim8 = [0.1 * 2 ** k for k in range(7)]
    passes, st = br.budget(np.array([[100.0, 0], [0.0, 0], [0.5, 0]], F), None, 8, lim8)
    assert passes.tolist() == [8, 1, 4] and st["by_passes"] == [0, 1, 0, 0, 1, 0, 0, 0, 1] and st["tile_passes"] == 13


def test_pass_mask_restatement():
    passes = np.array([0, 1, 2, 3, 4, 2], U)
    stop = np.array([0, 0, 0, 0, 9, 0], U)
    for r, want in ((0, [1, 0, 0, 0, 1, 0]), (1, [1, 1, 0, 0, 1, 0]), (2, [1, 1, 1, 0, 1, 1]), (3, [1] * 6)):
        assert br.pass_mask(stop, passes, r).tolist() == want
    assert br.pass_mask(None, passes, 3).tolist() == [1, 1, 1, 1, 0, 1]
    # the masks of the rounds trace every live tile exactly `passes` times
    traced = sum((br.pass_mask(stop, passes, r) == 0).astype(int) for r in range(4))
    assert traced.tolist() == [0, 1, 2, 3, 0, 2]


# ---- the fold at uniform counts: the progressive mix and the moments ----------------------------------

def test_fold_at_uniform_counts_is_mix_and_moments():
    W, H = 11, 9
    px, n_t = W * H, ar.n_tiles(W, H)
    rng = np.random.default_rng(4)
    acc = np.exp(rng.normal(-1.0, 1.0, 4 * px)).astype(F)
    sample = (acc + rng.normal(0.0, 0.5, 4 * px)).astype(F)
    mom = rng.random(4 * px).astype(F)
    for c in (0, 1, 2, 6, 1 << 24, 0xFFFFFFFE, 0xFFFFFFFF):
        n = F(min(c + 1, 0xFFFFFFFF))
        new, count, new_mom, length = br.fold(sample, acc, np.full(n_t, c, U), None, 0, W, H, mom)
        assert np.array_equal(bits(new), bits(vr.mix(acc, sample, n))), c
        assert np.array_equal(bits(new_mom), bits(vr.moments(acc, new, n, mom))), c
        assert (count == min(c + 1, 0xFFFFFFFF)).all() and (length == n).all()
    # at weight 1 the fold is still the mix, not a copy: old + (s - old) differs from s where the difference rounds
    new, *_ = br.fold(sample, acc, np.zeros(n_t, U), None, 0, W, H)
    assert np.array_equal(bits(new), bits((acc + (sample - acc)).astype(F))) and not np.array_equal(bits(new), bits(sample))


def test_fold_under_a_passes_plane():
    W, H = 11, 9  # 2 x 2 tiles, the right and upper ones partial
    px = W * H
    rng = np.random.default_rng(5)
    acc, sample, mom = (rng.random(4 * px).astype(F) for _ in range(3))
    count = np.array([0, 5, 0xFFFFFFFF, 1 << 24], U)
    passes = np.array([1, 0, 3, 2], U)
    for r, folded in ((0, [True, False, True, True]), (1, [False, False, True, True]), (2, [False, False, True, False])):
        new, cnt, new_mom, length = br.fold(sample, acc, count, passes, r, W, H, mom)
        f_px = np.array(folded)[ar.pixel_tiles(W, H)]
        assert cnt.tolist() == [1 if folded[0] else 0, 5, 0xFFFFFFFF, (1 << 24) + (1 if folded[3] else 0)]
        for got, kept in ((new, acc), (new_mom, mom)):
            g, k = got.reshape(-1, 4), kept.reshape(-1, 4)
            assert np.array_equal(bits(g[~f_px]), bits(k[~f_px]))
            if r == 0:  # (a saturated count's weight, 2^-32, moves nothing: tile 0 is the one sure to show a fold)
                assert not np.array_equal(bits(g[f_px]), bits(k[f_px]))
        assert np.array_equal(length, cnt[ar.pixel_tiles(W, H)].astype(F))
        # per tile the restatement at a uniform count
        for t in np.flatnonzero(folded):
            sel = np.repeat(ar.pixel_tiles(W, H) == t, 4)
            n = F(cnt[t])
            assert np.array_equal(bits(new[sel]), bits(vr.mix(acc[sel], sample[sel], n)))
            assert np.array_equal(bits(new_mom[sel]), bits(vr.moments(acc[sel], new[sel], n, mom[sel])))


# ---- the CLI's refusals -----------------------------------------------------------------------------

def test_cli_refusals():
    exe = str(ROOT / "pathtracer.cl_amd" / "rt_render")
    base = [exe, "--width", "16", "--height", "8"]

    def refused(args, word):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)

    refused(["--mesh", "100", "--events", "d", "--converge", "--budget"], "--adaptive")
    refused(["--mesh", "100", "--events", "d", "--converge", "--budget", "4", "--budget-limits", "0.1,0.2,0.4"], "--adaptive")
    refused(["--mesh", "100", "--events", "d", "--budget", "--adaptive"], "--converge")
    refused(["--mesh", "100", "--events", "d", "--converge", "--adaptive", "--counts-out", "x"], "--budget")
    refused(["--mesh", "100", "--events", "d", "--converge", "--adaptive", "--budget-log", "x"], "--budget")
