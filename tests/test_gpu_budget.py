"""GPU: per-tile sample counts.  The fold against the triangle kernel's own progressive mix
and against tests/budget_ref.py, on real masked renders and on made-up frames; the budget rule and the pass
mask against numpy; and ProgressiveViewHIP::setSampleBudget through the rt_render CLI: at one pass the bytes
of the view without it, at four passes the restatement's over the oracle's frames, and the display at which
it converges.  Every comparison is word for word.  Run on the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

import ctypes
import json

import numpy as np
import pytest

import adaptive_ref as ar
import budget_ref as br
import features_ref as fr
import noise_ref as nr
import render_state as rs
import variance_ref as vref
import view_ref as vr
from conftest import ROOT, bits
from test_gpu_adaptive import ADAPTIVE, EVENTS, Masked, RULE, device, host, masks, scene, tile_maps  # noqa: F401 (scene: a fixture)

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
RENDER_SIZES = [(8, 8), (37, 29), (64, 48)]
FRAME_SIZES = [(1, 1), (7, 5), (8, 8), (9, 8), (37, 29), (64, 48)]
PLANE_SIZES = FRAME_SIZES + [(300, 200)]
ODD_COUNTS = [0, 1, 1 << 24, 0xFFFFFFFF, 2, 6, (1 << 24) + 1, 0xFFFFFFFE]


def counts_plane(n, seed):
    """Non-uniform counts with the odd ones in: 0, 1, 2^24 (where float32 stops counting), 2^32 - 1 (saturated)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 40, n).astype(U)
    k = min(n, len(ODD_COUNTS))
    c[rng.permutation(n)[:k]] = ODD_COUNTS[:k]
    return c


def garbage(n, seed):
    """Finite floats of every size and sign (no NaN: its payload is no part of the contract)."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0.0, 1.0, n) * np.exp(rng.normal(0.0, 6.0, n))).astype(F)


# ---- 1. the fold is the kernel's own mix ----------------------------------------------------------------

@pytest.mark.parametrize("sr", [1, 2])
@pytest.mark.parametrize("W,H", RENDER_SIZES)
def test_fold_equals_the_kernels_mix(scene, tracer, W, H, sr):
    """From one state: progression c + 1 rendered the ordinary way, and progression 0 rendered into a scratch
    frame and folded with every count = c — weights 1, 1/2, 1/3, 1/7.  The frame, both seed planes and the
    moments (against rt_moments_accumulate) are identical, the counts read c + 1."""
    import torch

    px, n_t = W * H, ar.n_tiles(W, H)
    m = Masked(scene, W, H, sr)
    try:
        m.render(0, None)  # a real frame to refine
        mom0 = np.random.default_rng(W).random(4 * px).astype(F)
        for c in (0, 1, 2, 6):
            frame0, seeds0 = m.exp.copy(), m.seeds.copy()
            m.render(c + 1, None)  # (checked against the oracle)
            want, want_seeds = m.exp.copy(), m.seeds.copy()
            want_mom = np.zeros(4 * px, F)
            tracer.momentsAccumulate(frame0, want, float(c + 1), mom0, want_mom, W, H)
            m.restore(frame0, seeds0)
            scratch = device(garbage(4 * px, c))
            m.t.rayTrace(scratch, W, H, 0, kernel=2)
            acc, count, mom = device(frame0), device(np.full(n_t, c, U)), device(mom0)
            length = torch.zeros(px, dtype=torch.float32, device="cuda:0")
            m.t.foldTiles(scratch, acc, count, None, 0, W, H, mom_in=mom, mom_out=mom, len_out=length)
            what = (W, H, sr, c)
            assert np.array_equal(bits(host(acc)), bits(want)), what
            assert np.array_equal(m.t.getSeeds(), want_seeds), what
            assert np.array_equal(bits(host(mom)), bits(want_mom)), what
            assert (host(count) == c + 1).all() and (host(length) == F(c + 1)).all(), what
            m.restore(want, want_seeds)
        assert m.t.lastBudgetMs("fold") > 0.0
    finally:
        m.close()


# ---- 2. masked passes --------------------------------------------------------------------------------

SEQUENCES = [("random", "checker", "all"), ("one", "edges", "none")]


@pytest.mark.parametrize("W,H", RENDER_SIZES)
def test_masked_passes_follow_the_restatement(scene, W, H):
    """Three passes under different planes, from non-uniform counts and a garbage accumulation buffer: after
    each, frame, counts, moments and lengths are the restatement's, where the sample frame is select(live,
    oracle(progression 0), stale) — Masked.render checks that frame and the seeds — and the tiles that are
    not folded are untouched, partial edge tiles included.  The last pass runs on a side stream behind a
    render enqueued without a wait."""
    import torch

    px, n_t = W * H, ar.n_tiles(W, H)
    mk = masks(W, H, seed=4)
    tile = ar.pixel_tiles(W, H)
    for s, names in enumerate(SEQUENCES):
        m = Masked(scene, W, H, 1)
        try:
            acc, count, mom = garbage(4 * px, 10 + s), counts_plane(n_t, W + s), np.random.default_rng(s).random(4 * px).astype(F)
            d_acc, d_count, d_mom = device(acc), device(count), device(mom)
            d_len = device(np.full(px, -1.0, F))
            side = torch.cuda.Stream()
            for r, name in enumerate(names):
                live = mk[name] == 0
                passes = np.where(live, U(r + 1 + (r % 2)), U(r if r % 2 else 0)).astype(U)  # folded: passes > r
                assert np.array_equal(br.pass_mask(None, passes, r) == 0, live)
                d_passes = device(passes)
                last = r == len(names) - 1
                if not last:
                    m.render(0, mk[name])
                    m.t.foldTiles(m.frame, d_acc, d_count, d_passes, r, W, H, mom_in=d_mom, mom_out=d_mom, len_out=d_len)
                else:  # enqueued without a wait, the fold behind it on another stream
                    m.plane.copy_(device(mk[name]))
                    torch.cuda.synchronize()
                    if not m.on:
                        m.t.setTileStop(m.plane, W, H)
                        m.on = True
                    m.t.rayTrace(m.frame, W, H, 0, kernel=2, sync=False)
                    m.t.foldTiles(m.frame, d_acc, d_count, d_passes, r, W, H, mom_in=d_mom, mom_out=d_mom, len_out=d_len,
                                  stream=side.cuda_stream, sync=False)
                    m.t.synchronize()
                    torch.cuda.synchronize()
                    full, seeds_full = m.exp.copy(), m.seeds.copy()
                    scene["render"](full, W, H, 1, 0, seeds_full)
                    m.exp, m.seeds = ar.masked(mk[name], W, H, m.Wp, m.Hp, m.exp, full, m.seeds, seeds_full)
                    assert np.array_equal(bits(host(m.frame)), bits(m.exp)) and np.array_equal(m.t.getSeeds(), m.seeds)
                new_acc, new_count, new_mom, new_len = br.fold(m.exp, acc, count, passes, r, W, H, mom)
                what = (W, H, names, r)
                assert np.array_equal(bits(host(d_acc)), bits(new_acc)), what
                assert np.array_equal(host(d_count), new_count) and np.array_equal(bits(host(d_mom)), bits(new_mom)), what
                assert np.array_equal(bits(host(d_len)), bits(new_len)), what
                kept = np.repeat(~live[tile], 4)  # (the restatement says so too; said here without it)
                assert np.array_equal(bits(host(d_acc))[kept], bits(acc)[kept]) and np.array_equal(host(d_count)[~live], count[~live])
                assert np.array_equal(bits(host(d_mom))[kept], bits(mom)[kept])
                acc, count, mom = new_acc, new_count, new_mom
        finally:
            m.close()


@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_fold_equals_numpy(tracer, W, H):
    """Made-up frames at every size, non-uniform counts: host arrays and device tensors; with a passes plane
    and without; the moments and the lengths given, omitted, and written to another buffer; the inputs are
    only read."""
    px, n_t = W * H, ar.n_tiles(W, H)
    rng = np.random.default_rng(W * 100 + H)
    for seed in (0, 1):
        sample, acc, mom = garbage(4 * px, seed), garbage(4 * px, seed + 5), rng.random(4 * px).astype(F)
        count = counts_plane(n_t, seed + W)
        planes = [None, rng.integers(0, 4, n_t).astype(U), np.zeros(n_t, U)]
        for passes in planes:
            for r in (0, 2):
                exp_acc, exp_count, exp_mom, exp_len = br.fold(sample, acc, count, passes, r, W, H, mom)
                folded = br.folded_tiles(n_t, passes, r)
                for dev in (False, True):
                    wrap = device if dev else (lambda a: a.copy())
                    back = host if dev else (lambda a: a)
                    for variant in ("in place", "other buffer", "no moments", "no lengths"):
                        a = dict(sample=wrap(sample), acc=wrap(acc), count=wrap(count), passes=None if passes is None else wrap(passes))
                        mi = None if variant == "no moments" else wrap(mom)
                        mo = mi if variant in ("in place", "no moments") else wrap(np.full(4 * px, 5.0, F))
                        ln = None if variant == "no lengths" else wrap(np.full(px, -1.0, F))
                        tracer.foldTiles(a["sample"], a["acc"], a["count"], a["passes"], r, W, H, mom_in=mi, mom_out=mo, len_out=ln)
                        what = (W, H, seed, passes is None, r, dev, variant)
                        assert np.array_equal(bits(back(a["acc"])), bits(exp_acc)), what
                        assert np.array_equal(back(a["count"]), exp_count), what
                        assert np.array_equal(bits(back(a["sample"])), bits(sample)), what
                        if passes is not None:
                            assert np.array_equal(back(a["passes"]), passes), what
                        if mo is not None:
                            assert np.array_equal(bits(back(mo)), bits(exp_mom)), what
                            if variant == "other buffer":
                                assert np.array_equal(bits(back(mi)), bits(mom)), what
                        if ln is not None:
                            assert np.array_equal(bits(back(ln)), bits(exp_len)), what
                assert passes is not None or folded.all()
    assert tracer.lastBudgetMs("fold") > 0.0
    with pytest.raises(ValueError):
        tracer.foldTiles(sample, device(acc), count, None, 0, W, H)  # host and device buffers mixed


# ---- 3. the budget rule and the pass mask ---------------------------------------------------------------

@pytest.mark.parametrize("W,H", PLANE_SIZES)
def test_budget_and_mask_equal_numpy(tracer, W, H):
    n = ar.n_tiles(W, H)
    rng = np.random.default_rng(W + 7 * H)
    for seed, prm in enumerate((dict(), dict(max_passes=1), dict(max_passes=2, limits=[0.05]), dict(max_passes=8, limits=[0.01, 0.02, 0.04, 0.08, 0.16, 0.32, np.inf]),
                                dict(max_passes=3, limits=[0.0, 3e38]))):
        tiles = tile_maps(W, H, seed)
        for stop in (None, ((rng.random(n) < 0.3) * rng.integers(1, 1 << 32, n)).astype(U)):
            full = {**br.DEFAULTS, **prm}
            exp, exp_st = br.budget(tiles, stop, **full)
            got = np.full(n, 0xDEADBEEF, U)
            st = tracer.tileBudget(tiles, stop, got, W, H, **prm)
            assert np.array_equal(got, exp) and st == exp_st, (prm, st, exp_st)
            d_tiles, d_stop, d_got = device(tiles), None if stop is None else device(stop), device(np.full(n + 1, 0xDEADBEEF, U))
            st = tracer.tileBudget(d_tiles, d_stop, d_got, W, H, **prm)
            back = host(d_got)
            assert np.array_equal(back[:n], exp) and back[n] == 0xDEADBEEF and st == exp_st
            assert np.array_equal(bits(host(d_tiles)), bits(tiles)) and (stop is None or np.array_equal(host(d_stop), stop))
            for r in range(full["max_passes"] + 1):
                exp_mask = br.pass_mask(stop, exp, r)
                mask = np.full(n, 7, U)
                tracer.tilePassMask(stop, exp, r, mask, W, H)
                d_mask = device(np.full(n + 1, 7, U))
                tracer.tilePassMask(d_stop, device(exp), r, d_mask, W, H)
                assert np.array_equal(mask, exp_mask) and np.array_equal(host(d_mask)[:n], exp_mask) and host(d_mask)[n] == 7
            assert (br.pass_mask(stop, exp, full["max_passes"]) == 1).all()
    assert tracer.lastBudgetMs("budget") > 0.0 and tracer.lastBudgetMs("mask") > 0.0


def test_budget_on_hand_made_maps(tracer):
    """The maps of tests/test_budget_host.py through the kernel: a mean on each limit and its float neighbours,
    NaN, +inf, -0, stop words; and a plane larger than one block with every pass count in it."""
    up, down = (lambda x: np.nextafter(F(x), F(np.inf))), (lambda x: np.nextafter(F(x), F(-np.inf)))
    lim = [F(0.1), F(0.2), F(0.4)]
    means = [lim[0], down(lim[0]), up(lim[0]), lim[1], down(lim[1]), up(lim[1]), lim[2], down(lim[2]), up(lim[2]), np.nan, np.inf, -0.0,
             0.0, -1.0, 1e30]
    W, H = 8 * len(means), 8
    tiles = np.zeros((len(means), 2), F)
    tiles[:, 0], tiles[:, 1] = means, np.nan
    stop = np.zeros(len(means), U)
    stop[[2, 8, 9]] = [7, 0xFFFFFFFF, 1]
    for sp in (None, stop, np.ones(len(means), U)):
        exp, exp_st = br.budget(tiles, sp, 4, lim)
        got = np.zeros(len(means), U)
        assert tracer.tileBudget(tiles, sp, got, W, H) == exp_st and np.array_equal(got, exp)
    assert br.budget(tiles, None, 4, lim)[0].tolist() == [1, 1, 2, 2, 2, 3, 3, 3, 4, 1, 4, 1, 1, 1, 4]
    W, H = 300, 200  # 950 tiles: four blocks, fifteen waves
    n = ar.n_tiles(W, H)
    lim8 = [0.1 * 2 ** k for k in range(7)]
    tiles = np.zeros((n, 2), F)
    tiles[:, 0] = 0.07 * 2.0 ** (np.arange(n) % 9)
    stop = (np.arange(n) % 11 == 0).astype(U)
    exp, exp_st = br.budget(tiles, stop, 8, lim8)
    got = device(np.zeros(n, U))
    st = tracer.tileBudget(device(tiles), device(stop), got, W, H, max_passes=8, limits=lim8)
    assert st == exp_st and np.array_equal(host(got), exp) and all(exp_st["by_passes"]) and exp_st["rounds"] == 8
    assert sum(exp_st["by_passes"]) == n and exp_st["tile_passes"] == sum(i * c for i, c in enumerate(exp_st["by_passes"]))


def test_argument_checks(pt):
    """Every RT_ERR_ARG, on a context that has run none of the stages (their times are RT_ERR_STATE)."""
    ab = pt._abi
    t = pt.RayTracer(0)
    try:
        lib, p, h = t._lib, ab.ptr, t._h
        W, H = 20, 9  # 3 x 2 tiles
        n, px = ar.n_tiles(W, H), W * H
        tiles, stop, passes, stats = np.full(2 * n, 0.3, F), np.zeros(n, U), np.zeros(n, U), np.zeros(13, U)
        nan = float("nan")
        ms = ctypes.c_float()
        for slot in range(3):
            a = [None] * 3
            a[slot] = ctypes.byref(ms)
            assert lib.rt_last_budget_ms(h, *a) == ab.RT_ERR_STATE
        assert lib.rt_last_budget_ms(h, None, None, None) == ab.RT_ERR_ARG

        def budget(tl_=tiles, sp_=stop, ps_=passes, st_=stats, w_=W, h_=H, mp=4, lim=(0.1, 0.2, 0.4), prm=True, flags=0):
            pr = ab.RtBudgetParams()
            pr.max_passes = mp
            for k, v in enumerate(lim):
                pr.limits[k] = v
            return lib.rt_tile_budget(h, p(tl_), p(sp_), p(ps_), p(st_), w_, h_, ctypes.byref(pr) if prm else None, flags)

        for kw in (dict(mp=0), dict(mp=9), dict(lim=(0.4, 0.2, 0.1)), dict(lim=(0.1, 0.1, 0.4)), dict(lim=(0.1, nan, 0.4)),
                   dict(lim=(nan, 0.2, 0.4)), dict(lim=(-0.1, 0.2, 0.4)), dict(mp=8, lim=(0.1, 0.2, 0.4, 0.8, 1.6, 3.2, 3.0)),
                   dict(tl_=None), dict(ps_=None), dict(st_=None), dict(prm=False), dict(w_=0), dict(h_=0),
                   dict(w_=1 << 14, h_=1 << 14), dict(flags=2), dict(ps_=stop), dict(ps_=tiles.view(U)[2:]), dict(st_=passes),
                   dict(st_=tiles.view(U)), dict(st_=stop)):
            assert budget(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
            assert lib.rt_last_error(h)
        assert not passes.any() and not stats.any()
        # the limits past max_passes - 1 are not read; a null stop plane is none
        assert budget(mp=2, lim=(0.1, nan, -1.0)) == ab.RT_OK and budget(mp=1, lim=(nan,)) == ab.RT_OK and budget(sp_=None) == ab.RT_OK
        passes[:] = 0
        stats[:] = 0

        sample, acc, mom, mom2, ln = [np.zeros(4 * px, F) for _ in range(4)] + [np.zeros(px, F)]
        count = np.zeros(n, U)

        def fold(sm_=sample, ac_=acc, ct_=count, ps_=passes, mi_=mom, mo_=mom, ln_=ln, w_=W, h_=H, flags=0):
            return lib.rt_fold_tiles(h, p(sm_), p(ac_), p(ct_), p(ps_), 0, p(mi_), p(mo_), p(ln_), w_, h_, flags)

        for kw in (dict(sm_=None), dict(ac_=None), dict(ct_=None), dict(mi_=None), dict(mo_=None), dict(w_=0), dict(h_=0),
                   dict(w_=1 << 14, h_=1 << 14), dict(flags=2), dict(ac_=sample), dict(ac_=sample[4:]), dict(mo_=acc),
                   dict(mi_=sample), dict(mo_=mom[4:]), dict(mi_=mom2[8:], mo_=mom2), dict(ln_=acc[3:]), dict(ln_=mom),
                   dict(ln_=count.view(F)), dict(ps_=count), dict(ct_=acc.view(U)), dict(ps_=sample.view(U)[1:]),
                   dict(ct_=ln.view(U)[5:])):
            assert fold(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
            assert lib.rt_last_error(h)
        assert not acc.any() and not count.any() and not ln.any()
        assert fold() == ab.RT_OK and fold(ps_=None, mi_=None, mo_=None, ln_=None) == ab.RT_OK and fold(mo_=mom2) == ab.RT_OK

        mask = np.zeros(n, U)

        def pass_mask(sp_=stop, ps_=passes, mk_=mask, w_=W, h_=H, flags=0):
            return lib.rt_tile_pass_mask(h, p(sp_), p(ps_), 0, p(mk_), w_, h_, flags)

        for kw in (dict(ps_=None), dict(mk_=None), dict(w_=0), dict(h_=0), dict(flags=2), dict(mk_=stop), dict(mk_=passes),
                   dict(mk_=tiles.view(U)[:n], ps_=tiles.view(U)[n - 1:2 * n - 1])):
            assert pass_mask(**kw) == ab.RT_ERR_ARG, {k: type(v) for k, v in kw.items()}
        assert pass_mask() == ab.RT_OK and pass_mask(sp_=None) == ab.RT_OK
    finally:
        t.close()


def test_render_state_untouched(pt, golden, golden_meta):
    """The golden progressive frames with the fold, the budget rule and the pass mask in between — device
    tensors on a side stream behind a render enqueued without a wait, host buffers on the context's stream
    — are the frames, seeds, counter totals, render info and rt_read of the sequence without them.  The fold
    writes an accumulation buffer, but never the render's."""
    import torch

    with rs.untouched(pt, golden, golden_meta) as (t, frame_dev, g, m):
        W, H = m["W"], m["H"]
        n, px = ar.n_tiles(W, H), W * H
        tiles = tile_maps(W, H, 4)
        tiles[:, 0] *= F(3.0)  # (around the default limits)
        sample, acc, mom = garbage(4 * px, 1), garbage(4 * px, 2), np.random.default_rng(3).random(4 * px).astype(F)
        count, stop = counts_plane(n, 9), (np.arange(n) % 5 == 0).astype(U) * U(3)
        exp_passes, exp_st = br.budget(tiles, stop, **br.DEFAULTS)
        exp_mask = br.pass_mask(stop, exp_passes, 1)
        exp_fold = br.fold(sample, acc, count, exp_passes, 1, W, H, mom)
        d_tiles, d_stop, d_sample, d_ref_passes = (device(a) for a in (tiles, stop, sample, exp_passes))
        per = range(m["frames"])
        d_acc, d_count, d_mom = ([device(a) for _ in per] for a in (acc, count, mom))
        d_len = [torch.zeros(px, dtype=torch.float32, device="cuda:0") for _ in per]
        d_passes, d_mask = ([torch.zeros(n, dtype=torch.int32, device="cuda:0") for _ in per] for _ in range(2))
        d_stats = [torch.zeros(13, dtype=torch.int32, device="cuda:0") for _ in per]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        on_host = None
        for p in per:
            t.rayTrace(frame_dev, W, H, p, kernel=2, sync=False)
            kw = dict(stream=side.cuda_stream, sync=False)
            assert t.tileBudget(d_tiles, d_stop, d_passes[p], W, H, stats=d_stats[p], **kw) is None
            t.tilePassMask(d_stop, d_ref_passes, 1, d_mask[p], W, H, **kw)
            t.foldTiles(d_sample, d_acc[p], d_count[p], d_ref_passes, 1, W, H, mom_in=d_mom[p], mom_out=d_mom[p], len_out=d_len[p], **kw)
            if p == 1:  # and host buffers on the context's own stream
                h_passes, h_mask = np.zeros(n, U), np.zeros(n, U)
                h_acc, h_count, h_mom, h_len = acc.copy(), count.copy(), mom.copy(), np.zeros(px, F)
                st = t.tileBudget(tiles, stop, h_passes, W, H)
                t.tilePassMask(stop, exp_passes, 1, h_mask, W, H)
                t.foldTiles(sample, h_acc, h_count, exp_passes, 1, W, H, mom_in=h_mom, mom_out=h_mom, len_out=h_len)
                on_host = (st, h_passes, h_mask, (h_acc, h_count, h_mom, h_len))
    for p in per:
        w = host(d_stats[p])
        assert dict(tiles=int(w[0]), rounds=int(w[1]), tile_passes=int(w[2]), by_passes=[int(v) for v in w[4:13]]) == exp_st
        assert w[3] == 0 and np.array_equal(host(d_passes[p]), exp_passes) and np.array_equal(host(d_mask[p]), exp_mask)
        for got, exp in zip((d_acc[p], d_count[p], d_mom[p], d_len[p]), exp_fold):
            assert np.array_equal(bits(host(got)), bits(exp))
    assert on_host[0] == exp_st and np.array_equal(on_host[1], exp_passes) and np.array_equal(on_host[2], exp_mask)
    for got, exp in zip(on_host[3], exp_fold):
        assert np.array_equal(bits(got), bits(exp))
    assert exp_st["rounds"] >= 3 and 0 < (exp_mask == 0).sum() < n


# ---- ProgressiveViewHIP::setSampleBudget through rt_render --events --------------------------------------

VW, VH = 64, 48
PX = VW * VH
TILES = ar.n_tiles(VW, VH)
MIN_FRAMES = 4
N_DISPLAYS = EVENTS.count("d")
FIRST = EVENTS.split(",").index("l")  # the displays before the key


def converge_args(threshold):
    return ["--converge", str(threshold), "--converge-min-frames", str(MIN_FRAMES)]


def run_cli(tmp, args, outputs=("shown", "raw", "feat"), budget=False):
    """vr.run_view with the meter's log and tile map, the stop planes and (budget) the count planes and the
    budget log beside its own files."""
    files = {k: tmp / k for k in ("noise_map.f32", "stop_map.u32", "noise.log", "counts.u32", "budget.log")}
    for f in files.values():
        f.unlink(missing_ok=True)
    extra = ["--noise-map-out", str(files["noise_map.f32"]), "--stop-map-out", str(files["stop_map.u32"]), "--noise-log",
             str(files["noise.log"])]
    if budget:
        extra += ["--counts-out", str(files["counts.u32"]), "--budget-log", str(files["budget.log"])]
    r = vr.run_view(tmp, args + extra, outputs, VW, VH)
    r["map"], r["stops"] = np.fromfile(files["noise_map.f32"], F), np.fromfile(files["stop_map.u32"], U)
    r["noise"] = files["noise.log"].read_text().splitlines()
    if budget:
        r["counts"] = np.fromfile(files["counts.u32"], U)
        r["budget"] = [[int(v) for v in l.split()] for l in files["budget.log"].read_text().splitlines()]
    return r


BASE = ["--mesh", "2000", "--events", EVENTS] + converge_args(0.001) + ADAPTIVE  # (the frame-wide rule never fires here)


@pytest.fixture(scope="module")
def view_runs(tmp_path_factory):
    """test_gpu_adaptive's view — thirteen displays, a key, six more — alone, with --budget 1 and with --budget 4."""
    tmp = tmp_path_factory.mktemp("budget_view")
    return dict(plain=run_cli(tmp, BASE), one=run_cli(tmp, BASE + ["--budget", "1"], budget=True),
                four=run_cli(tmp, BASE + ["--budget", "4"], budget=True))


def progressions():
    """The progression of every display of EVENTS: 0, 1, ... and after the key 1, 2, ..."""
    return list(range(FIRST)) + list(range(1, N_DISPLAYS - FIRST + 1))


def test_view_at_one_pass_is_todays_view(view_runs):
    """With --budget 1 every display's shown, raw and feature frames, stop plane, tile map and noise-log line
    are the bytes of the run without --budget, through another path: a masked render at progression 0 into a
    scratch frame, and the fold.  The count planes read the frame each tile stopped at, else the progression
    (0 at a fresh view's first display, which is rendered straight into the accumulation buffer)."""
    plain, one = view_runs["plain"], view_runs["one"]
    for name in ("shown", "raw", "feat", "stops", "map"):
        assert plain[name].size and np.array_equal(bits(plain[name]), bits(one[name])), name
    assert plain["noise"] == one["noise"] and len(one["noise"]) == N_DISPLAYS
    assert plain["raw"].size == 4 * PX * N_DISPLAYS and np.array_equal(bits(one["shown"]), bits(one["raw"]))
    lines, ref = one["lines"][:-1], plain["lines"][:-1]
    assert all("rounds" in l and "tile_passes" in l for l in lines) and all("rounds" not in l for l in ref)
    assert [{k: v for k, v in l.items() if k not in ("rounds", "tile_passes")} for l in lines] == ref
    assert one["counts"].size == TILES * N_DISPLAYS and len(one["budget"]) == N_DISPLAYS
    for k, progression in enumerate(progressions()):
        stop = one["stops"][TILES * k:TILES * (k + 1)]
        assert np.array_equal(one["counts"][TILES * k:TILES * (k + 1)], np.where(stop != 0, stop, U(progression))), k
        live = int((stop == 0).sum())
        want = [0] * 11 if progression == 0 else [1 if live else 0, live, TILES - live, live] + [0] * 7
        assert one["budget"][k] == want, (k, one["budget"][k])
    assert (one["stops"] != 0).any()  # tiles did stop: the lengths and moments of frozen tiles were in play


def golden_views(pt, oracle, golden, golden_meta):
    """The oracle's in-place render of the CLI's view before and after the key (azimuth 105 and 108), with
    rt_variance's restatement on given features."""
    from oracle import MeshBVH

    g, m = golden("tris_64x48_sr1"), golden_meta["cases"]["tris_64x48_sr1"]
    sc = pt.scenes
    Wp, Hp = sc.padded_dims(VW, VH)
    spheres = g["spheres"].view(pt._abi.SPHERE_DTYPE)
    bvh = MeshBVH(oracle, g["verts"], g["idx"])

    def render_at(azimuth):
        cam = sc.camera_spherical(VW, **{**sc.PLY_CAMERA, "azimuth": azimuth})

        def render(acc, progression, seeds):
            oracle.render_tris(acc, cam, spheres, VW, VH, Wp, Hp, 1, m["max_depth"], progression, seeds, g["verts"], g["idx"], bvh=bvh)

        return render

    def variance_with(feat):
        return lambda shown, mom, length: vref.variance(oracle, shown, mom, length, feat, VW, VH)

    return dict(Wp=Wp, Hp=Hp, seeds=sc.default_seeds(Wp, Hp), render_at=render_at, variance_with=variance_with, g=g)


def restated(views, run, threshold, budget_prm, events=EVENTS):
    """The displays of `run` restated on the CPU (tests/budget_ref.py's refine over the oracle's frames, with
    the run's own feature frames for the variance): a fresh view, then after the key a restart."""
    first = events.split(",").index("l") if "l" in events else events.count("d")
    meter = lambda shown, var: nr.meter(shown, var, VW, VH, threshold=threshold)  # noqa: E731
    feat = run["feat"][:8 * PX]
    seq = br.refine(views["render_at"](105.0), views["variance_with"](feat), meter, VW, VH, views["Wp"], views["Hp"], views["seeds"],
                    first, threshold, MIN_FRAMES, RULE, budget_prm)
    if len(seq) == first and events.count("d") > first and not seq[-1]["converged"]:
        feat = run["feat"][8 * PX * first:8 * PX * (first + 1)]
        seq += br.refine(views["render_at"](108.0), views["variance_with"](feat), meter, VW, VH, views["Wp"], views["Hp"],
                         seq[-1]["seeds"], events.count("d") - first, threshold, MIN_FRAMES, RULE, budget_prm, first=1,
                         acc=seq[-1]["acc"], mom=seq[-1]["mom"])
    return seq


def check_against(run, seq, budget):
    for k, d in enumerate(seq):
        assert np.array_equal(bits(run["raw"][4 * PX * k:4 * PX * (k + 1)]), bits(d["acc"])), k
        assert np.array_equal(run["stops"][TILES * k:TILES * (k + 1)], d["stop"]), k
        assert np.array_equal(bits(run["map"][2 * TILES * k:2 * TILES * (k + 1)]), bits(d["tiles"])), k
        s = d["stats"]
        level = int(np.array([s["level"]], F).view(U)[0])
        assert run["noise"][k] == "%08x %u %u %u %d" % (level, s["counted"], s["skipped"], s["below"], int(d["converged"])), k
        if budget:
            assert np.array_equal(run["counts"][TILES * k:TILES * (k + 1)], d["count"]), k
            assert run["budget"][k] == [d["rounds"], d["tile_passes"]] + d["by_passes"], k
            line = run["lines"][k if k < FIRST else k + 1]
            assert line["rounds"] == d["rounds"] and line["tile_passes"] == d["tile_passes"] and line["tiles_active"] == d["active"]


def test_view_at_four_passes_follows_the_restatement(view_runs, pt, oracle, golden, golden_meta):
    """--budget 4 at the default limits: every display's raw frame, counts, stop plane, tile map, budget-log
    and noise-log line are the restatement's over the oracle's frames, before and after the key; at least
    three different pass counts occur at one display, and some tile has been traced more often than the
    view has displayed."""
    run = view_runs["four"]
    views = golden_views(pt, oracle, golden, golden_meta)
    g = views["g"]
    rays = np.zeros(PX, pt._abi.RAY_DTYPE)
    cam = pt.scenes.camera_spherical(VW, **pt.scenes.PLY_CAMERA)
    assert pt.load_library().rt_primary_rays(pt._abi.ptr(cam), VW, VH, pt._abi.ptr(rays)) == pt._abi.RT_OK
    assert np.array_equal(bits(run["feat"][:8 * PX]), bits(fr.features_tris(oracle, rays, g["verts"], g["idx"]).reshape(-1)))
    seq = restated(views, run, 0.001, dict(br.DEFAULTS))
    assert len(seq) == N_DISPLAYS == len(run["budget"]) and run["raw"].size == 4 * PX * N_DISPLAYS
    check_against(run, seq, budget=True)
    assert np.array_equal(bits(run["shown"]), bits(run["raw"]))
    assert max(sum(1 for c in d["by_passes"][1:] if c) for d in seq) >= 3
    assert max(int(d["count"].max()) for d in seq[:FIRST]) > FIRST - 1
    assert seq[FIRST]["count"].max() == 1 and seq[FIRST]["rounds"] >= 1  # the key zeroed the counts: one pass, weight 1
    print("rounds per display:", [d["rounds"] for d in seq], "passes:", [d["by_passes"][:5] for d in seq])


def test_flag_absent_changes_nothing(view_runs, tmp_path, pt, oracle, golden, golden_meta):
    """Without --budget: two runs are byte-equal, no line names the budget, and the shown and raw frames, the
    stop planes, the tile maps and the noise log are what the view did before there was a budget — the
    restatement of that path (adaptive_ref's masked render and moments) over the oracle's frames."""
    a = view_runs["plain"]
    b = run_cli(tmp_path, BASE)
    for name in ("shown", "raw", "feat", "stops", "map"):
        assert a[name].size and np.array_equal(bits(a[name]), bits(b[name])), name
    assert a["lines"] == b["lines"] and a["noise"] == b["noise"]
    assert all("rounds" not in l and "tile_passes" not in l for l in a["lines"])
    seq = restated(golden_views(pt, oracle, golden, golden_meta), a, 0.001, None)
    assert len(seq) == N_DISPLAYS
    check_against(a, seq, budget=False)
    assert np.array_equal(bits(a["shown"]), bits(a["raw"]))


def test_budget_converges_sooner(tmp_path, pt, oracle, golden, golden_meta):
    """It does what it is for.  profiles/budget/converge_table.py found on the CPU, at --converge 0.32, the
    display at which this view converges without and with --budget 4 (default limits); the device reproduces
    the restatement's bits, so both counts are exact, and the budgeted one is the smaller."""
    table = json.loads((ROOT / "profiles" / "budget" / "converge_table.json").read_text())
    assert table["converge_min_frames"] == MIN_FRAMES and table["adaptive"] == RULE and table["budget"] == \
        dict(max_passes=br.DEFAULTS["max_passes"], limits=list(br.DEFAULTS["limits"]))
    threshold = table["converge"]
    events = ",".join(["d"] * 40)
    base = ["--mesh", "2000", "--events", events] + converge_args(threshold) + ADAPTIVE
    at = {}
    for name, extra in (("plain", []), ("budgeted", ["--budget", "4"])):
        r = run_cli(tmp_path, base + extra, outputs=("raw",), budget=bool(extra))
        lines = r["lines"][:-1]
        traced = [l for l in lines if l["rendered"]]
        at[name] = len(traced)
        print(name, "converged at display", at[name])
        assert traced[-1]["converged"] is True and not any(l["converged"] for l in traced[:-1])
        assert all(l["converged"] and not l["rendered"] for l in lines[len(traced):]) and len(lines) == 40
        assert at[name] == table[name]["converged_at"], (name, at[name])
    assert at["budgeted"] < at["plain"]
