"""float32 numpy restatement of the per-tile sample counts: the fold of a frame's own
sample into the accumulation buffer with a weight per 8x8 tile, the budget rule on the noise meter's tile
map, the mask of one pass, and the pass loop of a display.  The mix and the moments are
tests/variance_ref.py's, the tiles tests/adaptive_ref.py's; the rules are comparisons and integers.  Shared
by tests/test_budget_host.py and tests/test_gpu_budget.py."""
from __future__ import annotations

import numpy as np

import adaptive_ref as ar
import variance_ref as vr

F = np.float32
U = np.uint32
MAX_PASSES = 8
DEFAULTS = dict(max_passes=4, limits=(0.1, 0.2, 0.4))
SATURATED = U(0xFFFFFFFF)


def folded_tiles(n_tiles: int, passes, pass_: int) -> np.ndarray:
    """Per tile: whether pass `pass_` folds it (passes None: every tile)."""
    if passes is None:
        return np.ones(n_tiles, bool)
    return np.asarray(passes, U).reshape(-1) > U(pass_)


def fold(sample, acc, count, passes, pass_: int, W: int, H: int, mom_in=None, mom_out=None):
    """rt_fold_tiles: (acc, count, moments or None, lengths).  A folded tile: p = count + 1 saturating,
    n = float32(p), acc = mix(acc, sample, n), the moments rt_moments_accumulate's with prev = old, cur =
    new, n_cur = n; others keep acc, count and `mom_in`, and their length is float32(count)."""
    count = np.asarray(count, U).reshape(-1)
    fold_t = folded_tiles(count.size, passes, pass_)
    new_count = np.where(fold_t & (count != SATURATED), count + U(1), count).astype(U)
    tile = ar.pixel_tiles(W, H)
    fold_p = fold_t[tile]
    n_px = new_count[tile].astype(F)  # (round to nearest even, as the device's conversion)
    old = np.asarray(acc, F).reshape(-1, 4)
    s = np.asarray(sample, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        w = (F(1.0) / n_px).astype(F)
        mixed = (old + (s - old) * w[:, None]).astype(F)
    new = np.where(fold_p[:, None], mixed, old).astype(F)
    mom = None
    if mom_in is not None:
        mom = np.asarray(mom_in, F).reshape(-1, 4).copy()
        for n in np.unique(n_px[fold_p]):  # one call of the moments' restatement per weight that occurs
            sel = fold_p & (n_px == n)
            mom[sel] = vr.moments(old[sel].reshape(-1), new[sel].reshape(-1), n, mom[sel].reshape(-1)).reshape(-1, 4)
        mom = mom.reshape(-1)
    return new.reshape(-1), new_count, mom, n_px


def budget(tiles, stop, max_passes=4, limits=(0.1, 0.2, 0.4)):
    """rt_tile_budget: (passes, stats).  0 where stop != 0, else 1 + #{k < max_passes - 1: mean > limits[k]}."""
    mean = np.asarray(tiles, F).reshape(-1, 2)[:, 0]
    passes = np.ones(mean.size, U)
    with np.errstate(all="ignore"):
        for k in range(int(max_passes) - 1):
            passes += (mean > F(limits[k])).astype(U)
    if stop is not None:
        passes[np.asarray(stop, U).reshape(-1) != 0] = 0
    by = [int((passes == i).sum()) for i in range(MAX_PASSES + 1)]
    stats = dict(tiles=int(mean.size), rounds=int(passes.max()), tile_passes=int(passes.astype(np.int64).sum()), by_passes=by)
    return passes, stats


def pass_mask(stop, passes, pass_: int) -> np.ndarray:
    """rt_tile_pass_mask: 0 (rendered) where the tile is not stopped and passes > pass_, else 1."""
    passes = np.asarray(passes, U).reshape(-1)
    live = passes > U(pass_)
    if stop is not None:
        live &= np.asarray(stop, U).reshape(-1) == 0
    return np.where(live, U(0), U(1)).astype(U)


def refine(render, variance, meter, W: int, H: int, Wpad: int, Hpad: int, seeds, displays: int, threshold, min_frames: int, rule: dict,
           budget_prm: dict | None = None, first: int = 0, acc=None, mom=None):
    """ProgressiveViewHIP with setConverge(threshold, min_frames), setAdaptive(rule) and, with `budget_prm`,
    setSampleBudget, display by display from where the frame count starts afresh — a fresh view (first = 0),
    or the first display after a restart (first = 1, with the accumulation buffer `acc` and the moments `mom`
    the view holds) — until it is converged or `displays` are shown.  `render(frame, progression, seeds)` is
    the unmasked render in place, `variance(shown, moments, lengths)` rt_variance with the view's features,
    `meter(shown, var)` rt_noise_meter as (stats, histogram, tiles).  Returns one dict per display: n, level,
    active, converged, rounds, tile_passes, traced (the tiles this display traced, passes counted), and the
    state after it (acc, seeds, mom, count, stop, passes, tiles)."""
    n_t = ar.n_tiles(W, H)
    acc = np.zeros(4 * W * H, F) if acc is None else np.asarray(acc, F).copy()
    seeds = np.asarray(seeds, U).copy()
    stop, count, passes, rounds = np.zeros(n_t, U), np.zeros(n_t, U), np.ones(n_t, U), 1
    out = []
    for k in range(first, first + displays):
        n = max(k, 1)
        if budget_prm is not None and k > 0:
            traced = int(sum((pass_mask(stop, passes, r) == 0).sum() for r in range(rounds)))
            acc, seeds, count, mom, length = display(render, acc, seeds, count, stop, passes, rounds, mom, W, H, Wpad, Hpad)
        else:  # today's path: one masked render with the launch's weight, then the masked moments
            traced = int((stop == 0).sum())
            prev, seeds_prev, full = acc.copy(), seeds.copy(), acc.copy()
            render(full, k, seeds)
            acc, seeds = ar.masked(stop, W, H, Wpad, Hpad, prev, full, seeds_prev, seeds)
            mom, length = ar.moments_tiles(prev, acc, n, mom, stop, W, H)
        stats, _, tiles = meter(acc, variance(acc, mom, length))
        active = int((stop == 0).sum())
        if n >= min_frames:
            stop, st = ar.select(tiles, stop, n, W, H, **rule)
            active = st["active"]
        bst = dict(rounds=0, tile_passes=0, by_passes=[0] * (MAX_PASSES + 1))
        if budget_prm is not None and (k > 0 or n >= min_frames):  # (after every fold, and after a stop rule at display 0)
            passes, bst = budget(tiles, stop, **budget_prm)
            rounds = bst["rounds"]
        converged = (n >= min_frames and int(stats["counted"]) > 0 and F(stats["level"]) <= F(threshold)) or active == 0
        out.append(dict(n=n, level=float(stats["level"]), stats=stats, active=active, converged=bool(converged), traced=traced,
                        rounds=bst["rounds"], tile_passes=bst["tile_passes"], by_passes=bst["by_passes"], acc=acc.copy(),
                        seeds=seeds.copy(), mom=mom.copy(), count=count.copy(), stop=stop.copy(), passes=passes.copy(), tiles=np.asarray(tiles, F).copy()))
        if converged:
            break
    return out


def display(render, acc, seeds, count, stop, passes, rounds: int, mom, W: int, H: int, Wpad: int, Hpad: int):
    """The pass loop of one display after the first: for r < rounds the mask of pass r, a masked render at
    progression 0 into a scratch frame, the fold of pass r.  `render(frame, progression, seeds)` is the
    unmasked render in place.  Returns (acc, seeds, count, moments, lengths)."""
    scratch = np.zeros(4 * W * H, F)
    length = np.asarray(count, U)[ar.pixel_tiles(W, H)].astype(F)  # (no round: what the last display left)
    for r in range(rounds):
        mask = pass_mask(stop, passes, r)
        full, seeds_full = scratch.copy(), seeds.copy()
        render(full, 0, seeds_full)
        scratch, seeds = ar.masked(mask, W, H, Wpad, Hpad, scratch, full, seeds, seeds_full)
        acc, count, mom, length = fold(scratch, acc, count, passes, r, W, H, mom)  # (a stopped tile's passes are 0)
    return acc, seeds, count, mom, length
