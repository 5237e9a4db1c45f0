"""float32 numpy restatement of adaptive sampling under the temporal stage: the temporal
merge and the trust test on per-pixel frame counts, every tile's shortest history length, the stop rule gated
by it, and ProgressiveViewHIP's chain with setAdaptiveHistory in effect.  The arithmetic is that of
tests/temporal_ref.py, tests/trust_ref.py and tests/adaptive_ref.py, whose functions take a plane where they
took a scalar; the chain's other stages are tests/budget_ref.py's, tests/variance_ref.py's and
tests/noise_ref.py's.  Shared by tests/test_adaptive_history_host.py and tests/test_gpu_adaptive_history.py."""
from __future__ import annotations

import numpy as np

import adaptive_ref as ar
import budget_ref as br
import features_ref as fr
import temporal_ref as tref
import trust_ref as tr

F = np.float32
U = np.uint32


def frames(cur_len) -> np.ndarray:
    """The accumulation buffer's frame count per pixel: cur_len where it is at least 1, else 1 (a NaN too)."""
    v = np.asarray(cur_len, F).reshape(-1)
    with np.errstate(all="ignore"):
        return np.where(v >= F(1.0), v, F(1.0)).astype(F)


def merge_len(hist_rgba, hist_len, cur_rgba, cur_len, max_history=32.0):
    """rt_temporal_merge_len: (out_rgba, out_len)."""
    return tref.merge(hist_rgba, hist_len, cur_rgba, frames(cur_len), max_history)


def trust_len(orc, hist_rgba, hist_len, cur_rgba, cur_len, feat, W, H, tolerance=1.5, sigma_normal=0.3, sigma_plane=0.1):
    """rt_history_trust_len: the plane of trusted lengths, every pixel's test with its own frame count."""
    return tr.trust(orc, hist_rgba, hist_len, cur_rgba, frames(cur_len).reshape(H, W), feat, W, H, tolerance, sigma_normal,
                    sigma_plane)


def tile_len_min(length, feat, W: int, H: int) -> np.ndarray:
    """rt_tile_len_min: per 8x8 tile the minimum of max(len, 0) (a NaN: 0) over its pixels inside the frame that
    met a surface (feat None: over all of them); +inf where none counts."""
    v = np.asarray(length, F).reshape(-1)
    with np.errstate(all="ignore"):
        v = np.where(v > F(0.0), v, F(0.0)).astype(F)
    counts = np.ones(W * H, bool)
    if feat is not None:
        counts = fr.feature_ids(np.asarray(feat, F)).reshape(-1) != fr.RT_FEAT_NONE
    out = np.full(ar.n_tiles(W, H), np.inf, F)
    np.minimum.at(out, ar.pixel_tiles(W, H)[counts], v[counts])
    return out


def select_frames(tiles, tile_frames, stop, n_frames: int, W: int, H: int, threshold=0.05, max_ratio=4.0, min_frames=16, dilate=1):
    """rt_tile_stop_select_frames: adaptive_ref.select with its frame gate open and the tiles whose own frames
    do not reach min_frames under no threshold (a NaN of the map is under none)."""
    t = np.asarray(tiles, F).reshape(-1, 2).copy()
    with np.errstate(all="ignore"):
        passes = np.asarray(tile_frames, F).reshape(-1) >= F(min_frames)
    t[~passes] = np.nan
    return ar.select(t, stop, n_frames, W, H, threshold, max_ratio, 0, dilate)


def golden_view(pt, oracle, golden, golden_meta, events: str, threshold, converge_min_frames: int, rule: dict, feats=None, **kw):
    """`view` over the oracle's frames of the golden triangle view at 64 x 48 that `rt_render --mesh 2000` shows
    (tests/test_gpu_budget.py's golden_views), before and after a key.  feats: the run's own --features-out
    file; None: the restatement's features of both cameras (tests/features_ref.py)."""
    import noise_ref as nr
    from test_gpu_budget import VH, VW, golden_views

    views = golden_views(pt, oracle, golden, golden_meta)
    sc, g, px = pt.scenes, views["g"], VW * VH
    camera_at = lambda az: sc.camera_spherical(VW, **{**sc.PLY_CAMERA, "azimuth": az})  # noqa: E731
    first = events.split(",").index("l") if "l" in events else 0

    def feat_at(az):
        if feats is not None:  # the first display's, or the first one's after the key
            k = 0 if az == 105.0 else first
            return np.ascontiguousarray(feats[8 * px * k:8 * px * (k + 1)])
        rays = np.zeros(px, pt._abi.RAY_DTYPE)
        assert pt.load_library().rt_primary_rays(pt._abi.ptr(camera_at(az)), VW, VH, pt._abi.ptr(rays)) == pt._abi.RT_OK
        return fr.features_tris(oracle, rays, g["verts"], g["idx"]).reshape(-1)

    meter = lambda shown, var: nr.meter(shown, var, VW, VH, threshold=threshold)  # noqa: E731
    return view(oracle, views["render_at"], views["variance_with"], meter, camera_at, feat_at, VW, VH, views["Wp"], views["Hp"],
                views["seeds"], events, threshold, converge_min_frames, rule, **kw)


class _History:
    def __init__(self, px):
        self.kept, self.kept_len = np.zeros(4 * px, F), np.zeros(px, F)
        self.carried, self.carried_len = np.zeros(4 * px, F), np.zeros(px, F)


def view(orc, render_at, variance_with, meter, camera_at, feat_at, W: int, H: int, Wpad: int, Hpad: int, seeds, events: str,
         threshold, converge_min_frames: int, rule: dict, max_history=32.0, budget_prm: dict | None = None, tolerance=None):
    """ProgressiveViewHIP (include/ProgressiveViewHIP.hpp) with setTemporal(max_history), setConverge(threshold,
    converge_min_frames), setAdaptive(rule), setAdaptiveHistory and, with `budget_prm`, setSampleBudget, with
    `tolerance` setHistoryTrust, over an event list of d and l (KEY_LEFT: the azimuth grows by 3), event by event.
    `render_at(azimuth)(frame, progression, seeds)` is the unmasked render in place, `variance_with(feat)(shown,
    moments, lengths)` rt_variance, `meter(shown, var)` rt_noise_meter as (stats, histogram, tiles),
    `camera_at(azimuth)` the view's Camera and `feat_at(azimuth)` its features.  Returns one dict per traced
    display: what it showed (shown, length), the accumulation state after it (acc, own: its per-pixel counts,
    stop, count), the meter's (stats, tiles), the rule's (tile_frames, active, stopped_now), the budget's (rounds,
    tile_passes, by_passes), converged, and n."""
    px, n_t = W * H, ar.n_tiles(W, H)
    acc, seeds = np.zeros(4 * px, F), np.asarray(seeds, U).copy()
    mom = None
    stop, count, passes, rounds = np.zeros(n_t, U), np.zeros(n_t, U), np.ones(n_t, U), 1
    colour, moments = _History(px), _History(px)
    az = 105.0
    realloc, progression, converged = True, 0, False
    feat_dirty, carry, have_hist, stop_reset, budget_active, have_budget = True, False, False, True, False, False
    n_frames = 0  # the frames in the view's own moments
    feat = feat_prev = hist_cam = None
    gate = dict(rule, min_frames=min(int(rule["min_frames"]), int(max_history)))
    out = []

    def trace():
        nonlocal acc, seeds, mom, stop, count, passes, rounds, feat, feat_prev, feat_dirty, carry, have_hist, hist_cam
        nonlocal stop_reset, budget_active, have_budget, n_frames, converged
        n = max(progression, 1)
        if budget_prm is None or (stop_reset and progression > 1):
            budget_active = False
        elif stop_reset:
            budget_active = True
        in_passes = budget_active and progression > 0
        if stop_reset:  # maskRenders: the planes start afresh
            stop = np.zeros(n_t, U)
            have_budget = False
            if budget_active:
                count, passes = np.zeros(n_t, U), np.ones(n_t, U)
        stop_reset = False
        render = render_at(az)
        if in_passes:
            acc, seeds, count, mom, own = br.display(render, acc, seeds, count, stop, passes, rounds if have_budget else 1, mom, W, H,
                                                     Wpad, Hpad)
        else:
            prev, seeds_prev, full = acc.copy(), seeds.copy(), acc.copy()
            render(full, progression, seeds)
            acc, seeds = ar.masked(stop, W, H, Wpad, Hpad, prev, full, seeds_prev, seeds)
            mom, own = ar.moments_tiles(prev, acc, n, mom, stop, W, H)
        n_frames = 1 if n == 1 else n_frames + 1
        hist_feat = feat
        if feat_dirty:  # rendered again: the old ones are kept, and the history is carried
            feat_prev, feat = feat, feat_at(az)
            hist_feat, feat_dirty, carry = feat_prev, False, True
        # mergeTemporal, on the per-pixel counts
        judged = tolerance is not None and have_hist
        if not have_hist:
            for hs in (colour, moments):
                hs.carried, hs.carried_len = np.zeros(4 * px, F), np.zeros(px, F)
        elif carry:
            kept_len = colour.kept_len
            for hs in (colour, moments):  # the moments with the colour's lengths
                hs.carried, hs.carried_len = tref.reproject(hs.kept, kept_len, hist_feat, hist_cam, feat, W, H, max_history=max_history)
        carry = False
        trusted = trust_len(orc, colour.carried, colour.carried_len, acc, own, feat, W, H, tolerance) if judged else None
        for hs, src in ((colour, acc), (moments, mom)):
            hs.kept, hs.kept_len = merge_len(hs.carried, trusted if judged else hs.carried_len, src, own, max_history)
        assert np.array_equal(colour.kept_len.view(U), moments.kept_len.view(U))
        hist_cam, have_hist = camera_at(az), True
        stats, _, tiles = meter(colour.kept, variance_with(feat)(colour.kept, moments.kept, colour.kept_len))
        tile_frames = tile_len_min(colour.kept_len, feat, W, H)
        stop, st = select_frames(tiles, tile_frames, stop, n, W, H, **gate)
        bst = dict(rounds=0, tile_passes=0, by_passes=[0] * (br.MAX_PASSES + 1))
        if budget_active:  # (the stop rule runs at every display, so the budget rule does)
            passes, bst = br.budget(tiles, stop, **budget_prm)
            rounds, have_budget = bst["rounds"], True
        converged = bool((n_frames >= converge_min_frames and int(stats["counted"]) > 0 and F(stats["level"]) <= F(threshold))
                         or st["active"] == 0)
        out.append(dict(n=n, shown=colour.kept.copy(), length=colour.kept_len.copy(), acc=acc.copy(), own=np.asarray(own, F).copy(),
                        stop=stop.copy(), count=count.copy(), stats=stats, tiles=np.asarray(tiles, F).copy(), tile_frames=tile_frames,
                        active=st["active"], stopped_now=st["stopped_now"], rounds=bst["rounds"], tile_passes=bst["tile_passes"],
                        by_passes=bst["by_passes"], converged=converged, budget=budget_active))

    for ev in filter(None, events.split(",")):
        if ev == "d":
            if realloc:
                realloc, progression = False, 0
                trace()
            elif not converged:
                progression += 1
                trace()
        elif ev == "l":
            az = float(np.fmod(F(F(az) + F(3.0)), F(360.0)))
            feat_dirty, progression, carry, stop_reset, converged = True, 0, True, True, False
        else:
            raise ValueError(f"event {ev!r}")
    return out
