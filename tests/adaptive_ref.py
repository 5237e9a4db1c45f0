"""numpy restatement of adaptive sampling: the stop rule on the noise meter's tile map,
the moments and history lengths that follow a stop plane, the pixel queue's order without the stopped
tiles, and what a masked render leaves of a frame.  Only comparisons and integers but for the moments,
which are tests/variance_ref.py's.  Shared by tests/test_adaptive_host.py and tests/test_gpu_adaptive.py."""
from __future__ import annotations

import numpy as np

import variance_ref as vr

F = np.float32
U = np.uint32
DEFAULTS = dict(threshold=0.05, max_ratio=4.0, min_frames=16, dilate=1)


def tile_grid(W: int, H: int) -> tuple[int, int]:
    """(tiles_x, tiles_y) of a W x H frame's 8x8 tiles."""
    return (W + 7) // 8, (H + 7) // 8


def n_tiles(W: int, H: int) -> int:
    tw, th = tile_grid(W, H)
    return tw * th


def max_limit(threshold, max_ratio) -> np.float32:
    """The bound on a tile's maximum: one float32 product, or +inf when max_ratio is (0 x inf is a NaN)."""
    if np.isinf(F(max_ratio)):
        return F(np.inf)
    with np.errstate(all="ignore"):
        return F(F(threshold) * F(max_ratio))


def quiet(tiles, n_frames: int, threshold=0.05, max_ratio=4.0, min_frames=16, **_) -> np.ndarray:
    """Per tile of the (mean, max) pairs: n_frames >= min_frames, mean <= threshold, max <= the limit."""
    t = np.asarray(tiles, F).reshape(-1, 2)
    with np.errstate(all="ignore"):
        return (int(n_frames) >= int(min_frames)) & (t[:, 0] <= F(threshold)) & (t[:, 1] <= max_limit(threshold, max_ratio))


def select(tiles, stop, n_frames: int, W: int, H: int, threshold=0.05, max_ratio=4.0, min_frames=16, dilate=1):
    """rt_tile_stop_select: (the new plane, stats).  Every tile is decided from `stop` as given."""
    tw, th = tile_grid(W, H)
    old = np.asarray(stop, U).reshape(th, tw)
    settled = (old != 0) | quiet(tiles, n_frames, threshold, max_ratio, min_frames).reshape(th, tw)
    d = int(dilate)
    padded = np.ones((th + 2 * d, tw + 2 * d), bool)  # outside the frame nothing objects
    padded[d:d + th, d:d + tw] = settled
    around = np.ones((th, tw), bool)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            around &= padded[dy:dy + th, dx:dx + tw]
    now = (old == 0) & around
    new = np.where(now, U(n_frames), old).astype(U)
    stats = dict(tiles=tw * th, active=int((new == 0).sum()), stopped_now=int(now.sum()), frames=int(n_frames))
    return new.reshape(-1), stats


def pixel_tiles(W: int, H: int) -> np.ndarray:
    """The tile index of every pixel of the row-major frame."""
    tw, _ = tile_grid(W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    return ((ys >> 3) * tw + (xs >> 3)).reshape(-1)


def pixel_mask(stop, W: int, H: int) -> np.ndarray:
    """Per pixel: whether its tile is live."""
    return np.asarray(stop, U).reshape(-1)[pixel_tiles(W, H)] == 0


def moments_tiles(prev_rgba, cur_rgba, n_cur, mom_in, stop, W: int, H: int, mom_out=None):
    """rt_moments_accumulate_tiles: (moments, lengths).  Without mom_in (n_cur == 1) a stopped tile keeps
    `mom_out`'s contents (zeros when that is not given either)."""
    live = pixel_mask(stop, W, H)
    full = vr.moments(prev_rgba, cur_rgba, n_cur, mom_in).reshape(-1, 4)
    kept = mom_in if mom_in is not None else (mom_out if mom_out is not None else np.zeros(4 * W * H, F))
    kept = np.asarray(kept, F).reshape(-1, 4)
    mom = np.where(live[:, None], full, kept).astype(F)
    length = np.where(live, F(n_cur), np.asarray(stop, U).reshape(-1)[pixel_tiles(W, H)].astype(F)).astype(F)
    return mom.reshape(-1), length


def variance_temporal(mom, length) -> np.ndarray:
    """rt_variance where len >= min_len: max(m.y - m.x m.x, 0) / (len - 1)."""
    m = np.asarray(mom, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        d = m[:, 1] - m[:, 0] * m[:, 0]
        return (np.where(d > 0, d, F(0.0)).astype(F) / (np.asarray(length, F) - F(1.0))).astype(F)


def order(base, stop) -> tuple[np.ndarray, int]:
    """The masked order: base's live entries in base's order (base None: 0, 1, ...), then n_tiles in every
    remaining position; and the live count.  An entry that is no tile index counts as stopped."""
    stop = np.asarray(stop, U).reshape(-1)
    n = stop.size
    b = np.arange(n, dtype=np.int64) if base is None else np.asarray(base, U).astype(np.int64)
    ok = b < n
    keep = ok & (stop[np.where(ok, b, 0)] == 0)
    live = b[keep]
    out = np.full(n, n, U)
    out[:live.size] = live
    return out, int(live.size)


def masked(stop, W: int, H: int, Wpad: int, Hpad: int, before, after, seeds_before, seeds_after):
    """select(mask, oracle(state), state): the frame (W*H*4 floats) and both seed planes (2 Wpad Hpad words)
    a masked render leaves, from the state before it and the state the unmasked render leaves."""
    live = pixel_mask(stop, W, H)
    frame = np.where(np.repeat(live, 4), np.asarray(after, F), np.asarray(before, F)).astype(F)
    seeds = np.asarray(seeds_before, U).copy()
    ys, xs = np.mgrid[0:H, 0:W]
    slots = (ys * Wpad + xs).reshape(-1)[live]
    for plane in (0, Wpad * Hpad):
        seeds[plane + slots] = np.asarray(seeds_after, U)[plane + slots]
    return frame, seeds
