"""numpy restatement of the noise meter: the relative standard error per pixel in
float32, its bin in integers, the tile figures by the butterfly's six levels over all 64 lanes, and the
statistic in Python integers, every operation one IEEE operation in the order the definition gives.
Shared by tests/test_noise_host.py and tests/test_gpu_noise.py."""
from __future__ import annotations

import numpy as np

from tonemap_ref import BIN0, BINS, lum

F = np.float32
U = np.uint32
DEFAULTS = dict(percentile=0.95, threshold=0.05, lum_floor=1e-3)
_LANES = np.arange(64)


def f_bits(u):
    return np.asarray(u, U).view(F)


def upper_edge(i: int) -> np.float32:
    """The upper edge of bin i: the lower edge of the next one, +inf for the last."""
    return F(np.inf) if i >= BINS - 1 else f_bits(np.array([(i + BIN0 + 1) << 19], U))[0]


def bin_of(e):
    """The bin of each float32 of `e` (its sign is dropped)."""
    u = np.ascontiguousarray(np.asarray(e, F)).view(U) & U(0x7FFFFFFF)
    return np.clip((u >> 19).astype(np.int64) - BIN0, 0, BINS - 1)


def errors(rgba, var, lum_floor=1e-3):
    """(valid, e) per pixel: e = sqrt(v) / (max(L, 0) + lum_floor) where the pixel is valid, else 0."""
    L = np.asarray(lum(np.asarray(rgba, F).reshape(-1, 4)), F)
    v = np.asarray(var, F).reshape(-1)
    with np.errstate(all="ignore"):
        valid = (v >= 0) & np.isfinite(v) & np.isfinite(L)
        Lp = np.where(L > 0, L, F(0.0)).astype(F)
        e = (np.sqrt(np.where(valid, v, F(0.0)).astype(F)).astype(F) / (Lp + F(lum_floor)).astype(F)).astype(F)
    return valid, np.where(valid, e, F(0.0)).astype(F)


def histogram(valid, e):
    return np.bincount(bin_of(e)[valid], minlength=BINS).astype(U)


def butterfly_sum(a):
    """[..., 64] float32 -> lane 0 after the six levels a_j = a_j + a_(j ^ (1 << k))."""
    a = np.asarray(a, F).copy()
    with np.errstate(all="ignore"):
        for k in range(6):
            a = (a + a[..., _LANES ^ (1 << k)]).astype(F)
    return a[..., 0]


def butterfly_max(a):
    """... with a_j = rt_maxf(a_j, a_(j ^ (1 << k))) = a_j < other ? other : a_j."""
    a = np.asarray(a, F).copy()
    for k in range(6):
        o = a[..., _LANES ^ (1 << k)]
        a = np.where(a < o, o, a).astype(F)
    return a[..., 0]


def tile_lanes(plane, W, H, fill):
    """A W*H plane as [tiles_y, tiles_x, 64]: lane j = (y & 7) 8 + (x & 7), `fill` outside the frame."""
    tw, th = (W + 7) // 8, (H + 7) // 8
    p = np.full((th * 8, tw * 8), fill, np.asarray(plane).dtype)
    p[:H, :W] = np.asarray(plane).reshape(H, W)
    return p.reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(th, tw, 64)


def tiles(valid, e, W, H):
    """The tile plane: ceil(H/8) x ceil(W/8) pairs (mean, max) as a flat float32 array."""
    a = tile_lanes(e, W, H, F(0.0))
    n = tile_lanes(valid, W, H, False).sum(axis=-1)
    s, m = butterfly_sum(a), butterfly_max(a)
    with np.errstate(all="ignore"):
        mean = np.where(n > 0, (s / np.maximum(n, 1).astype(F)).astype(F), F(0.0)).astype(F)
    mx = np.where(n > 0, m, F(0.0)).astype(F)
    return np.ascontiguousarray(np.stack([mean, mx], axis=-1).reshape(-1))


def rank(percentile, N: int) -> int:
    return min(int(np.float64(F(percentile)) * np.float64(N)), N - 1)


def stats(hist, npx: int, percentile=0.95, threshold=0.05) -> dict:
    n = [int(v) for v in hist]
    N = sum(n)
    if N == 0:
        return dict(level=F(0.0), counted=0, skipped=npx, below=0)
    r = rank(percentile, N)
    c = 0
    for i, ni in enumerate(n):
        c += ni
        if c > r:
            break
    below = sum(ni for k, ni in enumerate(n) if upper_edge(k) <= F(threshold))
    return dict(level=upper_edge(i), counted=N, skipped=npx - N, below=below)


def meter(rgba, var, W, H, percentile=0.95, threshold=0.05, lum_floor=1e-3):
    """(stats, histogram, tile plane) of the frame."""
    valid, e = errors(rgba, var, lum_floor)
    h = histogram(valid, e)
    return stats(h, W * H, percentile, threshold), h, tiles(valid, e, W, H)


def same_stats(a: dict, b: dict) -> bool:
    la, lb = (np.array([d["level"]], F).view(U)[0] for d in (a, b))
    return la == lb and all(int(a[k]) == int(b[k]) for k in ("counted", "skipped", "below"))
