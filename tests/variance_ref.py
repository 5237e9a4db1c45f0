"""float32 numpy restatement of the variance-guided display filter: the luminance
moments, the variance estimate and the filter, shared by tests/test_variance_host.py and
tests/test_gpu_variance.py.  Every operation is one IEEE float32 operation in the order the definition
gives (numpy float32 arrays round each product, sum, quotient and square root separately); the
exponential is the pinned one, through the oracle."""
from __future__ import annotations

import numpy as np

import features_ref as fr

F = np.float32


def lum(c):
    """(0.2126 x + 0.7152 y) + 0.0722 z over the last axis."""
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def mix(old, s, n):
    """The progressive render's update, OpenCL mix(old, s, 1 / n) = old + (s - old) * (1 / n), float32."""
    old, s = np.asarray(old, F), np.asarray(s, F)
    return (old + (s - old) * (F(1.0) / F(n))).astype(F)


def moments(prev_rgba, cur_rgba, n_cur, mom_in):
    """rt_moments_accumulate: returns the W*H*4 float32 moments frame."""
    cur = np.asarray(cur_rgba, F).reshape(-1, 4)[:, :3]
    n = F(n_cur)
    with np.errstate(all="ignore"):
        if n == F(1.0):
            s = cur
        else:
            prev = np.asarray(prev_rgba, F).reshape(-1, 4)[:, :3]
            s = prev + (cur - prev) * n
        s = np.where(s > 0, s, F(0.0)).astype(F)
        L = lum(s)
        out = np.zeros((len(cur), 4), F)
        if n == F(1.0):
            out[:, 0], out[:, 1] = L, L * L
        else:
            m = np.asarray(mom_in, F).reshape(-1, 4)
            f = F(1.0) / n
            out[:, 0] = m[:, 0] + (L - m[:, 0]) * f
            out[:, 1] = m[:, 1] + (L * L - m[:, 1]) * f
    return out.reshape(-1)


def _feature_terms(P, N, qy, qx, py, px, isn, isp):
    """(en isn, ep isp) of the taps (qy, qx) of pixels (py, px), as DESIGN.md §4.9."""
    dn = N[qy, qx] - N[py, px]
    en = dn[:, 0] * dn[:, 0] + dn[:, 1] * dn[:, 1] + dn[:, 2] * dn[:, 2]
    dp, n_p = P[qy, qx] - P[py, px], N[py, px]
    pl = dp[:, 0] * n_p[:, 0] + dp[:, 1] * n_p[:, 1] + dp[:, 2] * n_p[:, 2]
    ep = pl * pl
    return en * isn, ep * isp


def variance(orc, disp_rgba, mom_rgba, length, feat, W, H, sigma_normal=0.3, sigma_plane=0.1, min_len=4.0):
    """rt_variance: returns the W*H float32 variance plane."""
    c = np.asarray(disp_rgba, F).reshape(H, W, 4)
    m = np.asarray(mom_rgba, F).reshape(H, W, 4)
    l = np.asarray(length, F).reshape(H, W)
    f = np.asarray(feat, F).reshape(2, H, W, 4)
    P, N = f[0, :, :, :3], f[1, :, :, :3]
    _, isn, isp = fr.inverse_variances(1, 1.0, sigma_normal, sigma_plane)
    ml = F(min_len)
    ys, xs = np.mgrid[0:H, 0:W]
    L = lum(c)
    with np.errstate(all="ignore"):
        d = m[:, :, 1] - m[:, :, 0] * m[:, :, 0]
        temporal = np.where(d > 0, d, F(0.0)).astype(F) / (l - F(1.0))
        a1, a2, ws = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                qy, qx = ys + dy, xs + dx
                ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                if not ok.any():
                    continue
                py, px = ys[ok], xs[ok]
                tn, tp = _feature_terms(P, N, qy[ok], qx[ok], py, px, isn, isp)
                w = orc.math("exp", (-(tn + tp)).astype(F))
                Lq = L[qy[ok], qx[ok]]
                a1[py, px] = a1[py, px] + Lq * w
                a2[py, px] = a2[py, px] + (Lq * Lq) * w
                ws[py, px] = ws[py, px] + w
        m1, m2 = a1 / ws, a2 / ws
        d = m2 - m1 * m1
        spatial = np.where(d > 0, d, F(0.0)).astype(F) * (ml / np.where(l > F(1.0), l, F(1.0)).astype(F))
        out = np.where(l >= ml, temporal, spatial).astype(F)
    return out.reshape(-1)


def denoise_var(orc, col, var, feat, W, H, iterations=5, sigma_lum=4.0, sigma_normal=0.3, sigma_plane=0.1):
    """rt_denoise_var: returns (out_rgba W*H*4, out_var W*H) float32."""
    c = np.array(col, F).reshape(H, W, 4)
    v = np.array(var, F).reshape(H, W)
    f = np.asarray(feat, F).reshape(2, H, W, 4)
    P, N = f[0, :, :, :3], f[1, :, :, :3]
    _, isn, isp = fr.inverse_variances(1, 1.0, sigma_normal, sigma_plane)
    k = [F(0.375), F(0.25), F(0.0625)]
    kg = [F(0.25), F(0.125), F(0.0625)]
    sl = F(sigma_lum)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            ga, gs = np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    qy, qx = ys + dy, xs + dx
                    ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    py, px = ys[ok], xs[ok]
                    g = kg[abs(dx) + abs(dy)]
                    ga[py, px] = ga[py, px] + v[qy[ok], qx[ok]] * g
                    gs[py, px] = gs[py, px] + g
            g = ga / gs
            if np.isinf(sl):
                il = np.zeros((H, W), F)
            else:
                il = F(1.0) / (sl * np.sqrt(g) + F(1e-8))
            L = lum(c)
            acc = np.zeros((H, W, 3), F)
            wsum = np.zeros((H, W), F)
            vacc = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + s * dy, xs + s * dx
                    ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    if not ok.any():
                        continue
                    py, px = ys[ok], xs[ok]
                    cq = c[qy[ok], qx[ok], :3]
                    h = F(k[abs(dx)] * k[abs(dy)])
                    el = np.abs(L[qy[ok], qx[ok]] - L[py, px]) * il[py, px]
                    tn, tp = _feature_terms(P, N, qy[ok], qx[ok], py, px, isn, isp)
                    w = h * orc.math("exp", (-((el + tn) + tp)).astype(F))
                    acc[py, px] = acc[py, px] + cq * w[:, None]
                    wsum[py, px] = wsum[py, px] + w
                    vacc[py, px] = vacc[py, px] + v[qy[ok], qx[ok]] * (w * w)
            out = c.copy()
            out[:, :, :3] = acc / wsum[:, :, None]
            v = (vacc / (wsum * wsum)).astype(F)
            c = out
    return c.reshape(-1), v.reshape(-1)
