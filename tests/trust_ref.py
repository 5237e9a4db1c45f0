"""float32 numpy restatement of rt_history_trust, shared by tests/test_trust_host.py
and tests/test_gpu_trust.py, and its binary64 twin.  Every operation is one IEEE float32 operation in
the order the definition gives (numpy float32 arrays round each product, sum and quotient separately);
the exponential is the pinned one, through the oracle."""
from __future__ import annotations

import numpy as np

import features_ref as fr
from variance_ref import lum

F = np.float32
RADIUS = 3  # the 7 x 7 window


def _window_sums(T, expf, hist_rgba, hist_len, cur_rgba, feat, W, H, isn, isp):
    """The six sums of the window in dtype T (taps dy outer, dx inner; a tap that does not count leaves
    them as they are) and the masks (has a length, has a surface)."""
    h = np.asarray(hist_rgba, F).reshape(H, W, 4).astype(T)
    c = np.asarray(cur_rgba, F).reshape(H, W, 4).astype(T)
    m = np.asarray(hist_len, F).reshape(H, W)
    f = np.asarray(feat, F).reshape(2, H, W, 4)
    P, N = f[0, :, :, :3].astype(T), f[1, :, :, :3].astype(T)
    ids = np.ascontiguousarray(f[1, :, :, 3]).view(np.int32)
    if T is F:
        Lc, Lh = lum(c), lum(h)
    else:
        Lc = (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]
        Lh = (0.2126 * h[..., 0] + 0.7152 * h[..., 1]) + 0.0722 * h[..., 2]
    has = m > 0
    surf = ids != fr.RT_FEAT_NONE
    ys, xs = np.mgrid[0:H, 0:W]
    ws, w2, ac, ac2, ah, ah2 = (np.zeros((H, W), T) for _ in range(6))
    for dy in range(-RADIUS, RADIUS + 1):
        for dx in range(-RADIUS, RADIUS + 1):
            qy, qx = ys + dy, xs + dx
            ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W) & has & surf
            py, px = ys[ok], xs[ok]
            qy, qx = qy[ok], qx[ok]
            idp, idq = ids[py, px], ids[qy, qx]
            cnt = has[qy, qx] & (idq != fr.RT_FEAT_NONE) & (((idp >= 0) & (idq >= 0)) | (idp == idq))
            py, px, qy, qx = py[cnt], px[cnt], qy[cnt], qx[cnt]
            if py.size == 0:
                continue
            dn = N[qy, qx] - N[py, px]
            en = dn[:, 0] * dn[:, 0] + dn[:, 1] * dn[:, 1] + dn[:, 2] * dn[:, 2]
            dp, n_p = P[qy, qx] - P[py, px], N[py, px]
            pl = dp[:, 0] * n_p[:, 0] + dp[:, 1] * n_p[:, 1] + dp[:, 2] * n_p[:, 2]
            ep = pl * pl
            w = expf(-(en * isn + ep * isp))
            lc, lh = Lc[qy, qx], Lh[qy, qx]
            ws[py, px] = ws[py, px] + w
            w2[py, px] = w2[py, px] + w * w
            ac[py, px] = ac[py, px] + lc * w
            ac2[py, px] = ac2[py, px] + (lc * lc) * w
            ah[py, px] = ah[py, px] + lh * w
            ah2[py, px] = ah2[py, px] + (lh * lh) * w
    return (ws, w2, ac, ac2, ah, ah2), m, has, surf


def _statistic(T, sums, m, n_cur):
    """(ne, z2) in dtype T from the window sums, steps 4 to 7."""
    ws, w2, ac, ac2, ah, ah2 = sums
    mm, n = m.astype(T), T(F(n_cur))
    zero, one = T(0.0), T(1.0)
    mc, mh = ac / ws, ah / ws
    dc, dh = ac2 / ws - mc * mc, ah2 / ws - mh * mh
    vc, vh = np.where(dc > 0, dc, zero).astype(T), np.where(dh > 0, dh, zero).astype(T)
    ne = w2 / (ws * ws)
    vs = vh * (np.where(mm > one, mm, one).astype(T) / n)
    v = np.where(vc > vs, vc, vs).astype(T)
    vd = (v * ne) * (one + n / mm) + T(F(1e-12))
    d = mc - mh
    return ne, (d * d) / vd


def trust(orc, hist_rgba, hist_len, cur_rgba, n_cur, feat, W, H, tolerance=1.5, sigma_normal=0.3, sigma_plane=0.1):
    """rt_history_trust: returns the W*H float32 plane of trusted history lengths."""
    m0 = np.asarray(hist_len, F).reshape(-1)
    if np.isinf(F(tolerance)):
        return m0.copy()
    _, isn, isp = fr.inverse_variances(1, 1.0, sigma_normal, sigma_plane)
    k2 = F(tolerance) * F(tolerance)
    with np.errstate(all="ignore"):
        sums, m, has, surf = _window_sums(F, lambda a: orc.math("exp", a.astype(F)), hist_rgba, hist_len, cur_rgba, feat,
                                          W, H, isn, isp)
        ne, z2 = _statistic(F, sums, m, n_cur)
        cut = has & surf & ~(ne > F(0.5)) & (z2 > k2)
        out = np.where(cut, m * (k2 / z2), m).astype(F)
        out = np.where(has, out, F(0.0)).astype(F)
    return out.reshape(-1)


def trust64(hist_rgba, hist_len, cur_rgba, n_cur, feat, W, H, tolerance=1.5, sigma_normal=0.3, sigma_plane=0.1):
    """The binary64 twin: (out_len, z2 / k2, ne) float64 planes, z2 / k2 NaN where no test is made."""
    D = np.float64
    isn, isp = 1.0 / (D(F(sigma_normal)) ** 2), 1.0 / (D(F(sigma_plane)) ** 2)
    k2 = D(F(tolerance)) ** 2
    with np.errstate(all="ignore"):
        sums, m, has, surf = _window_sums(D, np.exp, hist_rgba, hist_len, cur_rgba, feat, W, H, isn, isp)
        ne, z2 = _statistic(D, sums, m, n_cur)
        tested = has & surf & ~(ne > 0.5)
        md = m.astype(D)
        out = np.where(tested & (z2 > k2), md * (k2 / z2), md)
        out = np.where(has, out, 0.0)
    return out.reshape(-1), np.where(tested, z2 / k2, np.nan).reshape(-1), ne.reshape(-1)
