"""float32 numpy restatement of the temporal reprojection and merge, shared by
tests/test_temporal_host.py and tests/test_gpu_temporal.py.  Every operation is one IEEE float32
operation in the order the definition gives (numpy float32 arrays round each product, sum, difference
and quotient separately)."""
from __future__ import annotations

import numpy as np

F = np.float32
RT_FEAT_NONE = -2


def _cross(a, b):
    return (F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])), F(F(a[0] * b[1]) - F(a[1] * b[0])))


def cofactors(cam16):
    """(position, cs, ca, cb, det) of a Camera: cs = right x up, ca = up x view, cb = view x right,
    det = view . cs — scalars, each product and sum rounded to float32."""
    cam = np.asarray(cam16, F).reshape(4, 4)
    v, u, r, pos = cam[0, :3], cam[1, :3], cam[2, :3], cam[3, :3]
    with np.errstate(all="ignore"):
        cs, ca, cb = _cross(r, u), _cross(u, v), _cross(v, r)
        det = F(F(F(v[0] * cs[0]) + F(v[1] * cs[1])) + F(v[2] * cs[2]))
    return pos, cs, ca, cb, det


def project(cam16, P, W, H):
    """The inverse of rt_primary_rays: (s, fx, fy) float32 arrays of points P (n, 3) under the camera
    (Cramer: s = ns / det, a = na / ns, b = nb / ns; fx = (a + W/2) - 0.5)."""
    pos, cs, ca, cb, det = cofactors(cam16)
    P = np.asarray(P, F)
    with np.errstate(all="ignore"):
        dx, dy, dz = P[:, 0] - pos[0], P[:, 1] - pos[1], P[:, 2] - pos[2]
        ns = (dx * cs[0] + dy * cs[1]) + dz * cs[2]
        na = (dx * ca[0] + dy * ca[1]) + dz * ca[2]
        nb = (dx * cb[0] + dy * cb[1]) + dz * cb[2]
        s = ns / det
        fx = ((na / ns) + F(W) / F(2.0)) - F(0.5)
        fy = ((nb / ns) + F(H) / F(2.0)) - F(0.5)
    return s.astype(F), fx.astype(F), fy.astype(F), det


def reproject(prev_rgba, prev_len, prev_feat, prev_cam, cur_feat, W, H, plane_tol=0.01, normal_min=0.9,
              max_history=32.0):
    """rt_reproject: returns (out_rgba W*H*4, out_len W*H) float32."""
    n = W * H
    pc = np.asarray(prev_rgba, F).reshape(n, 4)
    pl = np.asarray(prev_len, F).reshape(n)
    pf = np.asarray(prev_feat, F).reshape(2, n, 4)
    cf = np.asarray(cur_feat, F).reshape(2, n, 4)
    tol, nmin, mh = F(plane_tol), F(normal_min), F(max_history)
    Pp, tp, Np = cf[0, :, :3], cf[0, :, 3], cf[1, :, :3]
    idp = np.ascontiguousarray(cf[1, :, 3]).view(np.int32)
    idq_all = np.ascontiguousarray(pf[1, :, 3]).view(np.int32)
    s, fx, fy, det = project(prev_cam, Pp, W, H)
    out = np.zeros((n, 4), F)
    out_len = np.zeros(n, F)
    with np.errstate(all="ignore"):
        ok = (idp != RT_FEAT_NONE) & bool(det != 0) & (s > 0)
        ok &= (fx > F(-1.0)) & (fx < F(W)) & (fy > F(-1.0)) & (fy < F(H))
        k = np.flatnonzero(ok)
        if k.size == 0:
            return out.reshape(-1), out_len
        fx, fy = fx[k], fy[k]
        x0f, y0f = np.floor(fx), np.floor(fy)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        wx1, wy1 = fx - x0f, fy - y0f
        wx0, wy0 = F(1.0) - wx1, F(1.0) - wy1
        tolp = tol * tp[k]
        acc = np.zeros((k.size, 3), F)
        al = np.zeros(k.size, F)
        wsum = np.zeros(k.size, F)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                q = np.where(inside, qy * W + qx, 0)
                m = pl[q]
                idq = idq_all[q]
                cnt = inside & (m > 0) & (idq != RT_FEAT_NONE)
                cnt &= ((idp[k] >= 0) & (idq >= 0)) | (idp[k] == idq)
                Pq, Nq = pf[0, q, :3], pf[1, q, :3]
                d = Pq - Pp[k]
                pln = (d[:, 0] * Np[k, 0] + d[:, 1] * Np[k, 1]) + d[:, 2] * Np[k, 2]
                cnt &= np.abs(pln) <= tolp
                nn = (Nq[:, 0] * Np[k, 0] + Nq[:, 1] * Np[k, 1]) + Nq[:, 2] * Np[k, 2]
                cnt &= nn >= nmin
                w = (wx1 if i else wx0) * (wy1 if j else wy0)
                cq = pc[q, :3]
                acc = np.where(cnt[:, None], acc + w[:, None] * cq, acc).astype(F)
                al = np.where(cnt, al + w * m, al).astype(F)
                wsum = np.where(cnt, wsum + w, wsum).astype(F)
        have = wsum > 0
        rgb = acc / wsum[:, None]
        ln = al / wsum
        ln = np.where(ln < mh, ln, mh)
        out[k[have], :3] = rgb[have]
        out_len[k[have]] = ln[have]
    return out.reshape(-1), out_len


def merge(hist_rgba, hist_len, cur_rgba, n_cur, max_history=32.0):
    """rt_temporal_merge: returns (out_rgba, out_len) float32."""
    h = np.asarray(hist_rgba, F).reshape(-1, 4)
    m = np.asarray(hist_len, F).reshape(-1)
    c = np.asarray(cur_rgba, F).reshape(-1, 4)
    n, mh = F(n_cur), F(max_history)
    with np.errstate(all="ignore"):
        has = m > 0
        ln = np.where(has, n + m, n).astype(F)
        f = n / ln
        blend = h[:, :3] + (c[:, :3] - h[:, :3]) * f[:, None]
    out = c.copy()
    out[has, :3] = blend[has]
    out_len = np.where(ln < mh, ln, mh).astype(F)
    return out.reshape(-1), out_len
