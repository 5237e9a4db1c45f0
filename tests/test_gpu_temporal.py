"""GPU: the temporal reprojection and merge of the displayed frame (rt_reproject, rt_temporal_merge,
DESIGN.md §4.10) against their float32 numpy restatement (tests/temporal_ref.py), bit for bit; what
they must do independently of that restatement (identity, disocclusion, coverage); that they leave a
render's state alone; ProgressiveViewHIP::setTemporal through the rt_render CLI; and their effect on
an orbit of 1-spp frames.  Run on the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

import features_ref as fr
import render_state as rs
import temporal_ref as tr
import view_ref as vr
from conftest import bits

pytestmark = pytest.mark.gpu

CASE = "tris_64x48_sr1"
F = np.float32
TARGET = (0.0, -4.0, 0.0)
EL0, AZ0, DIST = 40.0, 105.0, 5.0  # the golden view
SIZES = [(1, 1), (5, 3), (37, 29), (64, 48)]
MOVES = {"same": (0.0, 0.0), "az+3": (0.0, 3.0), "el-3": (-3.0, 0.0), "az+30": (0.0, 30.0), "az+90": (0.0, 90.0)}


@pytest.fixture(scope="module")
def rt(pt, golden, golden_meta):
    g, m = golden(CASE), golden_meta["cases"][CASE]
    t = pt.RayTracer(0)
    t.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
    t.setSampleRate(1)
    t.setMaxPathDepth(m["max_depth"])
    t.setMesh(g["verts"], g["idx"])
    yield t
    t.close()


@pytest.fixture(scope="module")
def views(rt):
    """(w, h, elevation, azimuth) -> (Camera, feature buffer) of the golden scene, rendered once each."""
    cache = {}

    def get(w, h, el, az):
        key = (w, h, el, az)
        if key not in cache:
            rt.setCameraSpherical(TARGET, el, az, DIST)
            cam = rt.getCamera(w)
            feat = np.zeros(2 * w * h * 4, F)
            rt.renderFeatures(feat, w, h, kernel=2)
            cache[key] = (cam, feat)
        return cache[key]

    return get


def _history(w, h, seed, zero_share=0.2):
    rng = np.random.default_rng(seed)
    col = (rng.random(w * h * 4, dtype=F) * F(3.0) - F(1.0)).astype(F)
    ln = (rng.random(w * h, dtype=F) * F(40.0)).astype(F)
    ln[rng.random(w * h) < zero_share] = 0.0
    return col, ln


def _gpu_reproject(rt, col, ln, pfeat, pcam, cfeat, w, h, **kw):
    out = np.full(w * h * 4, np.nan, F)
    ol = np.full(w * h, np.nan, F)
    rt.reproject(col, ln, pfeat, pcam, cfeat, out, ol, w, h, **kw)
    return out, ol


@pytest.mark.parametrize("move", list(MOVES))
@pytest.mark.parametrize("w,h", SIZES)
def test_reproject_equals_numpy(w, h, move, rt, views):
    """Whole frames of the golden scene under two cameras; random finite history colours, random
    lengths with a fifth of them 0; the inputs are only read."""
    de, da = MOVES[move]
    pcam, pfeat = views(w, h, EL0, AZ0)
    ccam, cfeat = views(w, h, EL0 + de, AZ0 + da)
    col, ln = _history(w, h, 1000 * w + len(move))
    keep = [a.copy() for a in (col, ln, pfeat, cfeat, pcam)]
    out, ol = _gpu_reproject(rt, col, ln, pfeat, pcam, cfeat, w, h)
    exp, el = tr.reproject(col, ln, pfeat, pcam, cfeat, w, h)
    assert np.array_equal(bits(out), bits(exp))
    assert np.array_equal(bits(ol), bits(el))
    for a, b in zip((col, ln, pfeat, cfeat, pcam), keep):
        assert np.array_equal(bits(a), bits(b))
    assert rt.lastReprojectMs() > 0.0


AXIS_CAM = np.array([0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0], F)  # view +z, up +y, right +x, at the origin


def _synthetic(w, h, seed):
    """Feature buffers no scene produces.  Under AXIS_CAM a point (x, y, z) projects to fx = x / z +
    w/2 - 0.5 exactly where the quotient is exact.  The previous frame is the plane z = 2 seen through
    that camera, with jittered depths, normals and every kind of id; the current pixels aim at chosen
    places of it: integers and half-integers from 3 outside the frame to 3 outside on the other side
    (both borders exactly), behind the camera, at distances where the products overflow."""
    rng = np.random.default_rng(seed)
    n = w * h
    ids = np.array([fr.RT_FEAT_NONE, fr.RT_FEAT_BOX, fr.RT_FEAT_SPHERE0, fr.RT_FEAT_SPHERE0 - 1, 0, 7, 123], np.int32)
    ys, xs = np.divmod(np.arange(n), w)
    prev = np.zeros((2, n, 4), F)
    z = np.where(rng.random(n) < 0.8, 2.0, 2.0 + rng.random(n) * 0.1).astype(F)
    prev[0, :, 0] = (xs - w / 2 + 0.5).astype(F) * z
    prev[0, :, 1] = (ys - h / 2 + 0.5).astype(F) * z
    prev[0, :, 2] = z
    prev[0, :, 3] = z
    tilt = np.where(rng.random(n) < 0.7, 0.0, rng.random(n) * 0.8).astype(F)
    prev[1, :, 0], prev[1, :, 2] = tilt, -np.sqrt(F(1.0) - tilt * tilt).astype(F)
    prev[1, :, 3] = ids[rng.integers(0, len(ids), n)].view(F)
    cur = np.zeros((2, n, 4), F)
    fx = (rng.integers(-6, 2 * w + 6, n) / 2.0)  # halves from -3 to w + 2.5
    fy = (rng.integers(-6, 2 * h + 6, n) / 2.0)
    fx[rng.random(n) < 0.1] += 0.3
    zc = np.full(n, 2.0, F)
    kind = rng.random(n)
    zc[kind < 0.08] = -2.0        # behind the previous camera
    zc[(kind >= 0.08) & (kind < 0.12)] = 0.0
    zc[(kind >= 0.12) & (kind < 0.16)] = F(1e30)
    zc[(kind >= 0.16) & (kind < 0.20)] = F(3e38)   # x / y overflow to infinity, or NaN
    cid = ids[rng.integers(0, len(ids), n)]
    # every border of the frame met exactly, by pixels in front of the camera that met a surface
    edge = np.arange(100, 108)
    fx[edge] = [-1.0, 0.0, w - 1.0, w, 9.0, 9.0, 9.0, 9.0]
    fy[edge] = [7.0, 7.0, 7.0, 7.0, -1.0, 0.0, h - 1.0, h]
    zc[edge], cid[edge] = 2.0, 7
    with np.errstate(all="ignore"):
        cur[0, :, 0] = (F(1.0) * (fx - w / 2 + 0.5)).astype(F) * zc
        cur[0, :, 1] = (F(1.0) * (fy - h / 2 + 0.5)).astype(F) * zc
    cur[0, :, 2] = zc
    cur[0, :, 3] = np.abs(zc)
    cur[1, :, 2] = -1.0
    cur[1, :, 3] = cid.view(F)
    col, ln = _history(w, h, seed + 1, zero_share=0.15)
    ln[(xs < 6) & (ys < 5)] = 0.0  # a region where all four taps have no history
    finite = np.isfinite(cur[0]).all(axis=1)
    cur[0][~finite] = np.where(np.isfinite(cur[0][~finite]), cur[0][~finite], F(3e38))  # finite inputs only
    return col, ln, prev.reshape(-1), cur.reshape(-1)


def _skewed(cam):
    c = cam.copy().reshape(4, 4)
    c[1, :3] = c[1, :3] * F(1.25) + c[2, :3] * F(0.25)
    c[2, :3] = c[2, :3] + c[0, :3] * F(0.125)
    return c.reshape(-1)


def _singular(cam):
    c = cam.copy().reshape(4, 4)
    c[1] = c[2]  # up = right: the determinant is 0
    return c.reshape(-1)


@pytest.mark.parametrize("cam_kind", ["axis", "skewed", "singular", "zero"])
@pytest.mark.parametrize("kw", [{}, dict(plane_tol=float("inf"), normal_min=-1.0, max_history=4.0)])
def test_reproject_synthetic(cam_kind, kw, rt):
    w, h = 37, 11
    col, ln, prev, cur = _synthetic(w, h, 5)
    cam = {"axis": AXIS_CAM, "skewed": _skewed(AXIS_CAM), "singular": _singular(AXIS_CAM),
           "zero": np.zeros(16, F)}[cam_kind]
    out, ol = _gpu_reproject(rt, col, ln, prev, cam, cur, w, h, **kw)
    exp, el = tr.reproject(col, ln, prev, cam, cur, w, h, **kw)
    assert np.array_equal(bits(out), bits(exp))
    assert np.array_equal(bits(ol), bits(el))
    assert np.isfinite(out).all() and np.isfinite(ol).all()
    cid, pid = fr.feature_ids(cur), fr.feature_ids(prev)
    assert not ol[cid == fr.RT_FEAT_NONE].any()
    if cam_kind in ("singular", "zero"):
        assert not ol.any() and not out.any()
    elif cam_kind == "axis":
        assert not ol[cur.reshape(2, -1, 4)[0, :, 2] <= 0].any()  # behind the camera, or in its plane
        # the cases are there: history kept and dropped, every border met exactly
        assert (ol > 0).sum() > 20 and (ol == 0).sum() > 20
        s, fx, fy, _ = tr.project(cam, cur.reshape(2, -1, 4)[0, :, :3], w, h)
        for v, lim in ((fx, w), (fy, h)):
            for edge in (-1.0, 0.0, lim - 1.0, float(lim)):
                assert (v[s > 0] == F(edge)).any()
        # a sphere pixel takes history from that sphere only, a box pixel from the box only
        x0, y0 = np.floor(fx), np.floor(fy)
        for p in np.flatnonzero((ol > 0) & (cid < 0)):
            taps = [(int(x0[p]) + i, int(y0[p]) + j) for j in (0, 1) for i in (0, 1)]
            assert any(0 <= x < w and 0 <= y < h and pid[y * w + x] == cid[p] for x, y in taps)
        assert ((ol > 0) & (cid <= fr.RT_FEAT_SPHERE0)).any() and ((ol > 0) & (cid == fr.RT_FEAT_BOX)).any()
        if "max_history" in kw:
            assert ol.max() == F(4.0)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (37, 29)])
@pytest.mark.parametrize("n,mh", [(1.0, 32.0), (2.0, 32.0), (17.0, 8.0)])
def test_merge_equals_numpy(w, h, n, mh, rt):
    """Host arrays and device tensors, apart and in place; where the history is empty the current
    frame's bits come back (a -0.0 among them)."""
    import torch

    rng = np.random.default_rng(int(7 * w + n))
    hist, ln = _history(w, h, int(31 * w + n), zero_share=0.3)
    cur = (rng.random(w * h * 4, dtype=F) * F(2.0) - F(0.5)).astype(F)
    cur[0] = F(-0.0)
    ln[0] = 0.0
    exp, el = tr.merge(hist, ln, cur, n, mh)
    empty = np.repeat(ln == 0, 4)
    assert np.array_equal(bits(exp)[empty], bits(cur)[empty]) and empty.any()
    out, ol = np.full(w * h * 4, np.nan, F), np.full(w * h, np.nan, F)
    rt.temporalMerge(hist, ln, cur, n, out, ol, w, h, max_history=mh)
    assert np.array_equal(bits(out), bits(exp)) and np.array_equal(bits(ol), bits(el))
    assert np.array_equal(out[3::4], cur[3::4])  # alpha is the current frame's
    h2, l2, c2 = hist.copy(), ln.copy(), cur.copy()
    rt.temporalMerge(h2, l2, c2, n, h2, l2, w, h, max_history=mh)
    assert np.array_equal(bits(h2), bits(exp)) and np.array_equal(bits(l2), bits(el))
    assert np.array_equal(bits(c2), bits(cur))
    dh, dl, dc = (torch.from_numpy(a).cuda() for a in (hist, ln, cur))
    do, dol = torch.zeros_like(dh), torch.zeros_like(dl)
    rt.temporalMerge(dh, dl, dc, n, do, dol, w, h, max_history=mh)
    assert np.array_equal(bits(do.cpu().numpy()), bits(exp)) and np.array_equal(bits(dol.cpu().numpy()), bits(el))
    assert np.array_equal(bits(dh.cpu().numpy()), bits(hist)) and np.array_equal(bits(dl.cpu().numpy()), bits(ln))
    rt.temporalMerge(dh, dl, dc, n, dh, dl, w, h, max_history=mh)
    assert np.array_equal(bits(dh.cpu().numpy()), bits(exp)) and np.array_equal(bits(dl.cpu().numpy()), bits(el))
    assert np.array_equal(bits(dc.cpu().numpy()), bits(cur))
    assert rt.lastReprojectMs(merge=True) > 0.0
    # no history at all: the current frame
    rt.temporalMerge(hist, np.zeros_like(ln), cur, n, out, ol, w, h, max_history=mh)
    assert np.array_equal(bits(out), bits(cur)) and np.all(ol == min(n, mh))
    with pytest.raises(ValueError):
        rt.temporalMerge(dh, ln, dc, n, do, dol, w, h)  # host and device buffers mixed


def test_reproject_device_tensors(rt, views):
    import torch

    w, h = 37, 29
    pcam, pfeat = views(w, h, EL0, AZ0)
    _, cfeat = views(w, h, EL0, AZ0 + 3.0)
    col, ln = _history(w, h, 77)
    exp, el = tr.reproject(col, ln, pfeat, pcam, cfeat, w, h)
    dcol, dln, dpf, dcf = (torch.from_numpy(a).cuda() for a in (col, ln, pfeat, cfeat))
    dout, dol = torch.zeros_like(dcol), torch.zeros_like(dln)
    rt.reproject(dcol, dln, dpf, pcam, dcf, dout, dol, w, h)
    assert np.array_equal(bits(dout.cpu().numpy()), bits(exp)) and np.array_equal(bits(dol.cpu().numpy()), bits(el))
    for d, a in ((dcol, col), (dln, ln), (dpf, pfeat), (dcf, cfeat)):
        assert np.array_equal(bits(d.cpu().numpy()), bits(a))
    with pytest.raises(ValueError):
        rt.reproject(dcol, ln, dpf, pcam, dcf, dout, dol, w, h)


@pytest.mark.parametrize("kw", [dict(plane_tol=-0.01), dict(plane_tol=float("nan")), dict(normal_min=float("nan")),
                                dict(max_history=0.5), dict(max_history=float("nan")), dict(alias="rgba"),
                                dict(alias="len")])
def test_reproject_argument_checks(kw, rt, views, pt):
    w, h = 5, 3
    pcam, pfeat = views(w, h, EL0, AZ0)
    col, ln = _history(w, h, 3)
    out, ol = np.zeros_like(col), np.zeros_like(ln)
    kw = dict(kw)
    alias = kw.pop("alias", None)
    o_rgba, o_len = (col if alias == "rgba" else out), (ln if alias == "len" else ol)
    keep = col.copy(), ln.copy()
    with pytest.raises(pt._abi.RtError) as e:
        rt.reproject(col, ln, pfeat, pcam, pfeat, o_rgba, o_len, w, h, **kw)
    assert e.value.status == pt._abi.RT_ERR_ARG
    assert not out.any() and not ol.any()
    assert np.array_equal(bits(col), bits(keep[0])) and np.array_equal(bits(ln), bits(keep[1]))


@pytest.mark.parametrize("kw", [dict(n_cur=0.5), dict(n_cur=float("nan")), dict(max_history=0.0),
                                dict(max_history=float("nan"))])
def test_merge_argument_checks(kw, rt, pt):
    w, h = 5, 3
    col, ln = _history(w, h, 4)
    out, ol = np.zeros_like(col), np.zeros_like(ln)
    args = dict(n_cur=1.0, max_history=32.0)
    args.update(kw)
    with pytest.raises(pt._abi.RtError) as e:
        rt.temporalMerge(col, ln, col.copy(), args["n_cur"], out, ol, w, h, max_history=args["max_history"])
    assert e.value.status == pt._abi.RT_ERR_ARG
    assert not out.any() and not ol.any()


def test_identity(rt, views):
    """The same camera and the same features: every pixel that met a surface keeps its history, the
    length and a colour in [0, 1) to 1e-3.  The registration error is rounding (a few 1e-5 pixels,
    tests/test_temporal_host.py bounds it by 5e-3 at far larger frames), so an interpolated quantity
    moves by that times its neighbours' spread: lengths are drawn from [1, 4) to keep that product
    five times below the bound; registered one pixel off, random colours would differ by about 0.3
    and these lengths by about 1."""
    w, h = 64, 48
    cam, feat = views(w, h, EL0, AZ0)
    rng = np.random.default_rng(9)
    col = rng.random(w * h * 4, dtype=F)
    ln = (F(1.0) + rng.random(w * h, dtype=F) * F(3.0)).astype(F)
    out, ol = _gpu_reproject(rt, col, ln, feat, cam, feat, w, h)
    hit = fr.feature_ids(feat) != fr.RT_FEAT_NONE
    assert hit.all()  # the camera is inside the box
    assert (ol[hit] > 0).all()
    assert np.abs(ol - ln)[hit].max() <= 1e-3
    err = np.abs(out.reshape(-1, 4)[:, :3] - col.reshape(-1, 4)[:, :3])[hit].max()
    print(f"identity: colour error {err:.3e}, length error {np.abs(ol - ln)[hit].max():.3e}")
    assert err <= 1e-3
    assert not out[3::4].any()


def _project64(cam, P, w, h):
    c = np.asarray(cam, np.float64).reshape(4, 4)
    A = np.stack([c[0, :3], c[2, :3], c[1, :3]], axis=1)  # columns view, right, up
    sol = np.linalg.solve(A, (np.asarray(P, np.float64) - c[3, :3]).T).T
    s = sol[:, 0]
    return s, sol[:, 1] / s + w / 2 - 0.5, sol[:, 2] / s + h / 2 - 0.5


def test_disocclusion(rt, views):
    """After a +3 degree move: a box pixel whose place in the previous frame (float64, at least 0.05
    pixels from a change of taps) has all four taps on the mesh was hidden behind the mesh there, and
    gets no history."""
    w, h = 64, 48
    pcam, pfeat = views(w, h, EL0, AZ0)
    _, cfeat = views(w, h, EL0, AZ0 + 3.0)
    col, ln = _history(w, h, 21, zero_share=0.0)
    ln += F(0.5)
    out, ol = _gpu_reproject(rt, col, ln, pfeat, pcam, cfeat, w, h)
    cid, pid = fr.feature_ids(cfeat), fr.feature_ids(pfeat).reshape(h, w)
    s, fx, fy = _project64(pcam, cfeat.reshape(2, -1, 4)[0, :, :3], w, h)
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    stable = (np.abs(fx - np.round(fx)) >= 0.05) & (np.abs(fy - np.round(fy)) >= 0.05)
    sel = (cid == fr.RT_FEAT_BOX) & (s > 0) & stable & (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
    k = np.flatnonzero(sel)
    on_mesh = np.all([pid[y0[k] + j, x0[k] + i] >= 0 for j in (0, 1) for i in (0, 1)], axis=0)
    k = k[on_mesh]
    print(f"disocclusion: {k.size} box pixels behind the previous view's mesh")
    assert k.size >= 1
    assert not ol[k].any() and not out.reshape(-1, 4)[k].any()


def _cam128(pt, az, el=EL0):
    cam = pt.scenes.camera_spherical(64, target=TARGET, elevation=el, azimuth=az, distance=DIST)
    cam[0:4] *= 2
    return cam


def test_not_vacuous(rt, pt):
    """One +3 degree key press at 128 x 96: at least 0.9 of the pixels find history (0.9440 with the
    restatement over the oracle's features, evaluated on the CPU beforehand)."""
    w, h = 128, 96
    feats = []
    for az in (AZ0, AZ0 + 3.0):
        rt.setCamera(_cam128(pt, az))
        f = np.zeros(2 * w * h * 4, F)
        rt.renderFeatures(f, w, h, kernel=2)
        feats.append(f)
    col, ln = _history(w, h, 5, zero_share=0.0)
    ln += F(0.5)
    out, ol = _gpu_reproject(rt, col, ln, feats[0], _cam128(pt, AZ0), feats[1], w, h)
    share = float((ol > 0).mean())
    print(f"valid share after +3 degrees: {share:.4f}")
    assert share >= 0.9
    assert np.array_equal(bits(ol), bits(tr.reproject(col, ln, feats[0], _cam128(pt, AZ0), feats[1], w, h)[1]))


def test_render_state_untouched(pt, golden, golden_meta, views):
    """The golden progressive frames with reproject / merge calls in between — host buffers on the
    context's stream, device tensors on a side stream behind a render enqueued without a wait — are
    the frames, seeds, counter totals and render info of the sequence without those calls
    (tests/render_state.py); and the side-stream merge saw the frame of the render before it, not the
    one enqueued after it."""
    import torch

    with rs.untouched(pt, golden, golden_meta) as (t, frame, g, m):
        W, H = m["W"], m["H"]
        pcam, pfeat = views(W, H, EL0, AZ0)
        _, cfeat = views(W, H, EL0, AZ0 + 3.0)
        col, ln = _history(W, H, 13)
        car, cl = tr.reproject(col, ln, pfeat, pcam, cfeat, W, H)
        dcol, dln, dpf, dcf = (torch.from_numpy(a).cuda() for a in (col, ln, pfeat, cfeat))
        dcar, dcl = torch.zeros_like(dcol), torch.zeros_like(dln)
        merged = [(torch.zeros_like(dcol), torch.zeros_like(dln)) for _ in range(m["frames"])]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        host_out, host_len = np.zeros_like(col), np.zeros_like(ln)
        for p in range(m["frames"]):
            t.rayTrace(frame, W, H, p, kernel=2, sync=False)
            if p == 0:
                t.reproject(dcol, dln, dpf, pcam, dcf, dcar, dcl, W, H, stream=side.cuda_stream, sync=False)
            t.temporalMerge(dcar, dcl, frame, max(p, 1), merged[p][0], merged[p][1], W, H, stream=side.cuda_stream,
                            sync=False)
            if p == 1:  # and host buffers on the context's own stream
                t.reproject(col, ln, pfeat, pcam, cfeat, host_out, host_len, W, H)
                t.temporalMerge(host_out, host_len, g["frames"][0], 1.0, host_out, host_len, W, H)
    assert np.array_equal(bits(dcar.cpu().numpy()), bits(car)) and np.array_equal(bits(dcl.cpu().numpy()), bits(cl))
    for p in range(m["frames"]):
        exp, el = tr.merge(car, cl, g["frames"][p], max(p, 1))
        assert np.array_equal(bits(merged[p][0].cpu().numpy()), bits(exp)), f"merge behind frame {p}"
        assert np.array_equal(bits(merged[p][1].cpu().numpy()), bits(el))
    exp, el = tr.merge(car, cl, g["frames"][0], 1.0)
    assert np.array_equal(bits(host_out), bits(exp)) and np.array_equal(bits(host_len), bits(el))


@pytest.mark.parametrize("denoise", [False, True])
def test_progressive_view_temporal(denoise, rt, pt, tmp_path):
    """ProgressiveViewHIP::setTemporal through the rt_render CLI: two displays, a key press, one
    display, a key press, three displays.  The accumulation buffer of every displayed frame is that
    of the run without --temporal; every displayed frame is the recomposition of reproject /
    temporalMerge (/ denoise) through the Python API (tests/view_ref.py); the display differs from the
    run without --temporal from the second view on, and only there."""
    W, H = 64, 48
    px = W * H * 4
    events = "d,d,l,d,l,d,d,d"
    flags = vr.Flags(temporal=True, denoise=denoise)
    common = ["--mesh", "2000", "--events", events]
    off = vr.run_view(tmp_path, common + flags.without("temporal").cli(), ("shown",))
    on = vr.run_view(tmp_path, common + flags.cli())
    plain = vr.run_view(tmp_path, common, ("shown",)) if denoise else off
    assert plain["shown"].size == off["shown"].size == on["shown"].size == on["raw"].size == 6 * px and on["feat"].size == 12 * px
    assert np.array_equal(bits(on["raw"]), bits(plain["shown"]))
    # (view's azimuth, progression) of the six displayed frames: display() renders progression 0 only
    # after a (re)allocation; after a restart it counts on from 1, whose mix overwrites the buffer
    shown = [(AZ0, 0), (AZ0, 1), (AZ0 + 3.0, 1), (AZ0 + 6.0, 1), (AZ0 + 6.0, 2), (AZ0 + 6.0, 3)]
    assert [(l["azimuth"], l["progression"]) for l in on["lines"] if l.get("rendered")] == shown
    exp = vr.displayed(rt, pt.scenes, flags, events, on["raw"], on["feat"], W, H)
    assert len(exp.frames) == 6
    for k, disp in enumerate(exp.frames):
        got = on["shown"][px * k:px * (k + 1)]
        assert np.array_equal(bits(got), bits(disp)), f"displayed frame {k}"
        same = np.array_equal(bits(got), bits(off["shown"][px * k:px * (k + 1)]))
        assert same == (k < 2), f"displayed frame {k} against the run without --temporal"
    assert (exp.lengths[-1] > 3).mean() > 0.8  # three frames of this view, and what the two views before it left


def test_temporal_quality(rt, pt, golden_meta):
    """The golden view at 128 x 96 (camera[0:4] *= 2), an orbit of 12 views 2 degrees apart, 1 spp
    each, the history carried from view to view (cap 32); mean squared errors of the last view
    against a sampleRate-16 frame of it rendered from other seeds.  Evaluated beforehand with the
    restatements over the oracle's frames of exactly these inputs:
        1-spp frame 2.1977e-3, merged (unfiltered) 3.0344e-4: 7.24 times lower;
        a-trous alone 8.3248e-5 / 5.1573e-5 / 5.1154e-5 at 2 / 3 / 5 passes, merged then 3 passes
        2.8897e-5: 1.77 times below the best of them (merged then 2 passes: 3.5888e-5).
    The conditions, set in advance at half the measured gain and never below 1: the merged frame's
    error is at most 1 / 3.62 of the 1-spp frame's; merged then 3 passes is no worse than the best
    a-trous-alone frame (half of 1.77 is below 1)."""
    sc = pt.scenes
    W, H = 128, 96
    Wp, Hp = sc.padded_dims(W, H)
    depth = golden_meta["cases"][CASE]["max_depth"]
    rt.setSampleRate(1)
    rt.setMaxPathDepth(depth)
    rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp))
    hist = hl = pfeat = pcam = None
    for k in range(12):
        cam = _cam128(pt, AZ0 + 2.0 * k)
        rt.setCamera(cam)
        frame = np.zeros(W * H * 4, F)
        rt.rayTrace(frame, W, H, 0, kernel=2)
        feat = np.zeros(2 * W * H * 4, F)
        rt.renderFeatures(feat, W, H, kernel=2)
        car, cl = np.zeros(W * H * 4, F), np.zeros(W * H, F)
        if hist is not None:
            rt.reproject(hist, hl, pfeat, pcam, feat, car, cl, W, H)
        hist, hl = np.zeros(W * H * 4, F), np.zeros(W * H, F)
        rt.temporalMerge(car, cl, frame, 1.0, hist, hl, W, H)
        pfeat, pcam = feat, cam
    ref = np.zeros(W * H * 4, F)
    rt.setSampleRate(16)
    rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp, skip=12345))
    rt.rayTrace(ref, W, H, 0, kernel=2)
    rt.setSampleRate(1)

    def mse(a):
        d = a.reshape(-1, 4)[:, :3].astype(np.float64) - ref.reshape(-1, 4)[:, :3].astype(np.float64)
        return float((d * d).mean())

    def filtered(src, it):
        out = np.zeros_like(src)
        rt.denoise(src, feat, out, W, H, iterations=it)
        return out

    alone = {it: mse(filtered(frame, it)) for it in (2, 3, 5)}
    merged3 = mse(filtered(hist, 3))
    print(f"mse 1-spp {mse(frame):.4e} merged {mse(hist):.4e} ratio {mse(frame) / mse(hist):.2f}; a-trous alone "
          f"{alone}; merged then 3 passes {merged3:.4e} ratio {min(alone.values()) / merged3:.2f}")
    assert mse(hist) <= mse(frame) / 3.62
    assert merged3 <= min(alone.values())
