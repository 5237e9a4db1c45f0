"""GPU: the variance-guided display filter (rt_moments_accumulate, rt_variance, rt_denoise_var,
DESIGN.md §4.11) against its float32 numpy restatement (tests/variance_ref.py, the pinned exponential
through the oracle), bit for bit; its argument checks; that it leaves a render's state alone;
ProgressiveViewHIP::setVarianceGuided through the rt_render CLI; and its effect on a resting view.
Run on the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import pytest

import features_ref as fr
import render_state as rs
import variance_ref as vr
import view_ref
from conftest import bits

pytestmark = pytest.mark.gpu

CASE = "tris_64x48_sr1"
F = np.float32
W0, H0 = 64, 48
AZ0 = 105.0  # the golden view's azimuth, where the view starts
# (w, h) -> window origin in the golden view: the small windows straddle the mesh's silhouette
WINDOWS = {(1, 1): (20, 20), (5, 3): (8, 30), (37, 29): (3, 9), (64, 48): (0, 0)}
SIZES = list(WINDOWS)


@pytest.fixture(scope="module")
def view(pt, golden, golden_meta):
    """A tracer on the golden triangle view and its real feature buffer at 64 x 48."""
    g, m = golden(CASE), golden_meta["cases"][CASE]
    rt = pt.RayTracer(0)
    rt.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
    rt.setCamera(g["camera"])
    rt.setSampleRate(1)
    rt.setMaxPathDepth(m["max_depth"])
    rt.setMesh(g["verts"], g["idx"])
    feat = np.zeros(2 * W0 * H0 * 4, F)
    rt.renderFeatures(feat, W0, H0, kernel=2)
    ids = fr.feature_ids(feat)
    assert (ids >= 0).any() and (ids == fr.RT_FEAT_BOX).any()
    yield rt, feat
    rt.close()


def _colour(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(w * h * 4, dtype=F) * F(1.5)).astype(F)


def _lengths(w, h, seed, min_len):
    """History lengths mixing 0, 1, 2.5, exactly min_len and 40, every one present where the frame has
    five pixels."""
    vals = np.array([0.0, 1.0, 2.5, min_len, 40.0], F)
    ln = vals[np.arange(w * h) % 5]
    np.random.default_rng(seed).shuffle(ln)
    return ln


def _variance_plane(w, h, seed):
    """Variances up to 1e-2 with exact zeros: a fifth of the pixels, and a block of them (a 3 x 3
    neighbourhood of zeros: the prefiltered variance is 0 there)."""
    rng = np.random.default_rng(seed)
    v = (rng.random(w * h, dtype=F) * F(0.01)).astype(F)
    v[rng.random(w * h) < 0.2] = 0.0
    v.reshape(h, w)[:5, :6] = 0.0
    return v


def _features(feat, w, h):
    x0, y0 = WINDOWS[(w, h)]
    return fr.crop_features(feat, W0, H0, x0, y0, w, h)


# ---- moments ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 17])
@pytest.mark.parametrize("w,h", SIZES)
def test_moments_equal_numpy(w, h, n, view):
    """Host arrays and device tensors, apart and in place (mom_out is mom_in).  The accumulation after
    the frame is the float32 mix of the one before it with samples drawn from [-0.5, 1.5): a quarter
    of the recovered components are negative and count as 0.  With n = 1 the current frame (negative
    components among its own) is the sample, and the other two inputs may be None."""
    import torch

    rt, _ = view
    rng = np.random.default_rng(100 * w + n)
    prev = _colour(w, h, 7 * w + n)
    s = (rng.random(w * h * 4, dtype=F) * F(2.0) - F(0.5)).astype(F)
    cur = vr.mix(prev, s, n) if n > 1 else s
    mom = np.zeros(w * h * 4, F)
    mom[0::4] = rng.random(w * h, dtype=F)
    mom[1::4] = rng.random(w * h, dtype=F)
    exp = vr.moments(prev, cur, n, mom)
    with np.errstate(all="ignore"):
        rec = cur if n == 1 else prev + (cur - prev) * F(n)
    if w * h >= 15:
        assert (rec.reshape(-1, 4)[:, :3] < 0).any() and (rec.reshape(-1, 4)[:, :3] > 0).any()
    keep = prev.copy(), cur.copy(), mom.copy()
    out = np.full(w * h * 4, np.nan, F)
    rt.momentsAccumulate(prev, cur, n, mom, out, w, h)
    assert np.array_equal(bits(out), bits(exp))
    for a, b in zip((prev, cur, mom), keep):
        assert np.array_equal(bits(a), bits(b))  # the inputs are only read
    assert not out[2::4].any() and not out[3::4].any()
    m2 = mom.copy()
    rt.momentsAccumulate(prev, cur, n, m2, m2, w, h)
    assert np.array_equal(bits(m2), bits(exp))
    dprev, dcur, dmom = (torch.from_numpy(a).cuda() for a in (prev, cur, mom))
    dout = torch.zeros_like(dmom)
    rt.momentsAccumulate(dprev, dcur, n, dmom, dout, w, h)
    assert np.array_equal(bits(dout.cpu().numpy()), bits(exp))
    rt.momentsAccumulate(dprev, dcur, n, dmom, dmom, w, h)
    assert np.array_equal(bits(dmom.cpu().numpy()), bits(exp))
    assert np.array_equal(bits(dprev.cpu().numpy()), bits(prev)) and np.array_equal(bits(dcur.cpu().numpy()), bits(cur))
    if n == 1:
        out[:] = np.nan
        rt.momentsAccumulate(None, cur, 1, None, out, w, h)
        assert np.array_equal(bits(out), bits(exp))
    assert rt.lastVarianceMs("moments") > 0.0


# ---- variance --------------------------------------------------------------------------------

@pytest.mark.parametrize("min_len", [4.0, 2.0])
@pytest.mark.parametrize("w,h", SIZES)
def test_variance_equals_numpy(w, h, min_len, view, oracle):
    """Both estimates in one frame: lengths of 0, 1, 2.5, exactly min_len and 40; moments whose
    m2 - m1^2 is negative at some pixels (clamped); the spatial windows cross the frame's edges and
    the mesh's silhouette."""
    rt, feat = view
    f = _features(feat, w, h)
    rng = np.random.default_rng(int(10 * w + min_len))
    disp = _colour(w, h, 3 * w + 1)
    ln = _lengths(w, h, w, min_len)
    mom = np.zeros(w * h * 4, F)
    m1 = rng.random(w * h, dtype=F)
    mom[0::4] = m1
    mom[1::4] = m1 * m1 + (rng.random(w * h, dtype=F) * F(0.1) - F(0.02))
    keep = [a.copy() for a in (disp, mom, ln, f)]
    out = np.full(w * h, np.nan, F)
    rt.variance(disp, mom, ln, f, out, w, h, min_len=min_len)
    exp = vr.variance(oracle, disp, mom, ln, f, w, h, min_len=min_len)
    assert np.array_equal(bits(out), bits(exp))
    assert np.isfinite(out).all() and (out >= 0).all()
    for a, b in zip((disp, mom, ln, f), keep):
        assert np.array_equal(bits(a), bits(b))
    if w * h >= 5:
        assert {0.0, 1.0, 2.5, min_len, 40.0} == set(ln.tolist())
    if w * h >= 1000:
        assert (out[ln >= min_len] == 0).any() and (out[ln >= min_len] > 0).any()  # clamped temporal estimates, and others
    assert rt.lastVarianceMs("variance") > 0.0


def test_variance_device_tensors(view, oracle):
    import torch

    rt, feat = view
    w, h = 37, 29
    f = _features(feat, w, h)
    disp, ln = _colour(w, h, 5), _lengths(w, h, 5, 4.0)
    mom = _colour(w, h, 6)
    exp = vr.variance(oracle, disp, mom, ln, f, w, h, sigma_normal=0.5, sigma_plane=0.2)
    dd, dm, dl, df = (torch.from_numpy(a).cuda() for a in (disp, mom, ln, f))
    dout = torch.zeros_like(dl)
    rt.variance(dd, dm, dl, df, dout, w, h, sigma_normal=0.5, sigma_plane=0.2)
    assert np.array_equal(bits(dout.cpu().numpy()), bits(exp))
    with pytest.raises(ValueError):
        rt.variance(dd, mom, dl, df, dout, w, h)  # host and device buffers mixed


# ---- the filter ------------------------------------------------------------------------------

@pytest.mark.parametrize("it", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("w,h", SIZES)
def test_denoise_var_equals_numpy(w, h, it, view, oracle):
    """Random finite colours and a variance plane with exact zeros over real features: both outputs,
    the colour alone (out_var None), and in place (dst is src, dst_var is var), as host arrays and
    as device tensors."""
    import torch

    rt, feat = view
    f = _features(feat, w, h)
    col, var = _colour(w, h, 100 * w + it), _variance_plane(w, h, 50 * w + it)
    exp, ev = vr.denoise_var(oracle, col, var, f, w, h, iterations=it)
    src, v0 = col.copy(), var.copy()
    out, ov = np.full(w * h * 4, np.nan, F), np.full(w * h, np.nan, F)
    rt.denoiseVar(src, v0, f, out, ov, w, h, iterations=it)
    assert np.array_equal(bits(out), bits(exp))
    assert np.array_equal(bits(ov), bits(ev))
    assert np.array_equal(bits(src), bits(col)) and np.array_equal(bits(v0), bits(var))  # only read
    assert np.array_equal(out[3::4], col[3::4])  # alpha is copied
    assert rt.lastVarianceMs("denoise_var") > 0.0
    out[:] = np.nan
    rt.denoiseVar(src, v0, f, out, None, w, h, iterations=it)
    assert np.array_equal(bits(out), bits(exp))
    rt.denoiseVar(src, v0, f, src, v0, w, h, iterations=it)
    assert np.array_equal(bits(src), bits(exp)) and np.array_equal(bits(v0), bits(ev))
    dcol, dvar, dfeat = (torch.from_numpy(a).cuda() for a in (col, var, f))
    dout, dov = torch.zeros_like(dcol), torch.zeros_like(dvar)
    rt.denoiseVar(dcol, dvar, dfeat, dout, dov, w, h, iterations=it)
    assert np.array_equal(bits(dout.cpu().numpy()), bits(exp)) and np.array_equal(bits(dov.cpu().numpy()), bits(ev))
    assert np.array_equal(bits(dcol.cpu().numpy()), bits(col)) and np.array_equal(bits(dvar.cpu().numpy()), bits(var))
    dout.zero_()
    rt.denoiseVar(dcol, dvar, dfeat, dout, None, w, h, iterations=it)
    assert np.array_equal(bits(dout.cpu().numpy()), bits(exp))
    rt.denoiseVar(dcol, dvar, dfeat, dcol, dvar, w, h, iterations=it)
    assert np.array_equal(bits(dcol.cpu().numpy()), bits(exp)) and np.array_equal(bits(dvar.cpu().numpy()), bits(ev))


@pytest.mark.parametrize("lds_max", ["0", "1", "2"])
def test_denoise_var_kernel_forms_agree(lds_max, view, oracle, monkeypatch):
    """Steps 1 and 2 read their taps from a tile staged in LDS, the larger ones gather them from
    global memory (the default); RTMI_ATROUS_LDS moves the boundary for these kernels too (0: every
    step gathers).  Every choice gives the restatement's bits."""
    rt, feat = view
    monkeypatch.setenv("RTMI_ATROUS_LDS", lds_max)
    for w, h, it in [(37, 29, 3), (64, 48, 2)]:
        f = _features(feat, w, h)
        col, var = _colour(w, h, 31 + it), _variance_plane(w, h, 32 + it)
        out, ov = np.zeros_like(col), np.zeros_like(var)
        rt.denoiseVar(col, var, f, out, ov, w, h, iterations=it, sigma_lum=1.5)
        exp, ev = vr.denoise_var(oracle, col, var, f, w, h, iterations=it, sigma_lum=1.5)
        assert np.array_equal(bits(out), bits(exp)) and np.array_equal(bits(ov), bits(ev))


@pytest.mark.parametrize("it", [1, 3, 5])
def test_luminance_term_off_is_rt_denoise(it, view):
    """sigma_lum = +INFINITY: the colour is rt_denoise's with its colour term off, bit for bit."""
    rt, feat = view
    w, h = 37, 29
    f = _features(feat, w, h)
    col, var = _colour(w, h, 9 + it), _variance_plane(w, h, 10 + it)
    out, exp = np.zeros_like(col), np.zeros_like(col)
    rt.denoiseVar(col, var, f, out, None, w, h, iterations=it, sigma_lum=float("inf"))
    rt.denoise(col, f, exp, w, h, iterations=it, sigma_color=float("inf"))
    assert np.array_equal(bits(out), bits(exp)) and out.any()


@pytest.mark.parametrize("sigmas", [(4.0, np.inf, 0.1), (4.0, 0.3, np.inf), (0.5, 0.2, 0.3)])
def test_denoise_var_sigmas(sigmas, view, oracle):
    rt, feat = view
    w, h = 37, 29
    f = _features(feat, w, h)
    col, var = _colour(w, h, 7), _variance_plane(w, h, 8)
    out, ov = np.zeros_like(col), np.zeros_like(var)
    kw = dict(iterations=3, sigma_lum=sigmas[0], sigma_normal=sigmas[1], sigma_plane=sigmas[2])
    rt.denoiseVar(col, var, f, out, ov, w, h, **kw)
    exp, ev = vr.denoise_var(oracle, col, var, f, w, h, **kw)
    assert np.array_equal(bits(out), bits(exp)) and np.array_equal(bits(ov), bits(ev))


# ---- arguments -------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(iterations=0), dict(iterations=9), dict(sigma_lum=0.0), dict(sigma_lum=float("nan")),
                                dict(sigma_normal=-1.0), dict(sigma_normal=0.0), dict(sigma_plane=float("nan")),
                                dict(sigma_plane=-0.1)])
def test_denoise_var_argument_checks(kw, view, pt):
    rt, feat = view
    f = _features(feat, 5, 3)
    col, var = _colour(5, 3, 1), _variance_plane(5, 3, 2)
    out, ov = np.zeros_like(col), np.zeros_like(var)
    with pytest.raises(pt._abi.RtError) as e:
        rt.denoiseVar(col, var, f, out, ov, 5, 3, **kw)
    assert e.value.status == pt._abi.RT_ERR_ARG
    assert not out.any() and not ov.any()


@pytest.mark.parametrize("kw", [dict(min_len=1.5), dict(min_len=float("nan")), dict(sigma_normal=0.0),
                                dict(sigma_plane=float("nan"))])
def test_variance_argument_checks(kw, view, pt):
    rt, feat = view
    f = _features(feat, 5, 3)
    col, ln = _colour(5, 3, 1), _lengths(5, 3, 1, 4.0)
    out = np.zeros_like(ln)
    with pytest.raises(pt._abi.RtError) as e:
        rt.variance(col, col.copy(), ln, f, out, 5, 3, **kw)
    assert e.value.status == pt._abi.RT_ERR_ARG
    assert not out.any()


@pytest.mark.parametrize("case", ["n<1", "n nan", "out is cur", "out is prev", "no prev", "no moments"])
def test_moments_argument_checks(case, view, pt):
    rt, _ = view
    prev, cur, mom = _colour(5, 3, 1), _colour(5, 3, 2), _colour(5, 3, 3)
    out = np.zeros_like(mom)
    args = {"n<1": (prev, cur, 0.5, mom, out), "n nan": (prev, cur, float("nan"), mom, out),
            "out is cur": (prev, cur, 2.0, mom, cur), "out is prev": (prev, cur, 2.0, mom, prev),
            "no prev": (None, cur, 2.0, mom, out), "no moments": (prev, cur, 2.0, None, out)}[case]
    keep = prev.copy(), cur.copy()
    with pytest.raises(pt._abi.RtError) as e:
        rt.momentsAccumulate(*args, 5, 3)
    assert e.value.status == pt._abi.RT_ERR_ARG
    assert not out.any()
    assert np.array_equal(bits(prev), bits(keep[0])) and np.array_equal(bits(cur), bits(keep[1]))


def test_device_tensors_on_a_side_stream(view, oracle):
    """The three calls enqueued on a side stream without a wait, each reading what the one before it
    wrote."""
    import torch

    rt, feat = view
    w, h = 37, 29
    f = _features(feat, w, h)
    prev, s = _colour(w, h, 40), _colour(w, h, 41)
    cur = vr.mix(prev, s, 3)
    mom = np.zeros(w * h * 4, F)
    mom[0::4], mom[1::4] = 0.4, 0.3
    ln = _lengths(w, h, 42, 4.0)
    e_mom = vr.moments(prev, cur, 3, mom)
    e_var = vr.variance(oracle, cur, e_mom, ln, f, w, h)
    e_out, e_ov = vr.denoise_var(oracle, cur, e_var, f, w, h, iterations=3)
    dprev, dcur, dmom, dln, dfeat = (torch.from_numpy(a).cuda() for a in (prev, cur, mom, ln, f))
    dvar, dout = torch.zeros_like(dln), torch.zeros_like(dcur)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = side.cuda_stream
    rt.momentsAccumulate(dprev, dcur, 3, dmom, dmom, w, h, stream=st, sync=False)
    rt.variance(dcur, dmom, dln, dfeat, dvar, w, h, stream=st, sync=False)
    rt.denoiseVar(dcur, dvar, dfeat, dout, dvar, w, h, iterations=3, stream=st, sync=False)
    side.synchronize()
    assert np.array_equal(bits(dmom.cpu().numpy()), bits(e_mom))
    assert np.array_equal(bits(dout.cpu().numpy()), bits(e_out)) and np.array_equal(bits(dvar.cpu().numpy()), bits(e_ov))
    assert np.array_equal(bits(dcur.cpu().numpy()), bits(cur))


# ---- render state ----------------------------------------------------------------------------

def test_render_state_untouched(pt, golden, golden_meta, view, oracle):
    """The golden progressive frames with the three calls in between — device tensors on a side
    stream behind a render enqueued without a wait, host buffers on the context's stream — are the
    frames, seeds, counter totals and render info of the sequence without those calls
    (tests/render_state.py); and every side-stream call saw the frame of the render before it, not the
    one enqueued after it."""
    import torch

    _, feat = view
    with rs.untouched(pt, golden, golden_meta) as (t, frame, g, m):
        W, H, n_frames = m["W"], m["H"], m["frames"]
        frames = [np.ascontiguousarray(fm) for fm in g["frames"]]
        dfeat = torch.from_numpy(feat).cuda()
        dprevs = [torch.from_numpy(frames[max(p - 1, 0)]).cuda() for p in range(n_frames)]  # the buffer before frame p
        dmom = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
        dlens = [torch.full((W * H,), float(max(p, 1)), dtype=torch.float32, device="cuda:0") for p in range(n_frames)]
        dvars = [torch.zeros(W * H, dtype=torch.float32, device="cuda:0") for _ in range(n_frames)]
        douts = [torch.zeros_like(frame) for _ in range(n_frames)]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        st = side.cuda_stream
        h_mom, h_var, h_out = np.zeros(W * H * 4, F), np.zeros(W * H, F), np.zeros(W * H * 4, F)
        for p in range(n_frames):
            t.rayTrace(frame, W, H, p, kernel=2, sync=False)
            n = max(p, 1)
            t.momentsAccumulate(dprevs[p], frame, n, dmom, dmom, W, H, stream=st, sync=False)
            t.variance(frame, dmom, dlens[p], dfeat, dvars[p], W, H, min_len=2.0, stream=st, sync=False)
            t.denoiseVar(frame, dvars[p], dfeat, douts[p], None, W, H, stream=st, sync=False)
            if p == 1:  # and host buffers on the context's own stream
                t.momentsAccumulate(None, frames[0], 1, None, h_mom, W, H)
                t.variance(frames[0], h_mom, np.ones(W * H, F), feat, h_var, W, H)
                t.denoiseVar(frames[0], h_var, feat, h_out, None, W, H)
    mom = None
    for p in range(n_frames):
        n = max(p, 1)
        mom = vr.moments(frames[max(p - 1, 0)], frames[p], n, mom)
        var = vr.variance(oracle, frames[p], mom, np.full(W * H, n, F), feat, W, H, min_len=2.0)
        assert np.array_equal(bits(dvars[p].cpu().numpy()), bits(var)), f"variance behind frame {p}"
        exp = vr.denoise_var(oracle, frames[p], var, feat, W, H)[0]
        assert np.array_equal(bits(douts[p].cpu().numpy()), bits(exp)), f"filter behind frame {p}"
    assert np.array_equal(bits(dmom.cpu().numpy()), bits(mom))
    e_mom = vr.moments(None, frames[0], 1, None)
    e_var = vr.variance(oracle, frames[0], e_mom, np.ones(W * H, F), feat, W, H)
    assert np.array_equal(bits(h_mom), bits(e_mom)) and np.array_equal(bits(h_var), bits(e_var))
    assert np.array_equal(bits(h_out), bits(vr.denoise_var(oracle, frames[0], e_var, feat, W, H)[0]))


# ---- the view, through the CLI ---------------------------------------------------------------

@pytest.mark.parametrize("temporal", [False, True])
def test_progressive_view_variance_guided(temporal, view, pt, tmp_path):
    """ProgressiveViewHIP::setVarianceGuided through the rt_render CLI: three displays, a key press,
    two displays.  The accumulation buffer of every displayed frame is that of the run without the
    flag; every displayed frame is the recomposition of momentsAccumulate / (reproject / temporalMerge
    of colour and moments, with one plane of lengths /) variance / denoiseVar through the Python API
    (tests/view_ref.py); the display differs from the --denoise run's."""
    rt, _ = view
    W, H = 64, 48
    px = W * H * 4
    events = "d,d,d,l,d,d"
    flags = view_ref.Flags(variance_guided=True, temporal=temporal)
    common = ["--mesh", "2000", "--events", events]
    plain = view_ref.run_view(tmp_path, common, ("shown",))
    den = view_ref.run_view(tmp_path, common + replace(flags, variance_guided=False, denoise=True).cli(), ("shown",))
    on = view_ref.run_view(tmp_path, common + flags.cli())
    assert plain["shown"].size == den["shown"].size == on["shown"].size == on["raw"].size == 5 * px and on["feat"].size == 10 * px
    assert np.array_equal(bits(on["raw"]), bits(plain["shown"]))
    # (view's azimuth, progression) of the five displayed frames: display() renders progression 0 only
    # after a (re)allocation; after a restart it counts on from 1, whose mix overwrites the buffer
    shown = [(AZ0, 0), (AZ0, 1), (AZ0, 2), (AZ0 + 3.0, 1), (AZ0 + 3.0, 2)]
    assert [(l["azimuth"], l["progression"]) for l in on["lines"] if l.get("rendered")] == shown
    exp = view_ref.displayed(rt, pt.scenes, flags, events, on["raw"], on["feat"], W, H)
    assert len(exp.frames) == 5
    for k, out in enumerate(exp.frames):
        got = on["shown"][px * k:px * (k + 1)]
        assert np.array_equal(bits(got), bits(out)), f"displayed frame {k}"
        assert not np.array_equal(bits(got), bits(den["shown"][px * k:px * (k + 1)])), f"displayed frame {k} against --denoise"
    if temporal:
        assert (exp.lengths[-1] > 2).mean() > 0.8  # two frames of this view, and what the view before it left


# ---- quality ---------------------------------------------------------------------------------

def test_variance_guided_quality(pt, golden, golden_meta):
    """The golden view at 128 x 96 (camera[0:4] *= 2), 64 progressive 1-spp frames of it from the
    default seeds (progression 1..64), no camera move (the history length is n everywhere); mean
    squared errors against a sampleRate-32 (1024-spp) frame of the view rendered from other seeds, at
    n = 1, 4, 16 and 64.  Evaluated beforehand on the CPU with the restatements over the oracle's
    frames of exactly these inputs (rt_denoise's defaults; the variance-guided filter's defaults but
    for sigma_lum):

          n   accumulation  rt_denoise  sigma_lum 2   sigma_lum 4   sigma_lum 8
          1   1.9398e-3     4.4888e-5   8.5754e-5     5.3495e-5     4.3431e-5
          2   9.7942e-4     3.4280e-5   4.7110e-5     3.3183e-5     2.9863e-5
          4   4.6976e-4     3.1990e-5   4.9388e-5     2.5543e-5     2.5235e-5
         16   1.1550e-4     3.0578e-5   1.9594e-5     1.8386e-5     2.0906e-5
         64   3.1733e-5     3.1013e-5   1.0643e-5     1.4543e-5     1.8386e-5

    sigma_lum 4 reads 1.19 times rt_denoise at n = 1, above the 1.1 allowed for an early frame, so the
    test runs sigma_lum 8, the one of the three that meets every condition: 0.97 and 0.79 at n = 1 and
    4; at n = 64 its gain is 1.69 over rt_denoise and 1.73 over the accumulation.  The conditions, set
    from this table and not from the GPU: at n = 1 and 4 at most 1.1 times rt_denoise; at n = 16 at
    most rt_denoise; at n = 64 at most rt_denoise and at most the accumulation (half of either gain is
    below 1, and the divisor is never below 1)."""
    import torch

    g, m = golden(CASE), golden_meta["cases"][CASE]
    sc = pt.scenes
    W, H = 128, 96
    Wp, Hp = sc.padded_dims(W, H)
    cam = g["camera"].copy()
    cam[0:4] *= 2
    rt = pt.RayTracer(0)
    rt.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
    rt.setCamera(cam)
    rt.setMaxPathDepth(m["max_depth"])
    rt.setMesh(g["verts"], g["idx"])
    ref = np.zeros(W * H * 4, F)
    rt.setSampleRate(32)
    rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp, skip=12345))
    rt.rayTrace(ref, W, H, 0, kernel=2)
    rt.setSampleRate(1)
    rt.setSeeds(Wp, Hp, sc.default_seeds(Wp, Hp))

    def dev(n_floats):
        return torch.zeros(n_floats, dtype=torch.float32, device="cuda:0")

    feat, acc, prev, mom, var, out = dev(W * H * 8), dev(W * H * 4), dev(W * H * 4), dev(W * H * 4), dev(W * H), dev(W * H * 4)
    rt.renderFeatures(feat, W, H, kernel=2)

    def mse(a):
        d = a.cpu().numpy().reshape(-1, 4)[:, :3].astype(np.float64) - ref.reshape(-1, 4)[:, :3].astype(np.float64)
        return float((d * d).mean())

    got = {}
    for n in range(1, 65):
        prev.copy_(acc)
        torch.cuda.synchronize()
        rt.rayTrace(acc, W, H, n, kernel=2)
        rt.momentsAccumulate(prev, acc, n, mom, mom, W, H)
        if n in (1, 4, 16, 64):
            ln = torch.full((W * H,), float(n), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            rt.variance(acc, mom, ln, feat, var, W, H)
            rt.denoiseVar(acc, var, feat, out, None, W, H, sigma_lum=8.0)
            vg = mse(out)
            rt.denoise(acc, feat, out, W, H)
            got[n] = (mse(acc), mse(out), vg)
            print(f"n {n}: accumulation {got[n][0]:.4e} rt_denoise {got[n][1]:.4e} variance-guided {vg:.4e}")
    rt.close()
    for n in (1, 4):
        assert got[n][2] <= 1.1 * got[n][1], n
    assert got[16][2] <= got[16][1]
    assert got[64][2] <= got[64][1]
    assert got[64][2] <= got[64][0]
