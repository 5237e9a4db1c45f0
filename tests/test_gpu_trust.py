"""GPU: lag-adaptive trust of the carried display history.  rt_history_trust against
its float32 numpy restatement (tests/trust_ref.py), bit for bit, on the golden frames and on a
synthetic one; that the call leaves a render's state alone; ProgressiveViewHIP::setHistoryTrust and
sceneChanged through the rt_render CLI; that the test is not vacuous; and its effect on the three
experiments of tests/trust_cases.py, whose figures tests/test_trust_host.py measured on the CPU.  Run on
the MI355X box with `pytest -m gpu`."""
from __future__ import annotations

import ctypes
from dataclasses import replace

import numpy as np
import pytest

import render_state as rs
import trust_cases as tc
import trust_ref as tref
import view_ref as vr
from conftest import bits
from test_trust_host import EXPECTED, GAIN_B, R_AT_REST

pytestmark = pytest.mark.gpu

CASE = "tris_64x48_sr1"
F = np.float32
W0, H0 = tc.W0, tc.H0
TOL = 1.5  # rt_trust_defaults


@pytest.fixture(scope="module")
def view(pt, golden, golden_meta):
    """A tracer on the golden triangle view and its feature buffer at 64 x 48."""
    g, m = golden(CASE), golden_meta["cases"][CASE]
    rt = pt.RayTracer(0)
    rt.setSpheres(g["spheres"].view(pt._abi.SPHERE_DTYPE))
    rt.setCamera(g["camera"])
    rt.setSampleRate(1)
    rt.setMaxPathDepth(m["max_depth"])
    rt.setMesh(g["verts"], g["idx"])
    feat = np.zeros(2 * W0 * H0 * 4, F)
    rt.renderFeatures(feat, W0, H0, kernel=2)
    yield rt, feat, g
    rt.close()


@pytest.mark.parametrize("n_cur", [1.0, 5.0])
@pytest.mark.parametrize("source", ["golden", "synthetic"])
@pytest.mark.parametrize("w,h", list(tc.WINDOWS))
def test_trust_equals_numpy(w, h, source, n_cur, view, oracle):
    """Host arrays and device tensors, apart and in place (out_len is hist_len); the inputs are only
    read.  (33, 9) lies one pixel beyond a block's edge in both directions: the halo crosses a tile
    both ways; (64, 48) has 2 x 6 blocks."""
    import torch

    rt, feat0, g = view
    hist, ln, cur, feat = tc.golden_inputs(g, feat0, w, h) if source == "golden" else tc.synthetic_inputs(w, h, 100 * w + h)
    exp = tref.trust(oracle, hist, ln, cur, n_cur, feat, w, h, tolerance=TOL)
    keep = [a.copy() for a in (hist, ln, cur, feat)]
    out = np.full(w * h, np.nan, F)
    rt.historyTrust(hist, ln, cur, n_cur, feat, out, w, h)  # the default tolerance
    assert np.array_equal(bits(out), bits(exp))
    for a, b in zip((hist, ln, cur, feat), keep):
        assert np.array_equal(bits(a), bits(b))
    assert rt.lastTrustMs() > 0.0
    inplace = ln.copy()
    rt.historyTrust(hist, inplace, cur, n_cur, feat, inplace, w, h, tolerance=TOL)
    assert np.array_equal(bits(inplace), bits(exp))
    dhist, dln, dcur, dfeat = (torch.from_numpy(a).cuda() for a in (hist, ln, cur, feat))
    dout = torch.full_like(dln, float("nan"))
    rt.historyTrust(dhist, dln, dcur, n_cur, dfeat, dout, w, h, tolerance=TOL)
    assert np.array_equal(bits(dout.cpu().numpy()), bits(exp))
    for d, b in zip((dhist, dln, dcur, dfeat), keep):
        assert np.array_equal(bits(d.cpu().numpy()), bits(b))
    rt.historyTrust(dhist, dln, dcur, n_cur, dfeat, dln, w, h, tolerance=TOL)
    assert np.array_equal(bits(dln.cpu().numpy()), bits(exp))
    with pytest.raises(ValueError):
        rt.historyTrust(hist, ln, dcur, n_cur, feat, out, w, h)  # host and device buffers mixed
    # another tolerance, and everything trusted: hist_len's bits, NaN and negative lengths among them
    out[:] = np.nan
    rt.historyTrust(hist, ln, cur, n_cur, feat, out, w, h, tolerance=0.5)
    assert np.array_equal(bits(out), bits(tref.trust(oracle, hist, ln, cur, n_cur, feat, w, h, tolerance=0.5)))
    odd = ln.copy()
    odd[::3] = np.array([np.nan, -2.0, 1e30], F)[np.arange(len(odd[::3])) % 3]
    out[:] = 7.0
    rt.historyTrust(hist, odd, cur, n_cur, feat, out, w, h, tolerance=np.inf)
    assert np.array_equal(bits(out), bits(odd))
    if (w, h) == (64, 48):  # both outcomes are there
        has = ln > 0
        assert (exp[has] < ln[has]).sum() >= 30 and (exp[has] == ln[has]).sum() >= 30 and (ln == 0).sum() >= 30


def test_argument_checks(pt, view):
    ab = pt._abi
    rt, feat0, g = view
    w, h = 5, 3
    hist, ln, cur, feat = tc.golden_inputs(g, feat0, w, h)
    out = np.zeros(w * h, F)
    lib, p = rt._lib, ab.ptr

    def call(hist_=hist, ln_=ln, cur_=cur, n=1.0, feat_=feat, out_=out, w_=w, h_=h, prm=(1.5, 0.3, 0.1), flags=0):
        pr = ab.RtTrustParams(*(prm or (1.5, 0.3, 0.1)))
        return lib.rt_history_trust(rt._h, p(hist_), p(ln_), p(cur_), n, p(feat_), p(out_), w_, h_,
                                    ctypes.byref(pr) if prm else None, flags)

    assert call() == ab.RT_OK
    out[:] = 0.0
    for kw in (dict(hist_=None), dict(ln_=None), dict(cur_=None), dict(feat_=None), dict(out_=None), dict(prm=None),
               dict(w_=0), dict(h_=0), dict(flags=2), dict(n=0.5), dict(n=float("nan")),
               dict(prm=(0.0, 0.3, 0.1)), dict(prm=(-1.0, 0.3, 0.1)), dict(prm=(float("nan"), 0.3, 0.1)),
               dict(prm=(1.5, 0.0, 0.1)), dict(prm=(1.5, 0.3, float("nan"))), dict(prm=(1.5, 0.3, -0.1)),
               dict(out_=cur), dict(out_=hist)):
        assert call(**kw) == ab.RT_ERR_ARG, kw
    assert not out.any()
    t = pt.RayTracer(0)
    try:
        ms = ctypes.c_float()
        assert t._lib.rt_last_trust_ms(t._h, ctypes.byref(ms)) == ab.RT_ERR_STATE
        assert t._lib.rt_last_trust_ms(t._h, None) == ab.RT_ERR_ARG
    finally:
        t.close()


def test_render_state_untouched(pt, golden, golden_meta, oracle):
    """The golden progressive frames with rt_history_trust in between — device tensors on a side stream
    behind a render enqueued without a wait, host buffers on the context's stream — are the frames,
    seeds, counter totals, render info and rt_read of the sequence without it (tests/render_state.py)."""
    import torch

    with rs.untouched(pt, golden, golden_meta) as (t, frame, g, m):
        W, H = m["W"], m["H"]
        feat0 = np.zeros(2 * W * H * 4, F)
        t.renderFeatures(feat0, W, H, kernel=2)
        hist, ln, cur, feat = tc.golden_inputs(g, feat0, W, H)
        exp = tref.trust(oracle, hist, ln, cur, 2.0, feat, W, H, tolerance=TOL)
        dhist, dln, dcur, dfeat = (torch.from_numpy(a).cuda() for a in (hist, ln, cur, feat))
        douts = [torch.zeros_like(dln) for _ in range(m["frames"])]
        host_out = np.zeros_like(ln)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        for p in range(m["frames"]):
            t.rayTrace(frame, W, H, p, kernel=2, sync=False)
            t.historyTrust(dhist, dln, dcur, 2.0, dfeat, douts[p], W, H, stream=side.cuda_stream, sync=False)
            if p == 1:  # and host buffers on the context's own stream
                t.historyTrust(hist, ln, cur, 2.0, feat, host_out, W, H)
    for d in douts:
        assert np.array_equal(bits(d.cpu().numpy()), bits(exp))
    assert np.array_equal(bits(host_out), bits(exp))


# ---- ProgressiveViewHIP through rt_render --events ----------------------------------------------

EV_PLAIN = "d,d,l,d,d"             # displayed: progression 0, 1, then the new view's 1, 2
EV_LIGHT = "d,d,e:0.4:0:0,d,d"     # the light moves by 0.4 in x between the second and the third display
PROGRESSION = [0, 1, 1, 2]


def _run(tmp_path, events, flags):
    run = vr.run_view(tmp_path, ["--mesh", "2000", "--events", events] + flags.cli())
    assert [l["progression"] for l in run["lines"] if l.get("rendered")] == PROGRESSION
    return run


class _RestatedTrust:
    """A tracer whose historyTrust is the restatement of rt_history_trust; it counts, call by call, the
    pixels whose history that shortened."""

    def __init__(self, rt, oracle):
        self.rt, self.oracle, self.shortened = rt, oracle, []

    def __getattr__(self, name):
        return getattr(self.rt, name)

    def historyTrust(self, car, cl, cur, n, feat, out, w, h, tolerance):
        out[:] = tref.trust(self.oracle, car, cl, cur, n, feat, w, h, tolerance=tolerance)
        self.shortened.append(int((out < cl).sum()))


@pytest.mark.parametrize("denoise", [False, True])
def test_progressive_view_history_trust(denoise, view, pt, oracle, tmp_path):
    """Without the new flag nothing changes: --history-trust inf displays the frames of --temporal alone
    bit for bit (no light move: sceneChanged itself treats the history differently).  Across a light
    move, --temporal alone drops the history (sceneChanged), --history-trust keeps and judges it: every
    displayed frame of both runs is the recomposition of reproject / the restatement of rt_history_trust
    / temporalMerge (/ denoise) (tests/view_ref.py), the accumulation buffers of both runs are the same,
    and the runs differ exactly from the first display after the move on."""
    W, H = 64, 48
    px = W * H * 4
    base = vr.Flags(temporal=True, denoise=denoise)
    plain = _run(tmp_path, EV_PLAIN, base)
    allin = _run(tmp_path, EV_PLAIN, replace(base, history_trust=True, tolerance=float("inf")))
    assert plain["shown"].size == 4 * px
    for k in ("shown", "raw", "feat"):
        assert np.array_equal(bits(plain[k]), bits(allin[k])), k
    variants = {"off": base, "on": replace(base, history_trust=True, tolerance=TOL)}
    runs = {name: _run(tmp_path, EV_LIGHT, fl) for name, fl in variants.items()}
    on, off = runs["on"], runs["off"]
    assert on["shown"].size == off["shown"].size == 4 * px and on["feat"].size == 8 * px
    assert np.array_equal(bits(on["raw"]), bits(off["raw"])) and np.array_equal(bits(on["feat"]), bits(off["feat"]))
    moved = [l for l in on["lines"] if l.get("event", "").startswith("e:")]
    assert len(moved) == 1 and moved[0]["progression"] == 0 and not moved[0]["rendered"]
    assert not np.array_equal(bits(on["raw"][px:2 * px]), bits(on["raw"][2 * px:3 * px]))  # the light did move
    rt = _RestatedTrust(view[0], oracle)
    for name, run in runs.items():
        exp = vr.displayed(rt, pt.scenes, variants[name], EV_LIGHT, run["raw"], run["feat"], W, H)
        assert len(exp.frames) == 4
        for k, disp in enumerate(exp.frames):
            assert np.array_equal(bits(run["shown"][px * k:px * (k + 1)]), bits(disp)), f"{name}: displayed frame {k}"
    # judged at every display that has a history, the three after the first, and only with the flag;
    # the test did shorten histories in the frames after the move
    assert len(rt.shortened) == 3 and sum(rt.shortened[1:]) > 100
    for k in range(4):
        same = np.array_equal(bits(on["shown"][px * k:px * (k + 1)]), bits(off["shown"][px * k:px * (k + 1)]))
        assert same == (k < 2), f"displayed frame {k} against the run without --history-trust"


def test_progressive_view_moments_take_the_trusted_length(tmp_path):
    """With --variance-guided the moments are merged by the same plane as the colour: --history-trust inf
    displays the frames of the run without the flag bit for bit, and across the light move a finite
    tolerance changes what is displayed from the first display after the move on."""
    px = 64 * 48 * 4
    vg = vr.Flags(temporal=True, variance_guided=True)
    trust_all = replace(vg, history_trust=True, tolerance=float("inf"))
    plain = _run(tmp_path, EV_PLAIN, vg)
    allin = _run(tmp_path, EV_PLAIN, trust_all)
    assert plain["shown"].size == 4 * px and np.array_equal(bits(plain["shown"]), bits(allin["shown"]))
    kept = _run(tmp_path, EV_LIGHT, trust_all)
    on = _run(tmp_path, EV_LIGHT, replace(trust_all, tolerance=TOL))
    assert np.array_equal(bits(on["raw"]), bits(kept["raw"])) and np.isfinite(on["shown"]).all()
    for k in range(4):
        same = np.array_equal(bits(on["shown"][px * k:px * (k + 1)]), bits(kept["shown"][px * k:px * (k + 1)]))
        assert same == (k < 2), f"displayed frame {k} against the run that trusts everything"


# ---- the experiments ------------------------------------------------------------------------------

class GpuBackend:
    """tests/trust_cases.py's experiments on the device: frames, features and every display stage."""

    def __init__(self, pt):
        self.pt, self.sc = pt, pt.scenes
        self.cam = tc.camera(self.sc)
        self.Wp, self.Hp = self.sc.padded_dims(tc.W, tc.H)
        self.rt = pt.RayTracer(0)
        self.warped = {}

    def close(self):
        self.rt.close()

    def frames(self, scenes, idx):
        rt, W, H = self.rt, tc.W, tc.H
        rt.setSpheres(scenes[0][0])
        rt.setCamera(self.cam)
        rt.setSampleRate(1)
        rt.setMaxPathDepth(6)
        rt.setMesh(scenes[0][1], idx)
        rt.setSeeds(self.Wp, self.Hp, self.sc.default_seeds(self.Wp, self.Hp))
        out = []
        for k, (S, v) in enumerate(scenes):
            if k:
                rt.setSpheres(S)
                if v is not scenes[k - 1][1]:
                    rt.updateMesh(v)
            frame, feat = np.zeros(W * H * 4, F), np.zeros(2 * W * H * 4, F)
            rt.rayTrace(frame, W, H, 0, kernel=2)
            rt.renderFeatures(feat, W, H, kernel=2)
            out.append((frame, feat))
        ref = np.zeros(W * H * 4, F)
        rt.setSampleRate(16)
        rt.setSeeds(self.Wp, self.Hp, self.sc.default_seeds(self.Wp, self.Hp, skip=12345))
        rt.rayTrace(ref, W, H, 0, kernel=2)
        return out, ref

    def warp(self, feat, idx, cur, prev):
        # the tracer is in the last pose by now: the warp reads the current pose from it (once per
        # frame: both chains of an experiment warp the same features)
        if id(feat) not in self.warped:
            self.rt.updateMesh(cur)
            out = np.zeros_like(feat)
            self.rt.warpFeatures(feat, prev, out, tc.W, tc.H)
            self.warped[id(feat)] = (feat, out)
        return self.warped[id(feat)][1]

    def reproject(self, hist, hl, pfeat, cfeat):
        car, cl = np.zeros(tc.W * tc.H * 4, F), np.zeros(tc.W * tc.H, F)
        self.rt.reproject(hist, hl, pfeat, self.cam, cfeat, car, cl, tc.W, tc.H, max_history=tc.CARRY_CAP)
        return car, cl

    def trust(self, car, cl, frame, n, feat, tol):
        out = np.zeros(tc.W * tc.H, F)
        self.rt.historyTrust(car, cl, frame, n, feat, out, tc.W, tc.H, tolerance=tol)
        return out

    def merge(self, car, cl, frame, n):
        hist, hl = np.zeros(tc.W * tc.H * 4, F), np.zeros(tc.W * tc.H, F)
        self.rt.temporalMerge(car, cl, frame, n, hist, hl, tc.W, tc.H, max_history=tc.MERGE_CAP)
        return hist, hl

    def atrous(self, src, feat, it):
        out = np.zeros_like(src)
        self.rt.denoise(src, feat, out, tc.W, tc.H, iterations=it)
        return out


@pytest.fixture(scope="module")
def figures(pt):
    """Each experiment once, shared by the tests below."""
    be = GpuBackend(pt)
    cache = {}

    def get(which):
        if which not in cache:
            cache[which] = r = tc.evaluate(be, which, (TOL,))
            print(f"{which}: a-trous alone {r['alone']}; untrusted merged {r['merged'][None]:.4e} +3 {r['merged3'][None]:.4e}; "
                  f"trusted merged {r['merged'][TOL]:.4e} +3 {r['merged3'][TOL]:.4e}; mesh pixels merged "
                  f"{r['mesh_merged'][None]:.4e} -> {r['mesh_merged'][TOL]:.4e}; cut {r['cut'][TOL]:.4f}")
        return cache[which]

    yield get
    be.close()


def test_not_vacuous(figures):
    """The share of pixels whose trusted length is below half the carried one in the last frame: where
    the light moves (B) at least half of what the CPU evaluation measured (0.5317), where nothing moves
    (A) at most twice what it measured (0.0083)."""
    a, b = figures("A")["cut"][TOL], figures("B")["cut"][TOL]
    print(f"share of pixels cut below half their length: A {a:.4f}, B {b:.4f}")
    assert b >= EXPECTED["B"]["cut"] / 2.0
    assert a <= 2.0 * EXPECTED["A"]["cut"]


@pytest.mark.parametrize("which", "ABC")
def test_trust_quality(which, figures):
    """The device gives the CPU evaluation's figures (tests/test_trust_host.py: identical inputs and
    arithmetic), and the conditions set in advance from them, at half the measured gain and never below
    1.  A, nothing moves: trusted +3 2.605e-5 against a-trous alone 5.994e-5 and untrusted +3 2.525e-5 —
    the price at rest is R = 1.032, the condition 1 + 2 (R - 1) = 1.063.  B, the light moves: trusted +3
    8.510e-5 against untrusted +3 1.831e-4 (2.15 times lower; the condition: 1.076 times) and a-trous
    alone 9.124e-5.  C, the mesh turns: on the mesh pixels the merged frame 7.271e-6 trusted against
    1.132e-5 untrusted; the whole frame +3 3.048e-5 against the best a-trous-alone frame 5.348e-5."""
    r, e = figures(which), EXPECTED[which]
    assert r["alone3"] == pytest.approx(e["alone3"], rel=2e-3)
    assert r["merged3"][None] == pytest.approx(e["untrusted3"], rel=2e-3)
    assert r["merged3"][TOL] == pytest.approx(e["trusted3"], rel=2e-3)
    if which == "A":
        assert r["merged3"][TOL] <= r["alone3"]
        assert r["merged3"][TOL] <= (1.0 + 2.0 * (R_AT_REST - 1.0)) * r["merged3"][None]
    if which == "B":
        assert r["merged3"][TOL] <= r["merged3"][None] / max(GAIN_B / 2.0, 1.0)
        assert r["merged3"][TOL] <= r["alone3"]
    if which == "C":
        assert r["mesh_merged"][TOL] <= r["mesh_merged"][None]
        assert r["merged3"][TOL] <= min(r["alone"].values())
