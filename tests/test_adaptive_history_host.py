"""CPU: adaptive sampling under the temporal stage — the new symbols and the checks that
need no device; the restatements (tests/adaptive_history_ref.py) against their scalar twins and on hand-made
planes; the CLI's refusals; and, over the oracle's frames, the precondition of the GPU view test: at the
first display after the key some tile stops on its history alone while others stay live."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

import adaptive_history_ref as ahr
import adaptive_ref as ar
import temporal_ref as tref
import trust_cases as tc
import trust_ref as tr
from conftest import ROOT, bits

F = np.float32
U = np.uint32
NEW_SYMBOLS = ["rt_temporal_merge_len", "rt_temporal_merge_len_async", "rt_history_trust_len", "rt_history_trust_len_async",
               "rt_tile_len_min", "rt_tile_len_min_async", "rt_last_tile_len_ms", "rt_tile_stop_select_frames",
               "rt_tile_stop_select_frames_async"]
# the GPU view test's configuration (tests/test_gpu_adaptive_history.py): tests/test_gpu_adaptive.py's view
RULE = dict(threshold=0.2, max_ratio=4.0, min_frames=4, dilate=0)
MIN_FRAMES = 4
CONVERGE = 0.001  # (the frame-wide rule never fires here)
EVENTS = ",".join(["d"] * 13 + ["l"] + ["d"] * 6)
FIRST = EVENTS.split(",").index("l")  # the displays before the key


def test_new_symbols_exported_and_bound(pt):
    lib = pt.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(pt._abi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_\w+)", nm))
    for n in NEW_SYMBOLS:
        assert n in exported, f"librtmi.so does not export {n}"
        assert n in pt._abi.SIGNATURES, f"_abi.py does not bind {n}"
        assert getattr(lib, n).argtypes is not None
    methods = ("temporalMergeLen", "historyTrustLen", "tileLenMin", "tileStopSelectFrames", "lastTileLenMs")
    for m in methods:
        assert callable(getattr(pt.RayTracer, m))
    hpp = (ROOT / "include" / "RayTracerHIP.hpp").read_text()
    for m in methods:
        assert re.search(rf"\b{m}\(", hpp), m
    view = (ROOT / "include" / "ProgressiveViewHIP.hpp").read_text()
    for m in ("setAdaptiveHistory", "adaptiveHistoryInEffect"):
        assert re.search(rf"\b{m}\(", view), m


def test_null_context_checks(pt):
    """The context entries refuse a null context before touching a device."""
    ab = pt._abi
    lib, p = pt.load_library(), ab.ptr
    a, ln, ft, tl, s, st = np.zeros(4, F), np.ones(1, F), np.zeros(8, F), np.zeros(2, F), np.zeros(1, U), np.zeros(4, U)
    trust, rule = ab.RtTrustParams(1.5, 0.3, 0.1), ab.RtAdaptiveParams(0.05, 4.0, 16, 1)
    merge = (p(a), p(ln), p(a.copy()), p(ln.copy()), 32.0, p(a.copy()), p(ln.copy()), 1, 1, 0)
    judge = (p(a), p(ln), p(a.copy()), p(ln.copy()), p(ft), p(ln.copy()), 1, 1, ctypes.byref(trust), 0)
    select = (p(tl), p(ln), p(s), 1, p(st), 1, 1, ctypes.byref(rule), 0)
    assert lib.rt_temporal_merge_len(None, *merge) == ab.RT_ERR_ARG and lib.rt_temporal_merge_len_async(None, *merge, None) == ab.RT_ERR_ARG
    assert lib.rt_history_trust_len(None, *judge) == ab.RT_ERR_ARG and lib.rt_history_trust_len_async(None, *judge, None) == ab.RT_ERR_ARG
    assert lib.rt_tile_len_min(None, p(ln), None, p(tl), 1, 1, 0) == ab.RT_ERR_ARG
    assert lib.rt_tile_len_min_async(None, p(ln), None, p(tl), 1, 1, 0, None) == ab.RT_ERR_ARG
    assert lib.rt_tile_stop_select_frames(None, *select) == ab.RT_ERR_ARG
    assert lib.rt_tile_stop_select_frames_async(None, *select, None) == ab.RT_ERR_ARG
    assert lib.rt_last_tile_len_ms(None, ctypes.byref(ctypes.c_float())) == ab.RT_ERR_ARG
    assert not st.any() and not s.any() and not tl.any()


# ---- the restatements against their scalar twins ------------------------------------------------------

def test_frames_clamp():
    got = ahr.frames(np.array([0.0, -0.0, 0.5, np.nan, 1.0, 1.5, 40.0, -3.0, np.inf, -np.inf], F))
    assert np.array_equal(bits(got), bits(np.array([1, 1, 1, 1, 1, 1.5, 40, 1, np.inf, 1], F)))


@pytest.mark.parametrize("n", [1.0, 2.0, 7.0, 40.0])
def test_constant_plane_is_the_scalar_merge(n):
    rng = np.random.default_rng(int(n))
    px = 37 * 29
    hist, cur = rng.random(4 * px).astype(F), rng.random(4 * px).astype(F)
    m = np.array([0.0, 1.0, 2.5, 31.5, 32.0], F)[rng.integers(0, 5, px)]
    for got, exp in zip(ahr.merge_len(hist, m, cur, np.full(px, n, F), 32.0), tref.merge(hist, m, cur, n, 32.0)):
        assert np.array_equal(bits(got), bits(exp))
    # a count under 1 is the scalar form's n = 1
    for low in (0.0, 0.5, np.nan):
        for got, exp in zip(ahr.merge_len(hist, m, cur, np.full(px, low, F), 32.0), tref.merge(hist, m, cur, 1.0, 32.0)):
            assert np.array_equal(bits(got), bits(exp))


def test_merge_by_hand():
    """n = 3 over m = 1: f = 3 / 4; no history: c's bits and l = n; the cap."""
    hist, cur = np.array([1, 1, 1, 9, 5, 5, 5, 9, 0, 0, 0, 9], F), np.array([5, 9, 1, 7, 2, 2, 2, 7, 4, 4, 4, 7], F)
    out, ln = ahr.merge_len(hist, np.array([1, 0, 30], F), cur, np.array([3, 0, 8], F), 32.0)
    assert out.tolist() == [4, 7, 1, 7, 2, 2, 2, 7] + [F(F(4) * F(F(8) / F(38)))] * 3 + [7] and ln.tolist() == [4, 1, 32]


@pytest.mark.parametrize("n", [1.0, 5.0])
def test_constant_plane_is_the_scalar_trust(oracle, n):
    w, h = 37, 29
    hist, m, cur, feat = tc.synthetic_inputs(w, h, 7)
    exp = tr.trust(oracle, hist, m, cur, n, feat, w, h)
    assert np.array_equal(bits(ahr.trust_len(oracle, hist, m, cur, np.full(w * h, n, F), feat, w, h)), bits(exp))
    assert (exp != m).any()  # (the test shortens some)
    stripes = np.where(np.arange(w * h) % w < 8, F(n), F(3.0 * n))  # another count elsewhere changes only what reads it
    got = ahr.trust_len(oracle, hist, m, cur, stripes, feat, w, h).reshape(h, w)
    assert np.array_equal(bits(got[:, :8]), bits(exp.reshape(h, w)[:, :8])) and (got[:, 8:] != exp.reshape(h, w)[:, 8:]).any()
    assert np.array_equal(bits(ahr.trust_len(oracle, hist, m, cur, stripes, feat, w, h, tolerance=np.inf)), bits(m))


def test_constant_frames_is_the_scalar_select():
    from test_gpu_adaptive import tile_maps

    rng = np.random.default_rng(3)
    for W, H, d in ((64, 48, 0), (37, 29, 1), (300, 200, 2)):
        n_t = ar.n_tiles(W, H)
        tiles = tile_maps(W, H, W)
        stop = ((rng.random(n_t) < 0.2) * rng.integers(1, 9, n_t)).astype(U)
        for n in (3, 4, 9):
            rule = dict(threshold=0.05, max_ratio=4.0, min_frames=4, dilate=d)
            got, st = ahr.select_frames(tiles, np.full(n_t, n, F), stop, n, W, H, **rule)
            exp, exp_st = ar.select(tiles, stop, n, W, H, **rule)
            assert np.array_equal(got, exp) and st == exp_st, (W, H, n)


def test_select_frames_by_hand():
    """The gate is the tile's: 3.99 and NaN do not pass, 4 and inf do; the word is n_frames, whatever the tile's
    frames; a gated tile holds its neighbours at dilate 1."""
    W, H = 40, 8
    tiles = np.full((5, 2), 0.01, F)
    frames = np.array([4.0, np.nextafter(F(4), F(0)), np.nan, np.inf, 32.0], F)
    rule = dict(threshold=0.05, max_ratio=4.0, min_frames=4)
    new, st = ahr.select_frames(tiles, frames, np.zeros(5, U), 1, W, H, dilate=0, **rule)
    assert new.tolist() == [1, 0, 0, 1, 1] and st == dict(tiles=5, active=2, stopped_now=3, frames=1)
    new, st = ahr.select_frames(tiles, frames, np.zeros(5, U), 1, W, H, dilate=1, **rule)
    assert new.tolist() == [0, 0, 0, 0, 1] and st["active"] == 4
    new, _ = ahr.select_frames(tiles, frames, np.array([0, 7, 7, 0, 0], U), 2, W, H, dilate=1, **rule)
    assert new.tolist() == [2, 7, 7, 2, 2]  # a stopped neighbour is settled, and keeps its word


# ---- the tile minimum on hand-made planes ---------------------------------------------------------------

def feat_with(ids):
    feat = np.zeros((2, ids.size, 4), F)
    feat[1, :, 3] = ids.astype(np.int32).reshape(-1).view(F)
    return feat.reshape(-1)


def test_tile_len_min_by_hand():
    W, H = 19, 10  # 3 x 2 tiles, the right column 3 wide, the upper row 2 high
    ln = np.full((H, W), 9.0, F)
    ids = np.full((H, W), 5, np.int32)
    ln[2, 3] = 4.0  # tile 0: an ordinary minimum
    ids[:8, 8:16] = -2  # tile 1: background only ...
    ln[1, 9] = 0.5  # ... whatever its lengths
    ln[7, 18], ln[7, 17] = 2.0, 1.5  # tile 2, partial: its own pixels only
    ln[8, 0], ln[9, 7] = np.nan, 6.0  # tile 3: a NaN reads 0
    ln[9, 12] = -3.0  # tile 4: a negative length reads 0
    ln[8, 16], ids[8, 16] = 1.0, -2  # tile 5: a background pixel does not count
    got = ahr.tile_len_min(ln, feat_with(ids), W, H)
    assert np.array_equal(bits(got), bits(np.array([4.0, np.inf, 1.5, 0.0, 0.0, 9.0], F)))
    assert ahr.tile_len_min(ln, None, W, H).tolist() == [4.0, 0.5, 1.5, 0.0, 0.0, 1.0]  # without features every pixel counts
    assert ahr.tile_len_min(np.array([7.0], F), None, 1, 1).tolist() == [7.0]


# ---- the CLI's refusals -----------------------------------------------------------------------------------

def test_cli_refusals():
    exe = str(ROOT / "pathtracer.cl_amd" / "rt_render")
    base = [exe, "--width", "16", "--height", "8", "--mesh", "100"]

    def refused(args, word):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (args, r.returncode, r.stderr)

    refused(["--events", "d", "--converge", "--temporal", "--adaptive-history"], "--adaptive-history needs --adaptive")
    refused(["--events", "d", "--converge", "--adaptive", "--adaptive-history"], "--adaptive-history needs --temporal")
    refused(["--events", "d", "--converge", "--adaptive-history"], "--adaptive-history needs")
    refused(["--events", "d", "--converge", "--adaptive", "--temporal"], "does not go with --temporal")  # today's refusal stays
    refused(["--events", "d", "--history-len-out", "x"], "--temporal")
    # the accepted combination parses: what is refused now is something else (--temporal without --events)
    refused(["--converge", "--adaptive", "--temporal", "--adaptive-history"], "--temporal needs --events")


# ---- the precondition of the GPU view test ----------------------------------------------------------------

def stopped_on_history(d):
    """Of a display's dict: the tiles stopped with a word under min_frames — their own accumulation was too
    short for the rule, their merged history was not — and the live ones."""
    return int(((d["stop"] != 0) & (d["stop"] < RULE["min_frames"])).sum()), int((d["stop"] == 0).sum())


def test_precondition_tiles_stop_on_history(pt, oracle, golden, golden_meta):
    """The view tests/test_gpu_adaptive_history.py runs through the CLI, over the oracle's frames: before the
    key it is the view without --temporal (no history: the merged frame is the accumulation buffer, a tile's
    length its own count); at the first display after the key, with one frame of its own, tiles the carried
    history covers stop at once with the word 1, and the disoccluded ones stay live."""
    seq = ahr.golden_view(pt, oracle, golden, golden_meta, EVENTS, CONVERGE, MIN_FRAMES, RULE)
    assert len(seq) == EVENTS.count("d") and not any(d["converged"] for d in seq)
    for d in seq[:FIRST]:
        assert np.array_equal(bits(d["shown"]), bits(d["acc"])) and np.array_equal(bits(d["length"]), bits(d["own"]))
        assert not d["stop"].any() or d["n"] >= RULE["min_frames"]
    assert [d["active"] for d in seq[4:FIRST]] == [17, 15, 13, 13, 13, 13, 12, 12, 11]  # tests/test_adaptive_host.py's
    after = seq[FIRST]
    early, live = stopped_on_history(after)
    print("after the key:", [stopped_on_history(d) for d in seq[FIRST:]], "tile frames:", np.sort(after["tile_frames"]))
    assert after["n"] == 1 and (after["stop"][after["stop"] != 0] == 1).all()
    assert early >= 1 and live >= 1
    assert (after["tile_frames"][after["stop"] != 0] >= RULE["min_frames"]).all()
    assert (after["own"][ar.pixel_mask(after["stop"], 64, 48)] == 1).all()
