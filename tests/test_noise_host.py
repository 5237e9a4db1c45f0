"""CPU: the noise meter — the new symbols and their defaults, and the properties of the
restatement tests/noise_ref.py that the GPU tests compare the kernels with."""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np

import noise_ref as nr
from conftest import ROOT

F = np.float32
U = np.uint32
NEW_SYMBOLS = ["rt_noise_defaults", "rt_noise_meter", "rt_noise_meter_async", "rt_last_noise_ms"]


def test_new_symbols_exported_and_bound(pt):
    lib = pt.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(pt._abi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (rt_\w+)", nm))
    for n in NEW_SYMBOLS:
        assert n in exported, f"librtmi.so does not export {n}"
        assert n in pt._abi.SIGNATURES, f"_abi.py does not bind {n}"
        assert getattr(lib, n).argtypes is not None
    for m in ("noiseMeter", "noiseDefaults", "lastNoiseMs"):
        assert callable(getattr(pt.RayTracer, m))


def test_defaults(pt):
    ab = pt._abi
    lib = pt.load_library()
    p = ab.RtNoiseParams(-1.0, -1.0, -1.0)
    assert lib.rt_noise_defaults(ctypes.byref(p)) == ab.RT_OK
    assert (F(p.percentile), F(p.threshold), F(p.lum_floor)) == (F(0.95), F(0.05), F(1e-3))
    assert lib.rt_noise_defaults(None) == ab.RT_ERR_ARG
    assert ctypes.sizeof(ab.RtNoiseParams) == 12 and ctypes.sizeof(ab.RtNoiseStats) == 16
    for k, v in nr.DEFAULTS.items():
        assert F(getattr(p, k)) == F(v)


def test_null_context_checks(pt):
    """The context entries refuse a null context before touching a device."""
    ab = pt._abi
    lib = pt.load_library()
    prm = ab.RtNoiseParams(0.95, 0.05, 1e-3)
    a, v, s = np.zeros(4, F), np.zeros(1, F), np.zeros(4, U)
    p = ab.ptr
    assert lib.rt_noise_meter(None, p(a), p(v), p(s), None, None, 1, 1, ctypes.byref(prm), 0) == ab.RT_ERR_ARG
    assert lib.rt_noise_meter_async(None, p(a), p(v), p(s), None, None, 1, 1, ctypes.byref(prm), 0, None) == ab.RT_ERR_ARG
    ms = ctypes.c_float()
    assert lib.rt_last_noise_ms(None, ctypes.byref(ms)) == ab.RT_ERR_ARG
    assert not s.any()


def test_bins_at_every_edge():
    """The lower edge of bin i is in bin i and the float below it in bin i - 1; 0, -0 and the subnormals
    are in bin 0, 2^8 upward and +inf in bin 383; the sign is dropped."""
    i = np.arange(nr.BINS, dtype=np.int64)
    edges = ((nr.BIN0 + i) << 19).astype(U)
    assert nr.bin_of(nr.f_bits(edges)).tolist() == i.tolist()
    assert nr.bin_of(nr.f_bits(edges - 1)).tolist() == [0] + i[:-1].tolist()
    assert nr.f_bits(edges[:1])[0] == F(2.0 ** -16) and nr.upper_edge(382) == F(2.0 ** 8 * 31 / 32)
    for k in range(nr.BINS - 1):
        assert nr.upper_edge(k) == nr.f_bits(edges[k + 1:k + 2])[0]
    assert nr.upper_edge(383) == F(np.inf)
    assert (nr.bin_of(np.array([0.0, -0.0, 1e-45, 1e-38, 2.0 ** -17], F)) == 0).all()
    assert (nr.bin_of(np.array([2.0 ** 8, 1e10, 3e38, np.inf], F)) == 383).all()
    assert nr.bin_of(np.array([-1.0], F))[0] == nr.bin_of(np.array([1.0], F))[0] == 256
    # the edges survive e = sqrt(fl(x x)) / (0 + 1): what the GPU test's constructed frames rely on
    x = nr.f_bits(np.concatenate([edges, edges - 1]))  # (from just under 2^-16 up: x x is normal)
    valid, e = nr.errors(np.zeros((x.size, 4), F), (x * x).astype(F), lum_floor=1.0)
    assert valid.all() and np.array_equal(e.view(U), x.view(U))


def test_validity():
    nan, inf = np.nan, np.inf
    rgba = np.array([[1, 1, 1, 1]] * 6 + [[nan, 1, 1, 1], [1, inf, 1, 1], [inf, -inf, 1, 1], [-1, -1, -1, 1], [1, 1, 1, nan]], F)
    var = np.array([0.0, -0.0, 1.0, -1.0, nan, inf, 1, 1, 1, 1, 1], F)
    valid, e = nr.errors(rgba, var, 1e-3)
    assert valid.tolist() == [True, True, True, False, False, False, False, False, False, True, True]
    assert e[9] == F(1.0) / F(1e-3)  # negative luminance: the floor alone
    assert e.view(U)[1] == 0x80000000 and not e[3:9].any()
    st = nr.stats(nr.histogram(valid, e), 11)
    assert (st["counted"], st["skipped"]) == (5, 6)


def test_level_bounds_the_percentile():
    """For random planes the level is above the sorted plane's element of rank r and at most 17/16 of it
    (the bin width: 16 bins an octave, each 1/16 of its octave's lower edge wide)."""
    rng = np.random.default_rng(3)
    for q in (0.5, 0.95, 1.0, 0.01):
        for k in range(8):
            n = int(rng.integers(1, 5000))
            e = np.exp(rng.normal(-4.0, 2.0, n)).astype(F).clip(2.0 ** -16, np.nextafter(F(256.0), F(0)))
            h = nr.histogram(np.ones(n, bool), e)
            st = nr.stats(h, n, percentile=q)
            x = np.sort(e)[nr.rank(q, n)]
            assert st["counted"] == n and x < st["level"] and np.float64(st["level"]) <= np.float64(x) * 17 / 16
    # below: whole bins at or under the threshold; on an edge, and on its float neighbours
    e = nr.f_bits(np.array([(nr.BIN0 + 100) << 19] * 3 + [((nr.BIN0 + 101) << 19)] * 2, U))
    h = nr.histogram(np.ones(5, bool), e)
    edge = nr.upper_edge(100)
    assert [nr.stats(h, 5, threshold=t)["below"] for t in (np.nextafter(edge, F(0)), edge, np.nextafter(edge, F(1)))] == [0, 3, 3]
    assert nr.stats(h, 5, threshold=nr.upper_edge(101))["below"] == 5
    assert nr.stats(np.zeros(nr.BINS, U), 7) == dict(level=F(0.0), counted=0, skipped=7, below=0)
    h = np.zeros(nr.BINS, U)
    h[383] = 1
    assert nr.stats(h, 1)["level"] == F(np.inf) and nr.stats(h, 1, threshold=3e38)["below"] == 0


def test_butterfly_mean_accuracy():
    """Six additions of half an ulp each and the division: within 7 * 2^-24 relative of the float64 mean."""
    rng = np.random.default_rng(4)
    a = np.exp(rng.normal(-3.0, 2.0, (2000, 64))).astype(F)
    a[:500] *= rng.random((500, 64)) < 0.3  # sparse tiles
    mean = (nr.butterfly_sum(a) / F(64.0)).astype(F)
    exact = a.astype(np.float64).mean(axis=1)
    assert (np.abs(mean - exact) <= 7 * 2.0 ** -24 * exact).all()
    assert np.array_equal(nr.butterfly_max(a), a.max(axis=1))
    # every lane ends with the sum's bits
    b = a.copy()
    for k in range(6):
        b = (b + b[:, np.arange(64) ^ (1 << k)]).astype(F)
    assert (b.view(U) == b.view(U)[:, :1]).all()


def test_partial_and_all_skipped_tiles():
    W, H = 11, 9  # tiles 2 x 2: a whole one, 3 x 8, 8 x 1, 3 x 1
    rng = np.random.default_rng(5)
    e = np.exp(rng.normal(-3.0, 1.0, W * H)).astype(F)
    valid = np.ones(W * H, bool)
    valid.reshape(H, W)[:, 8:] = False  # the right-hand tiles hold no valid pixel
    valid.reshape(H, W)[2, 3] = False
    e = np.where(valid, e, F(0.0)).astype(F)
    t = nr.tiles(valid, e, W, H).reshape(2, 2, 2)
    assert not t[:, 1].any()
    whole = e.reshape(H, W)[:8, :8]
    assert abs(t[0, 0, 0] - whole.astype(np.float64).sum() / 63) <= 7 * 2.0 ** -24 * t[0, 0, 0] and t[0, 0, 1] == whole.max()
    row = e.reshape(H, W)[8, :8]
    assert abs(t[1, 0, 0] - row.astype(np.float64).mean()) <= 7 * 2.0 ** -24 * t[1, 0, 0] and t[1, 0, 1] == row.max()


def test_converge_needs_events():
    exe = str(ROOT / "pathtracer.cl_amd" / "rt_render")
    r = subprocess.run([exe, "--width", "16", "--height", "8", "--converge", "0.1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--events" in r.stderr
    r = subprocess.run([exe, "--width", "16", "--height", "8", "--events", "d", "--noise-log", "x"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--converge" in r.stderr
