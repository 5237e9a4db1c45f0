"""rt_sincosf (one shared reduction) is bit-identical to rt_sinf / rt_cosf — the pinned
Cephes-style builtins of include/rt_math.h the parity model rests on.  Host build of the
header with the system C++ compiler (the device uses the same source)."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = r'''
#include <cstdio>
#include <cstring>
#include <cstdint>
#include "rt_math.h"
int main() {
    uint32_t bad = 0, n = 0;
    for (uint64_t k = 0; k < (1ull << 32); k += 4099) { /* strided over every float bit pattern */
        uint32_t u = (uint32_t)k; float x; std::memcpy(&x, &u, 4);
        float s, c; rt_sincosf(x, &s, &c);
        const float s2 = rt_sinf(x), c2 = rt_cosf(x);
        uint32_t a, b, d, e; std::memcpy(&a, &s, 4); std::memcpy(&b, &s2, 4); std::memcpy(&d, &c, 4); std::memcpy(&e, &c2, 4);
        if ((a != b && !(x != x)) || (d != e && !(x != x))) ++bad;
        ++n;
    }
    for (int i = -200000; i <= 200000; ++i) { /* dense around the sampling range 2 pi [0, 1) */
        const float x = (float)i * 1.0e-4f;
        float s, c; rt_sincosf(x, &s, &c);
        if (std::memcmp(&s, &(const float &)rt_sinf(x), 4) || std::memcmp(&c, &(const float &)rt_cosf(x), 4)) ++bad;
        ++n;
    }
    std::printf("%u %u\n", n, bad);
    return 0;
}
'''


def test_sincos_matches_sin_and_cos(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(SRC)
    exe = tmp_path / "t"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}", str(src), "-o",
                    str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=300).stdout.split()
    n, bad = int(out[0]), int(out[1])
    assert n > 1_000_000 and bad == 0


def _ulp_err(got: np.ndarray, exact: np.ndarray) -> np.ndarray:
    """|got - exact| in units of the binary32 ulp at the exact value (exact in binary64)."""
    ax = np.abs(exact)
    e = np.floor(np.log2(np.maximum(ax, np.finfo(np.float32).tiny)))
    return np.abs(got.astype(np.float64) - exact) / np.exp2(np.maximum(e, -126.0) - 23.0)


def _octant_switches() -> np.ndarray:
    """k pi / 4 rounded to float and its neighbours within 2 ulps, for every k with k pi / 4 < 8192."""
    k = np.arange(1, int(8192 * 4 / np.pi) + 1, dtype=np.float64)
    b = (k * (np.pi / 4)).astype(np.float32).view(np.uint32).astype(np.int64)
    x = (b[:, None] + np.arange(-2, 3)[None, :]).reshape(-1).astype(np.uint32).view(np.float32)
    return np.concatenate([x, -x])


def test_sin_cos_absolute_error_below_8192(oracle):
    """include/rt_math.h's first accuracy statement: for |x| < 8192 the absolute error of rt_sinf and
    rt_cosf (host build, against binary64) is at most 2^-23 — 2 ulps of a result in [0.5, 1).  It is
    not a bound in ulps of the result: near the zeros of sin / cos the error is ~100 ulps of the (tiny)
    result.  2^20 uniform arguments and every octant switch of the reduction."""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-8192, 8192, 1 << 20).astype(np.float32), _octant_switches()])
    x = x[np.abs(x) < 8192]
    x64 = x.astype(np.float64)
    worst = {}
    for fn, exact in (("sin", np.sin(x64)), ("cos", np.cos(x64)), ("sincos_s", np.sin(x64)), ("sincos_c", np.cos(x64))):
        worst[fn] = float(np.abs(oracle.math(fn, x).astype(np.float64) - exact).max())
    print("worst absolute error:", worst)
    assert max(worst.values()) <= 2.0 ** -23, worst


@pytest.mark.parametrize("fn", ["sin", "cos", "sincos_s", "sincos_c"])
def test_sin_cos_ulp_error_on_the_kernels_range(oracle, fn):
    """The second statement: on the kernels' own arguments phi = 2 pi k / 2^23 (every value frand can
    return, materials.h:21-35) the error is at most 2 ulps of the result, at every k.

    Measured (host build against binary64): sin 1.51 ulps, cos 1.47 ulps worst over all 2^23 arguments.
    With the reduction in binary32 alone, cos at the single argument k = 6291456 (r2 = 0.75,
    phi = 0x4096cbe4, the float next to 3 pi / 2) was 13.79 ulps off (1.1924868e-08 for 1.19248805e-08):
    the three Cody-Waite terms cancel down to their rounding error there.  rt_trig_reduce now redoes the
    reduction in binary64 where the binary32 result is below 2^-22; of the 2^23 arguments only that one
    changes its result."""
    r = (np.arange(1 << 23, dtype=np.float64) / (1 << 23)).astype(np.float32)
    phi = (np.float32(6.283185307) * r).astype(np.float32)
    p64 = phi.astype(np.float64)
    exact = np.sin(p64) if fn in ("sin", "sincos_s") else np.cos(p64)
    err = _ulp_err(oracle.math(fn, phi), exact)
    k = int(np.argmax(err))
    beyond = np.flatnonzero(err > 2.0)
    print(f"{fn}: worst {err[k]:.4f} ulp at k = {k} (phi bits {phi[k:k + 1].view(np.uint32)[0]:08x}); "
          f"{beyond.size} of {err.size} arguments beyond 2 ulps: k = {beyond[:8].tolist()}; "
          f"worst of the others {np.delete(err, beyond).max():.4f}")
    assert err[k] <= 2.0, (fn, k, float(err[k]))
