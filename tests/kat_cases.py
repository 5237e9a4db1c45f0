"""Inputs of the per-function device tests (tests/test_gpu_device_kat.py) and of their CPU
counterpart (tests/test_device_kat_host.py): deterministic generators, one per function family.

A case is a `Case`: the method of tests/devkat.py to call, its arguments, and `nan_ok` — which
elements may legitimately give a NaN (decided here from the inputs, never from a result: a NaN or
infinite argument, a negative argument of log / sqrt, 0/0, ...).  Everywhere else neither the
host nor the device may produce a NaN.  `row(i)` names the i-th input as hex bits for a failure
message.  Not a test file."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

f32 = np.float32
RT_SMALL_F = f32(1e-4)
BOX = (f32(6.0), f32(5.0), f32(6.0))


@dataclass
class Case:
    name: str          # the device function under test
    method: str        # method of devkat.Device / devkat.Host
    args: tuple        # its arguments (element-wise arrays first dimension n, or scalars)
    n: int             # number of elements
    nan_ok: np.ndarray | None = None      # per element: a NaN result is defined behaviour
    per_elem: tuple = ()                  # indices into args of the element-wise arrays
    note: str = ""
    extra: dict = field(default_factory=dict)

    def subset(self, idx) -> "Case":
        """The same case on the elements idx (for the n = 1 / n % 256 != 0 guard runs)."""
        idx = np.asarray(idx)
        args = tuple(np.ascontiguousarray(a[idx]) if i in self.per_elem else a for i, a in enumerate(self.args))
        nk = None if self.nan_ok is None else self.nan_ok[idx]
        return Case(self.name, self.method, args, len(idx), nk, self.per_elem, self.note)

    def row(self, i) -> str:
        parts = []
        for k in self.per_elem:
            a = np.ascontiguousarray(self.args[k][i:i + 1])
            parts.append("[" + " ".join(f"{w:08x}" for w in a.view(np.uint8).view("<u4").reshape(-1)) + "]")
        return " ".join(parts)


def u2f(u) -> np.ndarray:
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def f2u(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def ulps(x, lo=-4, hi=4) -> np.ndarray:
    """The floats lo..hi ulps from each (finite, non-zero) x, same sign."""
    b = f2u(np.atleast_1d(f32(x))).astype(np.int64)
    return u2f((b[:, None] + np.arange(lo, hi + 1)[None, :]).reshape(-1).astype(np.uint32))


def strided_bits() -> np.ndarray:
    """Every 4099th of the 2^32 float bit patterns (tests/test_math.py's stride)."""
    return u2f(np.arange(0, 1 << 32, 4099, dtype=np.uint64).astype(np.uint32))


SUB_MIN, SUB_MAX, FLT_MIN, FLT_MAX = u2f([1])[0], u2f([0x007fffff])[0], u2f([0x00800000])[0], u2f([0x7f7fffff])[0]
EDGES = np.array([0.0, -0.0, SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, np.inf,
                  -np.inf, np.nan, -np.nan, 1.0, -1.0], f32)


def _isnan(x):
    return np.isnan(x)


# --------------------------------------------------------------------------- math

def trig_inputs() -> np.ndarray:
    k = np.arange(1, int(8192 * 4 / np.pi) + 1, dtype=np.float64)
    octants = ulps((k * (np.pi / 4)).astype(f32), -2, 2)
    lim = ulps(f32(1.0e7), -4, 4)
    rng = np.random.default_rng(11)
    kernel = (f32(6.283185307) * (rng.integers(0, 1 << 23, 1 << 16).astype(f32) / f32(1 << 23))).astype(f32)
    return np.concatenate([strided_bits(), EDGES, octants, -octants, lim, -lim, kernel])


def exp_sweep() -> np.ndarray:
    """Dense over [-103.3, -87.3]: the arguments whose exp is subnormal (rt_ldexpf's n < -126)."""
    return np.linspace(-103.3, -87.3, 1 << 16, dtype=np.float64).astype(f32)


def exp_inputs() -> np.ndarray:
    th = np.concatenate([ulps(f32(88.72283905)), ulps(f32(-103.2789299)), ulps(f32(-87.3365))])
    rng = np.random.default_rng(12)
    return np.concatenate([strided_bits(), EDGES, th, exp_sweep(), rng.uniform(-20, 5, 1 << 14).astype(f32)])


def log_inputs() -> np.ndarray:
    pow2 = u2f(np.concatenate([(1 << np.arange(23)).astype(np.uint32),               # 2^-149 .. 2^-127
                               (np.arange(1, 255, dtype=np.uint32) << 23)]))         # 2^-126 .. 2^127
    rng = np.random.default_rng(13)
    sub = u2f(((1 << np.arange(23)).astype(np.uint32)[:, None] | rng.integers(0, 1 << 23, (23, 64), dtype=np.uint32)
               & ((1 << np.arange(23)).astype(np.uint32)[:, None] - 1)).reshape(-1))  # every subnormal exponent
    near = np.concatenate([ulps(f32(0.70710678) * f32(2.0) ** e) for e in (-100, -1, 0, 1, 10)] +
                          [ulps(f32(1.0)), ulps(f32(2.0))])
    return np.concatenate([strided_bits(), EDGES, pow2, sub, near, rng.uniform(1e-6, 3, 1 << 14).astype(f32)])


POW_KERNEL_N = (0.0, 10.0, 40.0, 50.0, 100.0, 1000.0, 99999.0, 1.0e6)


def pow_inputs():
    """(x, y) pairs: the edge cross product, the binary64 path's thresholds, subnormal results, the
    kernels' own pow(r1, 1 / (n + 1)), and random pairs."""
    rng = np.random.default_rng(14)
    ex = np.concatenate([EDGES, f32([2.0, -2.0, 0.5, -0.5, -3.0, 3.0, 10.0, -10.0, 0.99999994, 1.0000001])])
    ey = np.concatenate([EDGES, f32([2.0, -2.0, 3.0, -3.0, 0.5, -0.5, 2.5, -2.5, 16777216.0, -16777216.0,
                                     16777218.0, -16777218.0, 16777215.0, -16777215.0, 8388609.0, -8388609.0,
                                     8388608.5, 1e30, -1e30, 1e-30])])
    gx, gy = np.meshgrid(ex, ey, indexing="ij")
    xs, ys = [gx.reshape(-1)], [gy.reshape(-1)]
    # negative bases with integral and non-integral exponents
    nb = -rng.uniform(0.1, 10, 4096).astype(f32)
    xs += [nb, nb]
    ys += [rng.integers(-40, 41, 4096).astype(f32), rng.uniform(-40, 40, 4096).astype(f32)]
    # y log x within 1e-3 of the overflow (89) and underflow (-110) cuts, and subnormal results
    def at(t, base_lo, base_hi, m):
        x = rng.uniform(base_lo, base_hi, m).astype(f32)
        return x, (t / np.log(x.astype(np.float64))).astype(f32)
    for centre in (89.0, -110.0):
        for lo, hi in ((1.5, 100.0), (0.01, 0.9)):
            x, y = at(centre + rng.uniform(-1e-3, 1e-3, 4096), lo, hi, 4096)
            xs.append(x)
            ys.append(y)
    for lo, hi in ((1.5, 100.0), (0.01, 0.9)):
        x, y = at(rng.uniform(-103.3, -87.3, 8192), lo, hi, 8192)
        xs.append(x)
        ys.append(y)
    # subnormal bases
    sx = u2f(rng.integers(1, 1 << 23, 4096, dtype=np.uint32))
    xs.append(sx)
    ys.append(rng.uniform(-1.2, 1.2, 4096).astype(f32))
    # the kernels' own use (materials.h:85, :190-196): r1 = k / 2^23, y = 1 / (n + 1)
    k = np.concatenate([np.arange(0, 1 << 23, 128), [1, (1 << 23) - 1]]).astype(f32)
    r1 = (k / f32(1 << 23)).astype(f32)
    for n in POW_KERNEL_N:
        xs.append(r1)
        ys.append(np.full(r1.size, f32(1.0) / (f32(n) + f32(1.0)), f32))
    # random pairs: moderate and any bit pattern
    xs.append(np.exp(rng.uniform(-14, 14, 1 << 16)).astype(f32))
    ys.append(rng.uniform(-20, 20, 1 << 16).astype(f32))
    xs.append(u2f(rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)))
    ys.append(u2f(rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)))
    return np.concatenate(xs).astype(f32), np.concatenate(ys).astype(f32)


def ldexp_inputs():
    z = np.concatenate([np.linspace(0.5, 2.0, 97).astype(f32), ulps(f32(1.0)), u2f([0x3fffffff, 0x3f000001])])
    n = np.arange(-180, 261, dtype=np.int32)
    gz, gn = np.meshgrid(z, n, indexing="ij")
    rng = np.random.default_rng(15)
    rz = rng.uniform(0.5, 2.0, 1 << 14).astype(f32)
    rn = rng.integers(-180, 261, 1 << 14).astype(np.int32)
    return np.concatenate([gz.reshape(-1), rz]), np.concatenate([gn.reshape(-1), rn]).astype(np.int32)


def div_inputs():
    rng = np.random.default_rng(16)
    m = 1 << 16

    def mant(e_lo, e_hi, size):
        sign = rng.integers(0, 2, size, dtype=np.uint32) << 31
        e = rng.integers(e_lo + 127, e_hi + 128, size, dtype=np.uint32) << 23
        return u2f(sign | e | rng.integers(0, 1 << 23, size, dtype=np.uint32))

    sub = u2f(rng.integers(1, 1 << 23, m // 4, dtype=np.uint32))
    xs = [mant(-20, 20, m), sub, mant(-10, 10, m // 4), mant(-126, -90, m // 2), sub]
    ys = [mant(-20, 20, m), mant(-10, 10, m // 4), sub, mant(20, 60, m // 2), np.roll(sub, 7)]
    # exact halfway cases: an odd 24-bit integer m0 scaled so the quotient is m0 2^-150 (between two
    # subnormals: round to even), and odd subnormals halved
    m0 = (rng.integers(0, 1 << 23, 4096).astype(np.int64) * 2 + 1).astype(np.float64)
    xs += [(m0 * 2.0 ** -140).astype(f32), u2f(rng.integers(0, 1 << 22, 4096, dtype=np.uint32) * 2 + 1)]
    ys += [np.full(4096, f32(1024.0)), np.full(4096, f32(2.0))]
    sb = strided_bits()
    xs += [sb, EDGES.repeat(EDGES.size)]
    ys += [np.roll(sb, 12345), np.tile(EDGES, EDGES.size)]
    return np.concatenate(xs).astype(f32), np.concatenate(ys).astype(f32)


def sqrt_inputs() -> np.ndarray:
    rng = np.random.default_rng(17)
    sub = u2f(rng.integers(1, 1 << 23, 1 << 14, dtype=np.uint32))
    # squares of 13-bit integers +- 1 ulp (exact results and their neighbours), halves of odd squares
    q = rng.integers(1, 1 << 12, 4096).astype(np.float64)
    sq = ulps((q * q).astype(f32), -1, 1)
    return np.concatenate([strided_bits(), EDGES, sub, sq, np.exp(rng.uniform(-80, 80, 1 << 15)).astype(f32)])


def math_cases() -> list[Case]:
    out = []

    def add(name, fn, x, y=None, nan_ok=None):
        x = np.ascontiguousarray(x, f32)
        per = (1,) if y is None else (1, 2)
        out.append(Case(name, "math", (fn, x, y), x.size, nan_ok, per))

    t = trig_inputs()
    for name, fn in (("rt_sinf", "sin"), ("rt_cosf", "cos"), ("rt_sincosf.s", "sincos_s"), ("rt_sincosf.c", "sincos_c")):
        add(name, fn, t, nan_ok=_isnan(t) | np.isinf(t))
    e = exp_inputs()
    add("rt_expf", "exp", e, nan_ok=_isnan(e))
    lg = log_inputs()
    add("rt_logf", "log", lg, nan_ok=_isnan(lg) | (lg < 0))
    px, py = pow_inputs()
    with np.errstate(invalid="ignore"):
        add("rt_powf", "pow_xy", px, py, nan_ok=_isnan(px) | _isnan(py) | ((px < 0) & (np.floor(py) != py)))
    s = sqrt_inputs()
    add("rt_sqrtf", "sqrt", s, nan_ok=_isnan(s) | (s < 0))
    add("rt_rsqrtf", "rsqrt", s, nan_ok=_isnan(s) | (s < 0))
    lz, ln = ldexp_inputs()
    add("rt_ldexpf", "ldexp", lz, ln)
    dx, dy = div_inputs()
    add("x / y", "div", dx, dy, nan_ok=_isnan(dx) | _isnan(dy) | ((dx == 0) & (dy == 0)) | (np.isinf(dx) & np.isinf(dy)))
    add("rt_minf", "min", dx, dy, nan_ok=_isnan(dx) | _isnan(dy))
    add("rt_maxf", "max", dx, dy, nan_ok=_isnan(dx) | _isnan(dy))
    return out


# ---------------------------------------------------------------------------- rng

def frand_numpy(seeds):
    """frand (rng.h:24-42) in numpy: one draw from each seed pair -> (value, new seeds)."""
    s = np.ascontiguousarray(seeds, np.uint32).reshape(-1, 2).astype(np.uint64)
    x = (36969 * (s[:, 0] & 65535) + (s[:, 0] >> 16)) & 0xFFFFFFFF
    y = (18000 * (s[:, 1] & 65535) + (s[:, 1] >> 16)) & 0xFFFFFFFF
    bits = ((((x << 16) + y) & 0xFFFFFFFF) & 0x007FFFFF) | 0x40000000
    v = (u2f(bits.astype(np.uint32)) - f32(2.0)) / f32(2.0)
    return v.astype(f32), np.stack([x, y], axis=1).astype(np.uint32)


def rng_seeds(kat) -> np.ndarray:
    rng = np.random.default_rng(21)
    halves = np.array([0, 1, 0xFFFF, 0x10000, 0xFFFFFFFF], np.uint32)
    gx, gy = np.meshgrid(halves, halves, indexing="ij")
    special = np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1)
    mixed = np.stack([np.tile(halves, 5), rng.integers(0, 1 << 32, 25, dtype=np.uint64).astype(np.uint32)], axis=1)
    rand = rng.integers(0, 1 << 32, (1 << 14, 2), dtype=np.uint64).astype(np.uint32)
    return np.concatenate([kat["frand_seeds"].astype(np.uint32), special, mixed, mixed[:, ::-1], rand])


def rng_cases(kat) -> list[Case]:
    s = rng_seeds(kat)
    out = [Case("frand", "frand", (s, 64), len(s), None, (0,))]
    for total in (1, 2, 3, 16):
        out.append(Case(f"strat_rand(total={total})", "strat_rand", (s, 64, total), len(s), None, (0,)))
    return out


MWC_KS = (1, 7, 16, 17, 64, 255, 1024)


def mwc_cases() -> list[Case]:
    out = []
    for gen, a in enumerate((36969, 18000)):
        m = a * 65536 - 1
        rng = np.random.default_rng(a)  # tests/test_mwc_jump.py's own starts
        starts = [int(v) for v in rng.integers(0, 2**32, 100)] + [0, 1, 2, m - 1, m, m + 1, 2**32 - 1, 2**31 - 1]
        starts += [m + 2, m + 65535, m + 65536, 2**32 - 65536, 65535, 65536]
        x = np.repeat(np.array(starts, np.uint32), len(MWC_KS))
        k = np.tile(np.array(MWC_KS, np.uint32), len(starts))
        mul = np.array([pow(a, int(kk), m) for kk in k], np.uint32)
        out.append(Case(f"mwc_jump<{a}>", "mwc_jump", (gen, x, k, mul), x.size, None, (1, 2, 3)))
    return out


# ----------------------------------------------------------------------- geometry

def _rays(abi, o, d, tmin=RT_SMALL_F, tmax=np.inf):
    o = np.asarray(o, f32).reshape(-1, 3)
    r = np.zeros(len(o), abi.RAY_DTYPE)
    r["o"] = o
    r["d"] = np.broadcast_to(np.asarray(d, f32), o.shape)
    r["tmin"] = tmin
    r["tmax"] = tmax
    r["propagation"] = 1.0
    return r


def _signed_perms():
    """The 48 signed axis permutations (exact in float)."""
    import itertools

    mats = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3), f32)
            for i in range(3):
                m[i, p[i]] = s[i]
            mats.append(m)
    return mats


def mt_edge_cases(abi):
    """Constructed ray / triangle pairs -> (rays, tris[n, 9], tags).  Lattice geometry (small integers
    and powers of two, moved by signed axis permutations) keeps every product and sum of the test exact,
    so u = 0, v = 0, u + v = 1, t = tmin and t = tmax hold exactly, not nearly."""
    R, T, tags = [], [], []

    def add(o, d, v0, e1, e2, tag, tmin=RT_SMALL_F, tmax=np.inf):
        for m in _signed_perms():
            R.append((m @ f32(o), m @ f32(d), tmin, tmax))
            T.append(np.concatenate([m @ f32(v0), m @ f32(e1), m @ f32(e2)]))
            tags.append(tag)

    for a, b, v0 in ((2.0, 2.0, (0.0, 0.0, 0.0)), (4.0, 1.0, (1.0, -2.0, 0.5)), (0.5, 8.0, (-3.0, 1.0, -1.0))):
        e1, e2 = (a, 0.0, 0.0), (0.0, b, 0.0)
        pts = {"vertex": [(0, 0), (a, 0), (0, b)], "edge": [(a / 2, 0), (0, b / 2), (a / 2, b / 2)],
               "inside": [(a / 4, b / 4)], "outside": [(a, b), (-a / 4, b / 4), (a / 4, -b / 4)]}
        for tag, pl in pts.items():
            for px, py in pl:
                o = (v0[0] + px, v0[1] + py, v0[2] + 4.0)
                add(o, (0, 0, -1), v0, e1, e2, tag)                      # t = 4 exactly
                add(o, (0, 0, -2), v0, e1, e2, tag)                      # det = -2ab... t = 2
                if tag != "outside":
                    up = float(np.nextafter(f32(4.0), f32(5.0)))
                    dn = float(np.nextafter(f32(4.0), f32(3.0)))
                    add(o, (0, 0, -1), v0, e1, e2, "t==tmin", tmin=4.0)
                    add(o, (0, 0, -1), v0, e1, e2, "t==tmax", tmax=4.0)
                    add(o, (0, 0, -1), v0, e1, e2, "t<tmin", tmin=up)
                    add(o, (0, 0, -1), v0, e1, e2, "t>tmax", tmax=dn)
        # rays in the triangle's plane, along each edge and through the interior: det = 0 exactly,
        # 1 / det = inf, u, v, t = inf or NaN (0 * inf) — rejected by the determinant test alone
        for o, d in (((v0[0] - 1, v0[1], v0[2]), (1, 0, 0)), ((v0[0], v0[1] - 1, v0[2]), (0, 1, 0)),
                     ((v0[0] + a + 1, v0[1] - 1, v0[2]), (-a, b, 0)), ((v0[0] - 1, v0[1] + b / 4, v0[2]), (1, 0, 0)),
                     ((v0[0] - 1, v0[1], v0[2] + 1), (1, 0, 0)), ((v0[0], v0[1], v0[2]), (1, 0, 0))):
            add(o, d, v0, e1, e2, "det==0")
        # zero-area triangles
        for z1, z2 in (((a, 0, 0), (a, 0, 0)), ((0, 0, 0), (0, b, 0)), ((a, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 0, 0)),
                       ((a, 0, 0), (-2 * a, 0, 0))):
            add((v0[0] + a / 4, v0[1], v0[2] + 4.0), (0, 0, -1), v0, z1, z2, "zero-area")
    # |det| within +-8 ulps of RT_SMALL_F, both signs: e1 = (s, 0, 0), e2 = (0, 1, 0), d = (0, 0, -1)
    # give p = (1, 0, 0) and det = s exactly
    for s in np.concatenate([ulps(RT_SMALL_F, -8, 8), -ulps(RT_SMALL_F, -8, 8)]):
        add((float(s) / 4, 0.25, 1.0), (0, 0, -1), (0, 0, 0), (float(s), 0, 0), (0, 1, 0), "det~small")
    rays = np.zeros(len(R), abi.RAY_DTYPE)
    rays["o"] = [r[0] for r in R]
    rays["d"] = [r[1] for r in R]
    rays["tmin"] = [r[2] for r in R]
    rays["tmax"] = [r[3] for r in R]
    rays["propagation"] = 1.0
    return rays, np.array(T, f32), np.array(tags)


def mt_det64(rays, tris) -> np.ndarray:
    """det of geometryFuncs.h:160-167 in binary64."""
    d = rays["d"].astype(np.float64)
    e1, e2 = tris[:, 3:6].astype(np.float64), tris[:, 6:9].astype(np.float64)
    return (np.cross(d, e2) * e1).sum(axis=1)


def mt_cases(abi, kat) -> list[Case]:
    rays, tris, tags = mt_edge_cases(abi)
    rng = np.random.default_rng(31)
    m = 1 << 15  # near-edge random: rays aimed at random points of the triangles' edges and vertices
    t9 = rng.uniform(-1, 1, (m, 9)).astype(f32)
    w = rng.uniform(0, 1, (m, 2))
    sel = rng.integers(0, 4, m)
    w[sel == 0, 0] = 0
    w[sel == 1, 1] = 0
    w[sel == 2, 1] = 1 - w[sel == 2, 0]
    w[sel == 3] = np.array([[0, 0], [1, 0], [0, 1]])[rng.integers(0, 3, (sel == 3).sum())]
    target = t9[:, :3] + w[:, :1] * t9[:, 3:6] + w[:, 1:] * t9[:, 6:9]
    o = rng.uniform(-2, 2, (m, 3))
    d = target - o
    rr = _rays(abi, o, d / np.linalg.norm(d, axis=1, keepdims=True),
               tmax=np.where(rng.uniform(size=m) < 0.5, np.inf, rng.uniform(0.5, 4, m)))
    kr = kat["tri_rays"].view(abi.RAY_DTYPE).reshape(-1)
    return [Case("mt_test (kat.npz)", "mt_test", (kr, kat["tri"]), len(kr), None, (0, 1)),
            Case("mt_test (constructed edges)", "mt_test", (rays, tris), len(rays), None, (0, 1),
                 extra={"tags": tags}),
            Case("mt_test (rays at edges and vertices)", "mt_test", (rr, t9), m, None, (0, 1))]


def sphere_disc32(rays, c, radius) -> np.ndarray:
    """geometryFuncs.h:41-49's discriminant in the kernel's own float32 operation order."""
    o, d = rays["o"], rays["d"]
    ox, oy, oz = (o[:, k] - c[:, k] for k in range(3))
    dist2 = ox * ox + oy * oy + oz * oz
    b = -(ox * d[:, 0] + oy * d[:, 1] + oz * d[:, 2])
    return b * b - (dist2 - radius * radius)


def sphere_cases(abi, kat) -> list[Case]:
    kr = kat["tri_rays"].view(abi.RAY_DTYPE).reshape(-1)
    out = [Case("intersect_sphere (kat.npz)", "intersect_sphere", (kr, kat["sph_c"], kat["sph_r"]), len(kr), None,
                (0, 1, 2))]
    # tangent rays: o = (-4 s, h, 0), d = (1, 0, 0), c = 0: disc = 16 s^2 - ((16 s^2 + h^2) - r^2), zero at
    # h == r and within a few of its own ulps around it
    O, C, Rd = [], [], []
    for s in (0.125, 0.25, 1.0, 4.0):
        for r0 in (0.5, 1.0, 1.5, 2.0):
            h = ulps(f32(r0 * s), -8, 8)
            r = ulps(f32(r0 * s), -8, 8)
            gh, gr = np.meshgrid(h, r, indexing="ij")
            for sign in (1.0, -1.0):
                O.append(np.stack([np.full(gh.size, -4 * s, f32), sign * gh.reshape(-1), np.zeros(gh.size, f32)], 1))
                C.append(np.zeros((gh.size, 3), f32))
                Rd.append(gr.reshape(-1))
    O, C, Rd = np.concatenate(O), np.concatenate(C), np.concatenate(Rd)
    out.append(Case("intersect_sphere (tangent)", "intersect_sphere", (_rays(abi, O, (1, 0, 0)), C, Rd), len(O), None,
                    (0, 1, 2)))
    # origins inside, on and outside the sphere
    rng = np.random.default_rng(32)
    m = 1 << 15
    c = rng.uniform(-3, 3, (m, 3)).astype(f32)
    r = rng.uniform(0.2, 2, m).astype(f32)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    scale = np.array([0.0, 0.5, 1.0, 1.0, 2.0, 1.0 + 1e-6, 1.0 - 1e-6])[rng.integers(0, 7, m)]
    o = (c + (u * (scale * r)[:, None])).astype(f32)
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tang = rng.uniform(size=m) < 0.25  # on-surface origins leaving along the tangent plane
    d[tang] -= u[tang] * (d[tang] * u[tang]).sum(axis=1, keepdims=True)
    d[tang] /= np.linalg.norm(d[tang], axis=1, keepdims=True)
    out.append(Case("intersect_sphere (inside / on / outside)", "intersect_sphere", (_rays(abi, o, d), c, r), m, None,
                    (0, 1, 2), extra={"scale": scale}))
    return out


def box_cases(abi, kat) -> list[Case]:
    kb = kat["box_rays"].view(abi.RAY_DTYPE).reshape(-1)
    out = [Case("intersect_box + box_normal (kat.npz)", "intersect_box", (kb,), len(kb), None, (0,))]
    rng = np.random.default_rng(33)
    size = np.array(BOX, f32)
    O, D = [], []
    # one, two or three direction components exactly zero; that origin component inside, on and outside
    for zero in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
        for k in zero:
            s = size[k]
            for val in (0.0, -0.0, s, -s, np.nextafter(s, f32(0)), np.nextafter(s, f32(9)), s + 1, -(s + 1), 0.5 * s):
                for _ in range(16):
                    o = rng.uniform(-0.9, 0.9, 3) * size
                    d = rng.normal(size=3)
                    d /= np.linalg.norm(d)
                    d[list(zero)] = rng.choice([0.0, -0.0], len(zero))
                    o[k] = val
                    O.append(o)
                    D.append(d)
    # origins on a face (and on an edge / a corner), going in, out and along
    for k in range(3):
        for sgn in (1.0, -1.0):
            for _ in range(256):
                o = rng.uniform(-1, 1, 3) * size
                o[k] = sgn * size[k]
                if rng.uniform() < 0.2:
                    o[(k + 1) % 3] = rng.choice([1.0, -1.0]) * size[(k + 1) % 3]
                d = rng.normal(size=3)
                d /= np.linalg.norm(d)
                O.append(o)
                D.append(d)
    # hit points exactly on an edge or a corner: from an interior lattice origin along (target - o) / 8
    # (exact: every slab distance is 8), where box_normal's dx < dy && dx < dz / dy < dz ties decide
    for sx in (1, -1, 0):
        for sy in (1, -1, 0):
            for sz in (1, -1, 0):
                if (sx == 0) + (sy == 0) + (sz == 0) > 1:
                    continue
                for frac in (0.0, 0.25, -0.5):
                    tgt = np.array([sx * 6.0 if sx else frac * 6, sy * 5.0 if sy else frac * 5,
                                    sz * 6.0 if sz else frac * 6])
                    for o in ((0.0, 0.0, 0.0), (1.0, -1.0, 2.0)):
                        O.append(np.array(o))
                        D.append((tgt - np.array(o)) / 8.0)
    O, D = np.array(O, f32), np.array(D, f32)
    out.append(Case("intersect_box + box_normal (constructed edges)", "intersect_box", (_rays(abi, O, D),), len(O), None,
                    (0,)))
    m = 1 << 15
    o = (rng.uniform(-1.3, 1.3, (m, 3)) * size).astype(f32)
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out.append(Case("intersect_box + box_normal (random, origins in and out)", "intersect_box", (_rays(abi, o, d),), m,
                    None, (0,)))
    return out


def camera_pixels(W, H):
    """Pixel corners and centres of the 8x8 block at the frame's corner and at its centre:
    (fx, fy) float32 pixel coordinates."""
    pts = []
    for x0, y0 in ((0, 0), (W // 2 - 4, H // 2 - 4)):
        c = np.arange(9, dtype=f32)
        gx, gy = np.meshgrid(f32(x0) + c, f32(y0) + c, indexing="ij")
        pts.append(np.stack([gx.reshape(-1), gy.reshape(-1)], 1))
        m = np.arange(8, dtype=f32) + f32(0.5)
        gx, gy = np.meshgrid(f32(x0) + m, f32(y0) + m, indexing="ij")
        pts.append(np.stack([gx.reshape(-1), gy.reshape(-1)], 1))
    return np.concatenate(pts).astype(f32)


def camera_height(W) -> int:
    return max(16, (int(W) * 3 // 4) & ~1)


def camera_dir_numpy(cam16, a, b):
    """camera_dir (raytracer.cl:81-85) restated in float32 numpy, in the kernel's operation order."""
    cam = np.asarray(cam16, f32).reshape(4, 4)
    view, up, right = cam[0], cam[1], cam[2]
    v = [((view[k] + right[k] * a).astype(f32) + (up[k] * b).astype(f32)).astype(f32) for k in range(4)]
    ln = np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]).astype(f32)
    return np.stack([v[0] / ln, v[1] / ln, v[2] / ln], axis=-1).astype(f32)


def camera_cases(kat) -> list[Case]:
    cams = np.ascontiguousarray(kat["cams"], f32)
    idx, A, B, px = [], [], [], []
    for ci, W in enumerate(kat["cam_widths"]):
        W = int(W)
        H = camera_height(W)
        p = camera_pixels(W, H)
        idx.append(np.full(len(p), ci, np.int32))
        A.append(p[:, 0] - f32(W) / f32(2.0))
        B.append(p[:, 1] - f32(H) / f32(2.0))
        px.append(p)
    A, B = np.concatenate(A).astype(f32), np.concatenate(B).astype(f32)
    return [Case("camera_dir", "camera_dir", (cams, np.concatenate(idx), A, B), len(A), None, (1, 2, 3),
                 extra={"pixels": np.concatenate(px)})]


# --------------------------------------------------------------- frames and sampling

def unit_normals(m=1 << 14, seed=41) -> np.ndarray:
    """Axis normals, unit normals with |n.y| within +-4 ulps of perpendicular's 0.9 switch, random ones."""
    rng = np.random.default_rng(seed)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    y = np.concatenate([ulps(f32(0.9)), -ulps(f32(0.9))])
    y = np.repeat(y, 32)
    phi = rng.uniform(0, 2 * np.pi, y.size)
    s = np.sqrt(1.0 - y.astype(np.float64) ** 2)
    sw = np.stack([s * np.cos(phi), y, s * np.sin(phi)], 1).astype(f32)
    sw[:, 1] = y  # exactly the chosen float
    r = rng.normal(size=(m, 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    return np.concatenate([axes, sw, r.astype(f32)])


def unit_draws(m, seed) -> np.ndarray:
    """frand values k / 2^23 with the ends 0, 2^-23 and 1 - 2^-23 over-represented."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 23, m)
    ends = np.array([0, 1, (1 << 23) - 1])
    pick = rng.uniform(size=m) < 0.2
    k[pick] = ends[rng.integers(0, 3, pick.sum())]
    k[:9] = np.repeat(ends, 3)
    return (k.astype(f32) / f32(1 << 23)).astype(f32)


def tir_cases(abi):
    """sample_refraction around total internal reflection for ior 1.5: leaving (d.z < 0) with d.z^2 near
    1 - 1/2.25, entering at the same |d.z|, d.z = +-0, normal incidence; refExp below and at 100000."""
    rng = np.random.default_rng(42)
    crit = f32(np.sqrt(1.0 - 1.0 / 2.25))
    dz = np.concatenate([-ulps(crit, -64, 64), ulps(crit, -64, 64), f32([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, -0.7, -0.8]),
                         -rng.uniform(0, 1, 256).astype(f32), rng.uniform(0, 1, 256).astype(f32)])
    blur = f32([50.0, 99999.0, 100000.0, 1.0e6])
    dz, be = [g.reshape(-1) for g in np.meshgrid(dz, blur, indexing="ij")]
    n = dz.size
    phi = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(np.maximum(0.0, 1.0 - dz.astype(np.float64) ** 2))
    d = np.stack([s * np.cos(phi), s * np.sin(phi), dz], 1).astype(f32)
    d[:, 2] = dz
    rays = _rays(abi, np.zeros((n, 3), f32), d)
    rays["propagation"] = rng.uniform(0.1, 1, (n, 3)).astype(f32)
    ior = np.full(n, f32(1.5))
    return rays, ior, be.astype(f32), unit_draws(n, 43), unit_draws(n, 44)


def tir_cos_sq32(rays, ior) -> np.ndarray:
    """materials.h:146-160's cos_sq in the kernel's float32 operation order."""
    dz = rays["d"][:, 2]
    entering = dz > 0
    ei = np.where(entering, f32(1.0), ior).astype(f32)
    eo = np.where(entering, ior, f32(1.0)).astype(f32)
    ratio = (ei / eo).astype(f32)
    return (f32(1.0) - ((ratio * ratio).astype(f32) * (f32(1.0) - (dz * dz).astype(f32)).astype(f32)).astype(f32)).astype(f32)


def tir_cos_sq64(rays, ior) -> np.ndarray:
    dz = rays["d"][:, 2].astype(np.float64)
    ratio = np.where(dz > 0, 1.0 / ior.astype(np.float64), ior.astype(np.float64))
    return 1.0 - ratio * ratio * (1.0 - dz * dz)


def sampling_cases(abi, kat) -> list[Case]:
    out = []
    nrm = unit_normals()
    n = len(nrm)
    rng = np.random.default_rng(45)
    v = rng.normal(size=(n, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    out.append(Case("perpendicular", "frame", ("perpendicular", nrm), n, None, (1,)))
    out.append(Case("shading_to_world", "frame", ("shading_to_world", v, nrm), n, None, (1, 2)))
    out.append(Case("world_to_shading", "frame", ("world_to_shading", v, nrm), n, None, (1, 2)))
    m = 1 << 16
    r1, r2 = unit_draws(m, 46), unit_draws(m, 47)
    out.append(Case("cos_sample_hemisphere", "cos_sample_hemisphere", (r1, r2), m, None, (0, 1)))
    w = rng.normal(size=(m, 3))
    w[:, 2] = np.abs(w[:, 2])
    w = (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(f32)
    spec = f32([0.0, 10.0, 50.0, 100.0, 1000.0, 99999.0, 100000.0, 1.0e6])[rng.integers(0, 8, m)]
    out.append(Case("sample_phong", "sample_phong", (w, spec, r1, r2), m, None, (0, 1, 2, 3)))
    rays, ior, be, t1, t2 = tir_cases(abi)
    # cos_sq == 0 exactly makes the reference's own Fresnel term (1 - 1) / 0: a NaN by definition
    out.append(Case("sample_refraction", "sample_refraction", (rays, ior, be, t1, t2), len(rays),
                    tir_cos_sq32(rays, ior) == 0, (0, 1, 2, 3, 4)))
    # sphere_light_dir: the reference's own cases, then random origins outside lights of several radii
    em = kat["em_rays"].view(abi.RAY_DTYPE).reshape(-1)
    ne = len(em)
    # (the fixture holds origins inside the light, where sin_max > 1 and the reference's own sqrt is a NaN)
    inside = np.linalg.norm(em["o"].astype(np.float64) - kat["light_c"].astype(np.float64), axis=1) <= 0.5 * (1 + 1e-5)
    out.append(Case("sphere_light_dir (kat.npz)", "sphere_light_dir",
                    (np.ascontiguousarray(em["o"]), np.tile(kat["light_c"].astype(f32), (ne, 1)), np.full(ne, f32(0.5)),
                     np.ascontiguousarray(kat["em_r12"][:, 0]), np.ascontiguousarray(kat["em_r12"][:, 1])), ne, inside,
                    (0, 1, 2, 3, 4)))
    c = rng.uniform(-3, 3, (m, 3)).astype(f32)
    rad = rng.uniform(0.1, 1.0, m).astype(f32)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (c + u * (rad * rng.uniform(1.05, 12, m))[:, None]).astype(f32)
    out.append(Case("sphere_light_dir", "sphere_light_dir", (o, c, rad, r1, r2), m, None, (0, 1, 2, 3, 4)))
    return out


def boundary_materials(abi, seeds):
    """One material per seed pair and branch boundary of sample_material (rtcommon.h:205-245): with p the
    first frand draw of the seed, the thresholds ks, ks + kd and ks + kd + kt (the float sums the kernel
    forms) are set to p - 1 ulp, p and p + 1 ulp.  Returns (mats, which threshold, offset in ulps)."""
    p, _ = frand_numpy(seeds)
    n = len(p)
    mats = np.zeros(n, abi.SPHERE_DTYPE)
    rng = np.random.default_rng(51)
    mats["diffuse"] = rng.uniform(0.2, 1, (n, 3)).astype(f32)
    mats["extinction"] = f32(0.9)
    mats["ior"] = f32(1.5)
    mats["specExp"] = f32([10.0, 50.0, 1.0e6])[rng.integers(0, 3, n)]
    mats["refExp"] = f32([50.0, 1.0e6])[rng.integers(0, 2, n)]
    which = np.arange(n) % 4
    off = (np.arange(n) // 4) % 3 - 1
    target = u2f((f2u(p).astype(np.int64) + off).clip(0).astype(np.uint32))
    ks, kd, kt = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    a = which == 0                      # p against ks
    ks[a], kd[a], kt[a] = target[a], 0.3, 0.3
    a = which == 1                      # p against ks + kd (ks = 0: the sum is kd itself)
    kd[a], kt[a] = target[a], 0.5
    a = which == 2                      # p against ks + kd + kt (ks = kd = 0)
    kt[a] = target[a]
    a = (which == 3) & (target >= 0.5)  # all three lobes: (0.25 + 0.25) + (target - 0.5), both exact
    ks[a], kd[a], kt[a] = 0.25, 0.25, target[a] - f32(0.5)
    a = (which == 3) & (target < 0.5)   # a sum below 1: the absorbed return
    ks[a], kd[a], kt[a] = 0.05, 0.05, 0.05
    mats["ks"], mats["kd"], mats["kt"] = ks, kd, kt
    return mats, which, off, p


def material_cases(abi, kat) -> list[Case]:
    R = abi.RAY_DTYPE
    out = [Case("sample_material (kat.npz)", "sample_material",
                (kat["mat_in"].view(R).reshape(-1), kat["mat_hits"], kat["mats"].view(abi.SPHERE_DTYPE).reshape(-1),
                 kat["mat_idx"], kat["mat_seed"]), len(kat["mat_idx"]), None, (0, 1, 3, 4))]
    rng = np.random.default_rng(52)
    m = 1 << 14

    def rays_hits(m):
        r = np.zeros(m, R)
        r["o"] = rng.uniform(-1, 1, (m, 3)).astype(f32)
        d = rng.normal(size=(m, 3))
        r["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
        r["tmin"] = RT_SMALL_F
        r["tmax"] = rng.uniform(0.5, 5, m).astype(f32)
        r["propagation"] = rng.uniform(0.1, 1, (m, 3)).astype(f32)
        nrm = unit_normals(m, seed=53)[:m]
        return r, np.concatenate([r["o"] + f32(0.5), nrm], axis=1).astype(f32)

    # the reference's materials and an absorbing one (sum 0.7), many seeds
    base = kat["mats"].view(abi.SPHERE_DTYPE).reshape(-1)
    absorb = np.zeros(1, abi.SPHERE_DTYPE)
    absorb["ks"], absorb["kd"], absorb["kt"] = 0.2, 0.3, 0.2
    absorb["diffuse"], absorb["ior"], absorb["specExp"], absorb["refExp"] = 0.5, 1.5, 50.0, 40.0
    absorb["extinction"] = 0.9
    mats = np.concatenate([base, absorb])
    r, h = rays_hits(m)
    seeds = rng.integers(0, 1 << 32, (m, 2), dtype=np.uint64).astype(np.uint32)
    out.append(Case("sample_material (reference materials + absorbing)", "sample_material",
                    (r, h, mats, rng.integers(0, len(mats), m).astype(np.int32), seeds), m, None, (0, 1, 3, 4)))
    # one material per branch boundary
    seeds = rng.integers(0, 1 << 32, (m, 2), dtype=np.uint64).astype(np.uint32)
    bm, which, off, p = boundary_materials(abi, seeds)
    r, h = rays_hits(m)
    out.append(Case("sample_material (branch boundaries)", "sample_material",
                    (r, h, bm, np.arange(m, dtype=np.int32), seeds), m, None, (0, 1, 3, 4),
                    extra={"which": which, "off": off, "p": p}))
    return out


def all_cases(abi, kat) -> dict[str, Case]:
    cases = (math_cases() + rng_cases(kat) + mwc_cases() + mt_cases(abi, kat) + sphere_cases(abi, kat) +
             box_cases(abi, kat) + camera_cases(kat) + sampling_cases(abi, kat) + material_cases(abi, kat))
    out = {c.name: c for c in cases}
    assert list(out) == CASE_NAMES, [n for n in out if n not in CASE_NAMES] + [n for n in CASE_NAMES if n not in out]
    return out


# the names all_cases() yields, fixed here so that tests can be parametrised before any fixture exists
CASE_NAMES = [
    "rt_sinf", "rt_cosf", "rt_sincosf.s", "rt_sincosf.c", "rt_expf", "rt_logf", "rt_powf", "rt_sqrtf", "rt_rsqrtf",
    "rt_ldexpf", "x / y", "rt_minf", "rt_maxf", "frand", "strat_rand(total=1)", "strat_rand(total=2)",
    "strat_rand(total=3)", "strat_rand(total=16)", "mwc_jump<36969>", "mwc_jump<18000>", "mt_test (kat.npz)",
    "mt_test (constructed edges)", "mt_test (rays at edges and vertices)", "intersect_sphere (kat.npz)",
    "intersect_sphere (tangent)", "intersect_sphere (inside / on / outside)", "intersect_box + box_normal (kat.npz)",
    "intersect_box + box_normal (constructed edges)", "intersect_box + box_normal (random, origins in and out)",
    "camera_dir", "perpendicular", "shading_to_world", "world_to_shading", "cos_sample_hemisphere", "sample_phong",
    "sample_refraction", "sphere_light_dir (kat.npz)", "sphere_light_dir", "sample_material (kat.npz)",
    "sample_material (reference materials + absorbing)", "sample_material (branch boundaries)",
]

# one case per entry of the device module (and per generator of mwc_jump) for the bounds-guard runs
GUARD_NAMES = ["rt_expf", "rt_powf", "frand", "strat_rand(total=3)", "mwc_jump<36969>", "mwc_jump<18000>",
               "mt_test (rays at edges and vertices)", "intersect_sphere (inside / on / outside)",
               "intersect_box + box_normal (random, origins in and out)", "camera_dir", "perpendicular",
               "shading_to_world", "cos_sample_hemisphere", "sample_phong", "sample_refraction", "sphere_light_dir",
               "sample_material (branch boundaries)"]


def kat_answers(abi, kat) -> dict[str, dict]:
    """The reference's own answers (tests/golden/kat.npz) in the result layout of tests/devkat.py, per case
    name; `frand` covers the first rows of its case (the fixture's seeds come first)."""
    R = abi.RAY_DTYPE
    em = kat["em_out"].view(R).reshape(-1)
    return {
        "frand": {"vals": kat["frand"]},
        "mt_test (kat.npz)": {"hit": kat["tri_hit"].astype(np.int32), "t": np.ascontiguousarray(kat["tri_uvt"][:, 2]),
                              "hit_any": kat["tri_p"].astype(np.int32)},
        "intersect_sphere (kat.npz)": {"d": kat["sph_d"]},
        "intersect_box + box_normal (kat.npz)": {"t": kat["box_t"], "normal": kat["box_n"]},
        "sample_material (kat.npz)": {"rays": kat["mat_out"].view(np.uint32).reshape(-1, 15),
                                      "seeds_out": kat["mat_seed_out"].astype(np.uint32),
                                      "ret": kat["mat_ret"].astype(np.int32)},
        "sphere_light_dir (kat.npz)": {"d": np.ascontiguousarray(em["d"]), "tmax": np.ascontiguousarray(em["tmax"])},
    }


def guard_subsets(case: Case):
    """The same entry at n = 1 and at an n that is no multiple of 256 (the kernel's bounds guard):
    65 537 elements (tiled if the case has fewer)."""
    idx = np.arange(65537) % case.n
    return [case.subset(np.array([case.n // 2])), case.subset(idx)]
