"""Two answers to the same per-function questions (tests/kat_cases.py), with one calling
convention: `Device` runs tests/cpp/libdevkat.so (the device build of include/rt_math.h and of
the kernels' helpers, one launch per call), `Host` runs the CPU oracle's batch forms
(oracle/pt_oracle.c).  Every method takes numpy arrays and returns a dict of named result arrays,
so a test compares `dev.f(*args)` with `host.f(*args)` key by key, bit for bit.

Not a test file: imported by tests/test_device_kat_host.py and tests/test_gpu_device_kat.py."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
LIBDEVKAT = ROOT / "tests" / "cpp" / "libdevkat.so"

ENTRIES = ["dk_math", "dk_frand", "dk_strat_rand", "dk_mwc_jump", "dk_mt_test", "dk_intersect_sphere",
           "dk_intersect_box", "dk_camera_dir", "dk_frame", "dk_cos_sample_hemisphere", "dk_sample_phong",
           "dk_sample_refraction", "dk_sphere_light_dir", "dk_sample_material"]

MATH_FN = {"sin": 0, "cos": 1, "exp": 2, "log": 3, "pow": 4, "sincos_s": 5, "sincos_c": 6, "pow_xy": 7, "sqrt": 8,
           "rsqrt": 9, "ldexp": 10, "div": 11, "min": 12, "max": 13}
MATH_BINARY = ("pow_xy", "ldexp", "div", "min", "max")
FRAME_FN = {"perpendicular": 0, "shading_to_world": 1, "world_to_shading": 2}

BOX = (6.0, 5.0, 6.0)  # raytracer.cl:16-17


def build_module() -> Path:
    """tests/cpp/libdevkat.so, (re)built by make from the library's own flags."""
    subprocess.run(["make", "-s", "-C", str(ROOT / "tests" / "cpp"), "libdevkat.so"], check=True)
    return LIBDEVKAT


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _f(a, cols=None):
    a = np.ascontiguousarray(a, np.float32)
    return a if cols is None else a.reshape(-1, cols)


def _i(a):
    return np.ascontiguousarray(a, np.int32)


def _u(a, cols=None):
    a = np.ascontiguousarray(a, np.uint32)
    return a if cols is None else a.reshape(-1, cols)


def _math_y(fn, x, y):
    if fn in MATH_BINARY:
        yy = np.ascontiguousarray(y, np.int32 if fn == "ldexp" else np.float32)
        assert yy.shape == x.shape
        return yy
    return np.array([0.0 if y is None else y], np.float32)


class DeviceError(RuntimeError):
    pass


class _Base:
    """The argument handling both sides share; a subclass supplies _call(name, *ctypes args)."""

    def __init__(self, abi):
        self.abi = abi  # pathtracer.cl_amd._abi: the record dtypes

    def _rays(self, rays):
        r = np.ascontiguousarray(rays).view(self.abi.RAY_DTYPE).reshape(-1).copy()
        assert r.dtype.itemsize == 60
        return r

    def math(self, fn, x, y=None):
        x = _f(x)
        yy = _math_y(fn, x, y)
        out = np.empty_like(x)
        self._call("math", MATH_FN[fn], _p(x), _p(yy), _p(out), x.size)
        return {"out": out}

    def frand(self, seeds, k):
        return self._rand("frand", seeds, k, None)

    def strat_rand(self, seeds, k, total):
        return self._rand("strat_rand", seeds, k, int(total))

    def _rand(self, name, seeds, k, total):
        seeds = _u(seeds, 2)
        n = len(seeds)
        vals = np.empty((n, k), np.float32)
        so = np.empty_like(seeds)
        extra = () if total is None else (total,)
        self._call(name, _p(seeds), int(k), *extra, _p(vals), _p(so), n)
        return {"vals": vals, "seeds_out": so}

    def mt_test(self, rays, tris):
        rays = self._rays(rays)
        tris = _f(tris, 9)
        n = len(rays)
        assert len(tris) == n
        hit, anyh = np.empty(n, np.int32), np.empty(n, np.int32)
        t = np.empty(n, np.float32)
        self._mt(rays, tris, hit, t, anyh, n)
        return {"hit": hit, "t": t, "hit_any": anyh}

    def intersect_sphere(self, rays, c, radius):
        rays, c, radius = self._rays(rays), _f(c, 3), _f(radius)
        out = np.empty(len(rays), np.float32)
        self._call("intersect_sphere", _p(rays), _p(c), _p(radius), _p(out), len(rays))
        return {"d": out}

    def intersect_box(self, rays):
        rays = self._rays(rays)
        n = len(rays)
        t, nrm = np.empty(n, np.float32), np.empty((n, 3), np.float32)
        f32 = ctypes.c_float
        self._call("intersect_box", _p(rays), f32(BOX[0]), f32(BOX[1]), f32(BOX[2]), _p(t), _p(nrm), n)
        return {"t": t, "normal": nrm}

    def camera_dir(self, cams, cam_idx, a, b):
        cams, cam_idx, a, b = _f(cams, 16), _i(cam_idx), _f(a), _f(b)
        assert cam_idx.min() >= 0 and cam_idx.max() < len(cams)
        out = np.empty((len(a), 3), np.float32)
        self._camera(cams, cam_idx, a, b, out)
        return {"d": out}

    def frame(self, fn, v, nrm=None):
        v = _f(v, 3)
        nrm = None if nrm is None else _f(nrm, 3)
        out = np.empty_like(v)
        self._call("frame", FRAME_FN[fn], _p(v), _p(nrm), _p(out), len(v))
        return {"out": out}

    def cos_sample_hemisphere(self, r1, r2):
        r1, r2 = _f(r1), _f(r2)
        out = np.empty((len(r1), 3), np.float32)
        self._call("cos_sample_hemisphere", _p(r1), _p(r2), _p(out), len(r1))
        return {"out": out}

    def sample_phong(self, w, spec_exp, r1, r2):
        w, spec_exp, r1, r2 = _f(w, 3), _f(spec_exp), _f(r1), _f(r2)
        out = np.empty_like(w)
        self._call("sample_phong", _p(w), _p(spec_exp), _p(r1), _p(r2), _p(out), len(w))
        return {"out": out}

    def sample_refraction(self, rays, ior, blur_exp, r1, r2):
        rays = self._rays(rays)
        ior, blur_exp, r1, r2 = _f(ior), _f(blur_exp), _f(r1), _f(r2)
        ret = np.empty(len(rays), np.int32)
        self._call("sample_refraction", _p(rays), _p(ior), _p(blur_exp), _p(r1), _p(r2), _p(ret), len(rays))
        return {"rays": rays.view(np.uint32).reshape(len(rays), 15), "ret": ret}

    def sample_material(self, rays, hits, mats, mat_idx, seeds):
        rays, hits, mat_idx = self._rays(rays), _f(hits, 6), _i(mat_idx)
        mats = np.ascontiguousarray(mats).view(np.uint8).reshape(-1, 80)[:, :64].copy()  # Sphere.mat
        seeds = _u(seeds, 2).copy()
        assert mat_idx.min() >= 0 and mat_idx.max() < len(mats)
        ret = np.empty(len(rays), np.int32)
        self._material(rays, hits, mats, mat_idx, seeds, ret)
        return {"rays": rays.view(np.uint32).reshape(len(rays), 15), "seeds_out": seeds, "ret": ret}


class Device(_Base):
    """libdevkat.so; every call is one kernel launch and raises DeviceError on a HIP error."""

    def __init__(self, abi, path: Path | None = None):
        super().__init__(abi)
        self.lib = ctypes.CDLL(str(path or build_module()))
        for e in ENTRIES:
            getattr(self.lib, e).restype = ctypes.c_int

    def _raw(self, name, *args):
        fixed = [ctypes.c_uint32(a) if isinstance(a, (int, np.integer)) and i == len(args) - 1 else a
                 for i, a in enumerate(args)]
        return getattr(self.lib, "dk_" + name)(*fixed)

    def _call(self, name, *args):
        st = self._raw(name, *args)
        if st != 0:
            raise DeviceError(f"dk_{name}: HIP status {st}")

    def _mt(self, rays, tris, hit, t, anyh, n):
        self._call("mt_test", _p(rays), _p(tris), _p(hit), _p(t), _p(anyh), n)

    def _camera(self, cams, cam_idx, a, b, out):
        self._call("camera_dir", _p(cams), ctypes.c_uint32(len(cams)), _p(cam_idx), _p(a), _p(b), _p(out), len(a))

    def _material(self, rays, hits, mats, mat_idx, seeds, ret):
        self._call("sample_material", _p(rays), _p(hits), _p(mats), ctypes.c_uint32(len(mats)), _p(mat_idx),
                   _p(seeds), _p(ret), len(rays))

    def mwc_jump(self, gen, x, k, mul):
        x, k, mul = _u(x), _u(k), _u(mul)
        out = np.empty_like(x)
        self._call("mwc_jump", int(gen), _p(x), _p(k), _p(mul), _p(out), x.size)
        return {"out": out}

    def sphere_light_dir(self, o, c, radius, r1, r2):
        o, c, radius, r1, r2 = _f(o, 3), _f(c, 3), _f(radius), _f(r1), _f(r2)
        d, tmax = np.empty_like(o), np.empty(len(o), np.float32)
        self._call("sphere_light_dir", _p(o), _p(c), _p(radius), _p(r1), _p(r2), _p(d), _p(tmax), len(o))
        return {"d": d, "tmax": tmax}


class Host(_Base):
    """The CPU oracle's batch forms (oracle/pt_oracle.c)."""

    NAMES = {"math": "or_math_vec", "frand": "or_frand_seq", "strat_rand": "or_strat_seq",
             "intersect_sphere": "or_sphere_batch", "intersect_box": "or_box_batch", "frame": "or_frame_batch",
             "cos_sample_hemisphere": "or_cos_hemisphere_batch", "sample_phong": "or_phong_batch",
             "sample_refraction": "or_refraction_batch"}

    def __init__(self, abi, oracle):
        super().__init__(abi)
        self.lib = oracle.lib
        for n in list(self.NAMES.values()) + ["or_triangle_batch", "or_camera_batch", "or_emissive_batch",
                                              "or_sample_material_batch"]:
            getattr(self.lib, n).restype = None

    def _call(self, name, *args):
        fixed = [ctypes.c_size_t(a) if isinstance(a, (int, np.integer)) and i == len(args) - 1 else a
                 for i, a in enumerate(args)]
        getattr(self.lib, self.NAMES[name])(*fixed)

    def _mt(self, rays, tris, hit, t, anyh, n):
        uvt = np.empty((n, 3), np.float32)
        self.lib.or_triangle_batch(_p(rays), _p(tris), _p(hit), _p(uvt), _p(anyh), ctypes.c_size_t(n))
        t[:] = uvt[:, 2]
        self.last_uvt = uvt

    def _camera(self, cams, cam_idx, a, b, out):
        self.lib.or_camera_batch(_p(cams), _p(cam_idx), _p(a), _p(b), _p(out), ctypes.c_size_t(len(a)))

    def _material(self, rays, hits, mats, mat_idx, seeds, ret):
        self.lib.or_sample_material_batch(_p(rays), _p(hits), _p(mats), _p(mat_idx), _p(seeds), _p(ret),
                                          ctypes.c_size_t(len(rays)))

    def mwc_jump(self, gen, x, k, mul):
        """Plain stepping, x <- a (x & 0xffff) + (x >> 16), k times, in 64-bit integers (mul is the
        device's shortcut; unused here)."""
        a = (36969, 18000)[gen]
        x, k = _u(x).astype(np.uint64), _u(k)
        for j in range(int(k.max()) if k.size else 0):
            x = np.where(k > j, (a * (x & 0xFFFF) + (x >> 16)) & 0xFFFFFFFF, x)
        return {"out": x.astype(np.uint32)}

    def sphere_light_dir(self, o, c, radius, r1, r2):
        o, c, radius, r1, r2 = _f(o, 3), _f(c, 3), _f(radius), _f(r1), _f(r2)
        rays = np.zeros(len(o), self.abi.RAY_DTYPE)
        rays["o"] = o
        self.lib.or_emissive_batch(_p(rays), _p(c), _p(radius), _p(r1), _p(r2), ctypes.c_size_t(len(o)))
        return {"d": np.ascontiguousarray(rays["d"]), "tmax": np.ascontiguousarray(rays["tmax"])}


def _bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.shape[0], -1) if a.size else a.view(np.uint32).reshape(0, 1)


def _float_cols(key, arr):
    """Which 32-bit columns of a result hold floats (the NaN rule applies to them only)."""
    arr = np.asarray(arr)
    if arr.dtype == np.float32:
        return slice(None)
    if key == "rays":  # rt_ray as 15 words: 14 floats and diffuse_bounce
        return slice(0, 14)
    return None


def compare(name, got, want, nan_ok=None, row=None) -> int:
    """Bit equality of two result dicts, key by key.  One exception: where `want` holds a NaN, `got`
    must hold a NaN, payload and sign free (x86 and gfx950 generate different default NaNs) — and
    a NaN may appear, on either side, only in elements flagged by nan_ok.  Returns the number of
    words accepted under the exception; raises AssertionError naming the function, the first
    differing element's input (hex bits) and both results."""
    accepted = 0
    for key in want:
        g, w = _bits(got[key]), _bits(want[key])
        assert g.shape == w.shape, (name, key, g.shape, w.shape)
        diff = g != w
        cols = _float_cols(key, want[key])
        if cols is not None:
            gn = np.zeros(g.shape, bool)
            wn = np.zeros(w.shape, bool)
            gn[:, cols] = (g[:, cols] & 0x7FFFFFFF) > 0x7F800000
            wn[:, cols] = (w[:, cols] & 0x7FFFFFFF) > 0x7F800000
            allowed = np.zeros(g.shape[0], bool) if nan_ok is None else np.asarray(nan_ok, bool)
            stray = (gn | wn) & ~allowed[:, None]
            if stray.any():
                i = int(np.argmax(stray.any(axis=1)))
                raise AssertionError(f"{name}: {key} is NaN outside the NaN/inf edge inputs at element {i}: input "
                                     f"{row(i) if row else '?'} got {_hex(g[i])} expected {_hex(w[i])}")
            both = gn & wn
            accepted += int(both.sum())
            diff &= ~both
        if diff.any():
            i = int(np.argmax(diff.any(axis=1)))
            raise AssertionError(f"{name}: {key} differs in {int(diff.any(axis=1).sum())} of {len(g)} elements, first "
                                 f"at {i}: input {row(i) if row else '?'} got {_hex(g[i])} expected {_hex(w[i])}")
    return accepted


def _hex(words) -> str:
    return "[" + " ".join(f"{int(v):08x}" for v in words) + "]"


def run(side, case):
    """case.method of `side` (a Device or a Host) on the case's arguments."""
    return getattr(side, case.method)(*case.args)


def _no_gpu_statuses():
    """Every entry called once with n = 1 (a child process of tests/test_device_kat_host.py on a
    machine without a GPU): prints one `name status` line per entry."""
    import sys

    sys.path.insert(0, str(ROOT))
    import ptload

    abi = ptload.load()._abi
    dev = Device(abi, LIBDEVKAT)
    one = np.ones(1, np.float32)
    v = np.array([[0.0, 0.6, 0.8]], np.float32)
    ray = np.zeros(1, abi.RAY_DTYPE)
    ray["d"] = v
    seeds = np.array([[2, 2]], np.uint32)
    u1 = np.ones(1, np.uint32)
    mat = np.zeros(1, abi.SPHERE_DTYPE)
    calls = {
        "dk_math": lambda: dev.math("sin", one),
        "dk_frand": lambda: dev.frand(seeds, 2),
        "dk_strat_rand": lambda: dev.strat_rand(seeds, 2, 2),
        "dk_mwc_jump": lambda: dev.mwc_jump(0, u1, u1, u1),
        "dk_mt_test": lambda: dev.mt_test(ray, np.ones((1, 9), np.float32)),
        "dk_intersect_sphere": lambda: dev.intersect_sphere(ray, v, one),
        "dk_intersect_box": lambda: dev.intersect_box(ray),
        "dk_camera_dir": lambda: dev.camera_dir(np.ones((1, 16), np.float32), np.zeros(1, np.int32), one, one),
        "dk_frame": lambda: dev.frame("perpendicular", v),
        "dk_cos_sample_hemisphere": lambda: dev.cos_sample_hemisphere(one * 0.5, one * 0.5),
        "dk_sample_phong": lambda: dev.sample_phong(v, one, one * 0.5, one * 0.5),
        "dk_sample_refraction": lambda: dev.sample_refraction(ray, one * 1.5, one, one * 0.5, one * 0.5),
        "dk_sphere_light_dir": lambda: dev.sphere_light_dir(v * 9, v, one, one * 0.5, one * 0.5),
        "dk_sample_material": lambda: dev.sample_material(ray, np.ones((1, 6), np.float32), mat, np.zeros(1, np.int32),
                                                          seeds),
    }
    assert sorted(calls) == sorted(ENTRIES)
    for name in ENTRIES:
        try:
            calls[name]()
            print(name, 0)
        except DeviceError as e:
            print(name, str(e).rsplit(" ", 1)[1])


if __name__ == "__main__":
    _no_gpu_statuses()
