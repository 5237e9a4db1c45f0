"""CPU side of the per-function device tests (tests/test_gpu_device_kat.py): the test module
tests/cpp/libdevkat.so builds for gfx950 with the library's own flags, exports every entry and
fails loudly without a GPU; the generators of tests/kat_cases.py, fed to the host oracle,
reproduce the reference's own answers (tests/golden/kat.npz), so a GPU failure cannot come
from the reference side; and the constructed edges really are edges (checked in binary64)."""
from __future__ import annotations

import subprocess
import sys

import numpy as np
import pytest

import devkat
import kat_cases as kc
from conftest import ROOT, bits, gpu_available

CPP = ROOT / "tests" / "cpp"
CSRC = ROOT / "pathtracer.cl_amd" / "csrc"


@pytest.fixture(scope="module")
def module_path():
    return devkat.build_module()


@pytest.fixture(scope="module")
def cases(pt, golden):
    return kc.all_cases(pt._abi, golden("kat"))


@pytest.fixture(scope="module")
def host(pt, oracle):
    return devkat.Host(pt._abi, oracle)


def test_module_builds_with_the_library_flags(module_path):
    """The compile line holds every flag of csrc/Makefile's COMMON and DEVFLAGS (read, not restated),
    -Werror and the gfx950 target; a full rebuild into a scratch name succeeds."""
    flags = subprocess.run(["make", "-s", "--no-print-directory", "-C", str(CSRC), "flags"], capture_output=True,
                           text=True, check=True).stdout.split()
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags and "-O3" in flags
    assert "-fhip-fp32-correctly-rounded-divide-sqrt" in flags
    line = subprocess.run(["make", "-n", "-B", "-C", str(CPP), "libdevkat.so"], capture_output=True, text=True,
                          check=True).stdout
    cmd = [ln for ln in line.splitlines() if "device_kat.hip" in ln and "hipcc" in ln]
    assert len(cmd) == 1, line
    words = cmd[0].split()
    for f in flags + ["-Werror"]:
        assert f in words, (f, cmd[0])
    assert not any(w.startswith("-fgpu-flush-denormals") or w == "-ffast-math" for w in words)
    assert module_path.exists()


def test_module_exports_every_entry(module_path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(module_path)], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(devkat.ENTRIES) <= exported, sorted(set(devkat.ENTRIES) - exported)
    assert not [s for s in exported if s.startswith("rt_")]  # it is not a second librtmi


def test_entries_fail_loudly_without_gpu(pt, module_path):
    """No GPU: every entry returns a non-zero HIP status and the process ends normally (a child process:
    a crash there is a failure here, not the end of the suite)."""
    if gpu_available():
        return  # tests/test_gpu_device_kat.py runs them
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "devkat.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split() for ln in r.stdout.splitlines())
    assert sorted(got) == sorted(devkat.ENTRIES)
    assert all(int(v) != 0 for v in got.values()), got


def test_compare_rejects_a_flushed_subnormal_a_zero_sign_and_a_stray_nan():
    """The comparison itself: bit equality incl. the sign of zero and subnormals; a NaN pair passes with
    any payload where it is allowed, and nowhere else."""
    want = {"out": kc.u2f([0x00000001, 0x80000000, 0x3f800000, 0xffc00000])}
    ok = np.array([False, False, False, True])
    assert devkat.compare("f", {"out": kc.u2f([0x00000001, 0x80000000, 0x3f800000, 0x7fc00001])}, want, ok) == 1
    for bad in ([0, 0x80000000, 0x3f800000, 0x7fc00000], [1, 0, 0x3f800000, 0x7fc00000],
                [1, 0x80000000, 0x3f800001, 0x7fc00000], [1, 0x80000000, 0x3f800000, 0x7f800000]):
        with pytest.raises(AssertionError, match="f: out differs"):
            devkat.compare("f", {"out": kc.u2f(bad)}, want, ok)
    with pytest.raises(AssertionError, match="NaN outside"):
        devkat.compare("f", {"out": want["out"]}, want, None)
    ints = {"hit": np.array([1, 0], np.int32)}
    with pytest.raises(AssertionError, match="hit differs"):
        devkat.compare("f", {"hit": np.array([1, 1], np.int32)}, ints)


def test_host_side_reproduces_the_reference_answers(pt, golden, cases, host):
    """Every kat.npz answer through the generators and the oracle's batch forms, bit for bit (the same
    fixture as test_oracle_golden.py's test_kat_*, through the path the GPU test uses)."""
    kat = golden("kat")
    ans = kc.kat_answers(pt._abi, kat)
    for name, want in ans.items():
        c = cases[name]
        got = devkat.run(host, c)
        if name == "frand":
            got = {"vals": got["vals"][:len(want["vals"])]}
        devkat.compare(name, got, want, c.nan_ok, c.row)
    # intersects_triangle's u and v too (the device's mt_test keeps only t)
    devkat.run(host, cases["mt_test (kat.npz)"])
    assert np.array_equal(bits(host.last_uvt), bits(kat["tri_uvt"]))
    assert 0.2 < kat["tri_hit"].mean() < 0.9


def test_host_nan_only_at_the_flagged_inputs(cases, host):
    """Outside the NaN / inf edge inputs (Case.nan_ok, decided from the inputs) the host side produces no
    NaN in any case: comparing each host result with itself applies exactly that rule."""
    for name, c in cases.items():
        got = devkat.run(host, c)
        devkat.compare(name, got, got, c.nan_ok, c.row)


def test_camera_cases_match_primary_rays_and_numpy(pt, golden, cases, host):
    """camera_dir's inputs: the oracle's camera ray, the float32 numpy restatement and rt_primary_rays
    (pixel centres) agree bit for bit at every generated pixel coordinate."""
    kat = golden("kat")
    c = cases["camera_dir"]
    cams, idx, a, b = c.args
    got = devkat.run(host, c)["d"]
    px = c.extra["pixels"]
    lib = pt.load_library()
    for ci, W in enumerate(kat["cam_widths"]):
        sel = idx == ci
        assert np.array_equal(bits(got[sel]), bits(kc.camera_dir_numpy(cams[ci], a[sel], b[sel])))
        W, H = int(W), kc.camera_height(int(W))
        rays = np.zeros(W * H, pt._abi.RAY_DTYPE)
        assert lib.rt_primary_rays(pt._abi.ptr(np.ascontiguousarray(cams[ci])), W, H, pt._abi.ptr(rays)) == pt._abi.RT_OK
        p = px[sel]
        centre = (p[:, 0] % 1 == 0.5) & (p[:, 1] % 1 == 0.5)
        assert centre.sum() == 128
        pix = p[centre, 1].astype(np.int64) * W + p[centre, 0].astype(np.int64)
        assert np.array_equal(bits(got[sel][centre]), bits(rays["d"][pix]))


def test_mwc_cases_host_is_plain_stepping(cases, host):
    """The host answer for mwc_jump is stepping in Python integers; mul is A^k mod M."""
    for gen, a in enumerate((36969, 18000)):
        c = cases[f"mwc_jump<{a}>"]
        _, x, k, mul = c.args
        got = devkat.run(host, c)["out"]
        m = a * 65536 - 1
        assert {m - 1, m, m + 1, 2**32 - 1} <= set(x.tolist()) and set(k.tolist()) == set(kc.MWC_KS)
        for i in range(0, len(x), 13):
            v = int(x[i])
            for _ in range(int(k[i])):
                v = (a * (v & 0xFFFF) + (v >> 16)) & 0xFFFFFFFF
            assert v == int(got[i]) and int(mul[i]) == pow(a, int(k[i]), m)


def test_constructed_edges_are_edges(pt, cases, host):
    f64 = np.float64
    small = f64(kc.RT_SMALL_F)
    # Moller-Trumbore: the det cases straddle RT_SMALL_F on both sides and both signs; det == 0 exactly;
    # the lattice rays meet u = 0, v = 0, u + v = 1, t = tmin and t = tmax exactly
    c = cases["mt_test (constructed edges)"]
    rays, tris = c.args
    tags = c.extra["tags"]
    det = kc.mt_det64(rays, tris)
    near = np.abs(det[tags == "det~small"])
    assert (near < small).any() and (near >= small).any() and (near == small).any()
    assert np.abs(near / small - 1).max() < 1e-6
    assert (det[tags == "det~small"] > 0).any() and (det[tags == "det~small"] < 0).any()
    assert (det[tags == "det==0"] == 0).all() and (det[tags == "zero-area"] == 0).all()
    res = devkat.run(host, c)
    uvt = host.last_uvt.astype(f64)
    assert not res["hit"][(tags == "det==0") | (tags == "zero-area")].any()
    assert not res["hit_any"][(tags == "det==0") | (tags == "zero-area")].any()
    hit = res["hit"] == 1
    u, v = uvt[:, 0], uvt[:, 1]
    on = hit & np.isin(tags, ["vertex", "edge"])
    assert on.sum() > 500 and (((u == 0) | (v == 0) | (u + v == 1))[on]).all()
    assert (hit[np.isin(tags, ["vertex", "edge", "inside"])]).all() and not hit[tags == "outside"].any()
    tmin, tmax = rays["tmin"].astype(f64), rays["tmax"].astype(f64)
    a = tags == "t==tmin"
    assert (uvt[a, 2] == tmin[a]).all() and res["hit"][a].all() and not res["hit_any"][a].any()
    a = tags == "t==tmax"
    assert (uvt[a, 2] == tmax[a]).all() and res["hit"][a].all() and not res["hit_any"][a].any()
    assert not res["hit"][np.isin(tags, ["t<tmin", "t>tmax"])].any()
    # det near the bound: accepted exactly where |det| >= RT_SMALL_F
    a = tags == "det~small"
    assert np.array_equal(res["hit"][a] == 1, np.abs(det[a]) >= small)

    # total internal reflection: cos_sq straddles 0 in binary64 and in the kernel's own arithmetic
    c = cases["sample_refraction"]
    rays, ior, blur = c.args[0], c.args[1], c.args[2]
    cs64, cs32 = kc.tir_cos_sq64(rays, ior), kc.tir_cos_sq32(rays, ior)
    leaving = rays["d"][:, 2] <= 0
    assert (cs64[leaving] < 0).sum() > 100 and (cs64[leaving] > 0).sum() > 100
    assert np.abs(cs64[leaving]).min() < 2.0 ** -23 and (cs32[leaving] < 0).any() and (cs32[leaving] > 0).any()
    assert (cs64[~leaving] > 0).all()
    assert {50.0, 99999.0, 100000.0, 1.0e6} == set(blur.tolist())
    assert (rays["d"][:, 2] == 0).sum() >= 8
    res = devkat.run(host, c)
    assert np.array_equal(res["ret"][leaving] == 1, cs32[leaving] < 0)  # TIR while leaving returns `!entering`

    # exp: the sweep's results are subnormal (rt_ldexpf's n < -126 branch), none flushed to zero
    sw = kc.exp_sweep()
    e64 = np.exp(sw.astype(f64))
    assert (e64 < f64(kc.FLT_MIN)).mean() > 0.95 and (e64 > f64(kc.SUB_MIN) / 2).all()  # all round to a non-zero subnormal
    got = host.math("exp", sw)["out"]
    sub = (got != 0) & (np.abs(got) < kc.FLT_MIN)
    assert sub.mean() > 0.95 and (got[sw >= np.float32(-103.2789299)] > 0).all()  # below it the model returns 0

    # perpendicular's switch: |n.y| on both sides of 0.9 and at it
    ny = np.abs(cases["perpendicular"].args[1][:, 1])
    assert (ny == np.float32(0.9)).any() and ((ny > np.float32(0.9)) & (ny < 0.9001)).any()
    assert ((ny < np.float32(0.9)) & (ny > 0.8999)).any()

    # sample_material: some drawn p equals each threshold, and lies 1 ulp to either side of it
    c = cases["sample_material (branch boundaries)"]
    mats, which, off, p = c.args[2], c.extra["which"], c.extra["off"], c.extra["p"]
    th = [mats["ks"], mats["ks"] + mats["kd"], (mats["ks"] + mats["kd"]) + mats["kt"]]
    pb = kc.f2u(p).astype(np.int64)
    for w in range(3):
        a = (which == w) & (p > 2.0 ** -20)
        d = kc.f2u(th[w].astype(np.float32)).astype(np.int64)[a] - pb[a]
        assert np.array_equal(d, off[a]) and {-1, 0, 1} == set(d.tolist())
    a = (which == 3) & (p >= 0.5)
    d = kc.f2u(th[2].astype(np.float32)).astype(np.int64)[a] - pb[a]
    assert {-1, 0, 1} <= set(d.tolist())
    res = devkat.run(host, c)
    assert (res["ret"] == 0).sum() > 100 and (res["ret"] == 1).sum() > 100  # absorbed and scattered
    first = np.ascontiguousarray(kc.frand_numpy(c.args[4])[0])
    assert np.array_equal(bits(first), bits(p))

    # sphere: the tangent rays' discriminant is negative, zero and positive
    c = cases["intersect_sphere (tangent)"]
    disc = kc.sphere_disc32(c.args[0], c.args[1], c.args[2])
    assert (disc == 0).sum() > 10 and (disc < 0).any() and (disc > 0).any()
    assert np.abs(disc).max() < 1e-3
    sc_ = cases["intersect_sphere (inside / on / outside)"].extra["scale"]
    assert {0.0, 0.5, 1.0, 2.0} <= set(sc_.tolist())

    # box: misses through a zero direction component (0), misses (inf) and hits; normals on every axis; the
    # exact corner and edge hit points
    c = cases["intersect_box + box_normal (constructed edges)"]
    res = devkat.run(host, c)
    t = res["t"]
    assert (t == 0).any() and np.isinf(t).any() and (np.isfinite(t) & (t > 0)).any()
    d = c.args[0]["d"]
    assert ((d == 0).sum(axis=1) == 3).any() and ((d == 0).sum(axis=1) == 1).any()
    o = c.args[0]["o"].astype(f64)
    with np.errstate(invalid="ignore"):
        hp = o + d.astype(f64) * t.astype(f64)[:, None]
        on_face = np.isfinite(t) & (t == 8.0)
        faces = (np.abs(np.abs(hp) - np.array([6.0, 5.0, 6.0])) == 0).sum(axis=1)
    assert (faces[on_face] == 3).sum() >= 8 and (faces[on_face] == 2).sum() >= 12
    for k in range(3):
        assert (res["normal"][:, k] == 1).any() and (res["normal"][:, k] == -1).any()
