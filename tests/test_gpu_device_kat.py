"""The device build of the arithmetic model and of the kernels' helpers, function by function.

tests/cpp/libdevkat.so (device_kat.hip, compiled with the library's own flags) evaluates
include/rt_math.h, csrc/rt_device.h, rt_traverse.h's mt_test and rt_kernel_util.h's camera_dir /
mwc_jump on the GPU, one thread per element, on the inputs of tests/kat_cases.py; the CPU oracle
(oracle/pt_oracle.c, the same header on x86) answers the same inputs.  The two must agree bit
for bit — the sign of zero, subnormals and every seed word included.  One exception: where the
host result is a NaN the device result must be a NaN, payload and sign free (x86 and gfx950
generate different default NaNs; the kernels never pass such arguments), and outside the inputs
flagged for it (Case.nan_ok) neither side may produce a NaN at all.  The count of values accepted
under the exception is printed.  No tolerance appears in this file.

Where tests/golden/kat.npz holds the reference's own answers the device is compared with those
directly; camera_dir also with rt_primary_rays and a float32 numpy restatement; mwc_jump's host
answer is plain stepping."""
from __future__ import annotations

import numpy as np
import pytest

import devkat
import kat_cases as kc
from conftest import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(tracer, pt):
    return devkat.Device(pt._abi)


@pytest.fixture(scope="module")
def host(pt, oracle):
    return devkat.Host(pt._abi, oracle)


@pytest.fixture(scope="module")
def cases(pt, golden):
    return kc.all_cases(pt._abi, golden("kat"))


@pytest.fixture(scope="module")
def device_results():
    """Device results by case name, kept for the tests that compare them with a second reference."""
    return {}


def _device(dev, cases, device_results, name):
    if name not in device_results:
        device_results[name] = devkat.run(dev, cases[name])
    return device_results[name]


@pytest.mark.parametrize("name", kc.CASE_NAMES)
def test_device_equals_host(tracer, dev, host, cases, device_results, name):
    c = cases[name]
    got = _device(dev, cases, device_results, name)
    want = devkat.run(host, c)
    accepted = devkat.compare(name, got, want, c.nan_ok, c.row)
    print(f"{name}: {c.n} elements bit-identical; NaN-payload exceptions: {accepted}")


@pytest.mark.parametrize("name", kc.GUARD_NAMES)
def test_bounds_guard(tracer, dev, host, cases, name):
    """The same entry at n = 1 and at n = 65 537 (no multiple of the 256-thread block)."""
    for sub in kc.guard_subsets(cases[name]):
        accepted = devkat.compare(f"{name} (n = {sub.n})", devkat.run(dev, sub), devkat.run(host, sub), sub.nan_ok,
                                  sub.row)
        print(f"{name}: n = {sub.n} bit-identical; NaN-payload exceptions: {accepted}")


def test_device_equals_reference_answers(tracer, pt, golden, dev, cases, device_results):
    """The device against the reference kernel's own recorded answers (frand, triangle, sphere, box and
    its normal, sample_material, emissive), not only against the restatement."""
    for name, want in kc.kat_answers(pt._abi, golden("kat")).items():
        c = cases[name]
        got = _device(dev, cases, device_results, name)
        if name == "frand":
            got = {"vals": got["vals"][:len(want["vals"])]}
        accepted = devkat.compare(f"{name} vs kat.npz", got, want, c.nan_ok, c.row)
        print(f"{name}: equals kat.npz; NaN-payload exceptions: {accepted}")


def test_camera_dir_equals_primary_rays_and_numpy(tracer, pt, golden, dev, cases, device_results):
    kat = golden("kat")
    c = cases["camera_dir"]
    cams, idx, a, b = c.args
    got = _device(dev, cases, device_results, "camera_dir")["d"]
    px = c.extra["pixels"]
    lib = pt.load_library()
    for ci, W in enumerate(kat["cam_widths"]):
        sel = idx == ci
        want = kc.camera_dir_numpy(cams[ci], a[sel], b[sel])
        devkat.compare(f"camera_dir vs numpy (camera {ci})", {"d": got[sel]}, {"d": want}, None,
                       lambda i, s=np.flatnonzero(sel): c.row(s[i]))
        W, H = int(W), kc.camera_height(int(W))
        rays = np.zeros(W * H, pt._abi.RAY_DTYPE)
        assert lib.rt_primary_rays(pt._abi.ptr(np.ascontiguousarray(cams[ci])), W, H, pt._abi.ptr(rays)) == pt._abi.RT_OK
        p = px[sel]
        centre = np.flatnonzero((p[:, 0] % 1 == 0.5) & (p[:, 1] % 1 == 0.5))
        pix = p[centre, 1].astype(np.int64) * W + p[centre, 0].astype(np.int64)
        devkat.compare(f"camera_dir vs rt_primary_rays (camera {ci})", {"d": got[sel][centre]},
                       {"d": np.ascontiguousarray(rays["d"][pix])}, None,
                       lambda i, s=np.flatnonzero(sel)[centre]: c.row(s[i]))


def test_subnormal_results_are_not_flushed(tracer, dev, cases, device_results):
    """Named on its own, since it is what a changed denormal mode breaks first: exp over the sweep whose
    results are subnormal, a division with subnormal quotients and rt_ldexpf's n < -126 branch return
    non-zero subnormals from the device."""
    got = dev.math("exp", kc.exp_sweep())["out"]
    sub = (got != 0) & (np.abs(got) < kc.FLT_MIN)
    assert sub.mean() > 0.95, f"rt_expf: {sub.mean():.4f} of the sweep's results are subnormal on the device"
    for name in ("x / y", "rt_ldexpf"):
        out = _device(dev, cases, device_results, name)["out"]
        nsub = int(((out != 0) & (np.abs(out) < kc.FLT_MIN)).sum())
        assert nsub > 1000, f"{name}: only {nsub} subnormal results on the device"
