"""The triangle kernel's device code keeps its f32 math unpacked — CPU only, needs hipcc.

`make asm` compiles rt_tris.hip to gfx950 assembly with the library's own flags.  -O3 alone
SLP-packs neighbouring scalar f32 multiplies and adds into v_pk_mul_f32 / v_pk_add_f32, which on
gfx950 issue in 4 cycles (as many as the two scalar ops they replace) and need their operands
moved into aligned register pairs; the Makefile's DEVFLAGS turn that off (-fno-slp-vectorize,
DESIGN.md §7).  Every k_tris instantiation must hold no packed f32 multiply, add or FMA, and must
keep the register budget the launch forms are sized for: at most 96 VGPRs,
occupancy 5.  A flag edit that brings the packing back fails here, not on a profile.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "pathtracer.cl_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.access(HIPCC, os.X_OK) or shutil.which(HIPCC)), reason="no hipcc")

PACKED_F32 = ("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32")


def kernel_bodies(text: str) -> dict[str, list[str]]:
    """symbol -> its lines, from the compiler's `-- Begin function` mark to the next one (the code
    and the resource comments after it), for every symbol that is a kernel (.amdhsa_kernel)."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out: dict[str, list[str]] = {}
    cur = None
    for ln in text.split("\n"):
        m = re.search(r"; -- Begin function (\S+)", ln)
        if m:
            cur = m.group(1) if m.group(1) in kernels else None
            if cur:
                out[cur] = []
        elif cur:
            out[cur].append(ln)
    return out


@pytest.fixture(scope="module")
def tris_kernels(tmp_path_factory):
    build = tmp_path_factory.mktemp("asm")
    r = subprocess.run(["make", "-s", "-C", str(CSRC), f"BUILD={build}", f"{build}/rt_tris.s"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("make asm failed:\n" + r.stdout[-3000:] + r.stderr[-3000:])
    ks = {k: v for k, v in kernel_bodies((build / "rt_tris.s").read_text()).items() if "k_tris" in k}
    assert ks, "no k_tris symbol in rt_tris.s"
    return ks


def test_device_flags_turn_slp_off():
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "flags"], capture_output=True, text=True, check=True)
    assert "-fno-slp-vectorize" in r.stdout.split()


def test_no_packed_f32_in_k_tris(tris_kernels):
    for sym, body in tris_kernels.items():
        bad = [ln.strip() for ln in body if ln.split() and ln.split()[0] in PACKED_F32]
        assert not bad, (sym, len(bad), bad[:4])


def test_k_tris_register_budget(tris_kernels):
    for sym, body in tris_kernels.items():
        text = "\n".join(body)
        occ = re.search(r";\s*Occupancy:\s*(\d+)", text)
        vg = re.search(r";\s*NumVgprs:\s*(\d+)", text)
        assert occ and vg, sym
        assert int(occ.group(1)) == 5, (sym, occ.group(0))
        assert int(vg.group(1)) <= 96, (sym, vg.group(0))
