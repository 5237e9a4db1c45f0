"""RT_BUILD_OPT_LIGHTS without a GPU: the library exports the entry points the Python layer
declares, the option's value is the header's, and the restated rules (tests/build_lights_cases.py)
split the meshes the GPU tests rely on."""
from __future__ import annotations

import re

import pytest

import build_lights_cases as bl
import test_light_cone_host as lh
from conftest import ROOT


def test_entry_points(pt):
    lib = pt.load_library()
    for name in ("rt_set_build_options", "rt_get_build_options"):
        assert name in pt._abi.SIGNATURES
        assert getattr(lib, name) is not None
    header = (ROOT / "include" / "pathtracer_rt.h").read_text()
    m = re.search(r"enum\s*\{\s*RT_BUILD_OPT_LIGHTS\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == pt._abi.RT_BUILD_OPT_LIGHTS == 1
    assert "rt_set_build_options" in header and "rt_get_build_options" in header
    assert hasattr(pt.RayTracer, "setBuildOptions")
    assert "RT_BUILD_OPT_LIGHTS" in (ROOT / "INTEGRATION.md").read_text()


@pytest.mark.parametrize("name", list(lh.SPLIT_CASES))
def test_restated_rules_split_the_cases(name, pt):
    verts, idx, lights = lh.make_case(name, pt)
    c = bl.classes(verts, idx, lights)
    assert bl.expect_split(verts, idx, lights) is True
    assert c["unsure"] == 0 and not (c["parked"] & c["occluder"]).any() and not (c["out"] & c["kept"]).any()
