"""The refit of rt_update_mesh, without a GPU: tests/refit_ref.py (the numpy restatement the GPU
tests compare the kernels with) against the host builder's own trees — with unchanged vertices it
reproduces them bit for bit, with deformed vertices its boxes pass the verifier — and the new
C-ABI entries' argument checks."""
from __future__ import annotations

import ctypes
import subprocess

import numpy as np
import pytest

import refit_ref as rr
import tree_cases as tc
import tree_ref as tr
from conftest import ROOT, bits, gpu_available
from test_tree_host import dump_tool, host_trees, scene_lights  # noqa: F401  (dump_tool: a fixture)


@pytest.mark.parametrize("name", tc.MESHES)
def test_reference_reproduces_the_built_trees(name, pt, dump_tool, tmp_path):  # noqa: F811
    """Identity: boxes recomputed bottom-up from the links, the record order and the vertices the
    tree was built from equal the builder's nodes4, nodes4_shadow and records bit for bit."""
    verts, idx = tc.make(name, pt.scenes)
    tree = host_trees(dump_tool, tmp_path, verts, idx, scene_lights(pt.scenes))
    ref = rr.refit(tree, verts, idx)
    np.testing.assert_array_equal(bits(ref["tris"]), bits(tree["tris"]), err_msg="records")
    np.testing.assert_array_equal(bits(ref["nodes4"]), bits(tree["nodes4"]), err_msg="closest-hit tree")
    if tree["n_nodes4_shadow"]:
        np.testing.assert_array_equal(bits(ref["nodes4_shadow"]), bits(tree["nodes4_shadow"]), err_msg="shadow tree")
    else:
        assert ref["nodes4_shadow"] is None and name in tc.NOT_ENCODABLE
    assert rr.half_area_sum(ref["nodes4"]) == rr.half_area_sum(tree["nodes4"])


NO_CULLED = ["sphere200_first1", "sphere200_first5", "sphere200_first9", "sphere2000", "one_centre600", "flat_grid",
             "far_grid"]


# (wobble moves triangles of mixed_scales and det_bound across the never-hit bound: there the update
# rebuilds, tests/test_gpu_refit.py)
CASES = [(n, d) for n in NO_CULLED for d in ("rigid", "wobble")] + [("mixed_scales", "rigid"), ("det_bound", "rigid")]


@pytest.mark.parametrize("name,deform", CASES)
def test_reference_boxes_hold_deformed_vertices(name, deform, pt, dump_tool, tmp_path):  # noqa: F811
    """The reference's boxes for moved vertices contain every vertex below them and keep the
    documented pad (check_tree's full-precision part), in both trees; the records are the moved
    triangles'.  (mixed_scales and det_bound have culled triangles: rigid only, which flips none.)"""
    verts, idx = tc.make(name, pt.scenes)
    tree = host_trees(dump_tool, tmp_path, verts, idx, scene_lights(pt.scenes))
    nv = rr.DEFORM[deform](verts)
    assert not np.array_equal(nv, np.asarray(verts, np.float32).reshape(-1, 3))
    before = tr.never_hit_rule(tr.triangle_terms(verts, idx))
    after = tr.never_hit_rule(tr.triangle_terms(nv, idx))
    assert (np.abs(before - 1) > 1e-6).all() and (np.abs(after - 1) > 1e-6).all()
    assert ((before < 1) == (after < 1)).all(), "precondition: no triangle crosses the never-hit bound"
    ref = rr.refit(tree, nv, idx)
    got = tr.check_tree(nv, idx, rr.closest_only(tree, ref), 0, builder="host")
    assert got["n_hit"] == tree["reported"][0]["n_hit"]
    assert tree["n_nodes4_shadow"] > 0
    got = tr.check_tree(nv, idx, rr.as_closest(tree, ref), 0, builder="host")
    assert got["n_hit"] == tree["reported"][0]["n_hit"]
    # and the verifier does reject the old boxes for the new vertices
    with pytest.raises(tr.TreeError):
        stale = dict(rr.closest_only(tree, ref), nodes4=tree["nodes4"])
        tr.check_tree(nv, idx, stale, 0, builder="host")


def build_view_program(out_dir):
    """tests/cpp/view_update_mesh.cpp (RayTracerHIP::updateMesh, ProgressiveViewHIP::updateMesh)
    compiled against the headers and the library of this tree."""
    lib_dir = ROOT / "pathtracer.cl_amd"
    exe = out_dir / "view_update_mesh"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "view_update_mesh.cpp"), f"-L{lib_dir}", "-lrtmi",
                    f"-Wl,-rpath,{lib_dir}"], check=True, timeout=300)
    return exe


def test_cpp_methods_compile_and_fail_loudly_without_gpu(pt, tmp_path):
    exe = build_view_program(tmp_path)
    if gpu_available():
        return  # tests/test_gpu_refit.py runs it
    r = subprocess.run([str(exe), "16", "12", "2000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "rt_create" in r.stderr  # no CPU fallback


def test_new_entries_reject_null(pt):
    """rt_update_mesh, rt_last_mesh_update and rt_set_mesh_dynamic exist and return RT_ERR_ARG for
    a null context (no GPU is touched)."""
    lib = pt.load_library()
    v = np.zeros(9, np.float32)
    info = pt._abi.RtMeshUpdateInfo()
    assert lib.rt_update_mesh(None, pt._abi.ptr(v), 3, 0) == pt._abi.RT_ERR_ARG
    assert lib.rt_last_mesh_update(None, ctypes.byref(info)) == pt._abi.RT_ERR_ARG
    assert lib.rt_set_mesh_dynamic(None, 1) == pt._abi.RT_ERR_ARG
    assert ctypes.sizeof(info) == 24
