"""The createNewMapPoints part of the host mirror (createNewMapPoints and unboundMasks in slam-module_amd/host/mi355slam/map_update.hpp) compiles,
links against the C ABI and, on the GPU, gives the per-adjacent results, tables and masks of a sequential restatement that keeps
Keyframe::mapPoints and `std::map<KfId, KpId>` observations on the host and hands host lists to the host-list entry points
(tests/create_points_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "create_points_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "create_points_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_the_validation_runs_without_a_device():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and re.search(r"no-gpu ok 12 cases", out), out


def test_no_host_walk_in_the_mirror():
    hpp = open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "map_update.hpp")).read()
    code = re.sub(r"//[^\n]*", "", hpp)
    body = code[code.index("inline std::vector<CreatedPoints> createNewMapPoints"):]
    body = body[:body.index("\n}\n")]
    assert "std::map" not in body and "TriangulateArgs" not in body and "ms_triangulate(" not in body and ".update(" not in body
    for call in ("create_E_21(", "ms_match_triangulation(", "ms_create_points_lists(", "ms_triangulate_lists(", "ms_create_points_bind("):
        assert call in body, call
    assert body.index("ms_match_triangulation(") < body.index("ms_create_points_lists(") < body.index("ms_triangulate_lists(") < body.index("ms_create_points_bind(")


@pytest.mark.gpu
def test_mirror_equals_the_std_map_restatement():
    build_smoke()
    out = subprocess.check_output([EXE], text=True)
    assert "createNewMapPoints ok" in out and "tables bit-equal" in out, out
