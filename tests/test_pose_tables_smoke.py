"""The pose-BA part of the host mirror (poseBundleAdjustOnTables and DevicePoseAdjuster in slam-module_amd/host/mi355slam/map_update.hpp)
compiles, links against the C ABI, runs the host validation without a device and, on the GPU, equals the mirror's own poseBundleAdjust on a
window the host builds from Keyframe::mapPoints and a map of MapPoints, bit for bit, with the reference's bool in both directions
(tests/pose_tables_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "pose_tables_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "pose_tables_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_the_host_half_runs_without_a_device():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and re.search(r"no-gpu ok 6 cases", out), out


def test_no_host_walk_in_the_mirror():
    hpp = open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "map_update.hpp")).read()
    code = re.sub(r"//[^\n]*", "", hpp)
    body = code[code.index("inline bool poseBundleAdjustOnTables"):]
    body = body[:body.index("\n}\n")]
    assert "std::map" not in body and "std::vector" not in body and ".update(" not in body and ".upload(" not in body and ".download(" not in body
    assert body.count("ms_pose_tables_solve(") == 1 and "ms_ba_" not in body


@pytest.mark.gpu
def test_mirror_equals_pose_bundle_adjust_on_the_host_built_window():
    build_smoke()
    out = subprocess.check_output([EXE], text=True)
    assert "poseBundleAdjustOnTables ok" in out and "both directions of the bool hold" in out, out
