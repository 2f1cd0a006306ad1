"""The observation-list part of the host mirror (DeviceKeypointTable, DeviceObservationLists in slam-module_amd/host/mi355slam/map_tables.hpp,
updateMapPoints, retriangulateCurrent in map_update.hpp) compiles, links against the C ABI and, on the GPU, gives the tables of a sequential
restatement that keeps std::map<KfId, KpId> observations per map point (tests/obs_lists_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "obs_lists_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "obs_lists_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_the_validation_runs_without_a_device():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and re.search(r"no-gpu ok 6 cases", out), out


def test_no_std_map_of_observations_in_the_mirror():
    hpp = open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "map_update.hpp")).read()
    code = re.sub(r"//[^\n]*", "", hpp)
    for name in ("updateMapPoints", "retriangulateCurrent"):
        body = code[code.index("inline", code.index(name) - 80):]
        body = body[:body.index("\n}\n")]
        assert "std::map" not in body and "MapObservation" not in body and "ms_map_refresh(" not in body and "ms_triangulate(" not in body, name


@pytest.mark.gpu
def test_mirror_equals_the_std_map_restatement():
    build_smoke()
    out = subprocess.check_output([EXE], text=True, timeout=120)
    assert "obs lists ok" in out and "tables bit-equal" in out, out
