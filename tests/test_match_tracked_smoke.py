"""The matchTrackedFeatures part of the host mirror (DeviceTrackTable in slam-module_amd/host/mi355slam/map_tables.hpp and matchTrackedFeatures in
map_update.hpp) compiles, links against the C ABI and, on the GPU, gives the outcomes, counters and tables of a sequential restatement that walks
keyPointToTrackId and trackIdToMapPoint in std::maps and hands host lists to the host-list entry points (tests/match_tracked_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "match_tracked_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "match_tracked_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_the_validation_runs_without_a_device():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and re.search(r"no-gpu ok 10 cases", out), out


def test_no_std_map_in_the_mirror():
    hpp = open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "map_update.hpp")).read()
    code = re.sub(r"//[^\n]*", "", hpp)
    body = code[code.index("inline MatchTrackedResult matchTrackedFeatures"):]
    body = body[:body.index("\n}\n")]
    assert "std::map" not in body and "MapObservation" not in body and "ms_map_refresh(" not in body and "ms_triangulate(" not in body
    for call in ("ms_match_tracked(", "ms_triangulate_lists(", "ms_match_tracked_finish(", "ms_map_refresh_lists("):
        assert call in body, call


@pytest.mark.gpu
def test_mirror_equals_the_std_map_restatement():
    build_smoke()
    out = subprocess.check_output([EXE], text=True)
    assert "matchTrackedFeatures ok descriptors 1" in out and "matchTrackedFeatures ok descriptors 0" in out and "tables bit-equal" in out, out
