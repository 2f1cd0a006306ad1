"""The local-BA part of the host mirror (localBundleAdjustOnTables in slam-module_amd/host/mi355slam/map_update.hpp) compiles, links against
the C ABI, builds the local-keyframe set of a std::set restatement without a device and, on the GPU, holds its window, its early-outs and
both write-back modes against a restatement that keeps Keyframe::mapPoints and `std::map<KfId, KpId>` observations on the host
(tests/ba_window_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "ba_window_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "ba_window_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_the_host_half_runs_without_a_device():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and re.search(r"no-gpu ok 9 cases, 24 local-keyframe sets", out), out


def test_no_host_walk_in_the_mirror():
    hpp = open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "map_update.hpp")).read()
    code = re.sub(r"//[^\n]*", "", hpp)
    body = code[code.index("inline LocalBaOnTables localBundleAdjustOnTables"):]
    body = body[:body.index("\n}\n")]
    assert "std::map" not in body and "std::set" not in body and ".update(" not in body and ".upload(" not in body
    calls = ("detail::local_keyframes(", "ms_map_point_union(", "lists.build(", "ms_ba_window_lists(", "localBundleAdjust(", "ms_ba_window_apply(")
    for call in calls:
        assert call in body, call
    at = [body.index(c) for c in calls]
    assert at == sorted(at)


@pytest.mark.gpu
def test_mirror_equals_the_std_map_restatement():
    build_smoke()
    out = subprocess.check_output([EXE], text=True)
    assert "localBundleAdjustOnTables ok" in out and "early-outs and NEIGHBOR hold" in out, out
