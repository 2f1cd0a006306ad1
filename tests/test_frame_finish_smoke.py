"""The end-of-frame step of the host mirror (finishFrame and removeKeyframes in slam-module_amd/host/mi355slam/map_update.hpp) compiles, links
against the C ABI, and its std::map / std::set restatement gives the hand-computed results without a device; on the GPU the mirror equals
that restatement on the hand-computed map -- the cloud, the removed rows in first-claim order, the relinked chain -- refuses the two cases
removeKeyframe asserts on with std::invalid_argument before any device call, and leaves every table as it was for a frame that became a
keyframe (tests/frame_finish_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "frame_finish_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "frame_finish_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_the_restatement_gives_the_hand_computed_results():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and "restatement ok" in out, out


def test_one_device_call_and_no_new_part_in_the_mirror():
    hpp = open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "map_update.hpp")).read()
    code = re.sub(r"//[^\n]*", "", hpp)
    body = code[code.index("inline FrameFinish finish_frame"):code.index("inline FrameFinish removeKeyframes")]
    assert body.count("ms_frame_finish(") == 1 and ".download(" not in body and ".upload(" not in body and "std::map" not in body
    assert body.index("std::invalid_argument") < body.index("ms_frame_finish(")                  # the refusals come before the device call
    assert "M.POINTS | M.FLAGS | M.LIVE | M.LINKS | M.IDS" in body and "M.observationCount" in body
    tables = open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "map_tables.hpp")).read()
    assert "FRAMES = 32768 }" in tables                      # MapTables::Part ends where it did


@pytest.mark.gpu
def test_mirror_equals_the_restatement_on_the_hand_computed_map():
    build_smoke()
    out = subprocess.check_output([EXE, "--gpu"], text=True)
    assert "keyframeDecision = true leaves every table as it was" in out and "finishFrame ok: cloud 4, removed rows 3, erased observations 7" in out, out
    assert "removeKeyframes ok: removed rows 3; relinked chain ok" in out and "invalid_argument ok 4 cases" in out, out
