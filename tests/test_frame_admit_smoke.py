"""The tracker-frame arrival step of the host mirror (admitTrackerFrame and makeKeyframeDecision in slam-module_amd/host/mi355slam/map_update.hpp)
compiles, links against the C ABI, and makeKeyframeDecision gives the hand-computed answers and those of a literal std::set restatement of
mapper_helpers.cpp:28-65 without a device; on the GPU admitTrackerFrame puts a hand-computed frame into the tables, fills the slot record
and the chain, and every refusal leaves all of them as they were (tests/frame_admit_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slam-module_amd", "host", "mi355slam")
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "frame_admit_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "frame_admit_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_the_decision_gives_the_hand_computed_answers():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and "decision ok" in out and "FAILED" not in out, out


def test_one_device_call_nothing_uploaded_and_no_new_part_of_the_tables():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(HOST, "map_update.hpp")).read())
    body = code[code.index("inline AdmittedTrackerFrame admitTrackerFrame"):code.index("struct KeyframeAdmission")]
    assert body.count("ms_frame_admit(") == 1 and ".download(" not in body and ".upload(" not in body and ".update(" not in body and ".clear(" not in body
    assert body.rindex("std::invalid_argument") < body.index("ms_frame_admit(")                           # the mirror's refusals come before the device call
    assert body.index("ms_frame_admit(") < body.index("S.id[slot] =")                                     # and the record is filled behind it
    assert "S.descBase[slot] = -1" in body and "S.frames[slot] = nullptr" in body
    decision = code[code.index("inline bool makeKeyframeDecision"):code.index("struct TrackerFrameAdmission")]
    assert "ms_" not in decision and "static_cast<float>(nTracks)" in decision and "prevCovisibilities <= maxCovis" in decision      # a plain host function, the reference's types
    tables = open(os.path.join(HOST, "map_tables.hpp")).read()
    assert "FRAMES = 32768 }" in tables                      # MapTables::Part ends where it did


@pytest.mark.gpu
def test_mirror_admits_a_hand_computed_frame_and_fills_the_record():
    build_smoke()
    run = subprocess.run([EXE, "--gpu"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = run.stdout
    assert run.returncode == 0 and "FAILED" not in out, out
    assert "refusals ok 6 cases" in out and "admitTrackerFrame ok: 3 keypoints of 6 features" in out and "chain ok: 40 -> 41 -> 42" in out and "mirror ok" in out, out
