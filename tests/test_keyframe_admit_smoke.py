"""The keyframe-arrival step of the host mirror (admitKeyframe in slam-module_amd/host/mi355slam/map_update.hpp, DeviceKeyframe(ctx, capacity),
DeviceDescriptorPool(ctx, capacity) with reserve(), BowIndex::assembleVector) compiles, links against the C ABI, and its std::map /
std::stable_sort restatement gives the hand-computed results without a device; on the GPU the mirror equals that restatement on two keyframes
admitted from a two-frame device view -- tables, DeviceKeyframe, slot record, chain, pool -- and every refusal leaves all of them as they were
(tests/keyframe_admit_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slam-module_amd", "host", "mi355slam")
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "keyframe_admit_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "keyframe_admit_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_the_restatement_gives_the_hand_computed_results():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and "restatement ok" in out, out


def test_one_device_call_nothing_uploaded_and_only_additions_in_the_mirror():
    code = re.sub(r"//[^\n]*", "", open(os.path.join(HOST, "map_update.hpp")).read())
    body = code[code.index("inline AdmittedKeyframe admitKeyframe"):code.index("struct FuseKeyframe")]
    assert body.count("ms_keyframe_admit(") == 1 and ".download(" not in body and ".upload(" not in body and "std::map" not in body and "ms_orb_download" not in body
    assert body.index("std::invalid_argument") < body.index("ms_keyframe_admit(") and "assembleVector(" in body and "FeatureVector" not in body
    tables = open(os.path.join(HOST, "map_tables.hpp")).read()
    assert "FRAMES = 32768 }" in tables                      # MapTables::Part ends where it did: no new part was needed
    assert "DeviceDescriptorPool(Context &ctx, std::size_t capacity)" in tables and "std::size_t reserve(std::size_t n)" in tables
    # the existing constructors are still there
    assert "DeviceDescriptorPool(Context &ctx, const std::vector<KeyPoint::Descriptor> &descriptors)" in tables
    matcher = open(os.path.join(HOST, "keyframe_matcher.hpp")).read()
    assert "DeviceKeyframe(Context &ctx, const KeyframeFeatures &kf)" in matcher and "DeviceKeyframe(Context &ctx, std::size_t capacity)" in matcher
    bow = open(os.path.join(HOST, "bow_index.hpp")).read()
    assert "static void assemble(" in bow and "static void assembleVector(" in bow


@pytest.mark.gpu
def test_mirror_equals_the_restatement_on_two_admitted_keyframes():
    build_smoke()
    run = subprocess.run([EXE, "--gpu"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = run.stdout
    assert run.returncode == 0 and "FAILED" not in out, out
    assert "refusals ok 4 cases" in out and "admitKeyframe ok: 5 keypoints, 1 node, 3 in the lists" in out and "chain ok: 40 -> 41, pool 7 of 9" in out and "mirror ok" in out, out
