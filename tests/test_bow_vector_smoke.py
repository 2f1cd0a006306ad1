"""The device BowVector in the host mirror (BowIndex::addAdmitted / addWords / bowVector in slam-module_amd/host/mi355slam/bow_index.hpp, DESIGN
9.20) compiles, links against the C ABI, and BowIndex::assembleVector gives the hand-computed vectors without a device; on the GPU an index
filled through admitKeyframe + addAdmitted and addWords equals its twin filled through assembleVector + add, entry by entry and in every
getBowSimilar result (tests/bow_vector_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "bow_vector_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "bow_vector_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_assemble_vector_gives_the_hand_computed_vectors():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and "restatement ok" in out, out


def test_the_mirror_adds_and_changes_nothing_that_was_there():
    hpp = open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "bow_index.hpp")).read()
    code = re.sub(r"//[^\n]*", "", hpp)
    for name, call in (("int addWords(", "ms_bow_db_add_words("), ("int addAdmitted(", "ms_keyframe_admit_words("), ("BowVector bowVector(", "ms_bow_db_entry(")):
        assert code.count(name) == 1 and code.count(call) == 1, name
    body = code[code.index("int addWords("):code.index("void remove(")]
    assert "std::map" not in body and ".upload(" not in body and "assembleVector" not in body and "ms_dev_download" not in body      # no host-side vector on the way in
    assert "static void assembleVector(" in code and "void add(const BowVector &bowVec, MapKf mapKf)" in code
    update = open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "map_update.hpp")).read()
    assert "BowIndex::assembleVector(word, weight, out.bowVector)" in update                     # admitKeyframe stays as it is


@pytest.mark.gpu
def test_both_indices_hold_the_same_entries_and_answer_alike():
    build_smoke()
    out = subprocess.check_output([EXE, "--gpu"], text=True)
    assert "bowVector ok: 4 entries" in out and "getBowSimilar ok:" in out and "refusals ok 4 cases" in out and "mirror ok" in out, out
