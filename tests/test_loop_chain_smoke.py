"""The loop closer's host mirror (tryLoopClosureOnTables in slam-module_amd/host/mi355slam/loop_closer.hpp) compiles, links against the C ABI and,
on the GPU, gives the codes, stages, transforms and match lists of a walk of tryLoopClosure over std::map observations built from the host-list
mirrors (tests/loop_chain_smoke.cpp)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "loop_chain_smoke")


def build_smoke():
    lib = os.path.join(ROOT, "slam-module_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "slam-module_amd", "host"),
                           os.path.join(ROOT, "tests", "loop_chain_smoke.cpp"), "-o", EXE, "-L", lib, "-lmi355slam", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_mirror_compiles_links_and_the_validation_runs_without_a_device():
    build_smoke()
    out = subprocess.check_output([EXE, "--no-gpu"], text=True)
    assert "link ok 1" in out and re.search(r"no-gpu ok 11 cases", out), out


def test_the_mirror_keeps_no_map_and_moves_no_table():
    """No std::map, no upload and no table update in tryLoopClosureOnTables; what comes down is tri_row and what the three calls return."""
    code = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "slam-module_amd", "host", "mi355slam", "loop_closer.hpp")).read())
    body = code[code.index("inline LoopClosureResult tryLoopClosureOnTables"):]
    body = body[:body.index("\n}\n")]
    assert "std::map" not in body and "ms_dev_upload" not in body and ".update(" not in body and ".upload(" not in body
    assert body.count(".download(") == 2 and body.count("triRow[") == 2                                         # the TRIANGULATED rows of the two sides
    order = ["cheapRejection(", "ms_loop_usable_mask(", "ms_match_loop_closure(", "ms_loop_pairs(", "minLoopClosureFeatureMatches", "ransacSolveAll(", "bestInliers[",
             "matchMapPointsSim3(", "ms_loop_sim3_lists(", "OptimizeSim3TransformAll(", "acceptGates(", "std::sort("]
    at = [body.index(k) for k in order]
    assert at == sorted(at), at
    for call in ("ms_loop_usable_mask(", "ms_match_loop_closure(", "ms_loop_pairs(", "ms_loop_sim3_lists("):
        assert body.count(call) == 1, call


@pytest.mark.gpu
def test_mirror_equals_the_std_map_walk():
    build_smoke()
    out = subprocess.check_output([EXE, "--gpu"], text=True)
    assert "tryLoopClosureOnTables ok" in out, out
    assert re.search(r"codes: OK 1, TOO_CLOSE_TIME 1, UNNECESSARY_EARLY 1, TOO_FEW_FEATURE_MATCHES \d+, RANSAC_FAILED 1, UNNECESSARY 1, not reached 1 of 15 listed", out), out
