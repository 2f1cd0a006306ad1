"""Pass 2 of k_describe's blur with pass 1's result as the B operand (slam-module_amd/csrc/describe_lanes.h: vert_operand, blur_store_*) on the CPU:
tests/describe_blur_operand_check.cpp models the i8 matrix instruction's lane layouts and checks that the permuted vertical operand gives the direct
banded sum in the chained high / low form (random, all-minimum and all-maximum intermediates), that rows 45 .. 47 and the fourth dword never reach a
patch row, that the swapped-argument BRIEF index addresses the column-major patch as the old one addressed the row-major one, and that the store map
covers the 39 x 10 dwords exactly once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "describe_blur_operand_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "describe_blur_operand_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "blur operand ok" in out.stdout


def test_blur_operand_is_exact():
    _build_and_run(EXE, [])


def test_blur_operand_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
