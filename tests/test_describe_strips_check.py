"""k_describe's launch plan (slam-module_amd/csrc/describe_strips.h) on the CPU: tests/describe_strips_check.cpp builds the plan for
frames in {1, 2, 3, 5, 256} x capacity in {1 .. 40, 500, 2000, 2003} x resident blocks in {1, 8, 2048} x forced r in {0 .. 8} and walks every block
as the kernel does: every (frame, slot) visited exactly once, no strip across a frame, at most four regions, the automatic plan's tail of
>= 2 x resident one-keypoint blocks (or all r = 1 for a small launch), the block count within the grid limit, and the multiply-high block decode
against the division."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "describe_strips_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "describe_strips_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "strips ok" in out.stdout


def test_plan_covers_every_slot_once():
    _build_and_run(EXE, [])


def test_plan_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
