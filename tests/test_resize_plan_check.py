"""k_resize8's plan (slam-module_amd/csrc/resize_plan.h) on the CPU: tests/resize_plan_check.cpp rebuilds the resize tables for source sizes
40 .. 1400 at ratios 1.0 .. 2.0 and for the levels of the usual frame sizes, checks the eligibility predicate against a brute-force walk, runs a
model of a lane's window extraction (16-byte load, edge shift, three funnels, selectors) over rows that end where the kernel must stop reading,
walks every block of both grid mappings for 1 .. 33 frames (each (frame, row group, chunk) exactly once; by frame, one XCD label per frame), and
checks the block decode's multiply-high division against the division."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "resize_plan_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "resize_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "resize plan ok" in out.stdout


def test_plan_and_window_model():
    _build_and_run(EXE, [])


def test_plan_and_window_model_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
