"""k_resize's vertical pass (slam-module_amd/csrc/resize_vpass.h) on the CPU: tests/resize_vpass_check.cpp compares the pre-shifted taps, the masked
horizontal sums, the 24-bit high-half products and the packed-pair byte gather with the shift / multiply / shift / or form they replace -- every
row tap against every horizontal sum (67 M pairs), every tap pair that sums to 2047, 2048 or 2049 with every pair of bytes, 2 * 10^7 whole pixels,
and every sum 0 .. 1023 in each position of the packed dword."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "resize_vpass_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "resize_vpass_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "vpass ok" in out.stdout


def test_vertical_pass_is_exact():
    _build_and_run(EXE, [])


def test_vertical_pass_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
