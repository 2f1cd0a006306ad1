"""k_describe's BRIEF byte index (slam-module_amd/csrc/describe_brief_index.h) on the CPU: tests/describe_brief_index_check.cpp checks that one float
add of 1.5 * 2^23 rounds like __float2int_rn on every float in [-64, 64] (2.2 * 10^9 bit patterns), and that the folded 24-bit multiply-add gives the
old index, inside the 39 x 40-byte patch, for all 512 pattern points under the steering of every angle 0 .. 360 degrees in steps of 1 / 64."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "slam-module_amd", "lib", "describe_brief_index_check")


def _build_and_run(exe, extra):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "slam-module_amd", "csrc"),
                           os.path.join(ROOT, "tests", "describe_brief_index_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "brief index ok" in out.stdout


def test_brief_index_is_exact():
    _build_and_run(EXE, [])


def test_brief_index_under_sanitizers():
    """The same stand-alone host program with AddressSanitizer and UBSan (plain executable, nothing preloaded)."""
    _build_and_run(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
